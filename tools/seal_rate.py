"""Rates of the device HPKE seal against the device open and the host oracle (the
section on the sealer).  A build-time measurement, not a test and not bench.py:

  python tools/seal_rate.py [--n 8192 262144] [--repeats 15] [--host-n 20000] [--json PATH]

For DHKEM(X25519) and DHKEM(P-256) with HKDF-SHA256 / AES-128-GCM and helper input shares of
Histogram(256,16)'s shape (32-byte public share, 48-byte helper share), per n:
  * seal: janus_hpke_seal_input_shares_device, reports/s;
  * open: janus_hpke_open_input_shares_device on the sealed rows, same n, suite and process;
  * seal / open, the figure to judge by (two scalar multiplications against one: about one half);
  * once per KEM, the OpenSSL oracle's host seal on 16 threads (reports/s, host clock).
Device times are HIP events around repeated launches on one stream after warm-up launches of the
same shape; the figure is the median launch.  Every opened share is compared with what was sealed
before any number is printed.  Needs the GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PUB_LEN, SHARE_LEN = 32, 48


def _median_ms(fn, repeats, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(repeats)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def measure(kem, n, repeats):
    import torch
    from janus_amd import hpke as G
    from oracle import hpke as H
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(kem + n)
    skR = H.kem_private(rng, kem)
    pkR = H.kem_public(skR, kem)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    g = torch.Generator(device=dev).manual_seed(n)
    u8 = dict(generator=g, device=dev, dtype=torch.uint8)
    sk = torch.randint(0, 256, (n, 32), **u8)
    if kem == H.KEM_P256:
        sk[:, 0] &= 0x7F  # below 2^255, hence below the group order
    ids = torch.randint(0, 256, (n, 16), **u8)
    pubs = torch.randint(0, 256, (n, PUB_LEN), **u8)
    shares = torch.randint(0, 256, (n, SHARE_LEN), **u8)
    times = 1_700_000_000 + torch.randint(0, 3600, (n,), generator=g, device=dev,
                                          dtype=torch.int64)
    enc = torch.empty((n, G.NENC[kem]), dtype=torch.uint8, device=dev)
    ct = torch.empty((n, G.sealed_stride(SHARE_LEN)), dtype=torch.uint8, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty((n, SHARE_LEN), dtype=torch.uint8, device=dev)
    ost = torch.empty(n, dtype=torch.uint8, device=dev)
    sealer = G.HpkeSealer(pkR, device=0, kem_id=kem)
    opener = G.HpkeOpener(skR, pkR, device=0, kem_id=kem)

    def seal():
        sealer.seal_input_shares_device(task, sk, ids, times, pubs, shares, enc, ct, cl, st)

    def open_():
        opener.open_input_shares_device(task, enc, ct, cl, ids, times, pubs, out, ost)

    seal_ms = _median_ms(seal, repeats)
    open_ms = _median_ms(open_, repeats)
    if int(st.any()) or int(ost.any()) or not torch.equal(out, shares):
        raise SystemExit(f"kem {kem:#x} n {n}: the opened shares differ from the sealed ones")
    return dict(kem=kem, n=n, seal_ms=seal_ms[0], seal_ms_min=seal_ms[1], seal_ms_max=seal_ms[2],
                open_ms=open_ms[0], open_ms_min=open_ms[1], open_ms_max=open_ms[2],
                seal_per_s=n / seal_ms[0] * 1e3, open_per_s=n / open_ms[0] * 1e3,
                seal_over_open=open_ms[0] / seal_ms[0])


def host_seal_rate(kem, n, threads=16):
    """The oracle's threaded sealer of whole input shares (hpke_make_input_shares_suite)."""
    from oracle import hpke as H
    H.make_batch_fast(256, SHARE_LEN, PUB_LEN, n_threads=threads, kem=kem)  # load, warm
    t0 = time.perf_counter()
    H.make_batch_fast(n, SHARE_LEN, PUB_LEN, n_threads=threads, kem=kem)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[8192, 262144])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host-n", type=int, default=20000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seal_rate.py measures on the GPU; none is available")
    from oracle import hpke as H
    rows = []
    for kem, name in ((H.KEM_X25519, "X25519"), (H.KEM_P256, "P-256")):
        host = host_seal_rate(kem, a.host_n)
        print(f"{name}: oracle host seal, 16 threads: {host / 1e3:.1f} K reports/s", flush=True)
        for n in a.n:
            r = measure(kem, n, a.repeats)
            r["name"], r["host_seal_per_s"] = name, host
            rows.append(r)
            print(f"{name} n={n}: seal {r['seal_per_s'] / 1e6:.3f} M/s ({r['seal_ms']:.3f} ms, "
                  f"{r['seal_ms_min']:.3f}-{r['seal_ms_max']:.3f}), open "
                  f"{r['open_per_s'] / 1e6:.3f} M/s ({r['open_ms']:.3f} ms, "
                  f"{r['open_ms_min']:.3f}-{r['open_ms_max']:.3f}), seal/open "
                  f"{r['seal_over_open']:.2f}, seal/host {r['seal_per_s'] / host:.0f}x",
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

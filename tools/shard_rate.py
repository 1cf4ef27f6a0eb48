"""Rates of the client role on the device (the section on the client).  A build-time
measurement, not a test and not bench.py:

  python tools/shard_rate.py [--repeats 7] [--cpu-n 20000] [--only NAME] [--json PATH]

For Histogram(256,16) at 1 Mi reports, Sum(32) at 1.25 M reports and
SumVecField64MultiproofHmacSha256Aes128 at the reference's parameters (proofs 2, bits 16, length 15,
chunk 16; k_shard_mp64) at 1,000,000 reports:
  * shard: prio3_client_shard_device (k_shard) alone, reports/s;
  * one call: prio3_client_prepare_reports_device with two X25519 / HKDF-SHA256 / AES-128-GCM
    sealers (shard, both seals, Report encode), reports/s, and the share of that time the
    leader-share seal takes when measured alone on rows of the same shape;
  * generator: prio3_client_generate_device at the same n -- it draws its own inputs and also runs
    the leader's prepare_init, so k_shard does a subset of its arithmetic plus the input reads;
  * CPU: the C restatement's orc_gen_reports on 16 threads (host clock; it includes the leader's
    prepare_init too).  Not for the multiproof instance: the C restatement's shard does not take
    32-byte seeds, so its sample is checked against the Python restatement instead.
Device times are HIP events around repeated calls on one stream after warm-up calls of the same
shape; the figure is the median call.  The generator synchronises inside its call, so its event
time includes that wait.  A sample of the shards is compared with the restatement before any
number is printed.  Needs the GPU: there is no fallback.
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

CASES = (("hist_256_c16", dict(kind="histogram", length=256, chunk_length=16), 1 << 20),
         ("sum32", dict(kind="sum", bits=32), 1_250_000),
         ("sumvec_f64_mp_2x16x15_c16",
          dict(kind="sumvec_f64_mp", bits=16, length=15, chunk_length=16, num_proofs=2), 1_000_000))


def _vdaf(J, cfg):
    if cfg["kind"] == "histogram":
        return J.Prio3Histogram(cfg["length"], cfg["chunk_length"])
    if cfg["kind"] == "sumvec_f64_mp":
        return J.Prio3SumVecField64MultiproofHmacSha256Aes128(
            cfg["num_proofs"], cfg["bits"], cfg["length"], cfg["chunk_length"])
    return J.Prio3Sum(cfg["bits"])


def _sample_shards(cfg, m, ids, rand):
    """The restatement's (public, leader, helper) of the sample rows."""
    if cfg["kind"] == "sumvec_f64_mp":  # ~40 ms a report in Python: eight of them
        from oracle.prio3_py import Prio3, Prio3Type
        v = Prio3(Prio3Type(**cfg))
        return [v.shard([int(x) for x in m[i]], ids[i].tobytes(), rand[i].tobytes())
                for i in range(8)]
    from oracle.oracle import Oracle
    o = Oracle(**cfg)
    return [o.shard(int(m[i, 0]), ids[i].tobytes(), rand[i].tobytes()) for i in range(len(m))]


def _median_ms(fn, repeats, warmup=2):
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


def measure(name, cfg, n, repeats, cpu_n):
    import torch
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle import hpke as H
    from oracle.oracle import Oracle
    dev = torch.device("cuda", 0)
    mp = cfg["kind"] == "sumvec_f64_mp"
    eng = J.HelperEngine(_vdaf(J, cfg), bytes(range(32 if mp else 16)), device=0)
    sz = eng.sz
    g = torch.Generator(device=dev).manual_seed(n)
    hi = cfg["length"] if cfg["kind"] == "histogram" else 1 << cfg["bits"]
    m = torch.randint(0, hi, (n, cfg["length"] if mp else 1), generator=g, device=dev,
                      dtype=torch.int64)
    u8 = dict(generator=g, device=dev, dtype=torch.uint8)
    ids = torch.randint(0, 256, (n, 16), **u8)
    rand = torch.randint(0, 256, (n, eng.rand_len), **u8)
    sk_l = torch.randint(0, 256, (n, 32), **u8)
    sk_h = torch.randint(0, 256, (n, 32), **u8)
    times = 1_700_000_000 + torch.randint(0, 3600, (n,), generator=g, device=dev,
                                          dtype=torch.int64)
    rng = np.random.default_rng(n)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    pk_l = H.kem_public(H.kem_private(rng))
    pk_h = H.kem_public(H.kem_private(rng))
    ls = G.HpkeSealer(pk_l, G.INFO_INPUT_SHARE_LEADER, device=0)
    hs = G.HpkeSealer(pk_h, G.INFO_INPUT_SHARE_HELPER, device=0)
    keep = {}

    def shard():
        keep["s"] = eng.shard_device(m, ids, rand)

    def one_call():
        keep["r"] = eng.prepare_reports_device(ls, hs, task, 300, m, ids, times, rand, sk_l, sk_h,
                                               1, 2)

    shard_ms = _median_ms(shard, repeats)
    # the shards of a sample against the restatement, before any number is printed
    s = {k: v[:64].cpu().numpy() for k, v in keep["s"].items()}
    hm, hi_, hr = m[:64].cpu().numpy(), ids[:64].cpu().numpy(), rand[:64].cpu().numpy()
    for i, (pub, lsh, hsh) in enumerate(_sample_shards(cfg, hm, hi_, hr)):
        if s["public_shares"][i].tobytes() != pub or s["leader_input_shares"][i].tobytes() != lsh \
                or s["helper_shares"][i].tobytes() != hsh or s["status"][i]:
            raise SystemExit(f"{name}: report {i} differs from the restatement")
    one_ms = _median_ms(one_call, repeats)
    if int(keep["r"]["status"].any()):
        raise SystemExit(f"{name}: the one call rejected a report")
    # the leader-share seal alone, rows of the same shape (at most the one call's sub-batch)
    ns = min(n, 65536)
    sh = keep["s"]
    enc = torch.empty((ns, ls.nenc), dtype=torch.uint8, device=dev)
    ct = torch.empty((ns, G.sealed_stride(sz.leader_input_share_len)), dtype=torch.uint8, device=dev)
    cl = torch.empty(ns, dtype=torch.int32, device=dev)
    st = torch.empty(ns, dtype=torch.uint8, device=dev)
    lrows = sh["leader_input_shares"][:ns].contiguous()
    prow = sh["public_shares"][:ns].contiguous()

    def leader_seal():
        ls.seal_input_shares_device(task, sk_l[:ns], ids[:ns], times[:ns], prow, lrows, enc, ct,
                                    cl, st)

    seal_ms = _median_ms(leader_seal, repeats)
    keep.clear()
    del sh, lrows, prow, enc, ct
    torch.cuda.empty_cache()

    def gen():
        eng.generate_reports_device(n, seed=3)

    gen_ms = _median_ms(gen, repeats)
    cpu = None
    if not mp:  # CPU: orc_gen_reports on 16 threads
        o = Oracle(**cfg)
        o.gen_reports(bytes(range(16)), 256, seed=1, n_threads=16)
        t0 = time.perf_counter()
        o.gen_reports(bytes(range(16)), cpu_n, seed=1, n_threads=16)
        cpu = cpu_n / (time.perf_counter() - t0)
    seal_share = (seal_ms[0] / ns) / (one_ms[0] / n)
    return dict(name=name, n=n, shard_ms=shard_ms[0], shard_ms_min=shard_ms[1],
                shard_ms_max=shard_ms[2], shard_per_s=n / shard_ms[0] * 1e3,
                one_call_ms=one_ms[0], one_call_ms_min=one_ms[1], one_call_ms_max=one_ms[2],
                one_call_per_s=n / one_ms[0] * 1e3, leader_seal_n=ns, leader_seal_ms=seal_ms[0],
                leader_seal_share=seal_share, generate_ms=gen_ms[0],
                generate_per_s=n / gen_ms[0] * 1e3, cpu_gen_per_s_16t=cpu, cpu_n=cpu_n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-n", type=int, default=20000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="measure this case alone (its name)")
    ap.add_argument("--scale", type=float, default=1.0, help="scale the batch sizes (trial runs)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shard_rate.py measures on the GPU; none is available")
    rows = []
    for name, cfg, n in CASES:
        if a.only and name != a.only:
            continue
        r = measure(name, cfg, max(64, int(n * a.scale)), a.repeats, a.cpu_n)
        rows.append(r)
        print(f"{name} n={r['n']}: k_shard {r['shard_per_s'] / 1e6:.3f} M/s ({r['shard_ms']:.2f} ms, "
              f"{r['shard_ms_min']:.2f}-{r['shard_ms_max']:.2f}); one call (X25519) "
              f"{r['one_call_per_s'] / 1e6:.3f} M/s ({r['one_call_ms']:.2f} ms), leader seal "
              f"{100 * r['leader_seal_share']:.0f}% of it; generator {r['generate_per_s'] / 1e6:.3f} "
              f"M/s ({r['generate_ms']:.2f} ms)" +
              ("" if r["cpu_gen_per_s_16t"] is None
               else f"; CPU restatement, 16 threads: {r['cpu_gen_per_s_16t'] / 1e3:.1f} K/s"),
              flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

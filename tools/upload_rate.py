"""Rates of the leader's upload call on the device (the section on the leader upload).
A build-time measurement, not a test and not bench.py:

  python tools/upload_rate.py [--n 262144] [--repeats 5] [--pairs 3] [--cpu-n 4096] [--json PATH]

For each instance (Histogram(256,16), Histogram(100,10), Histogram(10,3), Sum(32), Sum(8)) the
reports come from prio3_client_prepare_reports_device (X25519 / HKDF-SHA256 / AES-128-GCM), and
prio3_device_leader_upload is timed on them with engine option upload_aead = 1 (the one-lane AEAD
body of k_hpke_open) and 2 (k_aead_open_wide), interleaved A B A B ... on the same buffers:
HIP events around every call after a warm-up call, the median, minimum and maximum of each side.
Then, per side, one call with option timing = 1 gives the per-kernel times (decode, checks, gather,
KEM / key schedule, AEAD, share check), and janus_hpke_open_device alone on the extracted payloads
(aligned rows, explicit AAD) is the cross-check of the baseline.  The CPU column is the host
pipeline on 16 threads: janus_dap_report_decode_host, OpenSSL's open_ (oracle.hpke) and the
plaintext decode with the canonical check in Python.  Every call's statuses must be zero, and both
sides' leader shares are compared before any number is printed.  Needs the GPU: no fallback.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = (("hist_256_c16", dict(kind="histogram", length=256, chunk_length=16)),
         ("hist_100_c10", dict(kind="histogram", length=100, chunk_length=10)),
         ("hist_10_c3", dict(kind="histogram", length=10, chunk_length=3)),
         ("sum32", dict(kind="sum", bits=32)),
         ("sum8", dict(kind="sum", bits=8)))
INFO_LEADER = b"dap-09 input share" + bytes([1, 2])
INFO_HELPER = b"dap-09 input share" + bytes([1, 3])
T0 = 1_700_000_000
P128 = (0xffffffffffffffe4 << 64) | 1


def _times_ms(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(repeats)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def measure(name, cfg, n, repeats, pairs, cpu_n):
    import torch
    from janus_amd import dap
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle import hpke as H
    dev = torch.device("cuda", 0)
    vdaf = J.Prio3Histogram(cfg["length"], cfg["chunk_length"]) if cfg["kind"] == "histogram" \
        else J.Prio3Sum(cfg["bits"])
    eng = J.HelperEngine(vdaf, bytes(range(16)), device=0)
    sz = eng.sz
    g = torch.Generator(device=dev).manual_seed(n)
    hi = cfg["length"] if cfg["kind"] == "histogram" else 1 << cfg["bits"]
    m = torch.randint(0, hi, (n, 1), generator=g, device=dev, dtype=torch.int64)
    u8 = dict(generator=g, device=dev, dtype=torch.uint8)
    ids = torch.randint(0, 256, (n, 16), **u8)
    rand = torch.randint(0, 256, (n, eng.rand_len), **u8)
    sk_l = torch.randint(0, 256, (n, 32), **u8)
    sk_h = torch.randint(0, 256, (n, 32), **u8)
    times = T0 + torch.randint(0, 3600, (n,), generator=g, device=dev, dtype=torch.int64)
    rng = np.random.default_rng(n)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    sk = H.kem_private(rng)
    pk = H.kem_public(sk)
    ls = G.HpkeSealer(pk, INFO_LEADER, device=0)
    hs = G.HpkeSealer(H.kem_public(H.kem_private(rng)), INFO_HELPER, device=0)
    need = J.load_library().prio3_client_report_stride(C.byref(vdaf.params()), ls.handle,
                                                       hs.handle, 0)
    rep = eng.prepare_reports_device(ls, hs, task, 300, m, ids, times, rand, sk_l, sk_h, 42, 13,
                                     report_stride=-(-need // 16) * 16)
    torch.cuda.synchronize()
    if int(rep["status"].any()):
        raise SystemExit(f"{name}: the client rejected a report")
    del m, rand, sk_l, sk_h
    opener = G.HpkeOpener(sk, pk, INFO_LEADER, device=0)
    kw = dict(task_id=task, now=T0 + 4000, report_deadline=T0 + 4060, task_opener=opener,
              task_config_id=42, helper_ct_stride=G.sealed_stride(sz.helper_share_len))
    keep = {}

    def call():
        keep["u"] = eng.leader_upload_device(rep["reports"], rep["report_len"], **kw)

    side = {1: [], 2: []}
    shares = {}
    for _ in range(pairs):  # A B A B ...
        for aead in (1, 2):
            eng.set_option("upload_aead", aead)
            side[aead] += _times_ms(call, repeats)
            if int(keep["u"]["status"].any()):
                raise SystemExit(f"{name}: upload_aead {aead} rejected a report")
            shares.setdefault(aead, keep["u"]["leader_input_shares"][:4096].clone())
    if not torch.equal(shares[1], shares[2]) or not torch.equal(keep["u"]["report_ids"], ids):
        raise SystemExit(f"{name}: the two AEAD kernels disagree")
    stages = {}
    for aead in (1, 2):  # per-kernel times of one call each
        eng.set_option("upload_aead", aead)
        eng.set_option("timing", 1)
        eng.timing_reset()
        call()
        torch.cuda.synchronize()
        stages[aead] = {k: round(v[0], 3) for k, v in eng.timing().items()}
        eng.set_option("timing", 0)
    eng.set_option("upload_aead", 0)
    call()
    auto_ms = statistics.median(_times_ms(call, repeats))
    # cross-check: the parent's generic open alone on the extracted payloads
    psl = sz.public_share_len
    po, pl = 35 + psl + 32, 6 + sz.leader_input_share_len + 16
    ns = min(n, 65536)
    cs = -(-pl // 16) * 16
    ct = torch.zeros((ns, cs), dtype=torch.uint8, device=dev)
    ct[:, :pl] = rep["reports"][:ns, po:po + pl]
    al = 60 + psl
    aad = torch.zeros((ns, -(-al // 16) * 16), dtype=torch.uint8, device=dev)
    aad[:, :32] = torch.frombuffer(bytearray(task), dtype=torch.uint8).to(dev)
    aad[:, 32:al] = rep["reports"][:ns, :28 + psl]
    enc = rep["reports"][:ns, 31 + psl:63 + psl].contiguous()
    cl = torch.full((ns,), pl, dtype=torch.int32, device=dev)
    aln = torch.full((ns,), al, dtype=torch.int32, device=dev)
    pt = torch.empty((ns, cs), dtype=torch.uint8, device=dev)
    st = torch.empty(ns, dtype=torch.uint8, device=dev)
    L = J.load_library()
    L.janus_hpke_open_device.argtypes = [C.c_void_p] + [C.c_uint32] + [C.c_void_p] * 3 + \
        [C.c_uint32] + [C.c_void_p] * 2 + [C.c_uint32] + [C.c_void_p] * 3
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def generic_open():
        rc = L.janus_hpke_open_device(opener.handle, ns, p(enc), p(ct), p(cl), cs, p(aad), p(aln),
                                      aad.shape[1], p(pt), p(st), stream)
        if rc:
            raise SystemExit(f"janus_hpke_open_device failed (rc={rc})")

    open_ms = statistics.median(_times_ms(generic_open, repeats))
    if int(st.any()) or not torch.equal(pt[:64, 6:pl - 16], shares[1][:64]):
        raise SystemExit(f"{name}: the generic open disagrees")
    # CPU: C decode, OpenSSL open and the Python plaintext decode on 16 threads
    rows = rep["reports"][:cpu_n].cpu().numpy()
    ln = rep["report_len"][:cpu_n].cpu().numpy().view(np.uint32)
    Lsh, es = sz.leader_input_share_len, sz.field_bytes
    blind = sz.prep_msg_len if sz.joint_rand_len else 0

    def cpu_chunk(lo):
        r, k = rows[lo:lo + 256], ln[lo:lo + 256]
        d = dap.report_decode_host(r, k, 32, 64)
        ok = 0
        for i in range(r.shape[0]):
            f = d["fields"][i]
            b = r[i].tobytes()
            a = H.input_share_aad(task, b[:16], int(d["times"][i]), b[f[0]:f[0] + f[1]])
            x = H.open_(sk, pk, b[f[2]:f[2] + f[3]], INFO_LEADER, a, b[f[4]:f[4] + f[5]])
            el = int.from_bytes(x[:2], "big")
            share = x[6 + el:]
            v = np.frombuffer(share[:Lsh - blind], "<u8").reshape(-1, es // 8)
            hi_ = v[:, -1]
            ok += len(share) == Lsh and not bool((hi_ > 0xffffffffffffffe4).any())
        return ok

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(cpu_chunk, range(0, min(cpu_n, 512), 256)))
        t0 = time.perf_counter()
        done = sum(ex.map(cpu_chunk, range(0, cpu_n, 256)))
        cpu = cpu_n / (time.perf_counter() - t0)
    if done != cpu_n:
        raise SystemExit(f"{name}: the CPU pipeline rejected a report")
    out = dict(name=name, n=n, payload=pl, auto_ms=auto_ms, auto_per_s=n / auto_ms * 1e3,
               generic_open_n=ns, generic_open_ms=open_ms, generic_open_per_s=ns / open_ms * 1e3,
               cpu_per_s_16t=cpu, cpu_n=cpu_n, stages_ms=stages)
    for aead, key in ((1, "one_lane"), (2, "wide")):
        ms = side[aead]
        out[key + "_ms"] = statistics.median(ms)
        out[key + "_ms_min"], out[key + "_ms_max"] = min(ms), max(ms)
        out[key + "_per_s"] = n / statistics.median(ms) * 1e3
        out[key + "_all_ms"] = [round(x, 3) for x in ms]
    # the wide kernel wins a pair when its slowest call beats the one-lane side's fastest
    out["wide_wins_every_pair"] = all(
        max(side[2][k * repeats:(k + 1) * repeats]) < min(side[1][k * repeats:(k + 1) * repeats])
        for k in range(pairs))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=4096)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("upload_rate.py measures on the GPU; none is available")
    rows = []
    for name, cfg in CASES:
        if name not in a.cases.split(","):
            continue
        r = measure(name, cfg, a.n, a.repeats, a.pairs, min(a.cpu_n, a.n))
        rows.append(r)
        print(f"{name} n={r['n']} payload {r['payload']} B: one-lane {r['one_lane_per_s'] / 1e6:.3f} "
              f"M/s ({r['one_lane_ms']:.2f} ms, {r['one_lane_ms_min']:.2f}-{r['one_lane_ms_max']:.2f});"
              f" wide {r['wide_per_s'] / 1e6:.3f} M/s ({r['wide_ms']:.2f} ms, "
              f"{r['wide_ms_min']:.2f}-{r['wide_ms_max']:.2f}); wide wins every pair: "
              f"{r['wide_wins_every_pair']}; auto {r['auto_per_s'] / 1e6:.3f} M/s; generic open "
              f"alone {r['generic_open_per_s'] / 1e6:.3f} M/s; CPU, 16 threads: "
              f"{r['cpu_per_s_16t'] / 1e3:.1f} K/s", flush=True)
        print(f"  stages (ms): one-lane {r['stages_ms'][1]}; wide {r['stages_ms'][2]}", flush=True)
        torch.cuda.empty_cache()
        J = sys.modules["janus_amd.prio3"]
        J.trim_device_pool(0)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

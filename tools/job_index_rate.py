"""Time of the device job index against the same bookkeeping on the host.  A
build-time measurement, not a test and not bench.py:

  python tools/job_index_rate.py [--n 1048576] [--buckets 1 8 1024] [--repeats 15] [--json PATH]

Per bucket count, at n reports with distinct random IDs, time precision 300 and one closed bucket:
  * whole call: prio3_device_job_index, HIP events around repeated calls on one stream after
    warm-up calls of the same shape; the figure is the median call;
  * per kernel: the engine's "timing" option (HIP events around every launch), one call at a time,
    the median over the calls -- taken in a pass of its own, because the events slow the call;
  * host: what a caller pays today on one thread -- numpy.unique(..., return_inverse=True) over
    the starts and numpy.unique over the IDs viewed as 16-byte records (host clock, best of 3);
  * once: the k_prep_h launch of a Histogram(256,16) prepare of the same n (the headline step's
    main kernel), the figure the call's cost is a share of.
The call's outputs are compared with the host's before any number is printed.  Needs the GPU:
there is no fallback.
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

PRECISION = 300
KERNELS = ("k_jix_init", "k_jix_closed_put", "k_jix_insert", "k_jix_rank", "k_jix_assign")


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


def host_ms(ids, times):
    """One thread: the two numpy.unique calls a host caller would make (best of 3, ms)."""
    rec = np.ascontiguousarray(ids).view(np.dtype((np.void, 16))).reshape(-1)
    best = [1e30, 1e30]
    out = None
    for _ in range(3):
        t0 = time.perf_counter()
        start = times - times % np.uint64(PRECISION)
        uniq, inverse = np.unique(start, return_inverse=True)
        t1 = time.perf_counter()
        n_ids = len(np.unique(rec))
        t2 = time.perf_counter()
        best = [min(best[0], (t1 - t0) * 1e3), min(best[1], (t2 - t1) * 1e3)]
        out = (uniq, inverse, n_ids)
    return best, out


def measure(eng, n, buckets, repeats):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(buckets)
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # distinct
    times = (1_700_000_100 + rng.integers(0, buckets, n) * PRECISION +
             rng.integers(0, PRECISION, n)).astype(np.uint64)
    closed = [(int(times.min() - times.min() % np.uint64(PRECISION)), PRECISION)]
    max_segments = max(buckets, 8)
    d_ids = torch.from_numpy(ids).to(dev)
    d_times = torch.from_numpy(times.view(np.int64)).to(dev)
    seg = torch.empty(n, dtype=torch.int32, device=dev)
    acc, rej, dup = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
    starts = torch.empty(max_segments, dtype=torch.int64, device=dev)
    info = torch.empty(6, dtype=torch.int32, device=dev)

    def call():
        eng.job_index_device(d_ids, d_times, PRECISION, max_segments, seg, acc, info,
                             closed_intervals=closed, segment_starts=starts, reject=rej,
                             duplicate=dup)

    whole = _median_ms(call, repeats)
    (host_starts, host_ids), (uniq, inverse, n_ids) = host_ms(ids, times)
    got_info = info.cpu().numpy().view(np.uint32).tolist()
    ok = (got_info[0] == len(uniq) and got_info[1] == 0 and got_info[2] == n - n_ids and
          np.array_equal(seg.cpu().numpy().view(np.uint32), inverse.astype(np.uint32)) and
          np.array_equal(starts.cpu().numpy().view(np.uint64)[:len(uniq)], uniq) and
          np.array_equal(acc.cpu().numpy(), (inverse != 0).astype(np.uint8)) and
          not dup.any().item())
    if not ok:
        raise SystemExit(f"n {n}, {buckets} buckets: the device job index differs from the host's")
    eng.set_option("timing", 1)
    per = {k: [] for k in KERNELS}
    for _ in range(repeats):
        eng.timing_reset()
        call()
        torch.cuda.synchronize()
        t = eng.timing()
        for k in KERNELS:
            per[k].append(t.get(k, (0.0, 0))[0])
    eng.set_option("timing", 0)
    eng.timing_reset()
    return dict(n=n, buckets=buckets, call_ms=whole[0], call_ms_min=whole[1], call_ms_max=whole[2],
                kernels_ms={k: statistics.median(v) for k, v in per.items()},
                host_starts_ms=host_starts, host_ids_ms=host_ids)


def prep_h_ms(n, repeats):
    """Median k_prep_h launch of a Histogram(256,16) device prepare + aggregate of n reports."""
    import torch
    from janus_amd import prio3 as J
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), bytes(range(16)), device=0)
    d = eng.generate_reports_device(n, seed=3)
    dev = d["nonces"].device
    msgs = torch.empty((n, eng.sz.prep_msg_len), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)

    def call():
        eng.prepare_aggregate_device(d["nonces"], d["public_shares"], d["helper_shares"],
                                     d["leader_prep_shares"], None, 1, msgs, status)

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    eng.set_option("timing", 1)
    ms = []
    for _ in range(repeats):
        eng.timing_reset()
        call()
        torch.cuda.synchronize()
        t = eng.timing()
        ms.append(sum(v[0] for k, v in t.items() if k.startswith("k_prep_h")))
    eng.close()
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--buckets", type=int, nargs="+", default=[1, 8, 1024])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-prep", action="store_true", help="skip the k_prep_h reference launch")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("job_index_rate.py measures on the GPU; none is available")
    from janus_amd import prio3 as J
    eng = J.HelperEngine(J.Prio3Count(), bytes(16), device=0)
    rows = []
    for b in a.buckets:
        r = measure(eng, a.n, b, a.repeats)
        rows.append(r)
        ks = ", ".join(f"{k[6:]} {v * 1e3:.1f} us" for k, v in r["kernels_ms"].items())
        print(f"n={r['n']} buckets={b}: call {r['call_ms']:.3f} ms ({r['call_ms_min']:.3f}-"
              f"{r['call_ms_max']:.3f}); kernels: {ks}; host numpy.unique starts "
              f"{r['host_starts_ms']:.1f} ms, IDs {r['host_ids_ms']:.1f} ms "
              f"({(r['host_starts_ms'] + r['host_ids_ms']) / r['call_ms']:.0f}x the call)",
              flush=True)
    eng.close()
    if not a.no_prep:
        p = prep_h_ms(a.n, min(a.repeats, 7))
        print(f"n={a.n}: k_prep_h (Histogram(256,16)) {p:.3f} ms", flush=True)
        for r in rows:
            r["prep_h_ms"] = p
            print(f"  {r['buckets']} buckets: the call is {100 * r['call_ms'] / p:.1f} % of it",
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

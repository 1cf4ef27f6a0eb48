"""Ticketed job submission against the blocking calls (tool-measured, not bench.py).

  python tools/ticket_rate.py [--threads 16,128] [--k 1,2,4,8] [--rounds 5] [--tag run1]
                              [--out profiles/tickets]

Workload: K = 4 tasks of Prio3Histogram(256,16), 500-report jobs, host buffers, two job shapes:
  helper  prio3_helper_prepare_aggregate_batch (the jobs line of bench.py --role jobs), one segment
  job     prio3_helper_aggregate_job from sealed input shares under one X25519 / AES-128-GCM
          keypair: three batch intervals per job, the middle one closed, max_segments = 4
Per shape, thread count and K, after a warm-up, --rounds interleaved pairs in one process:
  A  every worker thread makes blocking calls (janus_jobs_run combined / janus_jobs_run_job form 1)
  B  every worker thread keeps K tickets outstanding through the _submit form: it submits until it
     holds K, then waits the oldest and submits the next (janus_jobs_run_tickets /
     janus_jobs_run_job_tickets)
Checks: every output of every job of B equals A's in every round, and a sample of jobs of each
task equals the CPU restatement (the C restatement of prio; for the job shape also
tests/job_index_ref.py, the OpenSSL HPKE oracle and hashlib).
Reported per (shape, threads, K): both arms' rates per round, whether B beat A in every pair, B's
median gain against A's own min-max spread, the group launches and the mean reports per launch,
and the nominal reports in flight (threads x K x 500) against the light/heavy threshold (32768).
Writes ticket_rate_<tag>.json and ticket_rate_<tag>.md under --out.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREC = 1200
TB = 1_699_999_200  # a multiple of PREC
S = 4               # max_segments of the job shape
JS = 500
K = 4
POOL = 1 << 15
HEAVY_DEFAULT = 32768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", default="16,128")
    ap.add_argument("--k", default="1,2,4,8", help="tickets outstanding per thread")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="helper,job")
    ap.add_argument("--sample", type=int, default=2, help="jobs per task checked against the CPU")
    ap.add_argument("--tag", default="run1")
    ap.add_argument("--ab-heavy", type=int, default=0,
                    help="A/B of the light/heavy threshold instead: both arms keep K tickets, arm A "
                         "at the default threshold, arm B at this many reports")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tickets"))
    args = ap.parse_args()
    import torch
    import bench as B
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle import hpke as H
    from oracle.oracle import Oracle
    from tests import job_index_ref as R
    torch.cuda.set_device(0)
    cores = B.cpu_threads()
    rng = np.random.default_rng(0x5449434B)
    vks = [bytes([0xA1 + t]) * 16 for t in range(K)]
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(K)]
    skR = H.kem_private(rng)
    pkR = H.kem_public(skR)
    engines, _ = B._job_engines(J.Prio3Histogram(256, 16), vks, None)
    sz = engines[0].sz
    shapes = args.shapes.split(",")
    cols = {k: [] for k in ("nonces", "public_shares", "helper_shares", "leader_prep_shares",
                            "times", "enc", "ct", "ct_len")}
    stride = 0
    for t, e in enumerate(engines):
        p = e.generate_reports_device(POOL, seed=0x5449434B00000001 + t)
        torch.cuda.synchronize()
        h = {k: p[k].cpu().numpy() for k in ("nonces", "public_shares", "helper_shares",
                                              "leader_prep_shares")}
        del p
        times = (TB + rng.integers(0, 3 * PREC, POOL)).astype(np.uint64)
        h["times"] = times
        if "job" in shapes:
            enc, ct, cl, stride = H.seal_input_shares(pkR, tasks[t], h["nonces"], times,
                                                      h["public_shares"], h["helper_shares"],
                                                      seed=0x71C + t, n_threads=cores)
            h.update(enc=enc, ct=ct, ct_len=cl)
        for k, v in h.items():
            cols[k].append(v)
    host = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in cols.items() if v}
    task_arr = np.frombuffer(b"".join(tasks), np.uint8).copy()
    closed = np.array([[TB + PREC, PREC]], np.uint64)
    op = G.HpkeOpener(skR, pkR, device=0)
    J.load_library()
    lib = C.CDLL(os.path.join(ROOT, "janus_amd", "libjanus_jobs.so"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    helper_args = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, C.c_int, u32, vp, vp, vp, vp, vp,
                   vp, vp, C.c_int]
    job_args = ([C.POINTER(vp), C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, u32, vp, vp, vp,
                 vp, u32, vp, vp, u32, vp, u64, vp, u32, u32] + [vp] * 10 + [C.c_int])
    for fn, a in (("janus_jobs_run", helper_args), ("janus_jobs_run_tickets", helper_args),
                  ("janus_jobs_run_job", job_args), ("janus_jobs_run_job_tickets", job_args)):
        getattr(lib, fn).restype = C.c_double
        getattr(lib, fn).argtypes = a
    eng_arr = (vp * K)(*[e.handle.value for e in engines])
    P = lambda a: a.ctypes.data_as(vp)
    o = Oracle("histogram", length=256, chunk_length=16)

    def buffers(shape, n_jobs):
        if shape == "helper":
            b = dict(status=np.zeros(n_jobs * JS, np.uint8), counts=np.zeros(n_jobs, np.uint64),
                     agg=np.zeros((n_jobs, sz.agg_share_len), np.uint8))
        else:
            b = dict(seg=np.zeros(n_jobs * JS, np.uint32), starts=np.zeros((n_jobs, S), np.uint64),
                     reject=np.zeros(n_jobs * JS, np.uint8), dup=np.zeros(n_jobs * JS, np.uint8),
                     info=np.zeros((n_jobs, 6), np.uint32), status=np.zeros(n_jobs * JS, np.uint8),
                     counts=np.zeros((n_jobs, S), np.uint64),
                     agg=np.zeros((n_jobs, S, sz.agg_share_len), np.uint8),
                     ck=np.zeros((n_jobs, S, 32), np.uint8), iv=np.zeros((n_jobs, S, 2), np.uint64))
        B._warm(*b.values())
        return b

    def run(shape, T, jobs, b, k, heavy=0):
        """k == 0: the blocking arm; k >= 1: k tickets outstanding per thread.  heavy: the
        executors' light/heavy threshold for this run (0: the default)."""
        engines[0].executor_control("heavy", heavy)
        for v in b.values():
            v.fill(0)
        b["status"].fill(0xFF)
        if shape == "helper":
            fn = lib.janus_jobs_run_tickets if k else lib.janus_jobs_run
            return fn(eng_arr, K, C.cast(C.pointer(sz), vp), T, jobs, JS, POOL, P(host["nonces"]),
                      P(host["public_shares"]), P(host["helper_shares"]),
                      P(host["leader_prep_shares"]), P(b["status"]), P(b["counts"]), P(b["agg"]),
                      k if k else 1)
        fn = lib.janus_jobs_run_job_tickets if k else lib.janus_jobs_run_job
        return fn(eng_arr, K, C.cast(C.pointer(sz), vp), op.handle, P(task_arr), T, jobs, JS, POOL,
                  P(host["nonces"]), P(host["public_shares"]), P(host["times"]), P(host["enc"]), 32,
                  P(host["ct"]), P(host["ct_len"]), stride, P(host["leader_prep_shares"]), PREC,
                  P(closed), 1, S, P(b["seg"]), P(b["starts"]), P(b["reject"]), P(b["dup"]),
                  P(b["info"]), P(b["status"]), P(b["counts"]), P(b["agg"]), P(b["ck"]), P(b["iv"]),
                  k if k else 1)

    def check_sample(shape, n_jobs, b):
        """A sample of each task's jobs against the restatement."""
        ok, checked = True, 0
        for t in range(K):
            jl, idx = B._job_windows(t, n_jobs, K, JS, POOL)
            for q in range(min(args.sample, len(jl))):
                j, rows = jl[q], idx[q * JS:(q + 1) * JS]
                sl = slice(j * JS, (j + 1) * JS)
                if shape == "helper":
                    _, st, agg, cnt = o.helper_batch(
                        vks[t], host["nonces"][rows], host["public_shares"][rows],
                        host["helper_shares"][rows], host["leader_prep_shares"][rows],
                        n_threads=cores)
                    ok &= bool(np.array_equal(b["status"][sl], st) and
                               np.array_equal(b["agg"][j], agg[0]) and
                               int(b["counts"][j]) == int(cnt[0]))
                    checked += 1
                    continue
                ref = R.job_index(host["nonces"][rows], host["times"][rows], PREC, S, closed)
                sh, hs = H.open_input_shares(skR, pkR, tasks[t], host["enc"][rows],
                                             host["ct"][rows], host["ct_len"][rows],
                                             host["nonces"][rows], host["times"][rows],
                                             host["public_shares"][rows], sz.helper_share_len,
                                             n_threads=cores)
                acc = ref["accept_mask"] & (hs == 0).astype(np.uint8)
                seg = ref["segment_ids"]
                _, st, agg, cnt = o.helper_batch(
                    vks[t], host["nonces"][rows], host["public_shares"][rows], sh,
                    host["leader_prep_shares"][rows], accept_mask=acc, n_threads=cores,
                    segment_ids=np.where(seg == 0xFFFFFFFF, 0, seg).astype(np.uint32),
                    n_segments=S)
                st = np.where(hs != 0, 0x80 | hs, st).astype(np.uint8)
                ck = np.zeros((S, 32), np.uint8)
                iv = np.zeros((S, 2), np.uint64)
                for s in range(S):
                    r = np.flatnonzero(seg == s)
                    if len(r):
                        lo = int(host["times"][rows][r].min())
                        iv[s] = (lo, int(host["times"][rows][r].max()) + 1 - lo)
                    for i in r[(st[r] == 0) & (acc[r] != 0)]:
                        ck[s] ^= np.frombuffer(
                            hashlib.sha256(host["nonces"][rows][i].tobytes()).digest(), np.uint8)
                info = [ref[f] for f in ("n_segments", "overflow", "n_duplicates",
                                         "first_duplicate", "n_closed", "n_time_errors")]
                ok &= bool(np.array_equal(b["seg"][sl], seg) and
                           np.array_equal(b["reject"][sl], ref["reject"]) and
                           np.array_equal(b["dup"][sl], ref["duplicate"]) and
                           np.array_equal(b["starts"][j], ref["segment_starts"]) and
                           list(b["info"][j]) == info and np.array_equal(b["status"][sl], st) and
                           np.array_equal(b["agg"][j], agg) and
                           np.array_equal(b["counts"][j], cnt.astype(np.uint64)) and
                           np.array_equal(b["ck"][j], ck) and np.array_equal(b["iv"][j], iv))
                checked += 1
        return ok, checked

    def groups():
        return engines[0].executor_stats(J.EXEC_PREPARE)["groups"]

    result = dict(tool="tools/ticket_rate.py", tag=args.tag,
                  arms=(dict(A=f"K tickets, default threshold ({HEAVY_DEFAULT})",
                             B=f"K tickets, threshold {args.ab_heavy}") if args.ab_heavy else
                        dict(A="blocking calls", B="K tickets outstanding per thread")),
                  workload=dict(vdaf="Prio3Histogram(256,16)", job_size=JS, tasks=K, pool=POOL,
                                job_shape=dict(batch_intervals_per_job=3, closed_intervals=1,
                                               max_segments=S,
                                               hpke="X25519-HKDF-SHA256 / AES-128-GCM"),
                                buffers="host", rounds=args.rounds,
                                heavy_threshold_reports=HEAVY_DEFAULT),
                  device=torch.cuda.get_device_name(0), lines=[])
    for shape in shapes:
        for T in [int(x) for x in args.threads.split(",")]:
            n_jobs = 1024 if T <= 16 else (1 << 21) // JS
            bA, bB = buffers(shape, n_jobs), buffers(shape, n_jobs)
            for k in [int(x) for x in args.k.split(",")]:
                # (arm's K, its buffers, its name, its threshold)
                arms = (((k, bA, "A", 0), (k, bB, "B", args.ab_heavy)) if args.ab_heavy else
                        ((0, bA, "A", 0), (k, bB, "B", 0)))
                for arm, b, _, hv in arms:  # warm-up: staging, streams, worker threads
                    if run(shape, T, max(K, min(n_jobs, 8 * T)), b, arm, hv) < 0:
                        raise RuntimeError(f"{shape} T={T} K={arm}: a C-ABI call failed")
                rounds, equal = [], True
                for _ in range(args.rounds):
                    row = {}
                    for arm, b, name, hv in arms:
                        g0 = groups()
                        dt = run(shape, T, n_jobs, b, arm, hv)
                        if dt < 0:
                            raise RuntimeError(f"{shape} T={T} K={arm}: a C-ABI call failed")
                        g = groups() - g0
                        row[name] = dict(ms=dt * 1e3, reports_per_s=n_jobs * JS / dt,
                                         group_launches=g,
                                         reports_per_launch=n_jobs * JS / max(g, 1))
                    equal &= all(np.array_equal(bA[c], bB[c]) for c in bA)
                    row["B_over_A"] = row["B"]["reports_per_s"] / row["A"]["reports_per_s"]
                    rounds.append(row)
                a = [r["A"]["reports_per_s"] for r in rounds]
                bb = [r["B"]["reports_per_s"] for r in rounds]
                okA, nA = check_sample(shape, n_jobs, bA)
                okB, nB = check_sample(shape, n_jobs, bB)
                in_flight = T * k * JS
                result["lines"].append(dict(
                    shape=shape, threads=T, k=k, jobs=n_jobs, reports=n_jobs * JS, rounds=rounds,
                    A_median=statistics.median(a), B_median=statistics.median(bb),
                    A_spread=max(a) - min(a), B_minus_A_median=statistics.median(bb) -
                    statistics.median(a),
                    B_beats_A_in_every_pair=all(r["B_over_A"] > 1.0 for r in rounds),
                    B_gain_exceeds_A_spread=statistics.median(bb) - statistics.median(a) >
                    max(a) - min(a),
                    B_within_A_spread=min(a) <= statistics.median(bb) <= max(a),
                    nominal_reports_in_flight=in_flight,
                    launcher="heavy" if in_flight >= HEAVY_DEFAULT else "light",
                    ab_heavy=args.ab_heavy,
                    checks=dict(B_equals_A_every_job_every_round=bool(equal),
                                sample_matches_cpu=dict(A=okA, B=okB, jobs_checked=nA + nB))))
            del bA, bB
    engines[0].executor_control("heavy", 0)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"ticket_rate_{args.tag}.json"), "w") as f:
        json.dump(result, f, indent=1)
    names = ((f"A: K tickets, threshold {HEAVY_DEFAULT}", f"B: K tickets, threshold {args.ab_heavy}")
             if args.ab_heavy else ("A blocking", "B tickets"))
    md = ["| shape | threads | K | %s (min / median / max) | %s (min / median / max) "
          "| B > A every pair | median gain | A spread | launcher (T x K x 500) "
          "| reports / launch A, B |" % names, "|---|---|---|---|---|---|---|---|---|---|"]
    for ln in result["lines"]:
        a = [r["A"]["reports_per_s"] / 1e6 for r in ln["rounds"]]
        b = [r["B"]["reports_per_s"] / 1e6 for r in ln["rounds"]]
        md.append("| %s | %d | %d | %.2f / %.2f / %.2f M/s | %.2f / %.2f / %.2f M/s | %s | %+.2f M/s "
                  "| %.2f M/s | %s (%d) | %.0f, %.0f |"
                  % (ln["shape"], ln["threads"], ln["k"], min(a), statistics.median(a), max(a),
                     min(b), statistics.median(b), max(b),
                     "yes" if ln["B_beats_A_in_every_pair"] else "no",
                     ln["B_minus_A_median"] / 1e6, ln["A_spread"] / 1e6, ln["launcher"],
                     ln["nominal_reports_in_flight"],
                     statistics.median(r["A"]["reports_per_launch"] for r in ln["rounds"]),
                     statistics.median(r["B"]["reports_per_launch"] for r in ln["rounds"])))
    with open(os.path.join(args.out, f"ticket_rate_{args.tag}.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print("\n".join(md))
    for ln in result["lines"]:
        print(json.dumps(dict(shape=ln["shape"], threads=ln["threads"], k=ln["k"],
                              checks=ln["checks"])))
    bad = [ln for ln in result["lines"]
           if not (ln["checks"]["B_equals_A_every_job_every_round"] and
                   ln["checks"]["sample_matches_cpu"]["A"] and
                   ln["checks"]["sample_matches_cpu"]["B"])]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

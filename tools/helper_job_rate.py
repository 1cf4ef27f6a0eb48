"""A whole helper job per call against the three calls it stands for (tool-measured, not bench.py).

  python tools/helper_job_rate.py [--threads 16,128] [--pairs 3] [--out profiles/helper_job]

Workload: the jobs line's (bench.py init_jobs_line) -- K = 4 tasks of Prio3Histogram(256,16) under
one X25519 / AES-128-GCM keypair, 500-report jobs from sealed input shares, host buffers -- with
what AggregationJobWriter needs per job: three batch intervals per job of which the middle one is
closed, max_segments = 4.  Four forms, timed in one process, alternating A, B, C, D for --pairs
rounds per thread count (native worker janus_jobs_run_job, libjanus_jobs.so):
  A  prio3_job_index + prio3_helper_aggregate_init_batch_ex + prio3_batch_metadata per job
  B  prio3_helper_aggregate_job
  C  prio3_helper_aggregate_init_batch_ex alone, one segment, no index and no metadata (the
     README's "helper's whole loop body" line): the ceiling
  D  the middle call of A alone, over the segment ids and accept bytes A's index left: B minus
     D is what the index and the metadata cost inside the launch, D against C what the job's
     three batch intervals cost the accumulate
Checks: every output of every job of B equals A's in every round, and a sample of jobs of each
task equals the restatement (tests/job_index_ref.py, the OpenSSL HPKE oracle, the C restatement
of prio, hashlib).  Then one held group of --held-jobs jobs per form B and D with the engine's
per-kernel timing events.  Writes helper_job_rate.json and helper_job_rate.md under --out.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREC = 1200
TB = 1_699_999_200  # a multiple of PREC
S = 4               # max_segments
JS = 500
K = 4
POOL = 1 << 15
FORMS = (("A", 0, "prio3_job_index + prio3_helper_aggregate_init_batch_ex + prio3_batch_metadata"),
         ("B", 1, "prio3_helper_aggregate_job"),
         ("C", 2, "prio3_helper_aggregate_init_batch_ex alone (no index, no metadata)"),
         ("D", 3, "the _ex call of A alone, over A's finished segment ids and accept bytes"))


def group_kernel_times(J, host, vk, task, op, closed, n_jobs, rounds=3):
    """Per-kernel times (the engine's `timing` events, us) of ONE group launch of n_jobs 500-report
    jobs of task 0 queued behind the executor's hold: form B, and form D's _ex call over the same
    segment ids -- what the index and the metadata add to a launch, kernel by kernel."""
    import threading
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, device=0)
    eng.set_option("timing", 1)  # an engine with timing shares no launch with the lines' engines
    cols = ("nonces", "times", "public_shares", "enc", "ct", "ct_len", "leader_prep_shares")
    jobs = [{k: host[k][j * JS:(j + 1) * JS] for k in cols} for j in range(n_jobs)]
    index = [None] * n_jobs

    def call(j, form):
        d = jobs[j]
        if form == "B":
            index[j] = eng.aggregate_job(op, task, *[d[k] for k in cols], PREC, S,
                                         closed_intervals=closed)
        else:
            acc = ((index[j]["segment_ids"] != 0xFFFFFFFF) &
                   (index[j]["reject"] == 0)).astype(np.uint8)
            eng.aggregate_init_batch(op, task, *[d[k] for k in cols], index[j]["segment_ids"],
                                     acc, S, report_deadline=(1 << 64) - 1)

    out = []
    for form in ("B", "D") * (rounds + 1):  # the first round of each form loads its kernels
        eng.timing_reset()
        s0 = eng.executor_stats(J.EXEC_PREPARE)
        eng.executor_control("hold", 1)
        th = [threading.Thread(target=call, args=(j, form), daemon=True) for j in range(n_jobs)]
        try:
            for x in th:
                x.start()
            t0 = time.monotonic()
            while (eng.executor_stats(J.EXEC_PREPARE)["jobs"] - s0["jobs"] < n_jobs and
                   time.monotonic() - t0 < 30):
                time.sleep(0.005)
            time.sleep(0.05)
        finally:
            eng.executor_control("hold", 0)
        for x in th:
            x.join(60)
        groups = eng.executor_stats(J.EXEC_PREPARE)["groups"] - s0["groups"]
        out.append(dict(form=form, jobs=n_jobs, group_launches=groups,
                        kernels_us={k: round(ms * 1e3, 1) for k, (ms, n) in eng.timing().items()
                                    if n}))
    return out[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--held-jobs", type=int, default=48,
                    help="jobs of the one held group whose kernels are timed")
    ap.add_argument("--threads", default="16,128")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--sample", type=int, default=6, help="jobs per task checked against the CPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "helper_job"))
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
    rng = np.random.default_rng(0x4A4F4253)
    vks = [bytes([0x91 + t]) * 16 for t in range(K)]
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(K)]
    skR = H.kem_private(rng)
    pkR = H.kem_public(skR)
    engines, _ = B._job_engines(J.Prio3Histogram(256, 16), vks, None)
    sz = engines[0].sz
    cols = {k: [] for k in ("nonces", "public_shares", "helper_shares", "leader_prep_shares",
                            "times", "enc", "ct", "ct_len")}
    stride = None
    for t, e in enumerate(engines):
        p = e.generate_reports_device(POOL, seed=0x4A4F425300000001 + t)
        torch.cuda.synchronize()
        h = {k: p[k].cpu().numpy() for k in ("nonces", "public_shares", "helper_shares",
                                              "leader_prep_shares")}
        del p
        times = (TB + rng.integers(0, 3 * PREC, POOL)).astype(np.uint64)
        enc, ct, cl, stride = H.seal_input_shares(pkR, tasks[t], h["nonces"], times,
                                                  h["public_shares"], h["helper_shares"],
                                                  seed=0x5EA2 + t, n_threads=cores)
        for k, v in dict(h, times=times, enc=enc, ct=ct, ct_len=cl).items():
            cols[k].append(v)
    host = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in cols.items()}
    task_arr = np.frombuffer(b"".join(tasks), np.uint8).copy()
    closed = np.array([[TB + PREC, PREC]], np.uint64)
    op = G.HpkeOpener(skR, pkR, device=0)
    J.load_library()
    lib = C.CDLL(os.path.join(ROOT, "janus_amd", "libjanus_jobs.so"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.janus_jobs_run_job.restype = C.c_double
    lib.janus_jobs_run_job.argtypes = ([C.POINTER(vp), C.c_int, vp, vp, vp, C.c_int, C.c_int,
                                        C.c_int, u32, vp, vp, vp, vp, u32, vp, vp, u32, vp, u64,
                                        vp, u32, u32] + [vp] * 10 + [C.c_int])
    eng_arr = (vp * K)(*[e.handle.value for e in engines])
    P = lambda a: a.ctypes.data_as(vp)
    o = Oracle("histogram", length=256, chunk_length=16)

    def buffers(n_jobs):
        b = dict(seg=np.zeros(n_jobs * JS, np.uint32), starts=np.zeros((n_jobs, S), np.uint64),
                 reject=np.zeros(n_jobs * JS, np.uint8), dup=np.zeros(n_jobs * JS, np.uint8),
                 info=np.zeros((n_jobs, 6), np.uint32), status=np.zeros(n_jobs * JS, np.uint8),
                 counts=np.zeros((n_jobs, S), np.uint64),
                 agg=np.zeros((n_jobs, S, sz.agg_share_len), np.uint8),
                 ck=np.zeros((n_jobs, S, 32), np.uint8), iv=np.zeros((n_jobs, S, 2), np.uint64))
        B._warm(*b.values())
        return b

    def run(T, jobs, form, b, index=None):
        for v in b.values():
            v.fill(0)
        b["status"].fill(0xFF)
        if index is not None:  # form D reads a finished index
            b = dict(b, seg=index["seg"], reject=index["reject"])
        return lib.janus_jobs_run_job(
            eng_arr, K, C.cast(C.pointer(sz), vp), op.handle, P(task_arr), T, jobs, JS, POOL,
            P(host["nonces"]), P(host["public_shares"]), P(host["times"]), P(host["enc"]), 32,
            P(host["ct"]), P(host["ct_len"]), stride, P(host["leader_prep_shares"]), PREC,
            P(closed), 1, S, P(b["seg"]), P(b["starts"]), P(b["reject"]), P(b["dup"]),
            P(b["info"]), P(b["status"]), P(b["counts"]), P(b["agg"]), P(b["ck"]), P(b["iv"]),
            form)

    def check_sample(n_jobs, b):
        """A sample of each task's jobs against the restatement."""
        ok, checked = True, 0
        for t in range(K):
            jl, idx = B._job_windows(t, n_jobs, K, JS, POOL)
            for q in range(min(args.sample, len(jl))):
                j, rows = jl[q], idx[q * JS:(q + 1) * JS]
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
                sl = slice(j * JS, (j + 1) * JS)
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

    result = dict(tool="tools/helper_job_rate.py",
                  workload=dict(vdaf="Prio3Histogram(256,16)", job_size=JS, tasks=K, pool=POOL,
                                batch_intervals_per_job=3, closed_intervals=1, max_segments=S,
                                hpke="X25519-HKDF-SHA256 / AES-128-GCM", buffers="host"),
                  forms={f: call for f, _, call in FORMS}, device=torch.cuda.get_device_name(0),
                  lines=[])
    for T in [int(x) for x in args.threads.split(",")]:
        n_jobs = 1024 if T <= 16 else (1 << 21) // JS
        bufs = {f: buffers(n_jobs) for f, _, _ in FORMS}
        for f, form, _ in FORMS:  # warmup: pools, pinned staging, streams, worker threads
            if run(T, max(K, min(n_jobs, 8 * T)), form, bufs[f],
                   bufs["A"] if f == "D" else None) < 0:
                raise RuntimeError(f"form {f}: a C-ABI call failed")
        rounds = []
        for r in range(args.pairs):
            row = {}
            for f, form, _ in FORMS:
                g0 = engines[0].executor_stats(J.EXEC_PREPARE)["groups"]
                dt = run(T, n_jobs, form, bufs[f], bufs["A"] if f == "D" else None)
                if dt < 0:
                    raise RuntimeError(f"form {f}: a C-ABI call failed")
                row[f] = dict(ms=dt * 1e3, reports_per_s=n_jobs * JS / dt, jobs_per_s=n_jobs / dt,
                              group_launches=engines[0].executor_stats(J.EXEC_PREPARE)["groups"]
                              - g0)
            row["B_equals_A_every_job"] = all(
                np.array_equal(bufs["A"][k], bufs["B"][k]) for k in bufs["A"])
            row["C_statuses_equal_A"] = bool(np.array_equal(bufs["A"]["status"],
                                                            bufs["C"]["status"]))
            row["D_equals_A"] = all(np.array_equal(bufs["A"][k], bufs["D"][k])
                                    for k in ("status", "agg", "counts"))
            row["B_over_A"] = row["B"]["reports_per_s"] / row["A"]["reports_per_s"]
            row["B_over_C"] = row["B"]["reports_per_s"] / row["C"]["reports_per_s"]
            row["B_over_D"] = row["B"]["reports_per_s"] / row["D"]["reports_per_s"]
            rounds.append(row)
        t0 = time.perf_counter()
        okA, nA = check_sample(n_jobs, bufs["A"])
        okB, nB = check_sample(n_jobs, bufs["B"])
        result["lines"].append(dict(
            threads=T, jobs=n_jobs, reports=n_jobs * JS, rounds=rounds,
            B_beats_A_in_every_pair=all(r["B_over_A"] > 1.0 for r in rounds),
            checks=dict(B_equals_A_every_job_every_round=all(r["B_equals_A_every_job"]
                                                             for r in rounds),
                        sample_matches_cpu=dict(A=okA, B=okB, jobs_checked=nA + nB),
                        all_counts_positive=bool((bufs["B"]["counts"][:, [0, 2]] > 0).all()),
                        closed_batch_counts_zero=bool((bufs["B"]["counts"][:, 1] == 0).all()),
                        check_seconds=time.perf_counter() - t0)))
        del bufs
    result["group_kernel_times"] = group_kernel_times(
        J, host, vks[0], tasks[0], op, closed, args.held_jobs)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "helper_job_rate.json"), "w") as f:
        json.dump(result, f, indent=1)
    md = ["| threads | round | A: three calls | B: one call | C: `_ex` alone | D: A's `_ex` "
          "| B / A | B / C | B / D |", "|---|---|---|---|---|---|---|---|---|"]
    for ln in result["lines"]:
        for i, r in enumerate(ln["rounds"]):
            md.append("| %d | %d | %.2f M/s | %.2f M/s | %.2f M/s | %.2f M/s | %.2f | %.2f | %.2f |"
                      % (ln["threads"], i + 1, r["A"]["reports_per_s"] / 1e6,
                         r["B"]["reports_per_s"] / 1e6, r["C"]["reports_per_s"] / 1e6,
                         r["D"]["reports_per_s"] / 1e6, r["B_over_A"], r["B_over_C"],
                         r["B_over_D"]))
    with open(os.path.join(args.out, "helper_job_rate.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print("\n".join(md))
    print(json.dumps({k: v for k, v in result.items() if k != "lines"}))
    for g in result["group_kernel_times"]:
        print(json.dumps(g))
    for ln in result["lines"]:
        print(json.dumps(dict(threads=ln["threads"], B_beats_A=ln["B_beats_A_in_every_pair"],
                              checks=ln["checks"])))
    bad = [ln for ln in result["lines"]
           if not (ln["checks"]["B_equals_A_every_job_every_round"] and
                   ln["checks"]["sample_matches_cpu"]["A"] and
                   ln["checks"]["sample_matches_cpu"]["B"])]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

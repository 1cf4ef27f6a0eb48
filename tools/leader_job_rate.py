"""A whole leader job per call against the four moves it stands for (tool-measured, not bench.py).

  python tools/leader_job_rate.py [--threads 16,128] [--pairs 5] [--out profiles/leader_job]

Workload: the leader jobs line's (bench.py leader_jobs_line) -- K = 4 tasks of
Prio3Histogram(256,16), 500-report jobs on explicit leader input shares and the helper's prepare
messages, host buffers -- with what AggregationJobWriter needs per job: three batch intervals per
job of which the middle one is closed, max_segments = 4, and a helper response that rejects a few
reports.  Three forms, timed in one process, alternating A, B, C for --pairs rounds per thread
count (native worker janus_jobs_run_leader_job, libjanus_jobs.so); every form runs
prio3_leader_prepare_init_batch per job first:
  A  the per-report overlay of prepare_error + prio3_job_index +
     prio3_leader_prepare_next_aggregate_batch + prio3_batch_metadata + the outcome pass, per job
  B  prio3_leader_finish_job
  C  prio3_leader_prepare_next_aggregate_batch alone, one segment, no index, overlay, metadata or
     outcome (the leader jobs line's combined form): the ceiling
Checks: every output of every job of B equals A's in every round, and a sample of jobs of each
task equals the restatement (tests/job_index_ref.py, the C restatement of prio's leader, hashlib).
Then one held group of --held-jobs jobs of form B with the engine's per-kernel timing events.
Writes leader_job_rate.json and leader_job_rate.md under --out.
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
NO_ERROR = 0xFF
FORMS = (("A", 0, "overlay + prio3_job_index + prio3_leader_prepare_next_aggregate_batch + "
                  "prio3_batch_metadata + outcome pass"),
         ("B", 1, "prio3_leader_finish_job"),
         ("C", 2, "prio3_leader_prepare_next_aggregate_batch alone (one segment, no index, no "
                  "metadata)"))
OUTS = ("ps", "seg", "starts", "reject", "dup", "info", "status", "outcome", "counts", "agg", "ck",
        "iv")


def group_kernel_times(J, host, vk, closed, n_jobs, rounds=3):
    """Per-kernel times (the engine's `timing` events, us) of ONE prepare_next group of n_jobs
    500-report jobs of task 0 queued behind the executor's hold, form B."""
    import threading
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, device=0)
    rows = [slice(j * JS, (j + 1) * JS) for j in range(n_jobs)]
    inits = [eng.leader_prepare_init_batch(host["nonces"][r], host["public_shares"][r],
                                           host["leader_input_shares"][r]) for r in rows]
    eng.set_option("timing", 1)

    def call(j):
        r = rows[j]
        inits[j][2].leader_finish_job(host["nonces"][r], host["times"][r], inits[j][1],
                                      host["msgs"][r], PREC, S, prepare_error=host["perr"][r],
                                      closed_intervals=closed)

    out = []
    for _ in range(rounds + 1):  # the first round loads the kernels
        eng.timing_reset()
        s0 = eng.executor_stats(J.EXEC_LEADER_NEXT)
        eng.executor_control("hold", 1, J.EXEC_LEADER_NEXT)
        th = [threading.Thread(target=call, args=(j,), daemon=True) for j in range(n_jobs)]
        try:
            for x in th:
                x.start()
            t0 = time.monotonic()
            while (eng.executor_stats(J.EXEC_LEADER_NEXT)["jobs"] - s0["jobs"] < n_jobs and
                   time.monotonic() - t0 < 30):
                time.sleep(0.005)
            time.sleep(0.05)
        finally:
            eng.executor_control("hold", 0, J.EXEC_LEADER_NEXT)
        for x in th:
            x.join(60)
        groups = eng.executor_stats(J.EXEC_LEADER_NEXT)["groups"] - s0["groups"]
        out.append(dict(form="B", jobs=n_jobs, group_launches=groups,
                        kernels_us={k: round(ms * 1e3, 1) for k, (ms, n) in eng.timing().items()
                                    if n}))
    for _, _, b in inits:
        b.free()
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--held-jobs", type=int, default=48,
                    help="jobs of the one held group whose kernels are timed")
    ap.add_argument("--threads", default="16,128")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=4, help="jobs per task checked against the CPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leader_job"))
    args = ap.parse_args()
    import torch
    import bench as B
    from janus_amd import dap
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    from tests import job_index_ref as R
    torch.cuda.set_device(0)
    cores = B.cpu_threads()
    rng = np.random.default_rng(0x4C4A4F42)
    vks = [bytes([0xB1 + t]) * 16 for t in range(K)]
    engines, _ = B._job_engines(J.Prio3Histogram(256, 16), vks, None)
    sz = engines[0].sz
    cols = {k: [] for k in ("nonces", "public_shares", "leader_input_shares", "msgs")}
    for t, e in enumerate(engines):
        p = e.generate_reports_device(POOL, seed=0x4C4A4F4200000001 + t, with_leader_inputs=True)
        msgs = torch.empty((POOL, sz.prep_msg_len), dtype=torch.uint8, device=p["nonces"].device)
        st = torch.empty(POOL, dtype=torch.uint8, device=p["nonces"].device)
        e.prepare_device(p["nonces"], p["public_shares"], p["helper_shares"],
                         p["leader_prep_shares"], msgs, st)  # the helper's prepare messages
        torch.cuda.synchronize()
        assert int((st != 0).sum().item()) == 0
        for k in ("nonces", "public_shares", "leader_input_shares"):
            cols[k].append(p[k].cpu().numpy())
        cols["msgs"].append(msgs.cpu().numpy())
        del p, msgs, st
    host = {k: np.ascontiguousarray(np.concatenate(v)) for k, v in cols.items()}
    host["times"] = (TB + rng.integers(0, 3 * PREC, K * POOL)).astype(np.uint64)
    # the helper's response: one report in 64 rejected (HpkeDecryptError), one in 128 tampered
    perr = np.full(K * POOL, NO_ERROR, np.uint8)
    perr[rng.random(K * POOL) < 1 / 64] = 2
    host["perr"] = perr
    if sz.prep_msg_len:
        host["msgs"][rng.random(K * POOL) < 1 / 128, 0] ^= 1
    closed = np.array([[TB + PREC, PREC]], np.uint64)
    J.load_library()
    lib = C.CDLL(os.path.join(ROOT, "janus_amd", "libjanus_jobs.so"))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.janus_jobs_run_leader_job.restype = C.c_double
    lib.janus_jobs_run_leader_job.argtypes = ([C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int,
                                               C.c_int, u32] + [vp] * 6 + [u64, vp, u32, u32] +
                                              [vp] * 12 + [C.c_int])
    eng_arr = (vp * K)(*[e.handle.value for e in engines])
    P = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    o = Oracle("histogram", length=256, chunk_length=16)

    def buffers(n_jobs):
        b = dict(ps=np.zeros((n_jobs * JS, sz.prep_share_len), np.uint8),
                 seg=np.zeros(n_jobs * JS, np.uint32), starts=np.zeros((n_jobs, S), np.uint64),
                 reject=np.zeros(n_jobs * JS, np.uint8), dup=np.zeros(n_jobs * JS, np.uint8),
                 info=np.zeros((n_jobs, 6), np.uint32), status=np.zeros(n_jobs * JS, np.uint8),
                 outcome=np.zeros(n_jobs * JS, np.uint8), counts=np.zeros((n_jobs, S), np.uint64),
                 agg=np.zeros((n_jobs, S, sz.agg_share_len), np.uint8),
                 ck=np.zeros((n_jobs, S, 32), np.uint8), iv=np.zeros((n_jobs, S, 2), np.uint64))
        B._warm(*b.values())
        return b

    def run(T, jobs, form, b):
        for v in b.values():
            v.fill(0)
        b["status"].fill(0xFF)
        return lib.janus_jobs_run_leader_job(
            eng_arr, K, C.cast(C.pointer(sz), vp), T, jobs, JS, POOL, P(host["nonces"]),
            P(host["public_shares"]), P(host["leader_input_shares"]), P(host["msgs"]),
            P(host["times"]), P(host["perr"]), PREC, P(closed), 1, S,
            *[P(b[k]) for k in OUTS], form)

    def check_sample(n_jobs, b):
        """A sample of each task's jobs against the restatement."""
        ok, checked = True, 0
        for t in range(K):
            jl, idx = B._job_windows(t, n_jobs, K, JS, POOL)
            for q in range(min(args.sample, len(jl))):
                j, rows = jl[q], idx[q * JS:(q + 1) * JS]
                ids, times, pe = host["nonces"][rows], host["times"][rows], host["perr"][rows]
                ref = R.job_index(ids, times, PREC, S, closed)
                seg, acc = ref["segment_ids"], ref["accept_mask"]
                rseg = np.where((pe == NO_ERROR) & (acc != 0) & (seg != 0xFFFFFFFF), seg, S)
                rps, rst, agg, cnt = o.leader_batch(
                    vks[t], ids, host["public_shares"][rows], host["leader_input_shares"][rows],
                    host["msgs"][rows], n_threads=cores, segment_ids=rseg.astype(np.uint32),
                    n_segments=S)
                st = np.where(pe != NO_ERROR, 5, rst).astype(np.uint8)
                outcome = np.array(dap.leader_outcome(np.zeros(JS, np.uint8), pe, st), np.uint8)
                outcome[(outcome == NO_ERROR) & (ref["reject"] != 0)] = 0
                ck = np.zeros((S, 32), np.uint8)
                iv = np.zeros((S, 2), np.uint64)
                for s in range(S):
                    r = np.flatnonzero(seg == s)
                    if len(r):
                        lo = int(times[r].min())
                        iv[s] = (lo, int(times[r].max()) + 1 - lo)
                    for i in r[(st[r] == 0) & (acc[r] != 0)]:
                        ck[s] ^= np.frombuffer(hashlib.sha256(ids[i].tobytes()).digest(), np.uint8)
                sl = slice(j * JS, (j + 1) * JS)
                info = [ref[f] for f in ("n_segments", "overflow", "n_duplicates",
                                         "first_duplicate", "n_closed", "n_time_errors")]
                ok &= bool(np.array_equal(b["ps"][sl], rps) and np.array_equal(b["seg"][sl], seg) and
                           np.array_equal(b["reject"][sl], ref["reject"]) and
                           np.array_equal(b["dup"][sl], ref["duplicate"]) and
                           np.array_equal(b["starts"][j], ref["segment_starts"]) and
                           list(b["info"][j]) == info and np.array_equal(b["status"][sl], st) and
                           np.array_equal(b["outcome"][sl], outcome) and
                           np.array_equal(b["agg"][j], agg) and
                           np.array_equal(b["counts"][j], cnt.astype(np.uint64)) and
                           np.array_equal(b["ck"][j], ck) and np.array_equal(b["iv"][j], iv))
                checked += 1
        return ok, checked

    result = dict(tool="tools/leader_job_rate.py",
                  workload=dict(vdaf="Prio3Histogram(256,16)", job_size=JS, tasks=K, pool=POOL,
                                batch_intervals_per_job=3, closed_intervals=1, max_segments=S,
                                helper_rejects="1 in 64", tampered_prepare_messages="1 in 128",
                                buffers="host"),
                  forms={f: call for f, _, call in FORMS}, device=torch.cuda.get_device_name(0),
                  lines=[])
    for T in [int(x) for x in args.threads.split(",")]:
        n_jobs = 1024 if T <= 16 else (1 << 20) // JS
        bufs = {f: buffers(n_jobs) for f, _, _ in FORMS}
        for f, form, _ in FORMS:  # warmup: pools, pinned staging, streams, worker threads
            if run(T, max(K, min(n_jobs, 8 * T)), form, bufs[f]) < 0:
                raise RuntimeError(f"form {f}: a C-ABI call failed")
        rounds = []
        for r in range(args.pairs):
            row = {}
            for f, form, _ in FORMS:
                g0 = engines[0].executor_stats(J.EXEC_LEADER_NEXT)["groups"]
                dt = run(T, n_jobs, form, bufs[f])
                if dt < 0:
                    raise RuntimeError(f"form {f}: a C-ABI call failed")
                row[f] = dict(ms=dt * 1e3, reports_per_s=n_jobs * JS / dt, jobs_per_s=n_jobs / dt,
                              next_group_launches=engines[0].executor_stats(
                                  J.EXEC_LEADER_NEXT)["groups"] - g0)
            row["B_equals_A_every_job"] = all(
                np.array_equal(bufs["A"][k], bufs["B"][k]) for k in bufs["A"])
            row["B_over_A"] = row["B"]["reports_per_s"] / row["A"]["reports_per_s"]
            row["B_over_C"] = row["B"]["reports_per_s"] / row["C"]["reports_per_s"]
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
    result["group_kernel_times"] = group_kernel_times(J, host, vks[0], closed, args.held_jobs)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "leader_job_rate.json"), "w") as f:
        json.dump(result, f, indent=1)
    md = ["| threads | round | A: four moves | B: one call | C: next + aggregate alone | B / A "
          "| B / C |", "|---|---|---|---|---|---|---|"]
    for ln in result["lines"]:
        for i, r in enumerate(ln["rounds"]):
            md.append("| %d | %d | %.2f M/s | %.2f M/s | %.2f M/s | %.2f | %.2f |"
                      % (ln["threads"], i + 1, r["A"]["reports_per_s"] / 1e6,
                         r["B"]["reports_per_s"] / 1e6, r["C"]["reports_per_s"] / 1e6,
                         r["B_over_A"], r["B_over_C"]))
    with open(os.path.join(args.out, "leader_job_rate.md"), "w") as f:
        f.write("\n".join(md) + "\n")
    print("\n".join(md))
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

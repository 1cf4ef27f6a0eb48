"""Rates of the leader's upload through the executor against the blocking batch call, at the size
Janus's ReportWriteBatcher hands over.  A build-time measurement, not a test and
not bench.py:

  python tools/upload_job_rate.py [--reports 100] [--seconds 0.5] [--pairs 5] [--out DIR] [--run N]
  python tools/upload_job_rate.py --render DIR/upload_job_rate_runN.json   (the .md of a kept run)

For Histogram(256,16) and Sum(32) (X25519 / HKDF-SHA256 / AES-128-GCM) the Report bodies come from
prio3_client_prepare_reports_device and are copied to the host once.  Caller threads (Python
threads around the raw C calls, which release the GIL; every thread owns its rows, its structs and
its output buffers) then upload jobs of --reports reports back to back for --seconds:

  blocking   prio3_leader_upload_job against prio3_leader_upload_batch, 16 and 128 threads
  tickets    prio3_leader_upload_job_submit with K = 4 and 8 tickets per thread against K = 1 (the
             blocking job call), 16 threads

--pairs interleaved pairs per setting (A B A B ...), in the same process.  After every measurement
the outputs of a sample of jobs (thread 0's and the last thread's last job) are compared byte for
byte with the batch form's on the same rows.  Printed per side: reports/s (median, min - max) and
the share of the 63 GB/s link the staged bytes take (in: the row and its meta; out: the output
block's rows), then the ratio of each pair; --out DIR keeps the run as upload_job_rate_runN.json and
the same figures as tables in upload_job_rate_runN.md.  Needs the GPU: no fallback.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = (("hist_256_c16", dict(kind="histogram", length=256, chunk_length=16)),
         ("sum32", dict(kind="sum", bits=32)))
INFO_LEADER = b"dap-09 input share" + bytes([1, 2])
INFO_HELPER = b"dap-09 input share" + bytes([1, 3])
T0 = 1_700_000_000
LINK = 63e9
POOL, TASKS = 64, 8  # distinct jobs' worth of reports on the host, of this many tasks


def make_keys():
    """The leader keypair the reports are sealed to, and the helper's public key."""
    from oracle import hpke as H
    rng = np.random.default_rng(5)
    sk = H.kem_private(rng)
    return sk, H.kem_public(sk), H.kem_public(H.kem_private(rng))


def make_rows(eng, vdaf, cfg, n, task, keys, seed):
    """n upload-ready Report rows of one task on the host (rows, lengths)."""
    import torch
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    p = vdaf.params()
    hi = cfg["length"] if cfg["kind"] == "histogram" else 1 << cfg["bits"]
    m = torch.randint(0, hi, (n, 1), generator=g, device=dev, dtype=torch.int64)
    u8 = dict(generator=g, device=dev, dtype=torch.uint8)
    ids = torch.randint(0, 256, (n, 16), **u8)
    rand = torch.randint(0, 256, (n, eng.rand_len), **u8)
    sk_l = torch.randint(0, 256, (n, 32), **u8)
    sk_h = torch.randint(0, 256, (n, 32), **u8)
    times = T0 + torch.randint(0, 3600, (n,), generator=g, device=dev, dtype=torch.int64)
    ls = G.HpkeSealer(keys[1], INFO_LEADER, device=0)
    hs = G.HpkeSealer(keys[2], INFO_HELPER, device=0)
    need = J.load_library().prio3_client_report_stride(C.byref(p), ls.handle, hs.handle, 0)
    rep = eng.prepare_reports_device(ls, hs, task, 300, m, ids, times, rand, sk_l, sk_h, 42, 13,
                                     report_stride=-(-need // 16) * 16)
    torch.cuda.synchronize()
    if int(rep["status"].any()):
        raise SystemExit("the client rejected a report")
    rows = rep["reports"].cpu().numpy()
    ln = rep["report_len"].cpu().numpy().view(np.uint32)
    return rows, ln


class Caller:
    """One thread's job: its rows, structs and K sets of output buffers."""

    def __init__(self, eng, rows, ln, task, opener, hct_stride, k):
        from janus_amd import prio3 as J
        sz = eng.sz
        n = rows.shape[0]
        self.rows, self.ln, self.n = np.ascontiguousarray(rows), np.ascontiguousarray(ln), n
        self.tid = (C.c_uint8 * 32).from_buffer_copy(task)
        self.outs, self.jouts = [], []
        for _ in range(k):
            o = dict(report_ids=np.zeros((n, 16), np.uint8), times=np.zeros(n, np.uint64),
                     public_shares=np.zeros((n, sz.public_share_len), np.uint8),
                     leader_input_shares=np.zeros((n, sz.leader_input_share_len), np.uint8),
                     extensions=np.zeros((n, 64), np.uint8), ext_len=np.zeros(n, np.uint32),
                     helper_config_ids=np.zeros(n, np.uint8), helper_enc=np.zeros((n, 32), np.uint8),
                     helper_ct=np.zeros((n, hct_stride), np.uint8),
                     helper_ct_len=np.zeros(n, np.uint32), leader_config_ids=np.zeros(n, np.uint8),
                     status=np.zeros(n, np.uint8))
            self.outs.append(o)
            self.jouts.append(J.Prio3UploadJobOut(
                **{key: (v.ctypes.data if v.size else None) for key, v in o.items()}))
        self.jin = J.Prio3UploadJobIn(
            task_opener=opener.handle.value, global_opener=None, task_config_id=42,
            global_config_id=0, n=n, task_id=self.tid, now=T0 + 4000, report_deadline=T0 + 4060,
            task_expiration=(1 << 64) - 1, report_expiry_age=(1 << 64) - 1,
            reports=self.rows.ctypes.data, report_len=self.ln.ctypes.data,
            report_stride=rows.shape[1], ext_stride=64, helper_enc_len=32,
            helper_ct_stride=hct_stride)
        self.opener, self.hct_stride = opener, hct_stride

    def batch_args(self, eng, o):
        p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        return (eng.handle, self.opener.handle, 42, None, 0, self.n, self.tid, T0 + 4000, T0 + 4060,
                (1 << 64) - 1, (1 << 64) - 1, self.rows.ctypes.data, self.rows.shape[1],
                self.ln.ctypes.data, p(o["report_ids"]), p(o["times"]), p(o["public_shares"]),
                p(o["leader_input_shares"]), p(o["extensions"]), p(o["ext_len"]), 64,
                p(o["helper_config_ids"]), p(o["helper_enc"]), 32, p(o["helper_ct"]),
                p(o["helper_ct_len"]), self.hct_stride, p(o["leader_config_ids"]), p(o["status"]))


def run_threads(eng, callers, mode, k, seconds):
    """Every caller loops `mode` ("batch", "job", "tickets") for `seconds`; returns reports/s."""
    from janus_amd import prio3 as J
    L = J.load_library()
    go, stop = threading.Barrier(len(callers) + 1), threading.Event()
    done = [0] * len(callers)
    errors = []

    def work(i, c):
        try:
            args = c.batch_args(eng, c.outs[0])
            jin, jouts = C.byref(c.jin), [C.byref(x) for x in c.jouts]
            ring = []
            go.wait(timeout=120)
            while not stop.is_set():
                if mode == "batch":
                    rc = L.prio3_leader_upload_batch(*args)
                elif mode == "job":
                    rc = L.prio3_leader_upload_job(eng.handle, jin, jouts[0])
                else:
                    if len(ring) == k:
                        rc = L.prio3_ticket_wait(ring.pop(0))
                        if rc:
                            raise RuntimeError(f"wait rc={rc}")
                        done[i] += 1
                    h = C.c_void_p()
                    rc = L.prio3_leader_upload_job_submit(eng.handle, jin,
                                                          jouts[(done[i] + len(ring)) % k], -1,
                                                          C.byref(h))
                    ring.append(h)
                    if rc:
                        raise RuntimeError(f"{mode} rc={rc}")
                    continue
                if rc:
                    raise RuntimeError(f"{mode} rc={rc}")
                done[i] += 1
            for h in ring:  # drained after the clock stops
                if L.prio3_ticket_wait(h):
                    raise RuntimeError("wait failed")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            stop.set()

    th = [threading.Thread(target=work, args=(i, c)) for i, c in enumerate(callers)]
    for t in th:
        t.start()
    go.wait(timeout=120)
    t0 = time.perf_counter()
    time.sleep(seconds)
    stop.set()
    n_done = sum(done)
    dt = time.perf_counter() - t0
    for t in th:
        t.join()
    if errors:
        raise SystemExit(f"{mode}: {errors[:3]}")
    return n_done * callers[0].n / dt


def check_sample(eng, callers):
    """The job outputs of a sample of callers against the batch form on the same rows."""
    from janus_amd import prio3 as J
    L = J.load_library()
    for c in (callers[0], callers[-1]):
        ref = {key: np.full_like(v, 0x5A) for key, v in c.outs[0].items()}
        if L.prio3_leader_upload_batch(*c.batch_args(eng, ref)):
            raise SystemExit("the batch form failed")
        if ref["status"].any():
            raise SystemExit("the batch form rejected a report")
        for o in c.outs:
            if not np.any(o["report_ids"]):
                continue  # a buffer set no job has used
            for key in ref:
                if not np.array_equal(ref[key], o[key]):
                    raise SystemExit(f"job output {key} differs from the batch form's")


def measure(name, cfg, args):
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    vdaf = J.Prio3Histogram(cfg["length"], cfg["chunk_length"]) if cfg["kind"] == "histogram" \
        else J.Prio3Sum(cfg["bits"])
    eng = J.HelperEngine(vdaf, bytes(range(16)), device=0)
    sz = eng.sz
    rng = np.random.default_rng(7)
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(TASKS)]
    n = args.reports
    hct = G.sealed_stride(sz.helper_share_len)
    # POOL jobs' worth of reports of TASKS tasks, all sealed to one leader keypair
    # (prepare_reports_device seals one task per call)
    keys = make_keys()
    pools = []
    for ti, task in enumerate(tasks):
        rows_t, ln_t = make_rows(eng, vdaf, cfg, n * (POOL // TASKS), task, keys, seed=ti)
        for s in range(POOL // TASKS):
            pools.append((rows_t[s * n:(s + 1) * n], ln_t[s * n:(s + 1) * n], task))
    opener = G.HpkeOpener(keys[0], keys[1], INFO_LEADER, device=0)
    stride = pools[0][0].shape[1]
    per_in = stride + 8
    per_out = 40 + 8 + 16 + 4 + 4 + sz.public_share_len + sz.leader_input_share_len + 64 + 3
    res = dict(instance=name, reports_per_job=n, report_stride=stride, bytes_in=per_in,
               bytes_out=per_out, settings=[])

    def setting(label, threads, a, b):
        k = max(a[1], b[1])
        callers = [Caller(eng, *pools[t % POOL], opener, hct, k) for t in range(threads)]
        for mode, kk in (a, b):  # warm-up: pools, stagings, streams
            run_threads(eng, callers, mode, kk, 0.15)
        sides = {0: [], 1: []}
        for _ in range(args.pairs):
            for i, (mode, kk) in enumerate((a, b)):
                sides[i].append(run_threads(eng, callers, mode, kk, args.seconds))
                check_sample(eng, callers)
        row = dict(setting=label, threads=threads)
        for i, (mode, kk) in enumerate((a, b)):
            v = sides[i]
            row["a" if i == 0 else "b"] = dict(
                mode=mode, k=kk, rates=[round(x) for x in v], median=round(statistics.median(v)),
                min=round(min(v)), max=round(max(v)),
                link_share=round(statistics.median(v) * (per_in + per_out) / LINK, 4))
        row["ratio_pairs"] = [round(y / x, 3) for x, y in zip(sides[0], sides[1])]
        row["b_ahead_in_every_pair"] = all(r > 1 for r in row["ratio_pairs"])
        res["settings"].append(row)
        print(f"{name:13s} {label:26s} {row['a']['median'] / 1e6:7.3f} -> "
              f"{row['b']['median'] / 1e6:7.3f} M reports/s  pairs {row['ratio_pairs']}  "
              f"link {row['b']['link_share']:.3f}", flush=True)

    for threads in (16, 128):
        setting(f"batch vs job, {threads} threads", threads, ("batch", 1), ("job", 1))
    for k in (4, 8):
        setting(f"job K=1 vs tickets K={k}, 16 threads", 16, ("job", 1), ("tickets", k))
    st = eng.executor_stats(J.EXEC_UPLOAD)
    res["executor"] = dict(jobs=st["jobs"], groups=st["groups"], reports=st["reports"])
    return res


def render_md(d) -> str:
    """The run's JSON as the markdown tables kept beside it (profiles/upload_jobs/*.md)."""
    lines = [f"# tools/upload_job_rate.py, run {d['run']}: {d['reports']}-report jobs, {d['pairs']} "
             f"interleaved pairs of {d['seconds']} s per setting", "",
             "M reports/s: median (min-max) of side A, of side B, the B/A ratio of every pair, B's "
             "share of the 63 GB/s link.", ""]
    for c in d["cases"]:
        lines += [f"## {c['instance']} (row {c['report_stride']} B; staged in {c['bytes_in']} B, out "
                  f"{c['bytes_out']} B per report)", "",
                  "| setting | A | B | B/A per pair | link |", "|---|---|---|---|---|"]
        for s in c["settings"]:
            f = lambda x: f"{x['median'] / 1e6:.3f} ({x['min'] / 1e6:.3f}-{x['max'] / 1e6:.3f})"  # noqa: E731
            lines.append(f"| {s['setting']} | {s['a']['mode']}: {f(s['a'])} | {s['b']['mode']}: "
                         f"{f(s['b'])} | {', '.join(str(r) for r in s['ratio_pairs'])} | "
                         f"{s['b']['link_share']:.3f} |")
        e = c["executor"]
        lines += ["", f"Upload executor over the case: {e['jobs']} jobs in {e['groups']} groups "
                  f"({e['jobs'] / e['groups']:.1f} jobs per group).", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reports", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--render", default=None, help="write the .md of an existing run's JSON")
    args = ap.parse_args()
    if args.render:
        with open(args.render) as f, open(os.path.splitext(args.render)[0] + ".md", "w") as g:
            g.write(render_md(json.load(f)))
        return
    out = dict(tool="upload_job_rate", run=args.run, reports=args.reports, seconds=args.seconds,
               pairs=args.pairs, cases=[measure(name, cfg, args) for name, cfg in CASES])
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"upload_job_rate_run{args.run}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        with open(os.path.join(args.out, f"upload_job_rate_run{args.run}.md"), "w") as f:
            f.write(render_md(out))


if __name__ == "__main__":
    main()

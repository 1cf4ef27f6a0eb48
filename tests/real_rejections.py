"""Cases, reference conditions and the child-process entry of tests/test_gpu_real_rejections.py.

The engine's test-rejection build (janus_amd/libjanus_prio3_rej.so, option test_reject_bits) and
the C restatement (oracle.set_test_reject) reject the same superset of candidates, so reports with
real rejections -- the retry of the byte-level sampler, stale fast-path results, sparse flags --
compare byte for byte.  `python -m tests.real_rejections GROUP` runs one group of cases in a
process of its own (the pytest process holds the default library) and prints one `CASE {json}`
line per case: the reference conditions computed from the restatement alone, and the outcome of
the device comparison.

Rates.  The default is 10 bits.  A case carries another rate where 10 bits cannot meet the
reference conditions, by the expected number of flagged reports n * (1 - (1 - 2^-bits)^c), c the
candidates a report draws:
  * sumvec_8x1000_c63 (c ~ 8400): 16 bits, or every report would be flagged;
  * sumvec_32x20_c7 (c ~ 910): 12 bits (10 bits flags 59 % of the reports, the bound is half);
  * the fused path (hist_256_c16, c ~ 330): 15 bits, since a wave of 64 reports stays flag-free
    with probability 0.73^64 at 10 bits but 0.52 at 15;
  * the leader samples only query and joint randomness (c <= 3) and the small client instances a
    few dozen elements: 5 to 8 bits give the 8 flagged reports a case needs.
"""
import json
import sys
import threading

import numpy as np

from tests.conftest import CONFIGS

HELPER_STREAMS = ("query", "meas", "proofs", "jr")
# group 1: (case id, config, n, seed, bits, entry points, engine options).  "host": prepare_batch +
# accumulate through the coalescing executor (one launch per group whatever `chunks` says);
# "device": prepare_aggregate_device + aggregate_finish_device, which cuts the batch into
# `chunks` stream-overlapped chunks (of a multiple of 256 reports; Histogram only on one lane per
# report) and runs the deferred redo after the last one
HELPER_CASES = [
    ("count", "count", 999, 30, 10, "host", {}),
    ("sum8", "sum8", 555, 11, 10, "host", {}),
    ("sum32", "sum32", 555, 11, 10, "host", {}),
    ("hist_10_c3", "hist_10_c3", 700, 11, 10, "host", {}),
    ("hist_256_c16-pair", "hist_256_c16", 700, 11, 10, "host", {"pair_max": 196608}),
    ("hist_256_c16-lane", "hist_256_c16", 700, 11, 10, "host", {"pair_max": 0}),
    ("hist_100_c4", "hist_100_c4", 333, 11, 10, "host", {}),
    ("sumvec_2x100_c10", "sumvec_2x100_c10", 333, 11, 10, "host", {}),
    ("sumvec_32x20_c7", "sumvec_32x20_c7", 333, 11, 12, "host", {}),
    ("sumvec_4x100_c10", "sumvec_4x100_c10", 333, 11, 10, "host", {}),
    ("sumvec_8x1000_c63", "sumvec_8x1000_c63", 101, 1, 16, "host", {}),
    ("hist_256_c16-chunks3", "hist_256_c16", 700, 11, 10, "device", {"chunks": 3, "pair_max": 0}),
    ("sum32-chunks3", "sum32", 555, 11, 10, "device", {"chunks": 3}),
    ("sumvec_32x20_c7-chunks3", "sumvec_32x20_c7", 333, 11, 12, "device", {"chunks": 3}),
    ("hist_256_c16-generic", "hist_256_c16", 700, 11, 10, "host", {"force_generic_query": 1}),
    ("sum32-generic", "sum32", 555, 11, 10, "host", {"force_generic_query": 1}),
]
# group 2: (case id, n, seed, bits, n_segments, engine options)
FUSED_CASES = [
    ("fused-1500-pair", 1500, 3, 15, 7, {"pair_max": 196608}),
    ("fused-1500-lane", 1500, 3, 15, 7, {"pair_max": 0}),
    ("fused-700-chunks2", 700, 3, 14, 1, {"pair_max": 0, "chunks": 2}),
]
# group 3: (config, n, seed, bits)
LEADER_CASES = [("hist_256_c16", 300, 31, 5), ("sum32", 300, 31, 5), ("count", 300, 31, 5),
                ("sumvec_32x20_c7", 300, 31, 5)]
# group 4: (config, n, seed, bits)
CLIENT_CASES = [("count", 130, 7, 6), ("sum8", 130, 7, 8), ("hist_10_c3", 130, 7, 8),
                ("sumvec_8x10_c9", 130, 7, 10)]
GEN_CASE = ("hist_256_c16", 70, 99, 10)
EXEC_CASE = ("hist_256_c16", 500, 4, 10)  # four concurrent jobs, seeds 40..43
SEMANTIC_CASE = ("hist_10_c3", 130, 7, 8)
GROUPS = ("helper", "fused", "leader", "client", "executor", "semantic")


# ---- reference side (CPU only) --------------------------------------------------------------
def helper_data(name, n, seed):
    """The reports of tests.test_gpu_parity._check_against_oracle(cfg, n, seed) (tampered)."""
    from tests.test_gpu_parity import VK, _oracle, _tamper
    o = _oracle(CONFIGS[name])
    d = o.gen_reports(VK, n, seed=seed, n_threads=8)
    return o, _tamper(o, d, np.random.default_rng(seed))


def flags_of(scan, streams):
    return np.array([any(s[k][0] for k in streams) for s in scan], bool)


def _mixed_run(flagged, good, width):
    """A width-aligned run of reports that holds a flagged report and an unflagged good one."""
    n = len(flagged)
    return any(flagged[a:a + width].any() and (good[a:a + width] & ~flagged[a:a + width]).any()
               for a in range(0, n, width))


def conditions(scan, streams, status, es, lens, tampered=None):
    """Per-case conditions and the module-wide coverage the scan of one case contributes.
    lens: stream -> elements of the stream; status: the reference statuses (0 = finished)."""
    fl = flags_of(scan, streams)
    good = np.asarray(status) == 0
    bad = ~good if tampered is None else np.asarray(tampered, bool)
    c = dict(n=len(scan), flagged=int(fl.sum()), mixed64=_mixed_run(fl, good, 64),
             mixed32=_mixed_run(fl, good, 32), tampered_flagged=bool((fl & bad).any()),
             streams=sorted({k for s in scan for k in streams if s[k][0]}), straddle=False,
             first=False, last=False, multi=False)
    for s in scan:
        for k in streams:
            cnt, recs = s[k]
            c["multi"] |= cnt >= 2
            for cand, elem in recs:
                c["first"] |= elem == 0
                c["last"] |= elem == lens[k] - 1
                c["straddle"] |= k == "meas" and es == 16 and cand % 21 == 10
    return c


def helper_conditions(o, d, status):
    from tests.test_gpu_parity import VK
    scan = o.reject_scan(VK, 1, d["nonces"], d["public_shares"], d["helper_shares"])
    lens = dict(query=o.qr_len, meas=o.meas_len, proofs=o.proof_len, jr=o.jr_len)
    return scan, conditions(scan, HELPER_STREAMS, status, o.es, lens)


def helper_inputs(name, n, seed, n_segments=5, seg_mode="random"):
    """One helper case: the tampered reports, their segment ids (random, or contiguous runs whose
    boundaries fall inside waves) and accept mask, the restatement's results for exactly these,
    and the reference conditions.  The device comparisons below take this and nothing else."""
    from tests.test_gpu_parity import VK
    o, d = helper_data(name, n, seed)
    rng = np.random.default_rng([seed, n_segments])
    if seg_mode == "runs":
        seg = np.zeros(n, np.uint32)
        for c in rng.choice(np.arange(1, n), n_segments - 1, replace=False):
            seg[c:] += 1
    else:
        seg = rng.integers(0, n_segments, n).astype(np.uint32)
    accept = (rng.random(n) > 0.1).astype(np.uint8)
    ref = o.helper_batch(VK, d["nonces"], d["public_shares"], d["helper_shares"],
                         d["leader_prep_shares"], segment_ids=seg, accept_mask=accept,
                         n_segments=n_segments, n_threads=8)
    scan, cond = helper_conditions(o, d, ref[1])
    return dict(o=o, d=d, seg=seg, accept=accept, nseg=n_segments, ref=ref, scan=scan, cond=cond)


def fused_conditions(fl, seg, width):
    """Full waves of `width` reports in one segment: one un-fused only by a flag, one flag-free."""
    n = len(fl)
    one = [a for a in range(0, n - width + 1, width) if len(set(seg[a:a + width])) == 1]
    return dict(unfused_by_flag=any(fl[a:a + width].any() for a in one),
                flag_free=any(not fl[a:a + width].any() for a in one))


# ---- device side (child process, test-rejection library) -------------------------------------
_BITS = [0]


def _set_bits(bits):
    from oracle import oracle as O
    O.set_test_reject(bits)
    _BITS[0] = bits


def engine(cfg, opts=None):
    """An engine of the test-rejection library with the current case's test_reject_bits."""
    from tests.test_gpu_parity import _engine
    e = _engine(cfg)
    e.set_option("test_reject_bits", _BITS[0])
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    return e


def host_compare(eng, x):
    """prepare_batch + accumulate (the host-buffer ABI) against the restatement's results."""
    d, (rm, rs, ra, rc) = x["d"], x["ref"]
    msgs, status, batch = eng.prepare_batch(d["nonces"], d["public_shares"], d["helper_shares"],
                                            d["leader_prep_shares"])
    np.testing.assert_array_equal(status, rs)
    np.testing.assert_array_equal(msgs, rm)
    agg, cnt = batch.accumulate(x["seg"], x["accept"], x["nseg"])
    np.testing.assert_array_equal(cnt, rc)
    np.testing.assert_array_equal(agg, ra)


def device_compare(eng, x, min_chunks=1):
    """prepare_aggregate_device + aggregate_finish_device against the restatement's results; with
    min_chunks > 1 the prepare chain must have been launched at least that often."""
    import torch
    d, (rm, rs, ra, rc) = x["d"], x["ref"]
    n, S, sz = len(rs), x["nseg"], eng.sz
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    msgs = torch.zeros((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    agg = torch.zeros((S, sz.agg_share_len), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(S, dtype=torch.int64, device=dev)
    eng.set_option("timing", 2)  # launches counted per kernel, nothing timed
    eng.timing_reset()
    eng.prepare_aggregate_device(t(d["nonces"]), t(d["public_shares"]) if sz.public_share_len
                                 else None, t(d["helper_shares"]), t(d["leader_prep_shares"]),
                                 t(x["seg"]), S, msgs, status)
    launches = {k: v[1] for k, v in eng.timing().items()}
    eng.aggregate_finish_device(status, t(x["accept"]), agg, cnt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), rs)
    np.testing.assert_array_equal(msgs.cpu().numpy()[:, :sz.prep_msg_len], rm)
    np.testing.assert_array_equal(cnt.cpu().numpy().astype(np.uint64), rc)
    np.testing.assert_array_equal(agg.cpu().numpy(), ra)
    assert max(launches.values(), default=0) >= min_chunks, launches


def _emit(case, cond, fn):
    res = dict(case=case, cond=cond, ok=False, err="")
    try:
        fn()
        res["ok"] = True
    except AssertionError as e:
        res["err"] = str(e)[:600] or "assertion failed"
    print("CASE " + json.dumps(res), flush=True)


def run_helper():
    import tests.test_gpu_parity as TP
    for case, name, n, seed, bits, path, opts in HELPER_CASES:
        _set_bits(bits)
        x = helper_inputs(name, n, seed)
        if path == "host":
            fn = lambda: host_compare(engine(CONFIGS[name], opts), x)  # noqa: E731
        else:
            fn = lambda: device_compare(engine(CONFIGS[name], opts), x, min_chunks=2)  # noqa: E731
        _emit(case, x["cond"], fn)
    # decode checks keep lt_p: a leader prep-share element with all its top bits set but < p
    # decodes (and fails decide), one >= p does not
    _set_bits(10)
    name, n = "hist_10_c3", 64
    o, eng = TP._oracle(CONFIGS[name]), engine(CONFIGS[name])
    d = o.gen_reports(TP.VK, n, seed=21, n_threads=4)
    p = 2**128 - 28 * 2**64 + 1
    d["leader_prep_shares"][5, :16] = np.frombuffer((p - 2).to_bytes(16, "little"), np.uint8)
    d["leader_prep_shares"][9, :16] = 0xFF
    ref = o.helper_batch(TP.VK, d["nonces"], d["public_shares"], d["helper_shares"],
                         d["leader_prep_shares"], n_threads=4)

    def decode_case():
        msgs, status, batch = eng.prepare_batch(d["nonces"], d["public_shares"],
                                                d["helper_shares"], d["leader_prep_shares"])
        np.testing.assert_array_equal(status, ref[1])
        np.testing.assert_array_equal(msgs, ref[0])
        assert status[5] != 0 and status[9] != 0 and status[5] != status[9], status[[5, 9]]
        assert (status == 0).sum() == n - 2
    _emit("decode_top_bits", dict(top_bits_status=int(ref[1][5]), ge_p_status=int(ref[1][9])),
          decode_case)


def run_fused():
    cfg = CONFIGS["hist_256_c16"]
    for case, n, seed, bits, nseg, opts in FUSED_CASES:
        _set_bits(bits)
        x = helper_inputs("hist_256_c16", n, seed, nseg, "runs")
        x["cond"].update(fused_conditions(flags_of(x["scan"], HELPER_STREAMS), x["seg"],
                                          32 if opts["pair_max"] else 64))
        chunks = opts.get("chunks", 1)
        _emit(case, x["cond"], lambda: device_compare(engine(cfg, opts), x, min_chunks=chunks))


def leader_data(name, n, seed):
    """Reports sharded by the restatement, the helper's prepare messages, and the tampering: the
    first flagged report and report 17 get a wrong prepare message, report 9 a non-canonical
    leader share."""
    from tests.test_gpu_leader import _reports
    from tests.test_gpu_parity import VK, _oracle
    cfg = CONFIGS[name]
    o = _oracle(cfg)
    d = _reports(o, cfg, n, seed)
    d["leader_shares"][9, :o.es] = 0xFF
    scan = o.reject_scan(VK, 0, d["nonces"], d["public_shares"], d["leader_shares"])
    fl = flags_of(scan, ("query", "jr"))
    ps = o.leader_batch(VK, d["nonces"], d["public_shares"], d["leader_shares"],
                        np.zeros((n, max(o.prep_msg_len, 1)), np.uint8))[0]
    msgs = o.helper_batch(VK, d["nonces"], d["public_shares"], d["helper_shares"], ps)[0].copy()
    tampered = np.zeros(n, bool)
    tampered[9] = True
    if o.prep_msg_len:
        for i in (int(np.flatnonzero(fl)[0]) if fl.any() else 17, 17):
            msgs[i, 0] ^= 1
            tampered[i] = True
    else:  # Count has no prepare message: the flagged tampered report is a non-canonical share
        i = int(np.flatnonzero(fl)[0]) if fl.any() else 17
        d["leader_shares"][i, :o.es] = 0xFF
        tampered[i] = True
    seg = (np.arange(n) % 2).astype(np.uint32)
    ref = o.leader_batch(VK, d["nonces"], d["public_shares"], d["leader_shares"], msgs,
                         segment_ids=seg, n_segments=2)
    lens = dict(query=o.qr_len, jr=o.jr_len)
    cond = conditions(scan, ("query", "jr"), ref[1], o.es, lens, tampered)
    return o, d, msgs, seg, ref, cond


def run_leader():
    for name, n, seed, bits in LEADER_CASES:
        _set_bits(bits)
        o, d, msgs, seg, ref, cond = leader_data(name, n, seed)

        def case():
            eng = engine(CONFIGS[name])
            ps, st, batch = eng.leader_prepare_init_batch(d["nonces"], d["public_shares"],
                                                          d["leader_shares"])
            ref_ps, ref_st, ref_agg, ref_cnt = ref
            # the restatement reports a non-canonical leader share as 1, the engine as 6
            init_bad = np.array([(d["leader_shares"][i, :o.es] == 0xFF).all() for i in range(n)])
            np.testing.assert_array_equal(st != 0, init_bad)
            np.testing.assert_array_equal(ps[~init_bad], ref_ps[~init_bad])
            st2, agg, cnt = batch.leader_prepare_next_aggregate(msgs, st, seg, None, 2)
            np.testing.assert_array_equal(np.where(st2 == 6, 1, st2), ref_st)
            np.testing.assert_array_equal(cnt, ref_cnt)
            np.testing.assert_array_equal(agg, ref_agg)
        _emit("leader-" + name, cond, case)


def client_conditions(o, cfg, m, nonces, rand):
    from oracle.oracle import RejectRecord
    from tests.test_gpu_client_shard import _meas_arg
    scan = []
    for i in range(len(m)):
        with RejectRecord() as rec:
            o.shard(_meas_arg(cfg, m[i]), nonces[i].tobytes(), rand[i].tobytes())
        scan.append(rec.streams())
    streams = ("meas", "jr", "prove", "proofs")
    lens = dict(meas=o.meas_len, jr=o.jr_len, prove=o.prove_rand_len, proofs=o.proof_len)
    return scan, conditions(scan, streams, np.zeros(len(m)), o.es, lens,
                            tampered=np.zeros(len(m), bool))


def run_client():
    import tests.test_gpu_client_shard as TC
    import tests.test_gpu_parity as TP
    for name, n, seed, bits in CLIENT_CASES:
        _set_bits(bits)
        cfg = CONFIGS[name]
        o = TP._oracle(cfg)
        m, nonces, rand = TC._inputs(name, n, seed)
        _, cond = client_conditions(o, cfg, m, nonces, rand)
        ref = TC._oracle_rows(name, m, nonces, rand)

        def case():
            out = TC._shard_device(engine(cfg), m, nonces, rand)
            assert not out["status"].any()
            TC._assert_rows(out, ref)
        _emit("shard-" + name, cond, case)
    # the synthetic generator has no redo: it marks a report whose expansions met a rejection
    # (flags) and the caller drops it.  Every rejection the restatement sees in the streams the
    # helper and the leader can re-derive must be marked, every unmarked report must equal the
    # restatement's, and the marks beyond those (prove randomness, whose seed no output holds)
    # stay a small minority.
    name, n, seed, bits = GEN_CASE
    _set_bits(bits)
    cfg = CONFIGS[name]
    o = TP._oracle(cfg)
    ref = o.gen_reports(TP.VK, n, seed=seed, n_threads=4)
    scan = o.reject_scan(TP.VK, 1, ref["nonces"], ref["public_shares"], ref["helper_shares"])
    seen = flags_of(scan, HELPER_STREAMS)
    lens = dict(query=o.qr_len, meas=o.meas_len, proofs=o.proof_len, jr=o.jr_len)
    cond = conditions(scan, HELPER_STREAMS, np.zeros(n), o.es, lens, tampered=np.zeros(n, bool))

    def gen_case():
        import torch
        g = engine(cfg).generate_reports_device(n, seed=seed, with_checks=True)
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in g.items()}
        flags = g["flags"].astype(bool)
        assert (flags | ~seen).all(), "a rejection the restatement saw was not marked"
        assert int((flags & ~seen).sum()) <= n // 8, int((flags & ~seen).sum())
        assert (~flags).sum() >= n // 2
        for k in ("nonces", "public_shares", "helper_shares", "leader_prep_shares",
                  "leader_out_shares"):
            np.testing.assert_array_equal(g[k][~flags], ref[k][~flags], err_msg=k)
    _emit("generate-" + name, cond, gen_case)


def run_executor():
    """Four concurrent 500-report helper jobs through the host-buffer ABI: the coalescing
    executor runs them as one group (the PULL kernels)."""
    name, n, seed, bits = EXEC_CASE
    _set_bits(bits)
    cfg = CONFIGS[name]
    xs = [helper_inputs(name, n, 10 * seed + j, 3) for j in range(4)]
    jobs = [(x["d"], x["seg"], x["accept"], x["ref"]) for x in xs]
    # the conditions hold for each job: `jobs` lists them, the top level is their conjunction
    # (counts: the smallest job's) and, for the module-wide coverage, their union
    conds = [x["cond"] for x in xs]
    cond = dict(conds[0], jobs=conds)
    for c in conds[1:]:
        for k, v in c.items():
            cond[k] = min(cond[k], v) if k == "flagged" else cond[k] if k == "n" else \
                sorted(set(cond[k]) | set(v)) if k == "streams" else (cond[k] and v) \
                if k in ("mixed64", "mixed32", "tampered_flagged") else (cond[k] or v)

    def case():
        eng = engine(cfg)
        got, errs = [None] * 4, []

        def work(j):
            d, seg, acc, _ = jobs[j]
            try:
                got[j] = eng.prepare_aggregate_batch(d["nonces"], d["public_shares"],
                                                     d["helper_shares"], d["leader_prep_shares"],
                                                     seg, acc, 3)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))
        from tests.test_gpu_executor import _Held
        groups0 = eng.executor_stats(0)["groups"]
        ts = [threading.Thread(target=work, args=(j,)) for j in range(4)]
        with _Held(eng, 4) as held:  # all four queued before the launcher takes any
            [t.start() for t in ts]
            held.wait()
            [t.join() for t in ts]
        assert 0 < eng.executor_stats(0)["groups"] - groups0 < 4, "the jobs did not coalesce"
        assert not errs, errs
        for j in range(4):
            msgs, status, agg, cnt = got[j]
            rm, rs, ra, rc = jobs[j][3]
            np.testing.assert_array_equal(status, rs, err_msg=f"job {j}")
            np.testing.assert_array_equal(msgs, rm, err_msg=f"job {j}")
            np.testing.assert_array_equal(cnt, rc, err_msg=f"job {j}")
            np.testing.assert_array_equal(agg, ra, err_msg=f"job {j}")
    _emit("executor-4x500", cond, case)


def run_semantic():
    """Independent of the restatement's sampler: client -> leader init -> helper -> leader next
    under the variant; every report finishes and the aggregates unshard to the plaintext."""
    import tests.test_gpu_client_shard as TC
    name, n, seed, bits = SEMANTIC_CASE
    _set_bits(bits)
    cfg = CONFIGS[name]
    m, nonces, rand = TC._inputs(name, n, seed)

    def case():
        client, leader, helper = engine(cfg), engine(cfg), engine(cfg)
        out = TC._shard_device(client, m, nonces, rand)
        assert not out["status"].any()
        lps, lst, lb = leader.leader_prepare_init_batch(nonces, out["public_shares"],
                                                        out["leader_input_shares"])
        msgs, hst, hb = helper.prepare_batch(nonces, out["public_shares"], out["helper_shares"],
                                             lps)
        assert not lst.any() and not hst.any(), (lst, hst)
        assert not lb.leader_prepare_next(msgs, lst).any()
        (la, lc), (ha, hc) = lb.accumulate(), hb.accumulate()
        assert int(lc[0]) == int(hc[0]) == n
        p = 2**128 - 28 * 2**64 + 1
        dec = lambda b: [int.from_bytes(b[i:i + 16], "little") for i in range(0, len(b), 16)]  # noqa: E731
        tot = [(a + b) % p for a, b in zip(dec(la[0].tobytes()), dec(ha[0].tobytes()))]
        assert tot == np.bincount(m[:, 0].astype(np.int64), minlength=cfg["length"]).tolist()
    _emit("semantic-" + name, {}, case)


def main(group):
    from janus_amd import prio3 as J
    assert J.LIB_PATH.endswith("libjanus_prio3_rej.so"), J.LIB_PATH
    {"helper": run_helper, "fused": run_fused, "leader": run_leader, "client": run_client,
     "executor": run_executor, "semantic": run_semantic}[group]()
    print("GROUP-DONE " + group, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])

"""The one-call leader job (prio3_leader_finish_job, PreparedBatch.leader_finish_job): the job
index in front of the coalesced prepare_next launch, the helper's prepare_error laid over the init
statuses inside it, the accumulate over the index's segment ids and the batch metadata behind it.

Every case asserts two things about the one call's outputs:
  (i)  they equal the four-move composition run through the library on the same batch -- the host
       overlay of prepare_error on the init status, prio3_job_index,
       prio3_leader_prepare_next_aggregate_batch over the index's segment ids and its accept bytes
       ANDed with the host mask, prio3_batch_metadata, dap.leader_outcome with the BatchCollected
       rule -- byte for byte;
  (ii) independently of the library, the index outputs equal tests/job_index_ref.job_index, the
       statuses, aggregate shares and counts equal Oracle.leader_batch (the C restatement of prio)
       fed the restatement's segment ids, and the checksums and intervals equal hashlib / numpy
       over the same rows.
Report data is made once per (instance, size) and shared; a case only chooses times, statuses and
the helper's errors."""
import functools
import threading

import numpy as np
import pytest

from janus_amd import dap
from tests import job_index_ref as R
from tests.conftest import CONFIGS
from tests.test_gpu_executor import _Held, _engine
from tests.test_gpu_helper_job import (BN, DUPS, MIDDLE_CLOSED, NO_SEG, PREC, TB, _bucket_case,
                                       _join_all, _meta_ref, _start_joined, _three_buckets)

pytestmark = pytest.mark.gpu

INDEX_KEYS = ("segment_ids", "reject", "duplicate", "n_segments", "overflow", "n_duplicates",
              "first_duplicate", "n_closed", "n_time_errors")
NO_ERROR = 0xFF
BATCH_COLLECTED = 0   # DAP PrepareError::BatchCollected
HELPER_REJECT = 2     # a DAP PrepareError the helper answered with (HpkeDecryptError)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import Oracle
    return Oracle(**CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _base(name, n, seed=0, vk=None):
    """n honest reports of the instance, the leader's input shares and the helper's prepare
    messages; never modified afterwards."""
    o = _oracle(name)
    vk = vk or bytes([0x50 + len(name)]) * 16
    d = o.gen_reports(vk, n, seed=2500 + n + seed, n_threads=4)
    eng = _engine(CONFIGS[name], vk)
    lin = eng.generate_reports_device(n, seed=2500 + n + seed, with_leader_inputs=True)
    lin = lin["leader_input_shares"].cpu().numpy()
    msgs = o.helper_batch(vk, d["nonces"], d["public_shares"], d["helper_shares"],
                          d["leader_prep_shares"], n_threads=4)[0].copy()
    for v in list(d.values()) + [lin, msgs]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return vk, d, lin, msgs


def _with_copies(d, lin, msgs, copies):
    """Whole reports copied: (src, dst) makes report dst a second upload of report src."""
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    lin, msgs = lin.copy(), msgs.copy()
    for src, dst in copies:
        for k in ("nonces", "public_shares"):
            d[k][dst] = d[k][src]
        lin[dst] = lin[src]
        msgs[dst] = msgs[src]
    return d, lin, msgs


def _failures(n, msgs, rng):
    """(prepare messages, leader_status override, prepare_error): a tampered prepare message, a
    non-zero init status, a helper Reject and a helper Finished (prepare_error 5) among the reports,
    as far as n has room for them (and the instance has prepare messages to tamper with)."""
    msgs = msgs.copy()
    ls = np.zeros(n, np.uint8)
    pe = np.full(n, NO_ERROR, np.uint8)
    rows = rng.permutation(n)[:5]
    if msgs.shape[1]:
        msgs[rows[0], 0] ^= 1
    if n >= 2:
        ls[rows[1]] = 6          # InputShareDecode at leader_initialized
    if n >= 3:
        pe[rows[2]] = HELPER_REJECT
    if n >= 4:
        pe[rows[3]] = dap.VDAF_PREP_ERROR  # the helper finished early: a mismatch for the leader
    if n >= 5:                   # both failed: the leader's own failure wins
        ls[rows[4]] = 1
        pe[rows[4]] = HELPER_REJECT
    return msgs, ls, pe


def _init(eng, d, lin):
    ps, lst, batch = eng.leader_prepare_init_batch(d["nonces"], d["public_shares"], lin)
    assert not lst.any()
    return batch


def _one_call(batch, d, times, ls, pe, msgs, precision, S, closed=None, mask=None):
    return batch.leader_finish_job(d["nonces"], times, ls, msgs, precision, S, prepare_error=pe,
                                   closed_intervals=closed, accept_mask=mask)


def _outcome(ls, pe, st, reject):
    out = np.array(dap.leader_outcome(ls, pe, st), np.uint8)
    out[(out == NO_ERROR) & (reject != 0)] = BATCH_COLLECTED
    return out


def _composition(eng, batch, d, times, ls, pe, msgs, precision, S, closed=None, mask=None):
    """The four moves through the library."""
    pe = np.full(len(ls), NO_ERROR, np.uint8) if pe is None else pe
    st_in = np.where(ls != 0, ls, np.where(pe != NO_ERROR, 5, 0)).astype(np.uint8)
    ji = eng.job_index(d["nonces"], times, precision, S, closed)
    acc = ji["accept_mask"] if mask is None else ji["accept_mask"] & (mask != 0).astype(np.uint8)
    st, agg, cnt = batch.leader_prepare_next_aggregate(msgs, st_in, ji["segment_ids"], acc, S)
    ck, iv = eng.batch_metadata(d["nonces"], times, st, acc, ji["segment_ids"], S)
    return dict(ji, status=st, agg=agg, counts=cnt, checksums=ck, intervals=iv,
                outcome=_outcome(ls, pe, st, ji["reject"]))


def _assert_equal_jobs(got, comp, precision):
    for k in INDEX_KEYS + ("status", "outcome", "agg", "counts", "checksums", "intervals"):
        np.testing.assert_array_equal(got[k], comp[k], err_msg=k)
    if precision:  # a fixed-size task has no starts (the array stays as the caller made it)
        np.testing.assert_array_equal(got["segment_starts"], comp["segment_starts"])


def _assert_reference(got, o, vk, d, lin, times, ls, pe, msgs, precision, S, closed, mask):
    """(ii): the restatements, independent of the library."""
    n = len(ls)
    pe = np.full(n, NO_ERROR, np.uint8) if pe is None else pe
    ref = R.job_index(d["nonces"], times, precision, S, closed)
    for k in INDEX_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    if precision:
        np.testing.assert_array_equal(got["segment_starts"], ref["segment_starts"])
    acc = ref["accept_mask"] if mask is None else ref["accept_mask"] & (mask != 0).astype(np.uint8)
    seg = ref["segment_ids"]
    # the restatement's leader makes the verdicts of prepare_next itself; a report the leader or
    # the helper had failed, or the index or the mask excludes, is out of every segment
    ok_in = (ls == 0) & (pe == NO_ERROR)
    rseg = np.where(ok_in & (acc != 0) & (seg != NO_SEG), seg, S).astype(np.uint32)
    _, rst, ragg, rcnt = o.leader_batch(vk, d["nonces"], d["public_shares"], lin, msgs,
                                        n_threads=4, segment_ids=rseg, n_segments=S)
    st = np.where(ls != 0, ls, np.where(pe != NO_ERROR, 5, rst)).astype(np.uint8)
    np.testing.assert_array_equal(got["status"], st)
    np.testing.assert_array_equal(got["agg"], ragg)
    np.testing.assert_array_equal(got["counts"], rcnt)
    ck, iv = _meta_ref(d["nonces"], times, seg, (st == 0) & (acc != 0), S)
    np.testing.assert_array_equal(got["checksums"], ck)
    np.testing.assert_array_equal(got["intervals"], iv)
    np.testing.assert_array_equal(got["outcome"], _outcome(ls, pe, st, ref["reject"]))
    if ref["overflow"]:
        assert not got["counts"].any() and not got["agg"].any() and not got["checksums"].any()
        assert (got["segment_ids"] == NO_SEG).all() and not got["intervals"].any()
    return ref, st


def _verify(eng, o, vk, d, lin, times, ls, pe, msgs, precision, S, closed=None, mask=None,
            batch=None):
    """Runs the one call on a fresh batch and asserts (i) and (ii); returns its outputs, the
    reference index, the reference statuses and the batch."""
    times = np.asarray(times).astype(np.uint64)
    batch = batch or _init(eng, d, lin)
    got = _one_call(batch, d, times, ls, pe, msgs, precision, S, closed, mask)
    _assert_equal_jobs(got, _composition(eng, batch, d, times, ls, pe, msgs, precision, S, closed,
                                         mask), precision)
    ref, st = _assert_reference(got, o, vk, d, lin, times, ls, pe, msgs, precision, S, closed,
                                mask)
    return got, ref, st, batch


# ---- instances and sizes -------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(nm, n) for nm in ("count", "hist_256_c16")
                                    for n in (1, 63, 64, 65, 255, 256, 257, 500)] +
                         [("sum32", 437), ("sumvec_8x10_c9", 437)])
def test_sizes(name, n):
    """Three batch intervals with the middle one closed, a host mask, a tampered prepare message,
    a non-zero init status, a helper Reject and a helper Finished, and a second upload of report
    0 at the end."""
    o = _oracle(name)
    vk, d, lin, msgs = _base(name, n)
    rng = np.random.default_rng(10 * n + len(name))
    d, lin, msgs = _with_copies(d, lin, msgs, [(0, n - 1)] if n > 2 else [])
    msgs, ls, pe = _failures(n, msgs, rng)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    eng = _engine(CONFIGS[name], vk)
    got, ref, st, batch = _verify(eng, o, vk, d, lin, _three_buckets(n, rng), ls, pe, msgs, PREC, 4,
                                  MIDDLE_CLOSED, mask)
    batch.free()
    if n >= 63:
        assert ref["n_segments"] == 3 and ref["n_closed"] > 0 and got["counts"][1] == 0
        assert ref["n_duplicates"] == 1 and ref["first_duplicate"] == n - 1
        assert got["counts"][3] == 0 and not got["intervals"][3].any()
        assert (got["status"] == 5).any() and (got["status"] == 6).any()
        assert (got["outcome"] == HELPER_REJECT).any() and (got["outcome"] == BATCH_COLLECTED).any()
        if msgs.shape[1]:
            assert (got["status"] == 4).sum() == 1
    if n >= 437:
        assert got["counts"][0] > 0 and got["counts"][2] > 0


def test_multiproof_takes_the_fallback():
    """Prio3SumVecField64MultiproofHmacSha256Aes128 shares no launch: the call runs the composition
    inside the entry point.  Against the composition through the library, the restated index,
    metadata and outcome; the aggregates against the helper's (they unshard to the column sums)."""
    from tests.test_gpu_client_shard_mp64 import P64, SHAPES, _inputs, _shard_device
    from tests.test_gpu_client_shard_mp64 import _engine as _mp_engine
    from janus_amd import prio3 as J
    shape = SHAPES[1]
    n, length = 65, shape[2]
    m, nonces, rand = _inputs(shape, n)
    eng = _mp_engine(shape)
    sh = _shard_device(eng, m, nonces, rand)
    pub = sh["public_shares"]
    d = dict(nonces=np.array(nonces), public_shares=pub)
    rng = np.random.default_rng(77)
    times = _three_buckets(n, rng)
    lps, lst, batch = eng.leader_prepare_init_batch(d["nonces"], pub, sh["leader_input_shares"])
    assert not lst.any()
    ref = R.job_index(d["nonces"], times, PREC, 3, MIDDLE_CLOSED)
    msgs, hst, hagg, hcnt = eng.prepare_aggregate_batch(
        d["nonces"], pub, sh["helper_shares"], lps, segment_ids=ref["segment_ids"],
        accept_mask=ref["accept_mask"], n_segments=3)
    ls = np.zeros(n, np.uint8)
    pe = np.full(n, NO_ERROR, np.uint8)
    s0 = eng.executor_stats(J.EXEC_LEADER_NEXT)
    got = _one_call(batch, d, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED)
    assert eng.executor_stats(J.EXEC_LEADER_NEXT)["jobs"] == s0["jobs"]  # not in the executor
    _assert_equal_jobs(got, _composition(eng, batch, d, times, ls, pe, msgs, PREC, 3,
                                         MIDDLE_CLOSED), PREC)
    batch.free()
    for k in INDEX_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert not got["status"].any() and not hst.any()
    np.testing.assert_array_equal(got["counts"], hcnt)
    ck, iv = _meta_ref(d["nonces"], times, ref["segment_ids"], ref["accept_mask"] != 0, 3)
    np.testing.assert_array_equal(got["checksums"], ck)
    np.testing.assert_array_equal(got["intervals"], iv)
    np.testing.assert_array_equal(got["outcome"], _outcome(ls, pe, got["status"], ref["reject"]))
    for s in range(3):
        dec = lambda a: [int.from_bytes(a[s, 8 * e:8 * e + 8].tobytes(), "little")  # noqa: E731
                         for e in range(length)]
        rows = (ref["segment_ids"] == s) & (ref["accept_mask"] != 0)
        want = [int(x) for x in m[rows].astype(object).sum(axis=0)] if rows.any() else [0] * length
        assert [(a + b) % P64 for a, b in zip(dec(got["agg"]), dec(hagg))] == want


@pytest.mark.parametrize("n,S,in_group", [(4096, 3, True), (4097, 3, False), (100, 65, False)])
def test_in_group_limits(n, S, in_group):
    """The largest in-group job is one job and one launch of the prepare_next executor; one report
    or one segment past the limits runs the composition inside the entry point (its
    prepare_next + aggregate is then that one job), with the same results."""
    from janus_amd import prio3 as J
    assert (J.JOB_GROUP_MAX_REPORTS, J.JOB_GROUP_MAX_SEGMENTS) == (4096, 64)
    o = _oracle("count")
    vk, d, lin, msgs = _base("count", n)
    rng = np.random.default_rng(n + S)
    d, lin, msgs = _with_copies(d, lin, msgs, [(1, n - 2)])
    msgs, ls, pe = _failures(n, msgs, rng)
    times = _three_buckets(n, rng)
    eng = _engine(CONFIGS["count"], vk)
    batch = _init(eng, d, lin)
    s0 = eng.executor_stats(J.EXEC_LEADER_NEXT)
    got = _one_call(batch, d, times, ls, pe, msgs, PREC, S, MIDDLE_CLOSED)
    s1 = eng.executor_stats(J.EXEC_LEADER_NEXT)
    assert s1["jobs"] - s0["jobs"] == 1 and s1["groups"] - s0["groups"] == 1
    again, _, _, _ = _verify(eng, o, vk, d, lin, times, ls, pe, msgs, PREC, S, MIDDLE_CLOSED,
                             batch=batch)
    batch.free()
    for k, v in got.items():
        assert np.asarray(v).tobytes() == np.asarray(again[k]).tobytes(), k
    assert got["n_duplicates"] == 1 and got["first_duplicate"] == n - 2


# ---- buckets -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one", "middle_closed", "alternating", "exactly_max", "overflow",
                                  "precision_0", "precision_1", "time_overflow",
                                  "closed_ends_at_start", "k0"])
def test_buckets(case):
    o = _oracle("count")
    vk, d, lin, msgs = _base("count", BN)
    rng = np.random.default_rng(len(case) * 31 + 1)
    times, precision, S, closed = _bucket_case(case, rng)
    msgs, ls, pe = _failures(BN, msgs, np.random.default_rng(len(case)))
    got, ref, st, batch = _verify(_engine(CONFIGS["count"], vk), o, vk, d, lin, times, ls, pe, msgs,
                                  precision, S, closed)
    batch.free()
    if case == "overflow":
        assert ref["overflow"] == 1 and got["n_segments"] == S + 1
        assert (got["status"] == 0).sum() * 4 >= BN  # the statuses stay valid
        assert not (got["outcome"] == BATCH_COLLECTED).any()
    if case == "exactly_max":
        assert got["n_segments"] == S and got["counts"][4] == 0 and got["counts"][:4].all()
    if case == "precision_0":
        assert got["n_segments"] == 1 and got["n_closed"] == 0 and got["counts"][0] > 0
    if case == "precision_1":
        assert got["n_segments"] == 64 and got["n_closed"] > 0
    if case == "time_overflow":
        assert got["n_time_errors"] == 3 and got["segment_ids"][4] == NO_SEG
        assert got["n_segments"] == 4 and got["segment_ids"][100] == 3
    if case == "closed_ends_at_start":
        assert got["counts"][0] == 0 and got["counts"][1] > 0 and got["counts"][2] > 0


# ---- duplicates ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(DUPS))
def test_duplicates(case):
    """A duplicate ID marks a report and rejects nothing; two runs give byte-identical outputs."""
    o = _oracle("count")
    vk, d, lin, msgs = _base("count", BN)
    rng = np.random.default_rng(len(case))
    d, lin, msgs = _with_copies(d, lin, msgs, DUPS[case])
    ls, pe = np.zeros(BN, np.uint8), np.full(BN, NO_ERROR, np.uint8)
    times = _three_buckets(BN, rng)
    eng = _engine(CONFIGS["count"], vk)
    got, ref, st, batch = _verify(eng, o, vk, d, lin, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED)
    marked = sorted({b for _, b in DUPS[case]})
    assert list(np.flatnonzero(got["duplicate"])) == marked
    assert got["n_duplicates"] == len(marked) and got["first_duplicate"] == marked[0]
    # nothing is rejected for it: every finished report of an open batch is counted
    assert got["counts"].sum() == ((st == 0) & (ref["accept_mask"] != 0)).sum()
    again = _one_call(batch, d, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED)
    batch.free()
    for k, v in got.items():
        assert np.asarray(v).tobytes() == np.asarray(again[k]).tobytes(), k


# ---- the host mask, the outcome, the batch afterwards ----------------------------------------
def test_host_accept_mask_and_outcome():
    """The mask is ANDed with the index's accept bytes: a masked report is in no aggregate, count
    or checksum, but it still widens its batch's interval.  A report the helper rejected that is
    also in a closed batch keeps the helper's error; its finished neighbours get BatchCollected."""
    name, n = "hist_256_c16", 437
    o = _oracle(name)
    vk, d, lin, msgs = _base(name, n)
    rng = np.random.default_rng(4370)
    times = _three_buckets(n, rng)
    times[10], times[12] = TB + 2 * PREC, TB + 3 * PREC - 1  # the ends of the third interval
    times[20], times[21] = TB + PREC + 1, TB + PREC + 2      # two reports of the closed batch
    ls, pe = np.zeros(n, np.uint8), np.full(n, NO_ERROR, np.uint8)
    pe[20] = HELPER_REJECT
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[[10, 12]] = 0
    eng = _engine(CONFIGS[name], vk)
    got, ref, st, b1 = _verify(eng, o, vk, d, lin, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED,
                               mask)
    full, _, _, b2 = _verify(eng, o, vk, d, lin, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED, None)
    b1.free()
    b2.free()
    assert st[10] == 0 and st[12] == 0 and ref["segment_ids"][10] == 2
    assert got["counts"][2] < full["counts"][2]
    assert got["counts"][2] == ((st == 0) & (mask != 0) & (ref["segment_ids"] == 2)).sum()
    np.testing.assert_array_equal(got["intervals"], full["intervals"])
    np.testing.assert_array_equal(got["intervals"][2], [TB + 2 * PREC, PREC])
    assert got["checksums"][2].tobytes() != full["checksums"][2].tobytes()
    np.testing.assert_array_equal(got["status"], full["status"])
    assert got["reject"][20] and got["reject"][21]
    assert got["outcome"][20] == HELPER_REJECT and got["outcome"][21] == BATCH_COLLECTED
    assert got["outcome"][10] == NO_ERROR  # masked out by the host: not an error of the report


@pytest.mark.parametrize("name", ["hist_256_c16", "sum32"])
def test_batch_keeps_its_output_shares(name):
    """prio3_accumulate over the call's segment ids and accept bytes gives the same aggregates."""
    n = 437
    o = _oracle(name)
    vk, d, lin, msgs = _base(name, n)
    rng = np.random.default_rng(99)
    msgs, ls, pe = _failures(n, msgs, rng)
    times = _three_buckets(n, rng)
    got, ref, st, batch = _verify(_engine(CONFIGS[name], vk), o, vk, d, lin, times, ls, pe, msgs,
                                  PREC, 3, MIDDLE_CLOSED)
    again = _one_call(batch, d, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED)
    agg, cnt = batch.accumulate(again["segment_ids"], ref["accept_mask"], 3)
    batch.free()
    np.testing.assert_array_equal(agg, got["agg"])
    np.testing.assert_array_equal(cnt, got["counts"])


# ---- coalescing ----------------------------------------------------------------------------
def test_concurrent_jobs_are_coalesced():
    """16 indexed jobs of 4 tasks and 4 plain leader_prepare_next_aggregate jobs queued behind the
    prepare_next executor's hold: different precisions, closed sets, max_segments and sizes.
    Indexed and plain jobs never share a group, the executor launched fewer groups than it took
    jobs, and every job equals its composition and the references."""
    from janus_amd import prio3 as J
    name = "hist_256_c16"
    o = _oracle(name)
    rng = np.random.default_rng(1616)
    vks = [bytes([0xA1 + t]) * 16 for t in range(4)]
    engines = [_engine(CONFIGS[name], vk) for vk in vks]
    jobs = []
    for j in range(20):
        t, n = j % 4, int(rng.integers(100, 501))
        _, d, lin, msgs = _base(name, n, seed=j, vk=vks[t])
        msgs, ls, pe = _failures(n, msgs, rng)
        precision = (PREC, 300, 0, 1 << 40)[j % 4]
        span = 3 * precision if 0 < precision <= PREC else 900
        times = (TB + rng.integers(0, span, n)).astype(np.uint64)
        closed = (None, [[TB + precision, precision]], [[TB, 1], [TB + 2 * precision, 5]])[j % 3]
        S = (3, 4, 7, 2)[(j // 4) % 4]  # 2 with three intervals: an overflowing job
        mask = None if j % 2 else (rng.random(n) < 0.9).astype(np.uint8)
        jobs.append((t, d, lin, msgs, ls, pe, times, precision, S, closed, mask))
    batches = [_init(engines[t], d, lin) for (t, d, lin, *_) in jobs]
    out = [None] * len(jobs)

    def run(j):
        t, d, lin, msgs, ls, pe, times, precision, S, closed, mask = jobs[j]
        if j < 16:
            out[j] = _one_call(batches[j], d, times, ls, pe, msgs, precision, S, closed, mask)
        else:
            seg = (np.arange(len(ls)) % 2).astype(np.uint32)
            out[j] = batches[j].leader_prepare_next_aggregate(msgs, ls, seg, mask, 2)

    s0 = engines[0].executor_stats(J.EXEC_LEADER_NEXT)
    with _Held(engines[0], len(jobs), J.EXEC_LEADER_NEXT) as h:
        th = _start_joined([threading.Thread(target=run, args=(j,), daemon=True)
                            for j in range(len(jobs))])
        h.wait()
        _join_all(th)
    s1 = engines[0].executor_stats(J.EXEC_LEADER_NEXT)
    assert s1["jobs"] - s0["jobs"] == len(jobs)
    # indexed and plain jobs never share a launch (at least two groups), and jobs are coalesced
    assert 2 <= s1["groups"] - s0["groups"] < len(jobs), (s0, s1)
    overflowed = 0
    for j, (t, d, lin, msgs, ls, pe, times, precision, S, closed, mask) in enumerate(jobs):
        assert out[j] is not None
        if j < 16:
            _assert_equal_jobs(out[j], _composition(engines[t], batches[j], d, times, ls, pe, msgs,
                                                    precision, S, closed, mask), precision)
            ref, _ = _assert_reference(out[j], o, vks[t], d, lin, times, ls, pe, msgs, precision, S,
                                       closed, mask)
            overflowed += ref["overflow"]
        else:
            seg = (np.arange(len(ls)) % 2).astype(np.uint32)
            acc = np.ones(len(ls), bool) if mask is None else mask != 0
            _, rst, ragg, rcnt = o.leader_batch(
                vks[t], d["nonces"], d["public_shares"], lin, msgs, n_threads=4,
                segment_ids=np.where(acc & (ls == 0), seg, 2), n_segments=2)
            np.testing.assert_array_equal(out[j][0], np.where(ls != 0, ls, rst))
            np.testing.assert_array_equal(out[j][1], ragg)
            np.testing.assert_array_equal(out[j][2], rcnt)
        batches[j].free()
    assert 0 < overflowed < 16


def test_one_engine_over_two_executors():
    """Eight concurrent jobs on an engine over the device list [0, 0]: wherever a batch was placed
    its job equals the composition and the references."""
    from janus_amd import prio3 as J
    name = "hist_256_c16"
    o = _oracle(name)
    vk = bytes([0x3F]) * 16
    rng = np.random.default_rng(1701)
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, devices=[0, 0])
    jobs = []
    for j in range(8):
        n = int(rng.integers(100, 400))
        _, d, lin, msgs = _base(name, n, seed=40 + j, vk=vk)
        msgs, ls, pe = _failures(n, msgs, rng)
        jobs.append((d, lin, msgs, ls, pe, _three_buckets(n, rng)))
    batches = [_init(eng, d, lin) for (d, lin, *_) in jobs]
    out = [None] * 8

    def run(j):
        d, lin, msgs, ls, pe, times = jobs[j]
        out[j] = _one_call(batches[j], d, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED)

    _join_all(_start_joined([threading.Thread(target=run, args=(j,), daemon=True)
                             for j in range(8)]))
    for j, (d, lin, msgs, ls, pe, times) in enumerate(jobs):
        assert out[j] is not None
        _assert_equal_jobs(out[j], _composition(eng, batches[j], d, times, ls, pe, msgs, PREC, 3,
                                                MIDDLE_CLOSED), PREC)
        _assert_reference(out[j], o, vk, d, lin, times, ls, pe, msgs, PREC, 3, MIDDLE_CLOSED, None)
        batches[j].free()


# ---- arguments -----------------------------------------------------------------------------
def test_empty_job():
    """n == 0 succeeds with the composition's outputs: zero rows, an all-zero info except
    first_duplicate."""
    vk = bytes([0x23]) * 16
    eng = _engine(CONFIGS["count"], vk)
    z = lambda *s, t=np.uint8: np.zeros(s, t)  # noqa: E731
    ps, lst, batch = eng.leader_prepare_init_batch(z(0, 16), z(0, 0),
                                                   z(0, eng.sz.leader_input_share_len))
    got = batch.leader_finish_job(z(0, 16), z(0, t=np.uint64), z(0), None, PREC, 3,
                                  prepare_error=z(0), closed_intervals=MIDDLE_CLOSED)
    batch.free()
    assert got["n_segments"] == 0 and got["overflow"] == 0 and got["n_duplicates"] == 0
    assert got["first_duplicate"] == NO_SEG and got["n_closed"] == 0
    for k in ("agg", "counts", "checksums", "intervals", "segment_starts"):
        assert got[k].shape[0] == 3 and not got[k].any(), k
    assert got["status"].shape == (0,) and got["outcome"].shape == (0,)


def test_argument_errors():
    """max_segments 0 and 4,097, k = 1,025 and a missing required buffer return PRIO3_EINVAL
    before anything is launched: the executor takes no job."""
    import ctypes as C
    from janus_amd import prio3 as J
    n = 63
    vk, d, lin, msgs = _base("hist_256_c16", n)
    eng = _engine(CONFIGS["hist_256_c16"], vk)
    batch = _init(eng, d, lin)
    rng = np.random.default_rng(6)
    times = _three_buckets(n, rng)
    ls, pe = np.zeros(n, np.uint8), np.full(n, NO_ERROR, np.uint8)
    s0 = eng.executor_stats(J.EXEC_LEADER_NEXT)
    for kw in (dict(S=0), dict(S=4097), dict(closed=np.zeros((1025, 2), np.uint64))):
        with pytest.raises(RuntimeError, match=r"rc=-1\)"):
            _one_call(batch, d, times, ls, pe, msgs, PREC, kw.get("S", 3), kw.get("closed"))
    with pytest.raises(ValueError):
        _one_call(batch, d, times, ls, pe, msgs, PREC, 3, None, np.ones(5, np.uint8))
    # a missing required buffer, through the C ABI itself
    seg, st = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    agg, cnt = np.zeros((3, eng.sz.agg_share_len), np.uint8), np.zeros(3, np.uint64)
    info = J.Prio3JobIndexInfo()
    ids = np.ascontiguousarray(d["nonces"])
    full_in = dict(report_ids=ids.ctypes.data, times=times.ctypes.data,
                   leader_status=ls.ctypes.data, prepare_error=pe.ctypes.data,
                   prep_msgs=np.ascontiguousarray(msgs).ctypes.data, time_precision=PREC,
                   closed_intervals=None, accept_mask=None, k=0, max_segments=3)
    full_out = dict(segment_ids=seg.ctypes.data, info=C.addressof(info), status=st.ctypes.data,
                    agg_shares=agg.ctypes.data, counts=cnt.ctypes.data)
    call = J.load_library().prio3_leader_finish_job
    for missing in ("report_ids", "times", "leader_status", "prep_msgs"):
        jin = J.Prio3LeaderJobIn(**dict(full_in, **{missing: None}))
        assert call(batch.handle, C.byref(jin), C.byref(J.Prio3LeaderJobOut(**full_out))) == -1
    for missing in ("segment_ids", "info", "status", "agg_shares", "counts"):
        jout = J.Prio3LeaderJobOut(**dict(full_out, **{missing: None}))
        assert call(batch.handle, C.byref(J.Prio3LeaderJobIn(**full_in)), C.byref(jout)) == -1
    assert call(None, C.byref(J.Prio3LeaderJobIn(**full_in)),
                C.byref(J.Prio3LeaderJobOut(**full_out))) == -1
    assert eng.executor_stats(J.EXEC_LEADER_NEXT)["jobs"] == s0["jobs"]
    assert call(batch.handle, C.byref(J.Prio3LeaderJobIn(**full_in)),
                C.byref(J.Prio3LeaderJobOut(**full_out))) == 0  # and the full set succeeds
    batch.free()

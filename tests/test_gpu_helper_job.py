"""The one-call helper job (prio3_helper_aggregate_job, HelperEngine.aggregate_job): the job index
in front of the coalesced group launch and the batch metadata behind its accumulate.

Every case asserts two things about the one call's outputs:
  (i)  they equal the three-call composition run through the library on the same inputs --
       prio3_job_index, prio3_helper_aggregate_init_batch_ex over the index's segment ids and its
       accept bytes ANDed with the host mask, prio3_batch_metadata -- byte for byte (prepare
       messages on the rows where they are defined: status < 0x80);
  (ii) independently of the library, the index outputs equal tests/job_index_ref.job_index, the
       statuses, aggregate shares and counts equal tests/test_gpu_init_contract._expected_ex (the
       OpenSSL HPKE oracle and the C restatement of prio) fed the restatement's segment ids and
       accept bytes, and the checksums and intervals equal hashlib / numpy over the same rows.
Report data is made once per (instance, size) and shared; a case only chooses times and reseals."""
import functools
import hashlib
import threading

import numpy as np
import pytest

from tests import job_index_ref as R
from tests.conftest import CONFIGS
from tests.test_gpu_executor import _Held, _engine
from tests.test_gpu_init_contract import (MP_CASES, NO_DEADLINE, VK32, _call, _check, _expected_ex,
                                          _job, _keys, _mp_reports)
from tests.test_gpu_parity import _tamper

pytestmark = pytest.mark.gpu

PREC = 1200
TB = 1_699_999_200  # a multiple of PREC: TB + [0, 3 PREC) is exactly three batch intervals
assert TB % PREC == 0
NO_SEG = 0xFFFFFFFF
JOIN_S = 120.0


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import Oracle
    return Oracle(**CONFIGS[name])


@functools.lru_cache(maxsize=None)
def _base(name, n, seed=0):
    """n reports of the instance with the VDAF failures of _tamper; never modified afterwards."""
    o = _oracle(name)
    vk = bytes([0x30 + len(name)]) * 16
    d = o.gen_reports(vk, n, seed=500 + n + seed, n_threads=4)
    if n > 1:
        d = _tamper(o, d, np.random.default_rng(n + seed))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return vk, d


@functools.lru_cache(maxsize=None)
def _keyset():
    rng = np.random.default_rng(0x6A6F62)
    return _keys(rng, 3), bytes(rng.integers(0, 256, 32, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _openers():
    from janus_amd import hpke as G
    keys, _ = _keyset()
    return tuple(G.HpkeOpener(k[0], k[1], device=0) for k in keys)


def _with_copies(d, copies):
    """d with whole reports copied: (src, dst) makes report dst a second upload of report src."""
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    for src, dst in copies:
        for k in ("nonces", "public_shares", "helper_shares", "leader_prep_shares"):
            d[k][dst] = d[k][src]
    return d


def _seal(o, vk, d, times, rng, row_key=None, tamper=True):
    n = d["nonces"].shape[0]
    keys, task = _keyset()
    rk = np.zeros(n, int) if row_key is None else row_key
    return _job(o, vk, n, 900 + n, rng, task, [k[1] for k in keys], rk,
                times=np.asarray(times, np.uint64), tamper=tamper, d=d)


def _three_buckets(n, rng):
    t = (TB + rng.integers(0, 3 * PREC, n)).astype(np.uint64)
    if n >= 3:
        t[:3] = [TB + 5, TB + PREC + 5, TB + 2 * PREC + 5]
    return t


MIDDLE_CLOSED = np.array([[TB + PREC, PREC]], np.uint64)


def _meta_ref(ids, times, seg, counted, S):
    ck = np.zeros((S, 32), np.uint8)
    iv = np.zeros((S, 2), np.uint64)
    for s in range(S):
        rows = np.flatnonzero(seg == s)
        if len(rows):
            lo, hi = int(times[rows].min()), int(times[rows].max()) + 1
            iv[s] = (lo, hi - lo)
        for r in rows[counted[rows]]:
            ck[s] ^= np.frombuffer(hashlib.sha256(ids[r].tobytes()).digest(), np.uint8)
    return ck, iv


def _job_call(eng, op, d, precision, S, closed=None, mask=None, fb=None, deadline=None):
    _, task = _keyset()
    return eng.aggregate_job(op, task, d["nonces"], d["times"], d["public_shares"], d["enc"],
                             d["ct"], d["ct_len"], d["leader_prep_shares"], precision, S,
                             closed_intervals=closed, accept_mask=mask, fallback_opener=fb,
                             report_deadline=deadline)


INDEX_KEYS = ("segment_ids", "reject", "duplicate", "n_segments", "overflow", "n_duplicates",
              "first_duplicate", "n_closed", "n_time_errors")


def _composition(eng, op, d, precision, S, closed=None, mask=None, fb=None, deadline=None):
    """The three calls through the library."""
    _, task = _keyset()
    ji = eng.job_index(d["nonces"], d["times"], precision, S, closed)
    acc = ji["accept_mask"] if mask is None else ji["accept_mask"] & (mask != 0).astype(np.uint8)
    msgs, st, agg, cnt = _call(eng, op, task, d, ji["segment_ids"], acc, S, fallback_opener=fb,
                               report_deadline=NO_DEADLINE if deadline is None else deadline)
    ck, iv = eng.batch_metadata(d["nonces"], d["times"], st, acc, ji["segment_ids"], S)
    return dict(ji, prep_msgs=msgs, status=st, agg=agg, counts=cnt, checksums=ck, intervals=iv)


def _assert_equal_jobs(got, comp, precision):
    for k in INDEX_KEYS + ("status", "agg", "counts", "checksums", "intervals"):
        np.testing.assert_array_equal(got[k], comp[k], err_msg=k)
    if precision:  # a fixed-size task has no starts (the array stays as the caller made it)
        np.testing.assert_array_equal(got["segment_starts"], comp["segment_starts"])
    ok = comp["status"] < 0x80
    np.testing.assert_array_equal(got["prep_msgs"][ok], comp["prep_msgs"][ok])


def _verify(eng, o, vk, d, precision, S, closed=None, mask=None, fb=False, deadline=None,
            opener=0):
    """Runs the one call and asserts (i) and (ii); returns its outputs and the reference index."""
    keys, task = _keyset()
    ops = _openers()
    op, fbo = ops[opener], (ops[1] if fb else None)
    got = _job_call(eng, op, d, precision, S, closed, mask, fbo, deadline)
    _assert_equal_jobs(got, _composition(eng, op, d, precision, S, closed, mask, fbo, deadline),
                       precision)
    ref = R.job_index(d["nonces"], d["times"], precision, S, closed)
    for k in INDEX_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    if precision:
        np.testing.assert_array_equal(got["segment_starts"], ref["segment_starts"])
    acc = ref["accept_mask"] if mask is None else ref["accept_mask"] & (mask != 0).astype(np.uint8)
    seg = ref["segment_ids"]
    exp = _expected_ex(o, vk, d, task, keys[opener], keys[1] if fb else None,
                       NO_DEADLINE if deadline is None else deadline,
                       np.where(seg == NO_SEG, 0, seg).astype(np.uint32), acc, S, quarter=False)
    _check((got["prep_msgs"], got["status"], got["agg"], got["counts"]), exp)
    ck, iv = _meta_ref(d["nonces"], d["times"], seg, (exp[1] == 0) & (acc != 0), S)
    np.testing.assert_array_equal(got["checksums"], ck)
    np.testing.assert_array_equal(got["intervals"], iv)
    if ref["overflow"]:
        assert not got["counts"].any() and not got["agg"].any() and not got["checksums"].any()
        assert (got["segment_ids"] == NO_SEG).all() and not got["intervals"].any()
    return got, ref, exp


# ---- instances and sizes -------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(nm, n) for nm in ("count", "hist_256_c16")
                                    for n in (1, 63, 64, 65, 437, 500)] + [("sum32", 437)])
def test_sizes(name, n):
    """Three batch intervals with the middle one closed, a host mask, every failure kind of the
    VDAF and of the open, and a second upload of report 0 at the end."""
    o = _oracle(name)
    vk, base = _base(name, n)
    rng = np.random.default_rng(10 * n + len(name))
    d = _seal(o, vk, _with_copies(base, [(0, n - 1)] if n > 2 else []), _three_buckets(n, rng),
              rng)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    got, ref, _ = _verify(_engine(CONFIGS[name], vk), o, vk, d, PREC, 4, MIDDLE_CLOSED, mask)
    if n >= 3:
        assert ref["n_segments"] == 3 and ref["n_closed"] > 0 and got["counts"][1] == 0
        assert ref["n_duplicates"] == 1 and ref["first_duplicate"] == n - 1
        assert got["counts"][3] == 0 and not got["intervals"][3].any()
    if n >= 437:
        assert got["counts"][0] > 0 and got["counts"][2] > 0


def test_multiproof():
    """Prio3SumVecField64MultiproofHmacSha256Aes128: 64-byte public shares, an engine that shares
    no launch; its 16 distinct reports tiled, so most IDs are duplicates."""
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    proofs, bits, length, chunk, _ = MP_CASES[1]
    n = 65
    o = Oracle("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk, num_proofs=proofs)
    rng = np.random.default_rng(77)
    d = _seal(o, VK32, _mp_reports(proofs, bits, length, chunk, n), _three_buckets(n, rng), rng)
    eng = J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(proofs, bits, length,
                                                                         chunk), VK32)
    got, ref, _ = _verify(eng, o, VK32, d, PREC, 3, MIDDLE_CLOSED)
    assert ref["n_duplicates"] == n - 16 and ref["first_duplicate"] == 16


@pytest.mark.parametrize("n,S", [(4096, 3), (4097, 3), (100, 65)])
def test_in_group_limits(n, S):
    """The largest in-group job, and one report / one segment past the limits: those two run the
    three calls inside the entry point, with the same results."""
    from janus_amd import prio3 as J
    assert (J.JOB_GROUP_MAX_REPORTS, J.JOB_GROUP_MAX_SEGMENTS) == (4096, 64)
    o = _oracle("count")
    vk, base = _base("count", n)
    rng = np.random.default_rng(n + S)
    d = _seal(o, vk, _with_copies(base, [(1, n - 2)]), _three_buckets(n, rng), rng)
    eng = _engine(CONFIGS["count"], vk)
    s0 = eng.executor_stats(0)
    got = _job_call(eng, _openers()[0], d, PREC, S, MIDDLE_CLOSED)
    s1 = eng.executor_stats(0)
    # in-group: one job, one launch, nothing else; outside: the _ex call inside is that one job
    assert s1["jobs"] - s0["jobs"] == 1 and s1["groups"] - s0["groups"] == 1
    _verify(eng, o, vk, d, PREC, S, MIDDLE_CLOSED)
    assert got["n_duplicates"] == 1 and got["first_duplicate"] == n - 2


# ---- buckets -------------------------------------------------------------------------------
BN = 200


def _bucket_case(case, rng):
    """(times, precision, max_segments, closed intervals)"""
    n = BN
    if case == "one":
        return TB + rng.integers(0, PREC, n), PREC, 2, None
    if case == "middle_closed":
        return _three_buckets(n, rng), PREC, 3, MIDDLE_CLOSED
    if case == "alternating":
        return TB + PREC * (np.arange(n) % 2) + 7, PREC, 2, None
    if case == "exactly_max":
        return TB + PREC * (np.arange(n) % 5), PREC, 5, [[TB + 4 * PREC, 1]]
    if case == "overflow":
        return TB + PREC * (np.arange(n) % 6), PREC, 5, [[TB, 10 * PREC]]
    if case == "precision_0":
        return TB + rng.integers(0, 3 * PREC, n), 0, 3, [[0, (1 << 64) - 1]]
    if case == "precision_1":
        return TB + (np.arange(n) % 64), 1, 64, [[TB + 3, 2]]
    if case == "time_overflow":
        t = _three_buckets(n, rng)
        # 2^64 - 1 = 15 mod PREC: the interval of a start of 2^64 - 16 would end past a u64 --
        # and the one before it, [2^64 - 1216, 2^64 - 16), is the last that fits
        t[[4, 70, n - 1]] = np.uint64((1 << 64) - 1) - np.array([0, 5, 15], np.uint64)
        t[100] = np.uint64((1 << 64) - 17)
        return t, PREC, 4, None
    if case == "closed_ends_at_start":
        # [TB, TB + PREC) ends exactly where the second bucket starts: only the first is closed
        return _three_buckets(n, rng), PREC, 3, [[TB, PREC], [TB + 3 * PREC, PREC]]
    assert case == "k0"
    return _three_buckets(n, rng), PREC, 3, None


@pytest.mark.parametrize("case", ["one", "middle_closed", "alternating", "exactly_max", "overflow",
                                  "precision_0", "precision_1", "time_overflow",
                                  "closed_ends_at_start", "k0"])
def test_buckets(case):
    o = _oracle("count")
    vk, base = _base("count", BN)
    rng = np.random.default_rng(len(case) * 31 + 1)
    times, precision, S, closed = _bucket_case(case, rng)
    d = _seal(o, vk, base, np.asarray(times).astype(np.uint64), rng)
    got, ref, _ = _verify(_engine(CONFIGS["count"], vk), o, vk, d, precision, S, closed)
    if case == "overflow":
        assert ref["overflow"] == 1 and got["n_segments"] == S + 1
        assert (got["status"] == 0).sum() * 4 >= BN  # statuses and prepare messages stay valid
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
DUPS = {"inside_a_wave": [(3, 9)], "across_waves": [(5, 130)], "first_and_last": [(0, BN - 1)],
        "three_copies": [(3, 7), (3, 9)], "all_equal": [(0, i) for i in range(1, BN)]}


@pytest.mark.parametrize("case", list(DUPS))
def test_duplicates(case):
    """A duplicate ID marks a report and rejects nothing; two runs give byte-identical outputs."""
    o = _oracle("count")
    vk, base = _base("count", BN)
    rng = np.random.default_rng(len(case))
    d = _seal(o, vk, _with_copies(base, DUPS[case]), _three_buckets(BN, rng), rng,
              tamper=case != "all_equal")
    eng = _engine(CONFIGS["count"], vk)
    got, ref, exp = _verify(eng, o, vk, d, PREC, 3, MIDDLE_CLOSED)
    marked = sorted({b for _, b in DUPS[case]})
    assert list(np.flatnonzero(got["duplicate"])) == marked
    assert got["n_duplicates"] == len(marked) and got["first_duplicate"] == marked[0]
    # nothing is rejected for it: every finished report of an open batch is counted
    assert got["counts"].sum() == ((exp[1] == 0) & (ref["accept_mask"] != 0)).sum()
    again = _job_call(eng, _openers()[0], d, PREC, 3, MIDDLE_CLOSED)
    for k, v in got.items():
        assert np.asarray(v).tobytes() == np.asarray(again[k]).tobytes(), k


# ---- the host mask and the _ex contract inside the job ---------------------------------------
def test_host_accept_mask():
    """The mask is ANDed with the index's accept bytes: a masked report is in no aggregate, count
    or checksum, but it still widens its batch's interval."""
    name, n = "hist_256_c16", 437
    o = _oracle(name)
    vk, base = _base(name, n)
    rng = np.random.default_rng(4370)
    times = _three_buckets(n, rng)
    # the ends of the third interval, on two rows the VDAF tampering leaves alone
    times[10], times[12] = TB + 2 * PREC, TB + 3 * PREC - 1
    d = _seal(o, vk, base, times, rng, tamper=False)
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[[10, 12]] = 0
    eng = _engine(CONFIGS[name], vk)
    got, ref, exp = _verify(eng, o, vk, d, PREC, 3, MIDDLE_CLOSED, mask)
    full, _, _ = _verify(eng, o, vk, d, PREC, 3, MIDDLE_CLOSED, None)
    assert exp[1][10] == 0 and exp[1][12] == 0 and ref["segment_ids"][10] == 2
    assert got["counts"][2] < full["counts"][2]
    assert got["counts"][2] == ((exp[1] == 0) & (mask != 0) & (ref["segment_ids"] == 2)).sum()
    np.testing.assert_array_equal(got["intervals"], full["intervals"])
    np.testing.assert_array_equal(got["intervals"][2], [TB + 2 * PREC, PREC])
    assert got["checksums"][2].tobytes() != full["checksums"][2].tobytes()
    np.testing.assert_array_equal(got["status"], full["status"])


def test_tampered_fallback_and_deadline_in_the_job():
    """Tampered ciphertexts, rows sealed to the fallback keypair and to a third one, a report
    deadline: rejected reports are in no count or checksum and in their batch's interval."""
    name, n = "hist_256_c16", 437
    o = _oracle(name)
    vk, base = _base(name, n)
    rng = np.random.default_rng(4371)
    row_key = rng.integers(0, 2, n)
    row_key[rng.choice(n, 9, replace=False)] = 2
    times = _three_buckets(n, rng)
    d = _seal(o, vk, base, times, rng, row_key=row_key)
    deadline = TB + 3 * PREC - 400
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    got, ref, exp = _verify(_engine(CONFIGS[name], vk), o, vk, d, PREC, 3, MIDDLE_CLOSED, mask,
                            fb=True, deadline=deadline)
    for c in (0, 3, 0x84, 0x88, 0x89):
        assert (got["status"] == c).any(), hex(c)
    assert ((exp[6] == 4) & (exp[4] == 0)).any()  # a row only the fallback keypair opens
    late = np.flatnonzero(got["status"] == 0x89)
    assert (ref["segment_ids"][late] == 2).all()
    iv = got["intervals"][2]
    assert int(iv[0]) + int(iv[1]) - 1 == int(times[ref["segment_ids"] == 2].max()) > deadline


# ---- coalescing ----------------------------------------------------------------------------
def _start_joined(threads):
    for x in threads:
        x.start()
    return threads


def _join_all(threads):
    for x in threads:
        x.join(JOIN_S)
    assert not any(x.is_alive() for x in threads), "a job did not return"


def test_concurrent_jobs_are_coalesced():
    """18 indexed jobs of 3 tasks and 4 _ex jobs queued behind the executor's hold: different
    precisions, closed sets, max_segments and sizes.  Every job equals its own composition and the
    references, and the executor launched fewer groups than it took jobs."""
    name = "hist_256_c16"
    o = _oracle(name)
    keys, task = _keyset()
    rng = np.random.default_rng(1818)
    vks = [bytes([0x71 + t]) * 16 for t in range(3)]
    engines = [_engine(CONFIGS[name], vk) for vk in vks]
    op = _openers()[0]
    jobs = []
    for j in range(22):
        t, n = j % 3, int(rng.integers(100, 501))
        dd = o.gen_reports(vks[t], n, seed=1800 + j, n_threads=4)
        if j % 4 != 3:
            dd = _tamper(o, dd, rng)
        precision = (PREC, 300, 0, 1 << 40)[j % 4]
        span = 3 * precision if 0 < precision <= PREC else 900
        times = (TB + rng.integers(0, span, n)).astype(np.uint64)
        d = _job(o, vks[t], n, 1800 + j, rng, task, [keys[0][1]], np.zeros(n, int), times=times,
                 tamper=j % 4 != 3, d=dd)
        closed = (None, [[TB + precision, precision]], [[TB, 1], [TB + 2 * precision, 5]])[j % 3]
        S = (3, 4, 7, 2)[(j // 3) % 4]  # 2 with three intervals: an overflowing job
        mask = None if j % 2 else (rng.random(n) < 0.9).astype(np.uint8)
        jobs.append((t, d, precision, S, closed, mask))
    out = [None] * len(jobs)

    def run(j):
        t, d, precision, S, closed, mask = jobs[j]
        if j < 18:
            out[j] = _job_call(engines[t], op, d, precision, S, closed, mask)
        else:
            seg = (np.arange(d["nonces"].shape[0]) % 2).astype(np.uint32)
            out[j] = _call(engines[t], op, task, d, seg, mask, 2, report_deadline=NO_DEADLINE)

    s0 = engines[0].executor_stats(0)
    with _Held(engines[0], len(jobs)) as h:
        th = _start_joined([threading.Thread(target=run, args=(j,), daemon=True)
                            for j in range(len(jobs))])
        h.wait()
        _join_all(th)
    s1 = engines[0].executor_stats(0)
    assert s1["jobs"] - s0["jobs"] == len(jobs)
    assert 2 <= s1["groups"] - s0["groups"] < len(jobs), (s0, s1)
    overflowed = 0
    for j, (t, d, precision, S, closed, mask) in enumerate(jobs):
        if j < 18:
            _assert_equal_jobs(out[j], _composition(engines[t], op, d, precision, S, closed, mask),
                               precision)
            _, ref, _ = _verify(engines[t], o, vks[t], d, precision, S, closed, mask)
            overflowed += ref["overflow"]
        else:
            seg = (np.arange(d["nonces"].shape[0]) % 2).astype(np.uint32)
            _check(out[j], _expected_ex(o, vks[t], d, task, keys[0], None, NO_DEADLINE, seg, mask,
                                        2, quarter=False))
    assert 0 < overflowed < 18


def test_one_engine_over_two_executors():
    """Eight concurrent jobs on an engine over the device list [0, 0]: wherever a job is placed it
    equals the composition and the references."""
    from janus_amd import prio3 as J
    name = "hist_256_c16"
    o = _oracle(name)
    vk = bytes([0x3E]) * 16
    rng = np.random.default_rng(1700)
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, devices=[0, 0])
    op = _openers()[0]
    jobs = []
    for j in range(8):
        n = int(rng.integers(100, 400))
        dd = _tamper(o, o.gen_reports(vk, n, seed=1700 + j, n_threads=4), rng)
        jobs.append(_seal(o, vk, dd, _three_buckets(n, rng), rng))
    out = [None] * 8

    def run(j):
        out[j] = _job_call(eng, op, jobs[j], PREC, 3, MIDDLE_CLOSED)

    m0 = eng.members()
    _join_all(_start_joined([threading.Thread(target=run, args=(j,), daemon=True)
                             for j in range(8)]))
    placed = [m["jobs"] - a["jobs"] for m, a in zip(eng.members(), m0)]
    assert sum(placed) == 8 and min(placed) > 0, placed
    single = _engine(CONFIGS[name], vk)
    for j in range(8):
        assert out[j] is not None
        _assert_equal_jobs(out[j], _composition(single, op, jobs[j], PREC, 3, MIDDLE_CLOSED), PREC)
        _verify(single, o, vk, jobs[j], PREC, 3, MIDDLE_CLOSED)


# ---- arguments -----------------------------------------------------------------------------
def test_empty_job():
    """n == 0 succeeds with the composition's outputs: zero rows, an all-zero info except
    first_duplicate."""
    vk = bytes([0x22]) * 16
    eng = _engine(CONFIGS["count"], vk)
    z = lambda *s, t=np.uint8: np.zeros(s, t)
    d = dict(nonces=z(0, 16), times=z(0, t=np.uint64), public_shares=z(0, 0), enc=z(0, 32),
             ct=z(0, 64), ct_len=z(0, t=np.uint32),
             leader_prep_shares=z(0, eng.sz.prep_share_len))
    got = _job_call(eng, _openers()[0], d, PREC, 3, MIDDLE_CLOSED)
    assert got["n_segments"] == 0 and got["overflow"] == 0 and got["n_duplicates"] == 0
    assert got["first_duplicate"] == NO_SEG and got["n_closed"] == 0
    for k in ("agg", "counts", "checksums", "intervals", "segment_starts"):
        assert got[k].shape[0] == 3 and not got[k].any(), k


def test_argument_errors():
    from janus_amd import hpke as G
    from oracle import hpke as H
    o = _oracle("count")
    vk, base = _base("count", 63)
    rng = np.random.default_rng(6)
    d = _seal(o, vk, base, _three_buckets(63, rng), rng, tamper=False)
    eng = _engine(CONFIGS["count"], vk)
    op = _openers()[0]
    (pkey,) = _keys(rng, 1, H.KEM_P256)
    p256 = G.HpkeOpener(pkey[0], pkey[1], kem_id=G.KEM_P256_HKDF_SHA256, device=0)
    for kw in (dict(S=0), dict(S=4097), dict(op=None), dict(fb=p256),
               dict(closed=np.zeros((1025, 2), np.uint64))):
        with pytest.raises(RuntimeError, match=r"rc=-1\)"):
            _job_call(eng, kw.get("op", op), d, PREC, kw.get("S", 3), kw.get("closed"), None,
                      kw.get("fb"))
    with pytest.raises(ValueError):
        _job_call(eng, op, d, PREC, 3, None, np.ones(5, np.uint8))

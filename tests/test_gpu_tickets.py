"""Ticketed job submission (prio3_*_submit, prio3_ticket_poll / _wait; HelperEngine.submit_*): a
caller keeps several job calls outstanding.

Every comparison is byte for byte against the blocking twin on the same inputs (prepare messages
on the rows where they are defined: status < 0x80), and the blocking results themselves are held
against the references of tests/test_gpu_helper_job.py and tests/test_gpu_leader_job.py.  The
contract pinned here: inputs are consumed inside submit, outputs are written only inside wait, a
shared eventfd receives exactly one count per ticket once its group is done, tickets of one thread
share groups, and the executors' active counters return to zero."""
import ctypes as C
import os
import select
import threading
import time

import numpy as np
import pytest

from tests import test_gpu_leader_job as LJ
from tests.conftest import CONFIGS
from tests.test_gpu_executor import _Held, _engine, _ref
from tests.test_gpu_helper_job import (MIDDLE_CLOSED, PREC, _assert_equal_jobs, _base, _job_call,
                                       _keyset, _openers, _oracle, _seal, _three_buckets, _verify)
from tests.test_gpu_init_contract import (MP_CASES, NO_DEADLINE, VK32, _call, _check,
                                          _expected_ex, _mp_reports)
from tests.test_gpu_parity import _tamper

pytestmark = pytest.mark.gpu

FILL = 0xA5
EINVAL = r"rc=-1\)"


# ---- helpers -------------------------------------------------------------------------------
class _EventFd:
    """One non-blocking eventfd shared by a test's tickets."""

    def __enter__(self):
        self.fd = os.eventfd(0, os.EFD_NONBLOCK)
        return self

    def __exit__(self, *exc):
        os.close(self.fd)

    def read(self):
        """The counts written since the last read (0: none)."""
        try:
            return os.eventfd_read(self.fd)
        except BlockingIOError:
            return 0

    def collect(self, want, timeout=60.0):
        """Sums reads until `want` counts have arrived (the fd becomes readable; no sleeping)."""
        got, t0 = 0, time.monotonic()
        while got < want:
            left = timeout - (time.monotonic() - t0)
            assert left > 0, f"{got} of {want} notifications within {timeout} s"
            if select.select([self.fd], [], [], left)[0]:
                got += self.read()
        return got


def _submit_job(eng, op, d, precision, S, closed=None, mask=None, fb=None, deadline=None, fd=None):
    _, task = _keyset()
    return eng.submit_aggregate_job(op, task, d["nonces"], d["times"], d["public_shares"],
                                    d["enc"], d["ct"], d["ct_len"], d["leader_prep_shares"],
                                    precision, S, closed_intervals=closed, accept_mask=mask,
                                    fallback_opener=fb, report_deadline=deadline, notify_fd=fd)


def _submit_ex(eng, op, d, seg, accept, S, fd=None, **kw):
    _, task = _keyset()
    return eng.submit_aggregate_init_batch(op, task, d["nonces"], d["times"], d["public_shares"],
                                           d["enc"], d["ct"], d["ct_len"],
                                           d["leader_prep_shares"], seg, accept, S, notify_fd=fd,
                                           **kw)


def _submit_pa(eng, d, seg, accept, S, fd=None):
    return eng.submit_prepare_aggregate_batch(d["nonces"], d["public_shares"], d["helper_shares"],
                                              d["leader_prep_shares"], seg, accept, S,
                                              notify_fd=fd)


def _block_pa(eng, d, seg, accept, S):
    return eng.prepare_aggregate_batch(d["nonces"], d["public_shares"], d["helper_shares"],
                                       d["leader_prep_shares"], seg, accept, S)


def _arrays(bufs):
    return [b for b in bufs if isinstance(b, np.ndarray) and b.size]


def _fill(ticket):
    """Overwrites the ticket's output buffers: nothing may write them until its own wait()."""
    for a in _arrays(ticket.outputs):
        a.view(np.uint8).reshape(-1)[:] = FILL


def _untouched(ticket):
    return all((a.view(np.uint8) == FILL).all() for a in _arrays(ticket.outputs))


def _scribble(ticket, rng):
    """Random bytes over every input buffer the library was given."""
    k = 0
    for b in ticket.inputs:
        if isinstance(b, np.ndarray) and b.size:
            raw = b.view(np.uint8).reshape(-1)
        elif isinstance(b, C.Array):
            raw = np.frombuffer(b, np.uint8)
        else:
            continue  # the engine, an opener, the batch
        raw[:] = rng.integers(0, 256, raw.size, dtype=np.uint8)
        k += 1
    return k


def _seg_acc(n, S, rng):
    return rng.integers(0, S, n).astype(np.uint32), (rng.random(n) < 0.9).astype(np.uint8)


def _active_is_zero(eng):
    for kind in (0, 2, 3):
        st = eng.executor_stats(kind)
        assert st["active_jobs"] == 0 and st["active_reports"] == 0, (kind, st)


# ---- 1. twin equality ----------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [(nm, n) for nm in ("count", "hist_256_c16")
                                    for n in (1, 65, 300)])
def test_submit_then_wait_equals_the_blocking_twin(name, n):
    """Each of the five submit forms followed by wait, on tampered reports and tampered
    ciphertexts, with an eventfd: one count per ticket."""
    o = _oracle(name)
    vk, base = _base(name, n)
    rng = np.random.default_rng(7000 + 10 * n + len(name))
    eng = _engine(CONFIGS[name], vk)
    ops = _openers()
    d = _seal(o, vk, base, _three_buckets(n, rng), rng, row_key=rng.integers(0, 2, n))
    seg, acc = _seg_acc(n, 3, rng)
    deadline = int(d["times"].max()) - 1 if n > 1 else None
    with _EventFd() as ev:
        t = _submit_pa(eng, base, seg, acc, 3, fd=ev.fd)
        _check(t.wait(), _block_pa(eng, base, seg, acc, 3))
        t = _submit_ex(eng, ops[0], d, seg, acc, 3, fd=ev.fd, fallback_opener=ops[1],
                       report_deadline=deadline)
        _, task = _keyset()
        _check(t.wait(), _call(eng, ops[0], task, d, seg, acc, 3, fallback_opener=ops[1],
                               report_deadline=deadline))
        t = _submit_job(eng, ops[0], d, PREC, 4, MIDDLE_CLOSED, acc, ops[1], deadline, fd=ev.fd)
        assert t.poll() in (True, False)
        _assert_equal_jobs(t.wait(), _job_call(eng, ops[0], d, PREC, 4, MIDDLE_CLOSED, acc, ops[1],
                                               deadline), PREC)
        # the leader: prepare_init, then finish_job on the batch the wait returned
        lvk, ld, lin, msgs = LJ._base(name, n)
        leng = _engine(CONFIGS[name], lvk)
        msgs, ls, pe = LJ._failures(n, msgs, rng)
        times = _three_buckets(n, rng)
        ps0, st0, b0 = leng.leader_prepare_init_batch(ld["nonces"], ld["public_shares"], lin)
        t = leng.submit_leader_prepare_init_batch(ld["nonces"], ld["public_shares"], lin,
                                                  notify_fd=ev.fd)
        ps1, st1, b1 = t.wait()
        np.testing.assert_array_equal(ps1, ps0)
        np.testing.assert_array_equal(st1, st0)
        want = LJ._one_call(b0, ld, times, ls, pe, msgs, PREC, 4, MIDDLE_CLOSED, acc)
        t = b1.submit_leader_finish_job(ld["nonces"], times, ls, msgs, PREC, 4, prepare_error=pe,
                                        closed_intervals=MIDDLE_CLOSED, accept_mask=acc,
                                        notify_fd=ev.fd)
        LJ._assert_equal_jobs(t.wait(), want, PREC)
        with pytest.raises(RuntimeError, match="waited already"):
            t.wait()
        b0.free()
        b1.free()
        assert ev.collect(5) == 5 and ev.read() == 0
    _active_is_zero(eng)
    _active_is_zero(leng)


def test_multiproof_through_aggregate_job():
    """The Field64 multiproof instance: an engine that shares no launch."""
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    proofs, bits, length, chunk, _ = MP_CASES[1]
    n = 65
    o = Oracle("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk, num_proofs=proofs)
    rng = np.random.default_rng(78)
    d = _seal(o, VK32, _mp_reports(proofs, bits, length, chunk, n), _three_buckets(n, rng), rng)
    eng = J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(proofs, bits, length,
                                                                         chunk), VK32)
    with _EventFd() as ev:
        t = _submit_job(eng, _openers()[0], d, PREC, 3, MIDDLE_CLOSED, fd=ev.fd)
        got = t.wait()
        assert ev.collect(1) == 1
    want, _, _ = _verify(eng, o, VK32, d, PREC, 3, MIDDLE_CLOSED)
    _assert_equal_jobs(got, want, PREC)


# ---- 2. one thread, many tickets -------------------------------------------------------------
def test_one_thread_holds_twelve_tickets():
    """12 helper jobs of three tasks from ONE thread behind the executor's hold: aggregate_job,
    the _ex form and prepare_aggregate, 100 to 300 reports.  Nothing is done and no output is
    written while held; afterwards the shared eventfd counts 12, the outputs are still untouched
    until each ticket's own wait (in reverse order), every job equals its blocking result and the
    references, and the executor launched fewer groups than it took jobs."""
    name = "hist_256_c16"
    o = _oracle(name)
    keys, task = _keyset()
    rng = np.random.default_rng(1212)
    vks = [bytes([0x81 + t]) * 16 for t in range(3)]
    engines = [_engine(CONFIGS[name], vk) for vk in vks]
    op = _openers()[0]
    jobs = []
    for j in range(12):
        t, n = j % 3, int(np.linspace(100, 300, 12)[j])
        dd = _tamper(o, o.gen_reports(vks[t], n, seed=1200 + j, n_threads=4), rng)
        d = _seal(o, vks[t], dd, _three_buckets(n, rng), rng)
        seg, acc = _seg_acc(n, 3, rng)
        jobs.append((t, ("job", "ex", "pa", "job")[j % 4], d, seg, acc))
    s0 = engines[0].executor_stats(0)
    tickets = []
    with _EventFd() as ev, _Held(engines[0], 12) as h:
        for t, form, d, seg, acc in jobs:
            if form == "job":
                tk = _submit_job(engines[t], op, d, PREC, 4, MIDDLE_CLOSED, acc, fd=ev.fd)
            elif form == "ex":
                tk = _submit_ex(engines[t], op, d, seg, acc, 3, fd=ev.fd)
            else:
                tk = _submit_pa(engines[t], d, seg, acc, 3, fd=ev.fd)
            _fill(tk)
            tickets.append(tk)
        assert not any(tk.poll() for tk in tickets) and ev.read() == 0
        assert all(_untouched(tk) for tk in tickets)
        h.wait()  # all 12 are queued: release
        assert ev.collect(12) == 12
        assert all(tk.poll() for tk in tickets)
        assert all(_untouched(tk) for tk in tickets)
        out = [None] * 12
        for j in reversed(range(12)):
            out[j] = tickets[j].wait()
            assert all(_untouched(tk) for tk in tickets[:j])
        assert ev.read() == 0  # exactly once per ticket
    s1 = engines[0].executor_stats(0)
    assert s1["jobs"] - s0["jobs"] == 12
    assert 1 <= s1["groups"] - s0["groups"] < 12, (s0, s1)
    _active_is_zero(engines[0])
    for j, (t, form, d, seg, acc) in enumerate(jobs):
        if form == "job":
            want, _, _ = _verify(engines[t], o, vks[t], d, PREC, 4, MIDDLE_CLOSED, acc)
            _assert_equal_jobs(out[j], want, PREC)
        elif form == "ex":
            _check(out[j], _call(engines[t], op, task, d, seg, acc, 3))
            _check(out[j], _expected_ex(o, vks[t], d, task, keys[0], None, NO_DEADLINE, seg, acc,
                                        3, quarter=False))
        else:
            _check(out[j], _block_pa(engines[t], d, seg, acc, 3))
            _check(out[j], _ref(o, vks[t], d, seg, acc, 3))


# ---- 3. inputs are consumed at submit --------------------------------------------------------
def test_helper_inputs_are_consumed_at_submit():
    """Every input array, the closed intervals, the accept mask and the task ID are overwritten
    with random bytes right after submit, behind a hold."""
    name, n = "hist_256_c16", 300
    o = _oracle(name)
    vk, base = _base(name, n)
    rng = np.random.default_rng(303)
    eng = _engine(CONFIGS[name], vk)
    op = _openers()[0]
    d = _seal(o, vk, base, _three_buckets(n, rng), rng)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    want = _job_call(eng, op, d, PREC, 4, MIDDLE_CLOSED, mask)
    mine = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    with _Held(eng, 1) as h:
        tk = _submit_job(eng, op, mine, PREC, 4, MIDDLE_CLOSED.copy(), mask.copy())
        # ids, times, public shares, enc, ct, ct_len, prep shares, closed, mask, task id
        assert _scribble(tk, rng) == 10
        assert not tk.poll()
        h.wait()
        got = tk.wait()
    assert not np.array_equal(mine["ct"], d["ct"])  # the caller's own arrays were overwritten
    _assert_equal_jobs(got, want, PREC)


def test_leader_inputs_are_consumed_at_submit():
    name, n = "hist_256_c16", 300
    vk, d, lin, msgs = LJ._base(name, n)
    rng = np.random.default_rng(304)
    eng = _engine(CONFIGS[name], vk)
    msgs, ls, pe = LJ._failures(n, msgs, rng)
    times = _three_buckets(n, rng)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    b0 = LJ._init(eng, d, lin)
    want = LJ._one_call(b0, d, times, ls, pe, msgs, PREC, 4, MIDDLE_CLOSED, mask)
    b1 = LJ._init(eng, d, lin)
    with _Held(eng, 1, kind=3) as h:
        tk = b1.submit_leader_finish_job(d["nonces"].copy(), times.copy(), ls.copy(), msgs.copy(),
                                         PREC, 4, prepare_error=pe.copy(),
                                         closed_intervals=MIDDLE_CLOSED.copy(),
                                         accept_mask=mask.copy())
        # ids, times, leader status, prepare_error, prepare messages, closed, mask
        assert _scribble(tk, rng) == 7
        assert not tk.poll()
        h.wait()
        got = tk.wait()
    LJ._assert_equal_jobs(got, want, PREC)
    b0.free()
    b1.free()


# ---- 4. group spill --------------------------------------------------------------------------
def test_tickets_of_one_thread_spill_into_a_second_group():
    """Five aggregating jobs of 300 segments each cannot share one group (1024 segments)."""
    name, n, S = "count", 100, 300
    o = _oracle(name)
    vk, base = _base(name, n)
    eng = _engine(CONFIGS[name], vk)
    rng = np.random.default_rng(1500)
    segs = [_seg_acc(n, S, rng) for _ in range(5)]
    s0 = eng.executor_stats(0)
    with _Held(eng, 5) as h:
        tickets = [_submit_pa(eng, base, seg, acc, S) for seg, acc in segs]
        h.wait()
        out = [tk.wait() for tk in tickets]
    s1 = eng.executor_stats(0)
    assert s1["jobs"] - s0["jobs"] == 5 and s1["groups"] - s0["groups"] >= 2, (s0, s1)
    for got, (seg, acc) in zip(out, segs):
        _check(got, _block_pa(eng, base, seg, acc, S))
        _check(got, _ref(o, vk, base, seg, acc, S))


# ---- 5. synchronous paths --------------------------------------------------------------------
def test_a_job_past_the_group_limit_and_an_empty_job_are_done_at_submit():
    o = _oracle("count")
    n = 4097
    vk, base = _base("count", n)
    rng = np.random.default_rng(n + 3)
    d = _seal(o, vk, base, _three_buckets(n, rng), rng)
    eng = _engine(CONFIGS["count"], vk)
    op = _openers()[0]
    z = lambda *s, t=np.uint8: np.zeros(s, t)
    empty = dict(nonces=z(0, 16), times=z(0, t=np.uint64), public_shares=z(0, 0), enc=z(0, 32),
                 ct=z(0, 64), ct_len=z(0, t=np.uint32),
                 leader_prep_shares=z(0, eng.sz.prep_share_len), helper_shares=z(0, 0))
    with _EventFd() as ev:
        tk = _submit_job(eng, op, d, PREC, 3, MIDDLE_CLOSED, fd=ev.fd)
        assert tk.poll() and ev.read() == 1  # written before submit returned
        _assert_equal_jobs(tk.wait(), _job_call(eng, op, d, PREC, 3, MIDDLE_CLOSED), PREC)
        tk = _submit_job(eng, op, empty, PREC, 3, MIDDLE_CLOSED, fd=ev.fd)
        assert tk.poll() and ev.read() == 1
        got, want = tk.wait(), _job_call(eng, op, empty, PREC, 3, MIDDLE_CLOSED)
        for k in want:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
        tk = _submit_ex(eng, op, empty, None, None, 2, fd=ev.fd)
        assert tk.poll() and ev.read() == 1
        assert not tk.wait()[3].any()
        assert ev.read() == 0
    _active_is_zero(eng)


# ---- 6. mixed callers --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_pool():
    """Six jobs of three tasks with their blocking results, each held against the references once."""
    name = "hist_256_c16"
    o = _oracle(name)
    rng = np.random.default_rng(4646)
    vks = [bytes([0x91 + t]) * 16 for t in range(3)]
    engines = [_engine(CONFIGS[name], vk) for vk in vks]
    op = _openers()[0]
    pool = []
    for j in range(6):
        t, n = j % 3, (100, 173, 300, 257, 129, 211)[j]
        dd = _tamper(o, o.gen_reports(vks[t], n, seed=4600 + j, n_threads=4), rng)
        d = _seal(o, vks[t], dd, _three_buckets(n, rng), rng)
        mask = (rng.random(n) < 0.9).astype(np.uint8)
        want, _, _ = _verify(engines[t], o, vks[t], d, PREC, 4, MIDDLE_CLOSED, mask)
        pool.append((t, d, mask, want))
    return engines, op, pool


@pytest.mark.parametrize("heavy", [1, 0])
def test_blocking_and_ticketed_callers_together(mixed_pool, heavy):
    """Eight threads over three tasks: four make blocking calls, four keep 4 tickets outstanding,
    6 jobs each; once on the heavy-load launcher, once in the default mode."""
    engines, op, pool = mixed_pool
    errors, lock = [], threading.Lock()

    def compare(got, j):
        try:
            _assert_equal_jobs(got, pool[j][3], PREC)
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            with lock:
                errors.append((j, repr(e)[:400]))

    def blocking(w):
        for i in range(6):
            j = (w + i) % 6
            t, d, mask, _ = pool[j]
            compare(_job_call(engines[t], op, d, PREC, 4, MIDDLE_CLOSED, mask), j)

    def ticketed(w):
        held = []
        for i in range(6):
            j = (w + i) % 6
            t, d, mask, _ = pool[j]
            if len(held) == 4:
                tk, jj = held.pop(0)
                compare(tk.wait(), jj)
            held.append((_submit_job(engines[t], op, d, PREC, 4, MIDDLE_CLOSED, mask), j))
        for tk, jj in held:
            compare(tk.wait(), jj)

    def guarded(fn, w):
        try:
            fn(w)
        except Exception as e:  # noqa: BLE001
            with lock:
                errors.append((w, repr(e)[:400]))

    if heavy:
        engines[0].executor_control("heavy", 1)
    try:
        th = [threading.Thread(target=guarded, args=(blocking if w % 2 else ticketed, w),
                               daemon=True) for w in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join(120.0)
        assert not any(x.is_alive() for x in th), "a caller did not return"
    finally:
        engines[0].executor_control("heavy", 0)
    assert not errors, errors
    _active_is_zero(engines[0])
    t, d, mask, want = pool[0]
    _assert_equal_jobs(_job_call(engines[t], op, d, PREC, 4, MIDDLE_CLOSED, mask), want, PREC)


# ---- 7. leader -------------------------------------------------------------------------------
def test_one_thread_keeps_three_leader_jobs_outstanding():
    name = "hist_256_c16"
    o = LJ._oracle(name)
    rng = np.random.default_rng(777)
    sizes = (120, 300, 211)
    base = [LJ._base(name, n) for n in sizes]
    eng = _engine(CONFIGS[name], base[0][0])
    s0 = eng.executor_stats(2), eng.executor_stats(3)
    with _EventFd() as ev:
        with _Held(eng, 3, kind=2) as h:
            tks = [eng.submit_leader_prepare_init_batch(d["nonces"], d["public_shares"], lin,
                                                        notify_fd=ev.fd)
                   for _, d, lin, _ in base]
            assert not any(t.poll() for t in tks)
            h.wait()
            inits = [t.wait() for t in tks]
        assert ev.collect(3) == 3
        cases = []
        for (vk, d, lin, msgs), n, (ps, lst, batch) in zip(base, sizes, inits):
            np.testing.assert_array_equal(ps, d["leader_prep_shares"])
            assert not lst.any() and batch.n == n
            m, ls, pe = LJ._failures(n, msgs, rng)
            cases.append((m, ls, pe, _three_buckets(n, rng), (rng.random(n) < 0.9).astype(np.uint8)))
        with _Held(eng, 3, kind=3) as h:
            tks = [b.submit_leader_finish_job(d["nonces"], times, ls, m, PREC, 4, prepare_error=pe,
                                              closed_intervals=MIDDLE_CLOSED, accept_mask=mask,
                                              notify_fd=ev.fd)
                   for (_, d, _, _), (_, _, b), (m, ls, pe, times, mask) in zip(base, inits, cases)]
            assert not any(t.poll() for t in tks) and ev.read() == 0
            h.wait()
            assert ev.collect(3) == 3
            out = [t.wait() for t in reversed(tks)][::-1]
    s1 = eng.executor_stats(2), eng.executor_stats(3)
    for a, b in zip(s0, s1):
        assert b["jobs"] - a["jobs"] == 3 and b["groups"] - a["groups"] < 3, (a, b)
    for (vk, d, lin, _), (_, _, b), (m, ls, pe, times, mask), got in zip(base, inits, cases, out):
        LJ._assert_equal_jobs(got, LJ._composition(eng, b, d, times, ls, pe, m, PREC, 4,
                                                   MIDDLE_CLOSED, mask), PREC)
        LJ._assert_reference(got, o, vk, d, lin, times, ls, pe, m, PREC, 4, MIDDLE_CLOSED, mask)
        b.free()
    _active_is_zero(eng)


# ---- 8. two executors --------------------------------------------------------------------------
def test_eight_tickets_on_an_engine_over_two_executors():
    from janus_amd import prio3 as J
    name = "hist_256_c16"
    o = _oracle(name)
    vk = bytes([0x4E]) * 16
    rng = np.random.default_rng(1708)
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, devices=[0, 0])
    op = _openers()[0]
    jobs = []
    for j in range(8):
        n = int(rng.integers(100, 301))
        dd = _tamper(o, o.gen_reports(vk, n, seed=1750 + j, n_threads=4), rng)
        jobs.append(_seal(o, vk, dd, _three_buckets(n, rng), rng))
    m0 = eng.members()
    tickets = [_submit_job(eng, op, d, PREC, 3, MIDDLE_CLOSED) for d in jobs]
    out = [tk.wait() for tk in tickets]
    placed = [m["jobs"] - a["jobs"] for m, a in zip(eng.members(), m0)]
    assert sum(placed) == 8 and min(placed) > 0, placed
    single = _engine(CONFIGS[name], vk)
    for d, got in zip(jobs, out):
        want, _, _ = _verify(single, o, vk, d, PREC, 3, MIDDLE_CLOSED)
        _assert_equal_jobs(got, want, PREC)


# ---- 9. arguments ------------------------------------------------------------------------------
def test_argument_errors_leave_no_ticket_and_no_notification():
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle import hpke as H
    from tests.test_gpu_init_contract import _keys
    o = _oracle("count")
    vk, base = _base("count", 63)
    rng = np.random.default_rng(6)
    d = _seal(o, vk, base, _three_buckets(63, rng), rng, tamper=False)
    eng = _engine(CONFIGS["count"], vk)
    op = _openers()[0]
    (pkey,) = _keys(rng, 1, H.KEM_P256)
    p256 = G.HpkeOpener(pkey[0], pkey[1], kem_id=G.KEM_P256_HKDF_SHA256, device=0)
    s0 = eng.executor_stats(0)
    with _EventFd() as ev:
        for kw in (dict(S=0), dict(S=4097), dict(op=None), dict(fb=p256),
                   dict(closed=np.zeros((1025, 2), np.uint64))):
            with pytest.raises(RuntimeError, match=EINVAL):  # the blocking form's code
                _job_call(eng, kw.get("op", op), d, PREC, kw.get("S", 3), kw.get("closed"), None,
                          kw.get("fb"))
            with pytest.raises(RuntimeError, match=EINVAL):
                _submit_job(eng, kw.get("op", op), d, PREC, kw.get("S", 3), kw.get("closed"), None,
                            kw.get("fb"), fd=ev.fd)
        # a NULL ticket_out, and a failed submit leaves *ticket_out NULL
        L = J.load_library()
        assert L.prio3_helper_aggregate_job_submit(eng.handle, None, None, ev.fd, None) == -1
        h = C.c_void_p(0x1234)
        assert L.prio3_helper_aggregate_job_submit(eng.handle, None, None, ev.fd,
                                                   C.byref(h)) == -1
        assert not h.value
        assert L.prio3_helper_prepare_aggregate_batch_submit(
            eng.handle, 0, None, None, None, None, None, None, 1, None, None, None, None, ev.fd,
            None) == -1
        assert L.prio3_ticket_wait(None) == -1
        assert ev.read() == 0
    assert eng.executor_stats(0)["jobs"] == s0["jobs"]
    _active_is_zero(eng)
    with pytest.raises(ValueError):
        _submit_job(eng, op, d, PREC, 3, None, np.ones(5, np.uint8))

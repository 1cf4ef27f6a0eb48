"""The status contract of the one-call helper init (prio3_helper_aggregate_init_batch_ex): the
report deadline (PrepareError::ReportTooEarly, aggregator.rs:2004-2015), the task-then-global
keypair retry inside the group launch (aggregator.rs:1864-1878) and the Field64 multiproof
instance (64-byte public shares in the InputShareAad).

Expected values are composed from the unchanged oracles, as tests/test_gpu_init.py does: the
OpenSSL HPKE oracle opens every row with the first key, then the rows that gave HpkeDecryptError
with the second key; the C restatement of prio prepares and aggregates what was opened with the
rejected and the late reports excluded; merged status = 0x80 | open status, else 0x89 if late, else
the VDAF status.  Everything is compared bit for bit.  _expected_ex also asserts the status classes
a test claims and that a quarter of the reports finish, so the data is checked on the CPU before
any device call."""
import threading

import numpy as np
import pytest

from tests.conftest import CONFIGS
from tests.test_gpu_executor import _Held, _engine
from tests.test_gpu_parity import _tamper

TASKPROV = 0xFF00
T0 = 1_700_000_000
NO_DEADLINE = (1 << 64) - 1
VK32 = bytes(range(0x40, 0x60))


def _job(o, vk, n, seed, rng, task, pks, row_key, times=None, tamper=True, d=None, ext_rows=(),
         clean=()):
    """n reports sealed under task: row r to pks[row_key[r]].  tamper: the VDAF failures of
    tests/test_gpu_parity._tamper and the HPKE failures of tests/test_gpu_init._sealed_job (flipped
    tags; resealed rows with an unexpected taskprov extension or a payload one byte too long).
    ext_rows: further rows resealed (to their own key) with the taskprov extension; clean: rows
    the HPKE tampering leaves alone."""
    from oracle import hpke as H
    if d is None:
        d = o.gen_reports(vk, n, seed=seed, n_threads=4)
        if tamper:
            d = _tamper(o, d, rng)
    else:
        d = dict(d)
    if times is None:
        times = (T0 + rng.integers(0, 3600, n)).astype(np.uint64)
    row_key = np.asarray(row_key)
    pubs = d["public_shares"] if d["public_shares"].shape[1] else None
    enc = ct = cl = None
    for k, pk in enumerate(pks):
        if not (row_key == k).any():
            continue
        e, c, l, stride = H.seal_input_shares(pk, task, d["nonces"], times, pubs,
                                              d["helper_shares"], seed=seed + 1000 * k,
                                              n_threads=4)
        if enc is None:
            enc, ct, cl = e.copy(), c.copy(), l.copy()
        m = row_key == k
        enc[m], ct[m], cl[m] = e[m], c[m], l[m]
    ct = np.concatenate([ct, np.zeros((n, 16), np.uint8)], axis=1)  # room for the resealed rows

    def reseal(r, pt):
        aad = H.input_share_aad(task, d["nonces"][r].tobytes(), int(times[r]),
                                b"" if pubs is None else pubs[r].tobytes())
        e, c = H.seal(pks[row_key[r]], bytes(rng.integers(0, 256, 32, dtype=np.uint8)),
                      H.INFO_INPUT_SHARE_HELPER, aad, pt)
        enc[r] = np.frombuffer(e, np.uint8)
        ct[r] = 0
        ct[r, :len(c)] = np.frombuffer(c, np.uint8)
        cl[r] = len(c)

    if tamper and n > 1:
        rows = np.array([r for r in range(n) if r not in set(clean) | set(ext_rows)])
        for r in rng.choice(rows, max(1, n // 20), replace=False):
            ct[r, cl[r] - 1] ^= 0x01  # the AEAD tag
        for i, r in enumerate(rng.choice(rows, max(2, n // 25), replace=False)):
            share = d["helper_shares"][r].tobytes()
            reseal(r, H.plaintext_input_share(share, [(TASKPROV, b"")]) if i % 2 == 0 else
                   H.plaintext_input_share(share + b"\x00"))
    for r in ext_rows:
        reseal(r, H.plaintext_input_share(d["helper_shares"][r].tobytes(), [(TASKPROV, b"")]))
    d.update(times=times, enc=enc, ct=ct, ct_len=cl)
    return d


def _expected_ex(o, vk, d, task, key, fallback=None, deadline=NO_DEADLINE, seg=None, accept=None,
                 n_segments=1, classes=(), quarter=True):
    """(msgs, merged status, agg, counts, open status, VDAF status, first open's status) of the
    oracles.  key / fallback: (sk, pk)."""
    from oracle import hpke as H
    pubs = d["public_shares"] if d["public_shares"].shape[1] else None
    n = d["nonces"].shape[0]

    def open_(k):
        return H.open_input_shares(k[0], k[1], task, d["enc"], d["ct"], d["ct_len"], d["nonces"],
                                   d["times"], pubs, d["helper_shares"].shape[1], n_threads=4)

    shares, hs = open_(key)
    hs1 = hs.copy()
    if fallback is not None:
        again = hs == 4  # hpke::Error::Hpke(_) only: a row that opened and failed decode stays 8
        s2, h2 = open_(fallback)
        shares, hs = shares.copy(), hs.copy()
        shares[again], hs[again] = s2[again], h2[again]
    late = d["times"] > np.uint64(deadline)
    acc = ((hs == 0) & ~late).astype(np.uint8)
    if accept is not None:
        acc &= accept
    msgs, st, agg, cnt = o.helper_batch(vk, d["nonces"], d["public_shares"], shares,
                                        d["leader_prep_shares"], segment_ids=seg, accept_mask=acc,
                                        n_segments=n_segments, n_threads=4)
    merged = np.where(hs != 0, 0x80 | hs, np.where(late, 0x89, st)).astype(np.uint8)
    for c in classes:
        assert (merged == c).any(), ("status class missing from the test data", hex(c))
    if quarter:
        assert 4 * int((merged == 0).sum()) >= n, ("too few finished reports", (merged == 0).sum())
    return msgs, merged, agg, cnt, hs, st, hs1


def _check(got, exp):
    msgs, st, agg, cnt = got
    emsgs, est, eagg, ecnt = exp[:4]
    np.testing.assert_array_equal(st, est)
    ok = est < 0x80  # the prepare message of a report rejected before its VDAF is not defined
    np.testing.assert_array_equal(msgs[ok], emsgs[ok])
    np.testing.assert_array_equal(agg, eagg)
    np.testing.assert_array_equal(cnt, ecnt)


def _call(eng, op, task, d, seg=None, accept=None, n_segments=1, **kw):
    return eng.aggregate_init_batch(op, task, d["nonces"], d["times"], d["public_shares"],
                                    d["enc"], d["ct"], d["ct_len"], d["leader_prep_shares"], seg,
                                    accept, n_segments, **kw)


def _keys(rng, k, kem=None):
    from oracle import hpke as H
    out = []
    for _ in range(k):
        sk = H.kem_private(rng) if kem is None else H.kem_private(rng, kem)
        out.append((sk, H.kem_public(sk) if kem is None else H.kem_public(sk, kem)))
    return out


# ---- 1. deadline ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hist_256_c16", "count"])
def test_report_deadline(name):
    """n = 437 with every failure kind, three segments, an accept mask; times over an hour and the
    deadline in its middle.  A report at exactly the deadline passes, one a second later is 0x89; a
    late report the open also rejected keeps 0x84 / 0x88; a late report whose VDAF would fail shows
    0x89; counts and aggregate shares are the oracle's.  Without deadline and fallback the _ex
    form equals the plain entry point."""
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    cfg = CONFIGS[name]
    o = Oracle(**cfg)
    rng = np.random.default_rng(71)
    vk = bytes(range(0x40, 0x50))
    (key,) = _keys(rng, 1)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    n, deadline = 437, T0 + 1800
    times = (T0 + rng.integers(0, 3600, n)).astype(np.uint64)
    # rows 0 and 2 are touched by no tampering of _tamper (1, 3, 5, 7, 11 mod their strides)
    times[0], times[2] = deadline, deadline + 1
    d = _job(o, vk, n, 7, rng, task, [key[1]], np.zeros(n, int), times=times, clean=(0, 2))
    seg = rng.integers(0, 3, n).astype(np.uint32)
    accept = (rng.random(n) < 0.9).astype(np.uint8)
    accept[0] = accept[2] = 1
    exp = _expected_ex(o, vk, d, task, key, None, deadline, seg, accept, 3,
                       classes=(0, 3, 0x84, 0x88, 0x89))
    merged, hs, st = exp[1], exp[4], exp[5]
    late = d["times"] > np.uint64(deadline)
    assert hs[0] == 0 and st[0] == 0 and merged[0] == 0        # at the deadline: accepted
    assert hs[2] == 0 and st[2] == 0 and merged[2] == 0x89     # one second after it
    assert (late & (hs == 4)).any() and (late & (hs == 8)).any()      # these show 0x84 / 0x88
    assert (late & (hs == 0) & (st != 0)).any()                       # these show 0x89
    assert (merged[late & (hs != 0)] == (0x80 | hs[late & (hs != 0)])).all()
    assert (merged[late & (hs == 0)] == J.STATUS_REPORT_TOO_EARLY).all()
    eng = _engine(cfg, vk)
    op = G.HpkeOpener(key[0], key[1], device=0)
    got = _call(eng, op, task, d, seg, accept, 3, report_deadline=deadline)
    _check(got, exp)
    # no deadline, no fallback: the four outputs of the plain entry point
    old = _call(eng, op, task, d, seg, accept, 3)
    new = _call(eng, op, task, d, seg, accept, 3, report_deadline=NO_DEADLINE)
    for a, b in zip(old, new):
        np.testing.assert_array_equal(a, b)
    _check(new, _expected_ex(o, vk, d, task, key, None, NO_DEADLINE, seg, accept, 3))


# ---- 2. fallback ---------------------------------------------------------------------------
def _fallback_job(o, vk, n, rng, task, keys, mode="mixed"):
    """Rows sealed to the task key (0), the global key (1) or a third key (2)."""
    pks = [k[1] for k in keys]
    if mode == "all_global":
        return _job(o, vk, n, 300 + n, rng, task, pks, np.ones(n, int), tamper=False), ()
    if mode == "none_global":
        return _job(o, vk, n, 300 + n, rng, task, pks, np.zeros(n, int), tamper=False), ()
    if n == 1:  # the one report is the global keypair's
        return _job(o, vk, 1, 301, rng, task, pks, np.ones(1, int), tamper=False), ()
    row_key = rng.integers(0, 2, n)
    third = rng.choice(n, max(2, n // 30), replace=False)
    row_key[third] = 2
    free = [r for r in range(n) if r not in set(third)]
    row_key[free[0]], row_key[free[1]] = 0, 1
    ext = (free[0], free[1])  # a task-sealed and a global-sealed row with the taskprov extension
    return _job(o, vk, n, 300 + n, rng, task, pks, row_key, ext_rows=ext), ext


@pytest.mark.gpu
@pytest.mark.parametrize("n,mode", [(1, "mixed"), (63, "mixed"), (437, "mixed"),
                                    (437, "all_global"), (437, "none_global")])
def test_fallback_keypair(n, mode):
    """Half the rows sealed to the task keypair, half to the global one (opened by the retry
    pass), a few to a third (0x84 after both tries), tag flips, and the taskprov fault once under
    each key: 0x88 from the first open is final (never retried), the global-sealed one gets 0x88
    from the second.  One call is one job and one group launch of the executor."""
    from janus_amd import hpke as G
    from oracle.oracle import Oracle
    cfg = CONFIGS["hist_256_c16"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(1000 + n)
    vk = bytes([0x66]) * 16
    keys = _keys(rng, 3)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    d, ext = _fallback_job(o, vk, n, rng, task, keys, mode)
    classes = (0, 3, 0x84, 0x88) if (mode == "mixed" and n > 1) else (0,)
    exp = _expected_ex(o, vk, d, task, keys[0], keys[1], classes=classes)
    merged, hs, hs1 = exp[1], exp[4], exp[6]
    if mode == "mixed":
        assert ((hs1 == 4) & (hs == 0)).any()  # a row only the fallback opens
    if mode == "mixed" and n > 1:
        assert ((hs1 == 0) & (hs == 0)).any()
        assert hs1[ext[0]] == 8 and merged[ext[0]] == 0x88        # task-sealed: first open's 8
        assert hs1[ext[1]] == 4 and merged[ext[1]] == 0x88        # global-sealed: second open's
    if mode == "all_global":
        assert (hs1 == 4).all() and (hs == 0).all()
    if mode == "none_global":
        assert (hs1 == 0).all()
    eng = _engine(cfg, vk)
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    s0 = eng.executor_stats(0)
    got = _call(eng, op, task, d, fallback_opener=fb)
    s1 = eng.executor_stats(0)
    _check(got, exp)
    assert s1["jobs"] - s0["jobs"] == 1 and s1["groups"] - s0["groups"] == 1, (s0, s1)


@pytest.mark.gpu
def test_fallback_on_the_one_lane_open():
    """The retry pass through the one-lane k_hpke_open (what opens of more than pair_max reports
    run): both openers with "pair_max" 0, three blocks of 256 lanes, the list shorter than one."""
    from janus_amd import hpke as G
    from oracle.oracle import Oracle
    cfg = CONFIGS["hist_256_c16"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(1500)
    vk = bytes([0x67]) * 16
    keys = _keys(rng, 3)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    d, ext = _fallback_job(o, vk, 600, rng, task, keys)
    exp = _expected_ex(o, vk, d, task, keys[0], keys[1], T0 + 3000,
                       classes=(0, 3, 0x84, 0x88, 0x89))
    assert 0 < int((exp[6] == 4).sum()) < 512
    eng = _engine(cfg, vk)
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    op.executor_control("pair_max", 0)
    fb.executor_control("pair_max", 0)
    _check(_call(eng, op, task, d, fallback_opener=fb, report_deadline=T0 + 3000), exp)


@pytest.mark.gpu
def test_fallback_and_deadline_on_an_engine_over_two_executors():
    """Eight concurrent jobs on an engine over the device list [0, 0]: wherever a job is placed,
    it opens, retries and applies its deadline like a one-executor engine's."""
    from concurrent.futures import ThreadPoolExecutor

    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    cfg = CONFIGS["hist_256_c16"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(1600)
    vk = bytes([0x3D]) * 16
    keys = _keys(rng, 2)
    pks = [k[1] for k in keys]
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    jobs = []
    for j in range(8):
        n = int(rng.integers(100, 400))
        d = _job(o, vk, n, 1600 + j, rng, task, pks, rng.integers(0, 2, n), tamper=j % 2 == 0)
        dl = T0 + 1200 + 300 * j
        jobs.append((d, dl, _expected_ex(o, vk, d, task, keys[0], keys[1], dl, quarter=False)))
    seen = np.concatenate([e[1] for _, _, e in jobs])
    for c in (0, 3, 0x84, 0x88, 0x89):
        assert (seen == c).any(), hex(c)
    assert 4 * int((seen == 0).sum()) >= seen.size
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), vk, devices=[0, 0])
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    m0 = eng.members()
    with ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda j: _call(eng, op, task, j[0], fallback_opener=fb,
                                          report_deadline=j[1]), jobs))
    placed = [m["jobs"] - a["jobs"] for m, a in zip(eng.members(), m0)]
    assert sum(placed) == 8 and min(placed) > 0, placed
    for (d, dl, exp), g in zip(jobs, got):
        _check(g, exp)


@pytest.mark.gpu
def test_fallback_call_errors():
    """A fallback opener of another KEM (P-256 against X25519) and a NULL opener are PRIO3_EINVAL."""
    from janus_amd import hpke as G
    from oracle import hpke as H
    from oracle.oracle import Oracle
    cfg = CONFIGS["hist_256_c16"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(5)
    vk = bytes([0x21]) * 16
    (key,) = _keys(rng, 1)
    (pkey,) = _keys(rng, 1, H.KEM_P256)
    task = bytes(32)
    d = _job(o, vk, 8, 3, rng, task, [key[1]], np.zeros(8, int), tamper=False)
    eng = _engine(cfg, vk)
    op = G.HpkeOpener(key[0], key[1], device=0)
    p256 = G.HpkeOpener(pkey[0], pkey[1], kem_id=G.KEM_P256_HKDF_SHA256, device=0)
    with pytest.raises(RuntimeError, match=r"rc=-1\)"):
        _call(eng, op, task, d, fallback_opener=p256)
    with pytest.raises(RuntimeError, match=r"rc=-1\)"):
        _call(eng, None, task, d, fallback_opener=op)
    with pytest.raises(RuntimeError, match=r"rc=-1\)"):
        _call(eng, None, task, d, report_deadline=T0)


# ---- 3. concurrent jobs --------------------------------------------------------------------
@pytest.mark.gpu
def test_concurrent_jobs_with_and_without_fallback_and_deadlines():
    """Twelve jobs of two tasks queued behind the executor's hold: jobs with and without a
    fallback keypair (they launch apart), different deadlines -- two jobs of the same task with
    different deadlines share a launch -- fewer launches than jobs, every job the oracle's."""
    from janus_amd import hpke as G
    from oracle.oracle import Oracle
    cfg = CONFIGS["hist_256_c16"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(83)
    vks = [bytes([0x51 + t]) * 16 for t in range(2)]
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(2)]
    keys = _keys(rng, 2)
    pks = [k[1] for k in keys]
    engines = [_engine(cfg, vk) for vk in vks]
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    deadlines = [T0 + 1800, T0 + 2700, NO_DEADLINE]
    jobs = []
    for j in range(12):
        t, use_fb = j % 2, (j // 2) % 2 == 0
        dl = deadlines[(j // 4) % 3] if j != 4 else T0 + 1234
        n = int(rng.integers(100, 501))
        row_key = rng.integers(0, 2, n) if use_fb else np.zeros(n, int)
        d = _job(o, vks[t], n, 700 + j, rng, tasks[t], pks, row_key, tamper=j % 3 != 2)
        seg = rng.integers(0, 2, n).astype(np.uint32)
        jobs.append((t, use_fb, dl, d, seg))
    # jobs 0 and 4: the same task, both with the fallback, different deadlines
    assert jobs[0][0] == jobs[4][0] and jobs[0][1] and jobs[4][1] and jobs[0][2] != jobs[4][2]
    exp = [_expected_ex(o, vks[t], d, tasks[t], keys[0], keys[1] if use_fb else None, dl, seg,
                        None, 2, quarter=False) for t, use_fb, dl, d, seg in jobs]
    seen = np.concatenate([e[1] for e in exp])
    assert 4 * int((seen == 0).sum()) >= seen.size
    for c in (0, 3, 0x84, 0x88, 0x89):
        assert (seen == c).any(), hex(c)
    out = [None] * len(jobs)

    def run(j):
        t, use_fb, dl, d, seg = jobs[j]
        out[j] = _call(engines[t], op, tasks[t], d, seg, None, 2,
                       fallback_opener=fb if use_fb else None,
                       report_deadline=None if (dl == NO_DEADLINE and use_fb) else dl)

    g0 = engines[0].executor_stats(0)["groups"]
    with _Held(engines[0], len(jobs)) as h:
        th = [threading.Thread(target=run, args=(j,)) for j in range(len(jobs))]
        for x in th:
            x.start()
        h.wait()
        for x in th:
            x.join()
    launches = engines[0].executor_stats(0)["groups"] - g0
    assert 2 <= launches < len(jobs), launches
    for j in range(len(jobs)):
        _check(out[j], exp[j])


# ---- 4. multiproof -------------------------------------------------------------------------
def _mp_reports(proofs, bits, length, chunk, n):
    """16 distinct reports of the Python restatement, tiled to n, with tests/test_mp64.py's
    tampering of the leader prep shares."""
    from oracle import prio3_py as P
    v = P.Prio3(P.Prio3Type("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk,
                            num_proofs=proofs))
    rng = np.random.default_rng(proofs * 100 + bits)
    base = []
    for _ in range(16):
        m = [int(x) for x in rng.integers(0, 2 ** bits, length)]
        nonce = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        pub, leader, helper = v.shard(m, nonce, bytes(rng.integers(0, 256, 160, dtype=np.uint8)))
        _, lps, _ = v.prepare_init(VK32, 0, nonce, pub, leader)
        base.append((nonce, pub, helper, lps))
    A = lambda k: np.array([list(base[i % 16][k]) for i in range(n)], np.uint8)
    d = dict(nonces=A(0), public_shares=A(1), helper_shares=A(2), leader_prep_shares=A(3))
    nv = v.t.verifier_len * proofs
    lps = d["leader_prep_shares"]
    for i in rng.choice(n, n // 4, replace=False):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            lps[i, 8 * int(rng.integers(0, nv))] ^= 1        # verifier value
        elif kind == 1:
            lps[i, 8 * nv + 3] ^= 0x20                       # leader joint-rand part
        else:
            lps[i, 8 * int(rng.integers(0, nv)) + 7] = 0xff  # out of range: decode
    return d


MP_CASES = [(2, 16, 15, 16, 40), (3, 2, 5, 3, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("proofs,bits,length,chunk,n", MP_CASES)
def test_multiproof_sealed(proofs, bits, length, chunk, n):
    """Prio3SumVecField64MultiproofHmacSha256Aes128 through the one-call init: 64-byte public
    shares in the AAD, 96-byte helper shares, 32-byte prepare messages; once plain (the _ex form
    with neither option is reached through a far deadline), once with a fallback keypair and a
    deadline.  The plain entry point still refuses the instance."""
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    o = Oracle("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk, num_proofs=proofs)
    rng = np.random.default_rng(n)
    keys = _keys(rng, 3)
    pks = [k[1] for k in keys]
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    base = _mp_reports(proofs, bits, length, chunk, n)
    assert base["public_shares"].shape[1] == 64 and base["helper_shares"].shape[1] == 96
    # plain: one keypair, no deadline
    d = _job(o, VK32, n, 11, rng, task, pks, np.zeros(n, int), d=base)
    exp = _expected_ex(o, VK32, d, task, keys[0], classes=(0, 3, 0x84, 0x88))
    # fallback keypair and a deadline, two segments
    row_key = rng.integers(0, 2, n)
    row_key[rng.choice(n, 2, replace=False)] = 2
    d2 = _job(o, VK32, n, 12, rng, task, pks, row_key, d=base)
    seg = rng.integers(0, 2, n).astype(np.uint32)
    exp2 = _expected_ex(o, VK32, d2, task, keys[0], keys[1], T0 + 2400, seg, None, 2,
                        classes=(0, 3, 0x84, 0x88, 0x89))
    assert ((exp2[6] == 4) & (exp2[4] == 0)).any()
    eng = J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(proofs, bits, length,
                                                                         chunk), VK32)
    assert eng.sz.prep_msg_len == 32
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    with pytest.raises(RuntimeError, match=r"rc=-3\)"):
        _call(eng, op, task, d)
    _check(_call(eng, op, task, d, report_deadline=NO_DEADLINE), exp)
    _check(_call(eng, op, task, d2, seg, None, 2, fallback_opener=fb, report_deadline=T0 + 2400),
           exp2)


@pytest.mark.gpu
def test_open_input_shares_with_64_byte_public_shares():
    """The two-call janus_hpke_open_input_shares with public_share_len = 64 (the wide-segment path
    of the init call goes through it): shares and statuses equal the OpenSSL oracle's, a wrong key
    gives 4."""
    from janus_amd import hpke as G
    from oracle import hpke as H
    from oracle.oracle import Oracle
    proofs, bits, length, chunk, n = MP_CASES[0]
    o = Oracle("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk, num_proofs=proofs)
    rng = np.random.default_rng(9)
    keys = _keys(rng, 2)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    row_key = np.zeros(n, int)
    row_key[::7] = 1
    d = _job(o, VK32, n, 13, rng, task, [k[1] for k in keys], row_key,
             d=_mp_reports(proofs, bits, length, chunk, n))
    es, eh = H.open_input_shares(keys[0][0], keys[0][1], task, d["enc"], d["ct"], d["ct_len"],
                                 d["nonces"], d["times"], d["public_shares"], 96, n_threads=4)
    for c in (0, 4, 8):
        assert (eh == c).any(), c
    assert (eh[::7] == 4).all()
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    gs, gh = op.open_input_shares(task, d["enc"], d["ct"], d["ct_len"], d["nonces"], d["times"],
                                  d["public_shares"], 96)
    np.testing.assert_array_equal(gh, eh)
    np.testing.assert_array_equal(gs, es)


# ---- 5. wide-segment path ------------------------------------------------------------------
@pytest.mark.gpu
def test_wide_segment_path_with_fallback_and_deadline():
    """1025 segments (one more than a group takes): the library's two-call form opens with the
    opener, opens the 4s again with the fallback, and overlays the deadline on the host."""
    from janus_amd import hpke as G
    from oracle.oracle import Oracle
    cfg = CONFIGS["count"]
    o = Oracle(**cfg)
    rng = np.random.default_rng(97)
    vk = bytes([0x5B]) * 16
    keys = _keys(rng, 3)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    n = 500
    row_key = rng.integers(0, 2, n)
    row_key[rng.choice(n, 5, replace=False)] = 2
    d = _job(o, vk, n, 9, rng, task, [k[1] for k in keys], row_key)
    seg = rng.integers(0, 1025, n).astype(np.uint32)
    exp = _expected_ex(o, vk, d, task, keys[0], keys[1], T0 + 1800, seg, None, 1025,
                       classes=(0, 3, 0x84, 0x88, 0x89))
    assert ((exp[6] == 4) & (exp[4] == 0)).any()
    eng = _engine(cfg, vk)
    op = G.HpkeOpener(keys[0][0], keys[0][1], device=0)
    fb = G.HpkeOpener(keys[1][0], keys[1][1], device=0)
    _check(_call(eng, op, task, d, seg, None, 1025, fallback_opener=fb,
                 report_deadline=T0 + 1800), exp)


# ---- 6. declarations (no GPU) --------------------------------------------------------------
def test_declarations_carry_the_ex_form_and_report_too_early():
    import os
    import re

    from janus_amd import prio3 as J
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "janus_prio3.h")).read()
    assert re.search(r"PRIO3_STATUS_REPORT_TOO_EARLY\s*=\s*0x89\b", hdr)
    m = re.search(r"int\s+prio3_helper_aggregate_init_batch_ex\s*\(([^;]*)\)\s*;", hdr)
    assert m, "the _ex declaration is missing from the header"
    params = " ".join(m.group(1).split())
    assert params.startswith("prio3_engine* engine, struct janus_hpke_opener* opener, "
                             "struct janus_hpke_opener* fallback_opener, "
                             "uint64_t report_deadline, uint32_t n, const uint8_t task_id[32], "
                             "int require_taskprov,")
    assert J.STATUS_REPORT_TOO_EARLY == 0x89
    assert "prio3_helper_aggregate_init_batch_ex" in J.EXPORTED_SYMBOLS
    import inspect
    sig = inspect.signature(J.HelperEngine.aggregate_init_batch)
    assert sig.parameters["fallback_opener"].default is None
    assert sig.parameters["report_deadline"].default is None
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    sec2 = doc[doc.index("## 2"):doc.index("## 3")]
    assert re.search(r"PRIO3_STATUS_REPORT_TOO_EARLY:\s*i64\s*=\s*0x89\b", sec2)
    m = re.search(r"pub fn prio3_helper_aggregate_init_batch_ex\s*\(([^;]*)\)\s*->\s*c_int;", sec2)
    assert m, "the _ex declaration is missing from INTEGRATION.md section 2"
    names = re.findall(r"(\w+)\s*:", m.group(1))
    assert names[:5] == ["engine", "opener", "fallback_opener", "report_deadline", "n"], names

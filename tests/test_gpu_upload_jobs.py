"""The leader's upload as an executor job (prio3_leader_upload_job / _submit): every output byte
for byte what prio3_leader_upload_batch writes for the same arguments -- one job, many jobs of
several tasks in one coalesced group (each with its own now / deadline / expiration / expiry age),
both AEAD kernels, two keypairs, tickets, the synchronous paths and the argument errors, and a
two-executor engine.  The verdicts are also checked against the plain-Python restatement of the
handler (_handle of tests/test_gpu_leader_upload.py)."""
import ctypes as C
import functools
import os
import select
import threading

import numpy as np
import pytest

from oracle import hpke as H
from tests.conftest import CONFIGS
from tests.test_gpu_leader_upload import (CFG_HELPER, CFG_LEADER, DEADLINE, DECODE, DECRYPT,
                                          EXPIRED, HOST, INFO_LEADER, MALFORMED, NOW, OK, OUTDATED,
                                          P64, P128, T0, TASK_EXPIRED, TOO_EARLY, Key, _check,
                                          _handle, _parse_report, _report, _rows, _same,
                                          _sealed_reports)
from tests.test_gpu_parity import _engine, _oracle
from tests.test_gpu_tickets import FILL, _EventFd

pytestmark = pytest.mark.gpu

N = 67  # one full wave and a ragged one
U64 = (1 << 64) - 1


# ---- helpers -------------------------------------------------------------------------------
def _kw(task, tkey, gkey, **kw):
    args = dict(task_id=task, now=NOW, report_deadline=DEADLINE,
                task_opener=None if tkey is None else tkey.opener,
                task_config_id=0 if tkey is None else tkey.cfg,
                global_opener=None if gkey is None else gkey.opener,
                global_config_id=0 if gkey is None else gkey.cfg)
    args.update(kw)
    return args


def _hkw(kw):
    """_handle's keywords for an upload call's."""
    h = dict(now=kw.get("now", NOW), deadline=kw.get("report_deadline", DEADLINE),
             ext_stride=kw.get("ext_stride", 64))
    if kw.get("task_expiration", U64) != U64:
        h["task_exp"] = kw["task_expiration"]
    if kw.get("report_expiry_age", U64) != U64:
        h["age"] = kw["report_expiry_age"]
    return h


class _Aead:
    """Engine option upload_aead for the calls inside (resolved when a job is submitted)."""

    def __init__(self, eng, aead):
        self.eng, self.aead = eng, aead

    def __enter__(self):
        self.eng.set_option("upload_aead", self.aead)

    def __exit__(self, *exc):
        self.eng.set_option("upload_aead", 0)


class _Hold:
    """Jobs submitted inside queue behind the upload executor's hold; leaving releases it."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        from janus_amd import prio3 as J
        self.eng.executor_control("hold", 1, kind=J.EXEC_UPLOAD)

    def __exit__(self, *exc):
        from janus_amd import prio3 as J
        self.eng.executor_control("hold", 0, kind=J.EXEC_UPLOAD)


def _stats(eng, member=0):
    from janus_amd import prio3 as J
    return eng.executor_stats(J.EXEC_UPLOAD, member)


def _verdicts(bodies, rows, sz, task, keys, kw, out):
    """out against _handle, report by report; returns the statuses."""
    st = []
    for i, b in enumerate(bodies):
        s, w = _handle(b, rows.shape[1], sz, task, keys, **_hkw(kw))
        _check(out, i, s, w)
        st.append(s)
    return st


def _mp64_engine():
    from janus_amd import prio3 as J
    return J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(2, 8, 10, 3),
                          bytes(range(32)), device=0)


# ---- 1. parity, one job ----------------------------------------------------------------------
TASK_EXP, AGE, EXT_STRIDE = T0 + 9000, 20_000, 32


@functools.lru_cache(maxsize=None)
def _every_status(name):
    """67 reports of instance `name` sealed to one X25519 key, single reports carrying each failure
    of the handler (the cases of test_gpu_leader_upload._contract_batch, and extension bytes above
    ext_stride); and three reports whose time + expiry age overflows a u64."""
    kem = H.KEM_X25519
    rng = np.random.default_rng([11, len(name)])
    key = Key(rng, kem, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    if name == "mp64":
        eng = _mp64_engine()
        gen = eng.generate_reports_device(N, seed=5, with_leader_inputs=True)
        ids = gen["nonces"].cpu().numpy()
        pubs, shares = gen["public_shares"].cpu().numpy(), gen["leader_input_shares"].cpu().numpy()
        parts = [(ids[i].tobytes(), pubs[i].tobytes(), shares[i].tobytes()) for i in range(N)]
        es, p = 8, P64
    else:
        cfg = CONFIGS[name]
        o = _oracle(cfg)
        hi = 2 if cfg["kind"] == "count" else cfg["length"] if cfg["kind"] == "histogram" \
            else 1 << cfg["bits"]
        parts = []
        for i in range(N):
            r = np.random.default_rng([13, i])
            rid = r.integers(0, 256, 16, dtype=np.uint8).tobytes()
            rand = r.integers(0, 256, 80, dtype=np.uint8).tobytes()
            pub, lshare, _ = o.shard(int(r.integers(0, hi)), rid, rand[:o.rand_size])
            parts.append((rid, pub, lshare))
        es, p = (8, P64) if cfg["kind"] == "count" else (16, P128)  # Prio3Count is over Field64

    def setel(k, v):  # element k of the share := v
        return lambda s: s[:es * k] + v.to_bytes(es, "little") + s[es * (k + 1):]
    bad_ext = lambda s: (3).to_bytes(2, "big") + bytes(3) + len(s).to_bytes(4, "big") + s  # noqa: E731
    long_ext = lambda s: H.plaintext_input_share(s, [(0, bytes(range(29)))])  # noqa: E731  33 bytes
    cases = {
        2: dict(time=DEADLINE + 1),                                   # TooEarly
        5: dict(time=TASK_EXP + 1), 6: dict(time=TASK_EXP),           # TaskExpired
        9: dict(time=NOW - AGE - 1), 10: dict(time=NOW - AGE),        # Expired
        12: dict(pub_cut=1),                                          # public share length
        17: dict(cfg=99),                                             # OutdatedHpkeConfig
        21: dict(flip="ct"), 22: dict(flip="tag"), 23: dict(flip="enc"), 30: dict(flip="short"),
        24: dict(flip="enc31"), 25: dict(flip="enc33"),  # `enc` is not the KEM's 32 bytes
        33: dict(pt_fn=lambda s: H.plaintext_input_share(s) + b"\0"),  # payload length
        38: dict(share_fn=lambda s: s[es:]),                          # one element short
        41: dict(share_fn=setel(1, p)), 44: dict(share_fn=setel(1, p - 1)),  # non-canonical
        52: dict(pt_fn=bad_ext),                                      # malformed extension list
        57: dict(pt_fn=long_ext),                                     # above ext_stride: the host's
        58: dict(pt_fn=lambda s: H.plaintext_input_share(s, [(0, bytes(range(28)))])),  # fits
        63: dict(cut=1),                                              # truncated Report
        64: dict(time=DEADLINE + 5, cfg=99), 66: dict(pub_cut=1, flip="tag"),  # the earlier wins
    }
    want = {2: TOO_EARLY, 5: TASK_EXPIRED, 9: EXPIRED, 12: DECODE, 17: OUTDATED, 21: DECRYPT,
            22: DECRYPT, 23: DECRYPT, 24: DECRYPT, 25: DECRYPT, 30: DECRYPT, 33: DECODE, 38: DECODE, 41: DECODE, 52: DECODE,
            57: HOST, 63: MALFORMED, 64: TOO_EARLY, 66: DECODE}
    if name == "count":  # no public share to cut: the reports are honest
        del want[12]
        want[66] = DECRYPT

    def make(i, time=None, cfg=CFG_LEADER, pub_cut=0, pt_fn=None, flip=None, cut=0, share_fn=None):
        r = np.random.default_rng([17, i])
        rid, pub, lshare = parts[i]
        t = T0 + 300 * int(r.integers(0, 24)) if time is None else time
        pub = pub[:len(pub) - pub_cut] if pub else pub
        share = lshare if share_fn is None else share_fn(lshare)
        pt = H.plaintext_input_share(share) if pt_fn is None else pt_fn(share)
        aad = H.input_share_aad(task, rid, t, pub)
        enc, ct = H.seal(key.pk, H.kem_private(r, kem), INFO_LEADER, aad, pt, kem=kem)
        enc, ct = bytearray(enc), bytearray(ct)
        if flip == "ct":
            ct[len(ct) // 2] ^= 0x10
        elif flip == "tag":
            ct[-1] ^= 1
        elif flip == "enc":
            enc[3] ^= 4
        elif flip == "short":
            ct = ct[:15]
        elif flip == "enc31":
            enc = enc[:31]
        elif flip == "enc33":
            enc = enc + b"\0"
        henc = r.integers(0, 256, 32, dtype=np.uint8).tobytes()
        hct = r.integers(0, 256, 40 + i % 9, dtype=np.uint8).tobytes()
        body = _report(rid, t, pub, cfg, bytes(enc), bytes(ct), CFG_HELPER, henc, hct)
        return body[:len(body) - cut]

    bodies = [make(i, **cases.get(i, {})) for i in range(N)]
    overflow = [make(i, time=U64 - 5) for i in range(3)]
    return dict(key=key, task=task, bodies=bodies, want=want, overflow=overflow)


@pytest.mark.parametrize("aead", [1, 2])
@pytest.mark.parametrize("name", ["count", "sum8", "hist_10_c3", "mp64"])
def test_one_job_equals_the_batch_form(name, aead):
    b = _every_status(name)
    eng = _mp64_engine() if name == "mp64" else _engine(CONFIGS[name])
    rows, ln = _rows(b["bodies"])
    kw = _kw(b["task"], b["key"], None, task_expiration=TASK_EXP, report_expiry_age=AGE,
             ext_stride=EXT_STRIDE, helper_ct_stride=48)
    g0 = _stats(eng)
    with _Aead(eng, aead):
        out = eng.leader_upload_job(rows, ln, **kw)
        ref = eng.leader_upload_batch(rows, ln, **kw)
    g1 = _stats(eng)
    assert (g1["jobs"] - g0["jobs"], g1["groups"] - g0["groups"]) == (1, 1)  # the executor ran it
    assert set(out) == set(ref) and len(out) == 12
    _same(ref, out)
    st = _verdicts(b["bodies"], rows, eng.sz, b["task"], (b["key"], None), kw, out)
    assert {i: s for i, s in enumerate(st) if s} == b["want"]
    # time + report_expiry_age overflows a u64: the reference's internal error
    rows, ln = _rows(b["overflow"], rows.shape[1])
    for age, want in ((10, HOST), (4, OK)):
        kw2 = _kw(b["task"], b["key"], None, report_deadline=U64, report_expiry_age=age,
                  helper_ct_stride=48)
        with _Aead(eng, aead):
            out = eng.leader_upload_job(rows, ln, **kw2)
            _same(eng.leader_upload_batch(rows, ln, **kw2), out)
        assert _verdicts(b["overflow"], rows, eng.sz, b["task"], (b["key"], None), kw2, out) == \
            [want] * 3


# ---- 2. one group, many tasks ----------------------------------------------------------------
SIZES = (1, 63, 64, 65, 67, 130)
TA, TB, TC = T0, T0 + 100, T0 + 200  # the report times of every job
BIG = T0 + 10 ** 6
# (task index, now, deadline, task expiration, expiry age): the same report time is accepted in
# one job and TooEarly / TaskExpired / Expired in another
JOBS = ((2, TC, BIG, BIG, BIG),       # everything passes
        (0, TB, TB, U64, U64),        # t == deadline passes, TC is too early
        (1, TB, TB - 1, U64, U64),    # TB == deadline + 1: too early
        (2, TB, BIG, TB, U64),        # t == task_exp passes, TC is expired with the task
        (0, TB + 50, BIG, U64, 50),   # now == TB + age passes, TA is expired
        (1, TB + 51, BIG, U64, 50))   # one second later TB is expired too
WANT = ((OK, OK, OK), (OK, OK, TOO_EARLY), (OK, TOO_EARLY, TOO_EARLY), (OK, OK, TASK_EXPIRED),
        (EXPIRED, OK, OK), (EXPIRED, EXPIRED, OK))  # per job: the verdict at TA, TB, TC
# (job, report): the leader `enc` of these is 33 and 31 bytes, in reports whose time passes --
# DecryptFailure by the length of `enc`, beside reports of other jobs in the same launch
BAD_ENC = {(4, 5): 33, (5, 8): 31, (1, 61): 31, (2, 0): 33}


def _with_enc_len(body, k):
    """The Report `body` with its leader `enc` cut or zero-extended to k bytes."""
    r = _parse_report(body)
    ld, h = r["leader"], r["helper"]
    enc = (ld["enc"] + bytes(k))[:k]
    return _report(r["report_id"], r["time"], r["public_share"], ld["config_id"], enc,
                   ld["payload"], h["config_id"], h["enc"], h["payload"])


@functools.lru_cache(maxsize=None)
def _many_tasks():
    cfg = CONFIGS["hist_10_c3"]
    o, sz = _oracle(cfg), _engine(cfg).sz
    rng = np.random.default_rng(23)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)]
    jobs = []
    for j, (n, (ti, *_)) in enumerate(zip(SIZES, JOBS)):
        bodies = []
        for k, t in enumerate((TA, TB, TC)):  # report i of the job carries time (TA, TB, TC)[i % 3]
            bodies.append(_sealed_reports(o, sz, tasks[ti], [key] * len(range(k, n, 3)),
                                          100 * j + k, time=t))
        order = [bodies[i % 3][i // 3] for i in range(n)]
        for (jj, i), k in BAD_ENC.items():
            if jj == j:
                order[i] = _with_enc_len(order[i], k)
        jobs.append(order)
    stride = max(len(b) for job in jobs for b in job)
    return dict(key=key, tasks=tasks, jobs=jobs, stride=-(-stride // 16) * 16)


@pytest.mark.parametrize("aead", [1, 2])
def test_one_group_serves_jobs_of_several_tasks(aead):
    m = _many_tasks()
    eng = _engine(CONFIGS["hist_10_c3"])
    calls = []
    for bodies, (ti, now, dl, exp, age) in zip(m["jobs"], JOBS):
        rows, ln = _rows(bodies, m["stride"])
        calls.append((bodies, rows, ln, m["tasks"][ti],
                      _kw(m["tasks"][ti], m["key"], None, now=now, report_deadline=dl,
                          task_expiration=exp, report_expiry_age=age, helper_ct_stride=48)))
    s0 = _stats(eng)
    with _Aead(eng, aead):
        with _Hold(eng):
            tickets = [eng.submit_leader_upload_job(rows, ln, **kw) for _, rows, ln, _, kw in calls]
            assert _stats(eng)["groups"] == s0["groups"]  # nothing launches behind the hold
        outs = [t.wait() for t in tickets]
        refs = [eng.leader_upload_batch(rows, ln, **kw) for _, rows, ln, _, kw in calls]
    s1 = _stats(eng)
    assert (s1["groups"] - s0["groups"], s1["jobs"] - s0["jobs"]) == (1, 6)
    assert s1["reports"] - s0["reports"] == sum(SIZES) and s1["active_jobs"] == 0
    for j, ((bodies, rows, ln, task, kw), out, ref) in enumerate(zip(calls, outs, refs)):
        _same(ref, out)
        st = _verdicts(bodies, rows, eng.sz, task, (m["key"], None), kw, out)
        want = [WANT[j][i % 3] for i in range(len(bodies))]
        for (jj, i) in BAD_ENC:
            if jj == j:
                assert want[i] == OK  # the time checks pass: the length of `enc` decides
                want[i] = DECRYPT
        assert st == want, j


@functools.lru_cache(maxsize=None)
def _three_small_jobs():
    cfg = CONFIGS["hist_10_c3"]
    o, sz = _oracle(cfg), _engine(cfg).sz
    rng = np.random.default_rng(29)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)]
    jobs = [_sealed_reports(o, sz, tasks[j], [key] * n, 300 + j, time=TB)
            for j, n in enumerate((1, 1, 2))]
    return key, tasks, jobs


def test_one_wave_of_the_wide_kernel_holds_three_jobs():
    """Jobs of 1, 1 and 2 reports of three tasks in one group: its four reports are one workgroup
    of the front and one wave of k_aead_open_wide, whatever order the list has, so three of the
    wave's 16-lane rows read three different job rows.  The second job's deadline rejects its
    report."""
    key, tasks, jobs = _three_small_jobs()
    eng = _engine(CONFIGS["hist_10_c3"])
    stride = -(-max(len(b) for j in jobs for b in j) // 16) * 16
    calls = []
    for j, bodies in enumerate(jobs):
        rows, ln = _rows(bodies, stride)
        calls.append((bodies, rows, ln, tasks[j],
                      _kw(tasks[j], key, None, now=TB, report_deadline=TB - 1 if j == 1 else TB,
                          helper_ct_stride=48)))
    s0 = _stats(eng)
    with _Aead(eng, 2):
        with _Hold(eng):
            tickets = [eng.submit_leader_upload_job(rows, ln, **kw) for _, rows, ln, _, kw in calls]
        outs = [t.wait() for t in tickets]
        refs = [eng.leader_upload_batch(rows, ln, **kw) for _, rows, ln, _, kw in calls]
    s1 = _stats(eng)
    assert (s1["groups"] - s0["groups"], s1["jobs"] - s0["jobs"]) == (1, 3)
    st = []
    for (bodies, rows, ln, task, kw), out, ref in zip(calls, outs, refs):
        _same(ref, out)
        st.append(_verdicts(bodies, rows, eng.sz, task, (key, None), kw, out))
    assert st == [[OK], [TOO_EARLY], [OK, OK]]
    # the same reports under a wrong task ID do not open: the AAD is each job's own
    swapped = eng.leader_upload_job(calls[0][1], calls[0][2], **dict(calls[0][4], task_id=tasks[2]))
    assert swapped["status"].tolist() == [DECRYPT]


# ---- 3. keypairs -----------------------------------------------------------------------------
@pytest.mark.parametrize("aead", [1, 2])
def test_keypairs(aead):
    cfg = CONFIGS["hist_10_c3"]
    eng, o = _engine(cfg), _oracle(cfg)
    rng = np.random.default_rng(31)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))

    def run(bodies, tkey, gkey, ticket=False):
        rows, ln = _rows(bodies)
        kw = _kw(task, tkey, gkey, helper_ct_stride=48,
                 helper_enc_len=32)
        if ticket:
            return rows, kw, eng.submit_leader_upload_job(rows, ln, **kw)
        out = eng.leader_upload_job(rows, ln, **kw)
        _same(eng.leader_upload_batch(rows, ln, **kw), out)
        return np.array(_verdicts(bodies, rows, eng.sz, task, (tkey, gkey), kw, out))

    with _Aead(eng, aead):
        # one config ID for both keypairs: the task's first, the global one for what it cannot open
        tk, gk = Key(rng, H.KEM_X25519, 7), Key(rng, H.KEM_X25519, 7)
        to = [tk if i % 3 else gk for i in range(N)]
        bodies = _sealed_reports(o, eng.sz, task, to, 5)
        assert not run(bodies, tk, gk).any()
        assert not run(bodies, gk, tk).any()  # the other order: most reports take the retry
        st = run(bodies, tk, None)  # task-only: the global keypair's reports do not open
        assert np.array_equal(st, np.where(np.arange(N) % 3 == 0, DECRYPT, OK))
        st = run(bodies, None, gk)  # global-only
        assert np.array_equal(st, np.where(np.arange(N) % 3 == 0, OK, DECRYPT))
        # different config IDs: each report goes to its own opener; a third ID is outdated
        g2 = Key(rng, H.KEM_X25519, 8)
        to2 = [tk if i % 2 else g2 for i in range(N)]
        cfg_of = [9 if i in (4, 65) else k.cfg for i, k in enumerate(to2)]
        bodies2 = _sealed_reports(o, eng.sz, task, to2, 6, cfg_of=cfg_of)
        st = run(bodies2, tk, g2)
        assert np.array_equal(np.flatnonzero(st), [4, 65]) and (st[[4, 65]] == OUTDATED).all()
        # a P-256 task key and an X25519 global key under one config ID: the length of `enc`
        # decides the list
        pk = Key(rng, H.KEM_P256, 7)
        to3 = [pk if i % 2 else gk for i in range(N)]
        bodies3 = _sealed_reports(o, eng.sz, task, to3, 7)
        assert not run(bodies3, pk, gk).any()
        # the same bodies through one opener: the other KEM's `enc` has the wrong length for it
        st = run(bodies3, None, gk)  # X25519 only: the 65-byte `enc` of the P-256 reports
        assert np.array_equal(st, np.where(np.arange(N) % 2 == 1, DECRYPT, OK))
        st = run(bodies3, pk, None)  # P-256 only: the 32-byte `enc` of the X25519 reports
        assert np.array_equal(st, np.where(np.arange(N) % 2 == 1, OK, DECRYPT))
        # two jobs with different opener pairs behind one hold: two groups, both correct
        s0 = _stats(eng)
        with _Hold(eng):
            r1, kw1, t1 = run(bodies, tk, gk, ticket=True)
            r2, kw2, t2 = run(bodies2, tk, g2, ticket=True)
        o1, o2 = t1.wait(), t2.wait()
        s1 = _stats(eng)
        assert (s1["groups"] - s0["groups"], s1["jobs"] - s0["jobs"]) == (2, 2)
        assert not np.array(_verdicts(bodies, r1, eng.sz, task, (tk, gk), kw1, o1)).any()
        st = np.array(_verdicts(bodies2, r2, eng.sz, task, (tk, g2), kw2, o2))
        assert np.array_equal(np.flatnonzero(st), [4, 65])


# ---- 4. tickets ------------------------------------------------------------------------------
def _out_buffers(sz, n, ext_stride, henc_len, hct_stride, fill=FILL):
    shapes = dict(report_ids=((n, 16), np.uint8), times=((n,), np.uint64),
                  public_shares=((n, sz.public_share_len), np.uint8),
                  leader_input_shares=((n, sz.leader_input_share_len), np.uint8),
                  extensions=((n, ext_stride), np.uint8), ext_len=((n,), np.uint32),
                  helper_config_ids=((n,), np.uint8), helper_enc=((n, henc_len), np.uint8),
                  helper_ct=((n, hct_stride), np.uint8), helper_ct_len=((n,), np.uint32),
                  leader_config_ids=((n,), np.uint8), status=((n,), np.uint8))
    out = {}
    for k, (shape, dt) in shapes.items():
        out[k] = np.zeros(shape, dt)
        out[k].view(np.uint8)[...] = fill
    return out


def _raw_job(eng, rows, ln, task, key, out, n=None, now=NOW, deadline=DEADLINE, ext_stride=64,
             henc_len=32, hct_stride=48, stride=None, opener=True):
    """The two structs of a raw C call (the caller keeps rows, ln and out alive)."""
    from janus_amd import prio3 as J
    a = lambda x: x.ctypes.data if x.size else None  # noqa: E731
    jin = J.Prio3UploadJobIn(
        task_opener=key.opener.handle.value if opener else None, global_opener=None,
        task_config_id=key.cfg, global_config_id=0, n=rows.shape[0] if n is None else n,
        task_id=(C.c_uint8 * 32).from_buffer_copy(task), now=now, report_deadline=deadline,
        task_expiration=U64, report_expiry_age=U64, reports=a(rows), report_len=a(ln),
        report_stride=rows.shape[1] if stride is None else stride, ext_stride=ext_stride,
        helper_enc_len=henc_len, helper_ct_stride=hct_stride)
    jout = J.Prio3UploadJobOut(**{k: a(v) for k, v in out.items()})
    return jin, jout


@functools.lru_cache(maxsize=None)
def _ticket_jobs():
    """Eight small jobs of three tasks (hist_10_c3), a few reports of each too early."""
    cfg = CONFIGS["hist_10_c3"]
    o, sz = _oracle(cfg), _engine(cfg).sz
    rng = np.random.default_rng(41)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    tasks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(3)]
    jobs = []
    for j in range(8):
        n = 5 + 3 * j
        bodies = _sealed_reports(o, sz, tasks[j % 3], [key] * n, 200 + j, time=T0 + j)
        jobs.append((tasks[j % 3], bodies, T0 + 4))  # the deadline: jobs 5-7 are too early
    stride = -(-max(len(b) for _, bs, _ in jobs for b in bs) // 16) * 16
    return key, jobs, stride


def test_tickets_read_inputs_in_submit_and_write_outputs_in_wait():
    from janus_amd import prio3 as J
    L = J.load_library()
    key, jobs, stride = _ticket_jobs()
    eng = _engine(CONFIGS["hist_10_c3"])
    rng = np.random.default_rng(43)
    refs, held, fds = [], [], []
    try:
        with _Hold(eng):
            for task, bodies, dl in jobs:
                rows, ln = _rows(bodies, stride)
                refs.append(eng.leader_upload_batch(rows, ln, **_kw(task, key, None,
                                                                    report_deadline=dl,
                                                                    helper_ct_stride=48)))
                out = _out_buffers(eng.sz, len(bodies), 64, 32, 48)
                jin, jout = _raw_job(eng, rows, ln, task, key, out, deadline=dl)
                fd = os.eventfd(0, os.EFD_NONBLOCK)
                fds.append(fd)
                h = C.c_void_p()
                assert L.prio3_leader_upload_job_submit(eng.handle, C.byref(jin), C.byref(jout),
                                                        fd, C.byref(h)) == 0 and h.value
                # every input is consumed: the arrays and both structs are overwritten at once
                rows[...] = rng.integers(0, 256, rows.shape, dtype=np.uint8)
                ln[...] = rng.integers(0, 1 << 32, ln.shape, dtype=np.uint32)
                for s in (jin, jout):
                    C.memmove(C.addressof(s), rng.bytes(C.sizeof(s)), C.sizeof(s))
                assert L.prio3_ticket_poll(h) == 0
                held.append((h, out))
            with pytest.raises(BlockingIOError):
                os.eventfd_read(fds[0])  # nothing is written behind the hold
        for (h, out), fd, ref in zip(held, fds, refs):
            assert select.select([fd], [], [], 60.0)[0]
            assert L.prio3_ticket_poll(h) == 1
            for k, v in out.items():  # done, not waited: no output byte is written yet
                assert (v.view(np.uint8) == FILL).all(), k
            assert L.prio3_ticket_wait(h) == 0
            assert os.eventfd_read(fd) == 1  # exactly once
            _same(ref, out)
        assert [int(r["status"][0]) for r in refs] == [OK] * 5 + [TOO_EARLY] * 3
    finally:
        for fd in fds:
            os.close(fd)


def test_blocking_and_ticketed_callers_share_the_executor():
    key, jobs, stride = _ticket_jobs()
    eng = _engine(CONFIGS["hist_10_c3"])
    refs = []
    for task, bodies, dl in jobs:
        rows, ln = _rows(bodies, stride)
        kw = _kw(task, key, None, report_deadline=dl, helper_ct_stride=48)
        refs.append((rows, ln, kw, eng.leader_upload_batch(rows, ln, **kw)))
    errors = []
    s0 = _stats(eng)

    def worker(t):
        try:
            mine = [refs[(t + k) % 8] for k in range(4)]
            if t % 2:  # four tickets at once
                tickets = [eng.submit_leader_upload_job(r, l, **kw) for r, l, kw, _ in mine]
                outs = [x.wait() for x in tickets]
            else:
                outs = [eng.leader_upload_job(r, l, **kw) for r, l, kw, _ in mine]
            for (_, _, _, ref), out in zip(mine, outs):
                _same(ref, out)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    s1 = _stats(eng)
    assert s1["jobs"] - s0["jobs"] == 32 and s1["active_jobs"] == 0


# ---- 5. synchronous paths and errors ---------------------------------------------------------
def test_synchronous_paths():
    from janus_amd import prio3 as J
    L = J.load_library()
    cfg = CONFIGS["count"]
    eng, o = _engine(cfg), _oracle(cfg)
    rng = np.random.default_rng(51)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    bodies = _sealed_reports(o, eng.sz, task, [key] * 8, 9)
    bodies[3] = bodies[3][:-1]  # one malformed
    with _EventFd() as ev:
        # an empty job: done at once
        s0 = _stats(eng)
        t = eng.submit_leader_upload_job(np.zeros((0, 256), np.uint8), np.zeros(0, np.uint32),
                                         notify_fd=ev.fd, **_kw(task, key, None))
        assert t.poll() and ev.read() == 1
        assert t.wait()["status"].shape == (0,)
        assert eng.leader_upload_job(np.zeros((0, 256), np.uint8), np.zeros(0, np.uint32),
                                     **_kw(task, key, None))["status"].shape == (0,)
        # one report above the limit: the batch form runs inside submit
        n = J.UPLOAD_JOB_MAX_REPORTS + 1
        rows8, ln8 = _rows(bodies)
        rows, ln = rows8[np.arange(n) % 8].copy(), ln8[np.arange(n) % 8].copy()
        kw = _kw(task, key, None, helper_ct_stride=48)
        ref = eng.leader_upload_batch(rows, ln, **kw)
        t = eng.submit_leader_upload_job(rows, ln, notify_fd=ev.fd, **kw)
        assert t.poll() and ev.read() == 1  # written inside submit
        _same(ref, t.outputs and dict(zip(ref, t.outputs)))  # and so are the outputs
        _same(ref, t.wait())
        _same(ref, eng.leader_upload_job(rows, ln, **kw))
        assert ev.read() == 0
        assert int(ref["status"][3]) == MALFORMED and int(ref["status"][n - 1]) == OK
        # an engine that does not coalesce
        eng.set_option("coalesce", 0)
        try:
            t = eng.submit_leader_upload_job(rows8, ln8, notify_fd=ev.fd, **kw)
            assert t.poll() and ev.read() == 1
            _same(eng.leader_upload_batch(rows8, ln8, **kw), t.wait())
        finally:
            eng.set_option("coalesce", 1)
        assert _stats(eng)["jobs"] == s0["jobs"]  # none of them was an executor job
        # the limit itself coalesces
        s0 = _stats(eng)
        _same({k: v[:n - 1] for k, v in ref.items()}, eng.leader_upload_job(rows[:n - 1], ln[:n - 1], **kw))
        assert _stats(eng)["jobs"] - s0["jobs"] == 1

        # argument errors: PRIO3_EINVAL, no ticket, the fd untouched
        out = _out_buffers(eng.sz, 8, 64, 32, 48)

        def submit(**edit):
            strip = edit.pop("strip", None)
            jin, jout = _raw_job(eng, rows8, ln8, task, key, out, **edit)
            if strip:
                setattr(jout if hasattr(jout, strip) else jin, strip, None)
            h = C.c_void_p(1)
            rc = L.prio3_leader_upload_job_submit(eng.handle, C.byref(jin), C.byref(jout), ev.fd,
                                                  C.byref(h))
            both = (rc, L.prio3_leader_upload_job(eng.handle, C.byref(jin), C.byref(jout)))
            assert h.value is None or rc == 0
            if rc == 0:
                assert L.prio3_ticket_wait(h) == 0 and ev.read() == 1
            return both
        assert submit() == (0, 0)
        assert submit(opener=False) == (-1, -1)            # both openers NULL
        assert submit(stride=rows8.shape[1] - 2) == (-1, -1)  # report_stride not a multiple of 4
        assert submit(ext_stride=30) == (-1, -1)
        assert submit(stride=1 << 31) == (-1, -1)
        assert submit(henc_len=0x10000) == (-1, -1)
        for missing in ("reports", "report_len", "report_ids", "times", "leader_input_shares",
                        "extensions", "ext_len", "helper_config_ids", "helper_enc", "helper_ct",
                        "helper_ct_len", "leader_config_ids", "status"):
            assert submit(strip=missing) == (-1, -1), missing
        jin, jout = _raw_job(eng, rows8, ln8, task, key, out)
        h = C.c_void_p(1)
        assert L.prio3_leader_upload_job_submit(None, C.byref(jin), C.byref(jout), ev.fd,
                                                C.byref(h)) == -1 and h.value is None
        assert L.prio3_leader_upload_job_submit(eng.handle, None, C.byref(jout), ev.fd,
                                                C.byref(h)) == -1
        assert L.prio3_leader_upload_job_submit(eng.handle, C.byref(jin), None, ev.fd,
                                                C.byref(h)) == -1
        assert L.prio3_leader_upload_job_submit(eng.handle, C.byref(jin), C.byref(jout), ev.fd,
                                                None) == -1
        assert ev.read() == 0
        # FPVec is PRIO3_EUNSUPPORTED in both forms
        fp = J.HelperEngine(J.Prio3FixedPointBoundedL2VecSum(4, 16), bytes(16), device=0)
        assert L.prio3_leader_upload_job(fp.handle, C.byref(jin), C.byref(jout)) == -3
        assert L.prio3_leader_upload_job_submit(fp.handle, C.byref(jin), C.byref(jout), ev.fd,
                                                C.byref(h)) == -3 and h.value is None
        with pytest.raises(NotImplementedError):
            fp.leader_upload_job(rows8, ln8, **kw)
        assert ev.read() == 0


# ---- 6. two executors on one GPU -------------------------------------------------------------
def test_two_executors_on_device_0():
    from janus_amd import prio3 as J
    key, jobs, stride = _ticket_jobs()
    one = _engine(CONFIGS["hist_10_c3"])
    eng = J.HelperEngine(J.Prio3Histogram(10, 3), bytes(range(0x40, 0x50)), devices=[0, 0])
    s0 = [_stats(eng, m) for m in (0, 1)]
    p0 = [m["jobs"] for m in eng.members()]
    tickets, refs = [], []
    for task, bodies, dl in jobs:
        rows, ln = _rows(bodies, stride)
        kw = _kw(task, key, None, report_deadline=dl, helper_ct_stride=48)
        refs.append(one.leader_upload_batch(rows, ln, **kw))
        tickets.append(eng.submit_leader_upload_job(rows, ln, **kw))
    for t, ref in zip(tickets, refs):
        _same(ref, t.wait())
    for task, bodies, dl in jobs[:2]:  # and blocking
        rows, ln = _rows(bodies, stride)
        kw = _kw(task, key, None, report_deadline=dl, helper_ct_stride=48)
        _same(one.leader_upload_batch(rows, ln, **kw), eng.leader_upload_job(rows, ln, **kw))
    d = [_stats(eng, m)["jobs"] - s0[m]["jobs"] for m in (0, 1)]
    assert sum(d) == 10 and min(d) >= 1, d  # both members' executors took jobs
    placed = [m["jobs"] - p for m, p in zip(eng.members(), p0)]
    assert placed == d

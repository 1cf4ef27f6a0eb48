"""The leader's upload handler in one device call (prio3_device_leader_upload /
prio3_leader_upload_batch): Report decode, the handler's checks in the reference's order, the HPKE
open of the leader input share with both AEAD kernels (option upload_aead 1: the one-lane body,
2: k_aead_open_wide), the PlaintextInputShare and leader share decode.  Bit-exact against the CPU
restatements: oracle.hpke (seal / open_ / input_share_aad / plaintext_input_share), Oracle.shard
and a plain-Python restatement of aggregator.rs:1552-1686 (_handle below)."""
import functools

import numpy as np
import pytest

from oracle import hpke as H
from tests.conftest import CONFIGS
from tests.test_gpu_parity import _engine, _oracle

pytestmark = pytest.mark.gpu

N = 67  # one full wave and a ragged one; no lane-group size divides it
G = 16  # lanes per report of k_aead_open_wide
T0 = 1_700_000_000
NOW = T0 + 10_000
DEADLINE = NOW + 60
INFO_LEADER = b"dap-09 input share" + bytes([1, 2])
INFO_HELPER = b"dap-09 input share" + bytes([1, 3])
CFG_LEADER, CFG_HELPER = 42, 13
P128 = (0xffffffffffffffe4 << 64) | 1
P64 = 0xffffffff00000001
(OK, INTERVAL_COLLECTED, DECRYPT, DECODE, TASK_EXPIRED, EXPIRED, TOO_EARLY, OUTDATED) = range(8)
MALFORMED, HOST = 0x40, 0x41
ROWS = ("report_ids", "times", "public_shares", "leader_input_shares", "extensions", "ext_len",
        "helper_config_ids", "helper_enc", "helper_ct", "helper_ct_len")


class Key:
    def __init__(self, rng, kem, cfg):
        self.kem, self.cfg = kem, cfg
        self.sk = H.kem_private(rng, kem)
        self.pk = H.kem_public(self.sk, kem)

    @functools.cached_property
    def opener(self):
        from janus_amd import hpke as G_
        return G_.HpkeOpener(self.sk, self.pk, INFO_LEADER, device=0, kem_id=self.kem)


def _report(rid, time, pub, lcfg, lenc, lpay, hcfg, henc, hpay) -> bytes:
    ct = lambda c, e, p: bytes([c]) + len(e).to_bytes(2, "big") + e + len(p).to_bytes(4, "big") + p  # noqa: E731
    return rid + time.to_bytes(8, "big") + len(pub).to_bytes(4, "big") + pub + \
        ct(lcfg, lenc, lpay) + ct(hcfg, henc, hpay)


def _parse_report(b: bytes) -> dict:
    """Plain-Python Report parser (as tests/test_gpu_client_reports.py), raising where the
    reference's decode fails."""
    def take(o, k):
        if o + k > len(b):
            raise ValueError("a field runs past the Report")
        return b[o:o + k], o + k
    out = {}
    out["report_id"], o = take(0, 16)
    t, o = take(o, 8)
    out["time"] = int.from_bytes(t, "big")
    ln, o = take(o, 4)
    out["public_share"], o = take(o, int.from_bytes(ln, "big"))
    for who in ("leader", "helper"):
        cfg, o = take(o, 1)
        el, o = take(o, 2)
        enc, o = take(o, int.from_bytes(el, "big"))
        pl, o = take(o, 4)
        pay, o = take(o, int.from_bytes(pl, "big"))
        out[who] = dict(config_id=cfg[0], enc=enc, payload=pay)
    if o != len(b):
        raise ValueError("trailing bytes after the Report")
    return out


def _handle(body, stride, sz, task, keys, now=NOW, deadline=DEADLINE, task_exp=None, age=None,
            ext_stride=64):
    """aggregator.rs:1552-1686 for one uploaded body: (status, outputs or None).  keys: the
    task's Key and the global one (either None)."""
    if len(body) > stride:
        return MALFORMED, None
    try:
        r = _parse_report(body)
    except ValueError:
        return MALFORMED, None
    t = r["time"]
    if t > deadline:
        return TOO_EARLY, None
    if task_exp is not None and t > task_exp:
        return TASK_EXPIRED, None
    if age is not None:
        if t + age >= 1 << 64:
            return HOST, None  # Time::add fails: an internal error, the host's to report
        if now > t + age:
            return EXPIRED, None
    if len(r["public_share"]) != sz.public_share_len:
        return DECODE, None
    ld = r["leader"]
    known = [k for k in keys if k is not None and k.cfg == ld["config_id"]]
    if not known:
        return OUTDATED, None
    aad = H.input_share_aad(task, r["report_id"], t, r["public_share"])
    pt = None
    for k in known:  # the task's keypair first, the global one if that open fails
        if len(ld["enc"]) != H.nenc(k.kem) or len(ld["payload"]) < 16:
            continue
        pt = H.open_(k.sk, k.pk, ld["enc"], INFO_LEADER, aad, ld["payload"], kem=k.kem)
        if pt is not None:
            break
    if pt is None:
        return DECRYPT, None
    # PlaintextInputShare::get_decoded
    if len(pt) < 2:
        return DECODE, None
    el = int.from_bytes(pt[:2], "big")
    if 2 + el > len(pt):
        return DECODE, None
    ext, q = pt[2:2 + el], 0
    while q < el:
        if q + 4 > el:
            return DECODE, None
        ty, dl = int.from_bytes(ext[q:q + 2], "big"), int.from_bytes(ext[q + 2:q + 4], "big")
        if q + 4 + dl > el or ty not in (0, 0xFF00):  # the codec's ExtensionType
            return DECODE, None
        q += 4 + dl
    rest = pt[2 + el:]
    if len(rest) < 4 or int.from_bytes(rest[:4], "big") != len(rest) - 4:
        return DECODE, None
    share = rest[4:]
    # Prio3InputShare (leader): measurement and proofs shares of canonical elements, then the blind
    if len(share) != sz.leader_input_share_len:
        return DECODE, None
    es = sz.field_bytes
    blind = sz.prep_msg_len if sz.joint_rand_len else 0
    p = P128 if es == 16 else P64
    for o in range(0, len(share) - blind, es):
        if int.from_bytes(share[o:o + es], "little") >= p:
            return DECODE, None
    if el > ext_stride:
        return HOST, None
    h = r["helper"]
    return OK, dict(report_ids=r["report_id"], times=t, public_shares=r["public_share"],
                    leader_input_shares=share, extensions=ext, ext_len=el,
                    helper_config_ids=h["config_id"], helper_enc=h["enc"], helper_ct=h["payload"],
                    helper_ct_len=len(h["payload"]), leader_config_ids=ld["config_id"])


def _rows(bodies, stride=None):
    need = max(map(len, bodies))
    stride = -(-need // 16) * 16 if stride is None else stride
    rows = np.full((len(bodies), stride), 0xEE, np.uint8)  # poison past each report
    for i, b in enumerate(bodies):
        rows[i, :min(len(b), stride)] = np.frombuffer(b[:stride], np.uint8)
    return rows, np.array([len(b) for b in bodies], np.uint32)


def _upload(eng, rows, ln, task, tkey, gkey, aead, host=False, **kw):
    """One upload call with option upload_aead = aead; numpy results."""
    import torch
    eng.set_option("upload_aead", aead)
    args = dict(task_id=task, now=NOW, report_deadline=DEADLINE,
                task_opener=None if tkey is None else tkey.opener,
                task_config_id=0 if tkey is None else tkey.cfg,
                global_opener=None if gkey is None else gkey.opener,
                global_config_id=0 if gkey is None else gkey.cfg)
    args.update(kw)
    try:
        if host:
            return eng.leader_upload_batch(rows, ln, **args)
        out = eng.leader_upload_device(torch.from_numpy(rows).cuda(),
                                       torch.from_numpy(ln.view(np.int32)).cuda(), **args)
        torch.cuda.synchronize()
    finally:
        eng.set_option("upload_aead", 0)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["times"] = out["times"].view(np.uint64)
    for k in ("ext_len", "helper_ct_len"):
        out[k] = out[k].view(np.uint32)
    return out


def _check(out, i, want_status, want):
    """Report i of an upload's outputs against _handle's verdict."""
    assert int(out["status"][i]) == want_status, (i, int(out["status"][i]), want_status)
    if want_status != OK:
        for k in ROWS:
            assert not np.any(out[k][i]), (i, k)
        return
    pad = lambda b, w: b + bytes(w - len(b))  # noqa: E731
    assert out["report_ids"][i].tobytes() == want["report_ids"]
    assert int(out["times"][i]) == want["times"]
    assert out["public_shares"][i].tobytes() == want["public_shares"]
    assert out["leader_input_shares"][i].tobytes() == want["leader_input_shares"]
    assert int(out["ext_len"][i]) == want["ext_len"]
    assert out["extensions"][i].tobytes() == pad(want["extensions"], out["extensions"].shape[1])
    assert int(out["helper_config_ids"][i]) == want["helper_config_ids"]
    assert int(out["leader_config_ids"][i]) == want["leader_config_ids"]
    assert out["helper_enc"][i].tobytes() == want["helper_enc"]
    assert int(out["helper_ct_len"][i]) == want["helper_ct_len"]
    assert out["helper_ct"][i].tobytes() == pad(want["helper_ct"], out["helper_ct"].shape[1])


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. round trip ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,kem", [("hist_10_c3", H.KEM_X25519), ("hist_10_c3", H.KEM_P256),
                                      ("sum8", H.KEM_X25519), ("sum8", H.KEM_P256),
                                      ("count", H.KEM_X25519), ("count", H.KEM_P256),
                                      ("hist_256_c16", H.KEM_X25519)])
def test_round_trip_from_client_reports_to_the_helper(name, kem):
    import ctypes as C
    import torch
    from janus_amd import dap
    from janus_amd import hpke as G_
    from janus_amd import prio3 as J
    cfg = CONFIGS[name]
    eng, o = _engine(cfg), _oracle(cfg)
    sz = eng.sz
    rng = np.random.default_rng([N, kem, sorted(CONFIGS).index(name)])
    hi = 2 if cfg["kind"] == "count" else cfg["length"] if cfg["kind"] == "histogram" \
        else 1 << cfg["bits"]
    m = rng.integers(0, hi, (N, 1), dtype=np.uint64)
    ids = rng.integers(0, 256, (N, 16), dtype=np.uint8)
    rl = eng.rand_len
    rand = rng.integers(0, 256, (N, rl), dtype=np.uint8)
    times = (T0 + 300 * rng.integers(0, 24, N)).astype(np.uint64)
    sk = lambda: np.stack([np.frombuffer(H.kem_private(rng, kem), np.uint8) for _ in range(N)])  # noqa: E731
    lkey, hkey = Key(rng, kem, CFG_LEADER), Key(rng, kem, CFG_HELPER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
    ls = G_.HpkeSealer(lkey.pk, INFO_LEADER, device=0, kem_id=kem)
    hs = G_.HpkeSealer(hkey.pk, INFO_HELPER, device=0, kem_id=kem)
    need = J.load_library().prio3_client_report_stride(
        C.byref(eng.vdaf.params()), ls.handle, hs.handle, 0)
    rep = eng.prepare_reports_device(
        leader_sealer=ls, helper_sealer=hs, task_id=task, time_precision=300, measurements=t(m),
        report_ids=t(ids), times=t(times), rand=t(rand), sk_e_leader=t(sk()), sk_e_helper=t(sk()),
        leader_config_id=CFG_LEADER, helper_config_id=CFG_HELPER, report_stride=-(-need // 16) * 16)
    assert not rep["status"].any().item()
    hstride = G_.sealed_stride(sz.helper_share_len)
    kw = dict(task_id=task, now=NOW, report_deadline=DEADLINE, task_opener=lkey.opener,
              task_config_id=CFG_LEADER, helper_enc_len=H.nenc(kem), helper_ct_stride=hstride)
    outs = []
    for aead in (1, 2):  # the one-lane AEAD body, then k_aead_open_wide: no host step in between
        eng.set_option("upload_aead", aead)
        up = eng.leader_upload_device(rep["reports"], rep["report_len"], **kw)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in up.items()})
    eng.set_option("upload_aead", 0)
    _same(outs[0], outs[1])
    up = outs[0]
    assert not up["status"].any()
    assert np.array_equal(up["report_ids"], ids)
    assert np.array_equal(up["times"].view(np.uint64), times - times % 300)  # the client rounds
    assert (up["leader_config_ids"] == CFG_LEADER).all() and (up["helper_config_ids"] == CFG_HELPER).all()
    assert not up["ext_len"].any() and not up["extensions"].any()
    for i in range(N):
        pub, lshare, _ = o.shard(int(m[i, 0]), ids[i].tobytes(), rand[i].tobytes())
        assert up["public_shares"][i].tobytes() == pub
        assert up["leader_input_shares"][i].tobytes() == lshare
    # the leader's prepare on the call's outputs, the request from its helper rows, the helper
    pub = up["public_shares"] if sz.public_share_len else None
    lps, lst, lbatch = eng.leader_prepare_init_batch(up["report_ids"], pub, up["leader_input_shares"])
    lbatch.free()
    assert not lst.any()
    body, index, ninc = dap.encode_req_host(
        b"", 1, None, up["report_ids"], up["times"].view(np.uint64), pub, up["helper_config_ids"],
        up["helper_enc"], up["helper_ct"], up["helper_ct_len"].view(np.uint32), lps, lst)
    assert ninc == N
    lay = dap.scan(body, sz.public_share_len, H.nenc(kem), sz.prep_share_len)
    d = dap.unpack_host(body, lay, N, dap.ct_stride_for(lay))
    assert (d["config_ids"] == CFG_HELPER).all() and not d["msg_status"].any()
    opener = G_.HpkeOpener(hkey.sk, hkey.pk, device=0, kem_id=kem)
    msgs, st, agg, cnt = eng.aggregate_init_batch(
        opener, task, d["report_ids"], d["times"], d["public_shares"] if sz.public_share_len else None,
        d["enc"], d["ct"], d["ct_len"], d["prep_shares"])
    assert not st.any() and int(cnt[0]) == N


# ---- 2. the rejection contract ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _contract_batch():
    """hist_10_c3 / X25519: honest reports sealed here with oracle.hpke.seal, and the same batch
    with single reports carrying each failure (two of them two failures at once)."""
    name, kem = "hist_10_c3", H.KEM_X25519
    o = _oracle(CONFIGS[name])
    rng = np.random.default_rng(2024)
    key = Key(rng, kem, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    task_exp, age = T0 + 9000, 20_000
    L = o.leader_share_len

    def make(i, time=None, cfg=CFG_LEADER, pub_cut=0, pt_fn=None, flip=None, cut=0, share_fn=None):
        r = np.random.default_rng([7, i])
        rid = r.integers(0, 256, 16, dtype=np.uint8).tobytes()
        rand = r.integers(0, 256, 80, dtype=np.uint8).tobytes()
        t = T0 + 300 * int(r.integers(0, 24)) if time is None else time
        pub, lshare, _ = o.shard(int(r.integers(0, 10)), rid, rand)
        pub = pub[:len(pub) - pub_cut]
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
        henc = r.integers(0, 256, 32, dtype=np.uint8).tobytes()
        hct = r.integers(0, 256, 64, dtype=np.uint8).tobytes()
        body = _report(rid, t, pub, cfg, bytes(enc), bytes(ct), CFG_HELPER, henc, hct)
        return body[:len(body) - cut]

    def setel(k, v):  # element k of the share := v
        return lambda s: s[:16 * k] + v.to_bytes(16, "little") + s[16 * (k + 1):]
    bad_ext = lambda s: (3).to_bytes(2, "big") + bytes(3) + len(s).to_bytes(4, "big") + s  # noqa: E731
    cases = {
        2: dict(time=DEADLINE + 1),                          # TooEarly
        5: dict(time=T0 + 9500),                             # TaskExpired (before the deadline)
        9: dict(time=T0 - 10_001),                           # Expired: now > time + age
        12: dict(pub_cut=1),                                 # public share one byte short
        17: dict(cfg=99),                                    # unknown leader config ID
        21: dict(flip="ct"), 22: dict(flip="tag"), 23: dict(flip="enc"),
        30: dict(flip="short"),                              # a payload of 15 bytes
        33: dict(pt_fn=lambda s: H.plaintext_input_share(s) + b"\0"),  # trailing byte
        38: dict(share_fn=lambda s: s[16:]),                 # one element short
        41: dict(share_fn=setel(3, P128)),                   # p in the measurement share
        47: dict(share_fn=setel(o.meas_len + 2, P128)),      # p in the proofs share
        52: dict(pt_fn=bad_ext),                             # malformed extension list
        63: dict(cut=1),                                     # truncated Report
        # two failures at once: the earlier check wins
        64: dict(time=DEADLINE + 5, cfg=99),                 # TooEarly before OutdatedHpkeConfig
        66: dict(pub_cut=1, flip="tag"),                     # DecodeFailure before DecryptFailure
        # boundaries that must pass
        0: dict(time=T0 + 9000), 1: dict(time=T0 - 10_000),
        44: dict(share_fn=setel(3, P128 - 1)),
    }
    want = {2: TOO_EARLY, 5: TASK_EXPIRED, 9: EXPIRED, 12: DECODE, 17: OUTDATED, 21: DECRYPT,
            22: DECRYPT, 23: DECRYPT, 30: DECRYPT, 33: DECODE, 38: DECODE, 41: DECODE, 47: DECODE,
            52: DECODE, 63: MALFORMED, 64: TOO_EARLY, 66: DECODE}
    honest = [make(i) for i in range(N)]
    mixed = [make(i, **cases.get(i, {})) for i in range(N)]
    assert L == len(o.shard(0, bytes(16), bytes(80))[1])
    return dict(name=name, key=key, task=task, task_exp=task_exp, age=age, honest=honest,
                mixed=mixed, want=want, deadline_ok=(0, 1, 44))


@pytest.mark.parametrize("aead", [1, 2])
def test_rejection_contract(aead):
    b = _contract_batch()
    eng = _engine(CONFIGS[b["name"]])
    kw = dict(task_expiration=b["task_exp"], report_expiry_age=b["age"], helper_ct_stride=64)
    hkw = dict(task_exp=b["task_exp"], age=b["age"])
    rows, ln = _rows(b["mixed"] + b["honest"][:1])  # one stride for both batches
    rows, ln = rows[:N], ln[:N]
    out = _upload(eng, rows, ln, b["task"], b["key"], None, aead, **kw)
    hrows, hln = _rows(b["honest"], rows.shape[1])
    ref = _upload(eng, hrows, hln, b["task"], b["key"], None, aead, **kw)
    assert not ref["status"].any()
    for i in range(N):
        st, w = _handle(b["mixed"][i], rows.shape[1], eng.sz, b["task"], (b["key"], None), **hkw)
        assert st == b["want"].get(i, OK), i  # the restatement itself
        _check(out, i, st, w)
        if i not in b["want"] and i not in b["deadline_ok"]:  # untouched by its neighbours
            for k in out:
                assert np.array_equal(out[k][i], ref[k][i]), (i, k)
    assert int(out["leader_config_ids"][17]) == 99  # the host names the outdated ID
    assert int(out["leader_config_ids"][63]) == 0   # malformed: nothing is known


def test_host_form_equals_device_form():
    b = _contract_batch()
    eng = _engine(CONFIGS[b["name"]])
    kw = dict(task_expiration=b["task_exp"], report_expiry_age=b["age"], helper_ct_stride=64)
    rows, ln = _rows(b["mixed"])
    _same(_upload(eng, rows, ln, b["task"], b["key"], None, 0, **kw),
          _upload(eng, rows, ln, b["task"], b["key"], None, 0, host=True, **kw))


# ---- 3. two keypairs -------------------------------------------------------------------------
def _sealed_reports(o, sz, task, keys_per_report, seed, cfg_of=None, exts=None, time=T0):
    """Honest reports of instance o, report i sealed to keys_per_report[i] (a Key)."""
    out = []
    for i, k in enumerate(keys_per_report):
        r = np.random.default_rng([seed, i])
        rid = r.integers(0, 256, 16, dtype=np.uint8).tobytes()
        rand = r.integers(0, 256, 80, dtype=np.uint8).tobytes()
        hi = 2 if o.kind == "count" else 10
        pub, lshare, _ = o.shard(int(r.integers(0, hi)), rid, rand[:o.rand_size])
        pt = H.plaintext_input_share(lshare, () if exts is None else exts[i])
        aad = H.input_share_aad(task, rid, time, pub)
        enc, ct = H.seal(k.pk, H.kem_private(r, k.kem), INFO_LEADER, aad, pt, kem=k.kem)
        cfg = k.cfg if cfg_of is None else cfg_of[i]
        out.append(_report(rid, time, pub, cfg, enc, ct, CFG_HELPER,
                           r.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                           r.integers(0, 256, 40, dtype=np.uint8).tobytes()))
    return out


@pytest.mark.parametrize("aead", [1, 2])
def test_two_keypairs(aead):
    cfg = CONFIGS["hist_10_c3"]
    eng, o = _engine(cfg), _oracle(cfg)
    rng = np.random.default_rng(31)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    kw = dict(helper_ct_stride=48)

    def run(bodies, tkey, gkey):
        rows, ln = _rows(bodies)
        out = _upload(eng, rows, ln, task, tkey, gkey, aead, **kw)
        want = [_handle(b, rows.shape[1], eng.sz, task, (tkey, gkey)) for b in bodies]
        for i, (st, w) in enumerate(want):
            _check(out, i, st, w)
        return np.array([st for st, _ in want])

    # one config ID for both keypairs: the task's first, the global one for what it cannot open
    tk, gk = Key(rng, H.KEM_X25519, 7), Key(rng, H.KEM_X25519, 7)
    to = [tk if i % 3 else gk for i in range(N)]
    bodies = _sealed_reports(o, eng.sz, task, to, 5)
    assert not run(bodies, tk, gk).any()
    st = run(bodies, tk, None)  # without the global keypair its reports do not open
    assert np.array_equal(st, np.where(np.arange(N) % 3 == 0, DECRYPT, OK))
    assert not run(bodies, gk, tk).any()  # the other order: most reports take the retry
    # different config IDs and KEMs: each report goes to its own opener; a third ID is outdated
    g2 = Key(rng, H.KEM_P256, 8)
    to = [tk if i % 2 else g2 for i in range(N)]
    cfg_of = [9 if i in (4, 65) else k.cfg for i, k in enumerate(to)]
    bodies = _sealed_reports(o, eng.sz, task, to, 6, cfg_of=cfg_of)
    st = run(bodies, tk, g2)
    assert np.array_equal(np.flatnonzero(st), [4, 65]) and (st[[4, 65]] == OUTDATED).all()
    st = run(bodies, None, g2)  # the global keypair alone: the task's reports are outdated
    assert (st[1::2] == OUTDATED).all() and not st[0:4:2].any()


# ---- 4. lengths through the wide path ---------------------------------------------------------
@pytest.mark.parametrize("kem", [H.KEM_X25519, H.KEM_P256])
@pytest.mark.parametrize("name", ["count", "hist_1_c1"])  # public shares of 0 and 32 bytes
def test_payload_lengths_through_the_wide_kernel(name, kem):
    """Payload offset in the row = 35 + public share length + Nenc: 67, 99 (X25519), 100, 132
    (P-256) -- all four byte alignments."""
    cfg = CONFIGS[name]
    eng, o = _engine(cfg), _oracle(cfg)
    sz = eng.sz
    assert sz.public_share_len == (0 if name == "count" else 32)
    L = sz.leader_input_share_len
    rng = np.random.default_rng([41, kem, len(name)])
    key = Key(rng, kem, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    lengths = [0, 1, 15, 16, 17] + list(range(16 * (G - 1), 16 * (2 * G + 1) + 2)) + [4200]
    ext_stride = 4200
    bodies, sealed = [], []
    for j, total in enumerate(lengths):
        r = np.random.default_rng([43, j])
        rid = r.integers(0, 256, 16, dtype=np.uint8).tobytes()
        rand = r.integers(0, 256, 80, dtype=np.uint8).tobytes()
        pub, lshare, _ = o.shard(int(r.integers(0, 2)) if name == "count" else 0, rid,
                                 rand[:o.rand_size])
        ptl = max(total - 16, 0)
        k = ptl - 6 - L - 4  # data bytes of one padding extension (type Tbd)
        if ptl == 6 + L:
            pt = H.plaintext_input_share(lshare)
        elif k >= 0:
            pt = H.plaintext_input_share(lshare, [(0, r.integers(0, 256, k, dtype=np.uint8).tobytes())])
        else:  # cannot hold a share: any bytes, sealed with a good tag
            pt = r.integers(0, 256, ptl, dtype=np.uint8).tobytes()
        assert len(pt) == ptl
        aad = H.input_share_aad(task, rid, T0, pub)
        enc, ct = H.seal(key.pk, H.kem_private(r, kem), INFO_LEADER, aad, pt, kem=kem)
        ct = ct[:total]  # totals below 16: no room for a tag
        tail = (CFG_HELPER, r.integers(0, 256, H.nenc(kem), dtype=np.uint8).tobytes(),
                r.integers(0, 256, 33, dtype=np.uint8).tobytes())
        bodies.append(_report(rid, T0, pub, CFG_LEADER, enc, ct, *tail))
        sealed.append(pt)
        if total:  # the same with one flipped bit in its last block
            bad = bytearray(ct)
            bad[-1 - int(r.integers(0, min(16, total)))] ^= 1 << int(r.integers(0, 8))
            bodies.append(_report(rid, T0, pub, CFG_LEADER, enc, bytes(bad), *tail))
            sealed.append(None)
    rows, ln = _rows(bodies)
    kw = dict(ext_stride=ext_stride, helper_enc_len=H.nenc(kem), helper_ct_stride=48)
    out = _upload(eng, rows, ln, task, key, None, 2, **kw)
    n_ok = 0
    for i, b in enumerate(bodies):
        st, w = _handle(b, rows.shape[1], sz, task, (key, None), ext_stride=ext_stride)
        pl = len(_parse_report(b)["leader"]["payload"])
        if sealed[i] is None or pl < 16:
            assert st == DECRYPT, (i, pl)
        else:
            assert st == (OK if pl - 16 == 6 + L or pl - 16 >= 10 + L else DECODE), (i, pl)
            if st == OK:  # what was sealed comes back byte for byte
                el = int.from_bytes(sealed[i][:2], "big")
                assert w["extensions"] == sealed[i][2:2 + el]
                assert w["leader_input_shares"] == sealed[i][6 + el:]
                n_ok += 1
        _check(out, i, st, w)
    assert n_ok >= 100
    # the one-lane body agrees on every byte
    _same(out, _upload(eng, rows, ln, task, key, None, 1, **kw))


# ---- 5. ext_stride, the time overflow, the multiproof instance ---------------------------------
def test_extensions_above_ext_stride_and_time_overflow_go_to_the_host():
    cfg = CONFIGS["hist_10_c3"]
    eng, o = _engine(cfg), _oracle(cfg)
    rng = np.random.default_rng(51)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    exts = [()] * N
    exts[5] = [(0, bytes(range(28)))]        # 32 bytes: fits ext_stride exactly
    exts[6] = [(0, bytes(range(29)))]        # 33 bytes: the host's
    exts[7] = [(0xFF00, b""), (0, b"ab")]    # two extensions
    bodies = _sealed_reports(o, eng.sz, task, [key] * N, 8, exts=exts)
    rows, ln = _rows(bodies)
    kw = dict(ext_stride=32, helper_ct_stride=48)
    ref = _upload(eng, *_rows(_sealed_reports(o, eng.sz, task, [key] * N, 8), rows.shape[1]),
                  task, key, None, 0, **kw)
    for aead in (1, 2):
        out = _upload(eng, rows, ln, task, key, None, aead, **kw)
        for i, b in enumerate(bodies):
            st, w = _handle(b, rows.shape[1], eng.sz, task, (key, None), ext_stride=32)
            assert st == (HOST if i == 6 else OK)
            _check(out, i, st, w)
            if i not in (5, 6, 7):  # nothing else changes
                for k in out:
                    assert np.array_equal(out[k][i], ref[k][i]), (i, k)
        assert out["ext_len"][[5, 7]].tolist() == [32, 10]
    # time + report_expiry_age overflows a u64: the reference's internal error
    big = (1 << 64) - 5
    bodies = _sealed_reports(o, eng.sz, task, [key] * 3, 9, time=big)
    rows, ln = _rows(bodies)
    kw = dict(report_deadline=(1 << 64) - 1, helper_ct_stride=48)
    out = _upload(eng, rows, ln, task, key, None, 0, report_expiry_age=10, **kw)
    assert out["status"].tolist() == [HOST] * 3 and not out["leader_input_shares"].any()
    out = _upload(eng, rows, ln, task, key, None, 0, report_expiry_age=4, **kw)
    assert out["status"].tolist() == [OK] * 3
    st = [_handle(b, rows.shape[1], eng.sz, task, (key, None), deadline=(1 << 64) - 1, age=a)[0]
          for b in bodies[:1] for a in (10, 4)]
    assert st == [HOST, OK]
    # a time equal to the deadline passes, one second later is too early
    bodies = _sealed_reports(o, eng.sz, task, [key] * 2, 10, time=DEADLINE) + \
        _sealed_reports(o, eng.sz, task, [key], 11, time=DEADLINE + 1)
    rows, ln = _rows(bodies)
    out = _upload(eng, rows, ln, task, key, None, 0, helper_ct_stride=48)
    assert out["status"].tolist() == [OK, OK, TOO_EARLY]
    assert [_handle(b, rows.shape[1], eng.sz, task, (key, None))[0] for b in bodies] == \
        [OK, OK, TOO_EARLY]


@pytest.mark.parametrize("aead", [1, 2])
def test_multiproof_field64_instance(aead):
    """PRIO3_SUMVEC_F64_MP: 64-byte public shares, Field64 elements, a 32-byte blind; leader shares
    from the synthetic client, sealed with the generic seal."""
    from janus_amd import hpke as G_
    from janus_amd import prio3 as J
    eng = J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(2, 8, 10, 3),
                         bytes(range(32)), device=0)
    sz = eng.sz
    assert (sz.public_share_len, sz.field_bytes, sz.prep_msg_len) == (64, 8, 32)
    gen = eng.generate_reports_device(N, seed=3, with_leader_inputs=True)
    ids = gen["nonces"].cpu().numpy()
    pubs = gen["public_shares"].cpu().numpy()
    shares = gen["leader_input_shares"].cpu().numpy().copy()
    ne = (sz.leader_input_share_len - 32) // 8
    shares[11, 8:16] = np.frombuffer(P64.to_bytes(8, "little"), np.uint8)           # p: rejected
    shares[12, 8:16] = np.frombuffer((P64 - 1).to_bytes(8, "little"), np.uint8)     # p - 1: fine
    shares[13, 8 * (ne - 1):8 * ne] = np.frombuffer(P64.to_bytes(8, "little"), np.uint8)  # last
    shares[14, 8 * ne:8 * ne + 8] = 0xFF  # the blind is no field element
    rng = np.random.default_rng(61)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    sealer = G_.HpkeSealer(key.pk, INFO_LEADER, device=0)
    pts = [H.plaintext_input_share(shares[i].tobytes()) for i in range(N)]
    aads = [H.input_share_aad(task, ids[i].tobytes(), T0 + i, pubs[i].tobytes()) for i in range(N)]
    sk_e = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    enc, cts, st = sealer.seal(sk_e, pts, aads)
    assert not st.any()
    bodies = [_report(ids[i].tobytes(), T0 + i, pubs[i].tobytes(), CFG_LEADER, enc[i].tobytes(),
                      cts[i], CFG_HELPER, bytes(32), bytes(range(40))) for i in range(N)]
    rows, ln = _rows(bodies)
    out = _upload(eng, rows, ln, task, key, None, aead, helper_ct_stride=48)
    for i, b in enumerate(bodies):
        st_i, w = _handle(b, rows.shape[1], sz, task, (key, None))
        assert st_i == (DECODE if i in (11, 13) else OK), i
        _check(out, i, st_i, w)
    assert np.array_equal(out["leader_input_shares"][20], shares[20])


# ---- 6. argument errors ----------------------------------------------------------------------
def test_argument_errors_raise():
    import ctypes as C
    from janus_amd import hpke as G_
    from janus_amd import prio3 as J
    eng = _engine(CONFIGS["count"])
    rng = np.random.default_rng(71)
    key = Key(rng, H.KEM_X25519, CFG_LEADER)
    task = bytes(32)
    rows, ln = np.zeros((4, 256), np.uint8), np.zeros(4, np.uint32)
    with pytest.raises(ValueError):  # no opener at all
        eng.leader_upload_batch(rows, ln, task, NOW, DEADLINE)
    with pytest.raises(ValueError):  # misaligned report_stride
        eng.leader_upload_batch(rows[:, :254], ln, task, NOW, DEADLINE, task_opener=key.opener)
    with pytest.raises(ValueError):  # misaligned ext_stride
        eng.leader_upload_batch(rows, ln, task, NOW, DEADLINE, task_opener=key.opener, ext_stride=30)
    with pytest.raises(ValueError):
        eng.leader_upload_batch(rows, ln, task[:31], NOW, DEADLINE, task_opener=key.opener)
    import types
    import torch
    with pytest.raises(ValueError):  # an opener of another GPU
        eng.leader_upload_batch(rows, ln, task, NOW, DEADLINE,
                                task_opener=types.SimpleNamespace(device=1, handle=None))
    # the C entry point itself: PRIO3_EINVAL, and the calling thread's device stays
    L = J.load_library()
    tid = (C.c_uint8 * 32)()
    p = lambda a: a.ctypes.data  # noqa: E731
    o = {k: np.zeros((4, 64), np.uint8) for k in "abcdefghijk"}

    def call(topener, gopener, stride=256, ext_stride=64):
        return L.prio3_leader_upload_batch(
            eng.handle, topener, 1, gopener, 2, 4, tid, NOW, DEADLINE, J.UINT64_MAX, J.UINT64_MAX,
            p(rows), stride, p(ln), p(o["a"]), p(o["b"]), None, p(o["c"]), p(o["d"]), p(o["e"]),
            ext_stride, p(o["f"]), p(o["g"]), 32, p(o["h"]), p(o["i"]), 48, p(o["j"]), p(o["k"]))
    assert call(None, None) == -1
    assert call(key.opener.handle, None, stride=254) == -1
    assert call(key.opener.handle, None, ext_stride=30) == -1
    if torch.cuda.device_count() > 1:
        other = G_.HpkeOpener(key.sk, key.pk, INFO_LEADER, device=1)
        assert call(key.opener.handle, other.handle) == -1
        assert torch.cuda.current_device() == 0
    assert call(key.opener.handle, None) == 0
    assert o["k"][0, :4].tolist() == [MALFORMED] * 4  # empty bodies do not decode
    # FPVec is PRIO3_EUNSUPPORTED, as in the client section
    fp = J.HelperEngine(J.Prio3FixedPointBoundedL2VecSum(4, 16), bytes(16), device=0)
    with pytest.raises(NotImplementedError):
        fp.leader_upload_batch(rows, ln, task, NOW, DEADLINE, task_opener=key.opener)
    assert L.prio3_leader_upload_batch(
        fp.handle, key.opener.handle, 1, None, 2, 4, tid, NOW, DEADLINE, J.UINT64_MAX,
        J.UINT64_MAX, p(rows), 256, p(ln), p(o["a"]), p(o["b"]), None, p(o["c"]), p(o["d"]),
        p(o["e"]), 64, p(o["f"]), p(o["g"]), 32, p(o["h"]), p(o["i"]), 48, p(o["j"]),
        p(o["k"])) == -3

"""Client::prepare_report in one device call (prio3_client_prepare_reports_device): every emitted
DAP `Report` is parsed here in plain Python and each field checked against the CPU restatements --
the shard (Oracle.shard), both HPKE ciphertexts (oracle.hpke.seal with the same ephemeral key, and
open_ with the recipient's key), the rounded time -- and the helper ciphertexts go through the
helper's one-call init."""
import functools

import numpy as np
import pytest

from oracle import hpke as H
from tests.conftest import CONFIGS
from tests.test_gpu_parity import _engine, _oracle

pytestmark = pytest.mark.gpu

N = 67
T0 = 1_700_000_000
PRECISION = 300
INFO_LEADER = b"dap-09 input share" + bytes([1, 2])
INFO_HELPER = b"dap-09 input share" + bytes([1, 3])
CFG_LEADER, CFG_HELPER = 42, 13


def _parse_report(b: bytes) -> dict:
    """Report = ReportMetadata { id[16], time u64 } || u32-prefixed public share ||
    2 x HpkeCiphertext { config_id u8, u16-prefixed enc, u32-prefixed payload }."""
    o = 24
    out = dict(report_id=b[:16], time=int.from_bytes(b[16:24], "big"))
    ln = int.from_bytes(b[o:o + 4], "big")
    out["public_share"] = b[o + 4:o + 4 + ln]
    o += 4 + ln
    for who in ("leader", "helper"):
        cfg = b[o]
        el = int.from_bytes(b[o + 1:o + 3], "big")
        enc = b[o + 3:o + 3 + el]
        o += 3 + el
        pl = int.from_bytes(b[o:o + 4], "big")
        out[who] = dict(config_id=cfg, enc=enc, payload=b[o + 4:o + 4 + pl])
        o += 4 + pl
    assert o == len(b), "trailing bytes after the Report"
    return out


@functools.lru_cache(maxsize=None)
def _case(name, kem, bad=()):
    """Inputs and keys of one batch (numpy), shared by the tests of a (config, KEM)."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng([N, kem, sorted(CONFIGS).index(name)])
    hi = cfg["length"] if cfg["kind"] == "histogram" else 1 << cfg["bits"]
    m = rng.integers(0, hi, (N, 1), dtype=np.uint64)
    for i in bad:
        m[i, 0] = hi
    sk = lambda: np.stack([np.frombuffer(H.kem_private(rng, kem), np.uint8)  # noqa: E731
                           for _ in range(N)])
    keys = {}
    for who in ("leader", "helper"):
        skR = H.kem_private(rng, kem)
        keys[who] = (skR, H.kem_public(skR, kem))
    return dict(m=m, ids=rng.integers(0, 256, (N, 16), dtype=np.uint8),
                rand=rng.integers(0, 256, (N, 80), dtype=np.uint8),  # both have joint randomness
                times=(T0 + rng.integers(0, 7200, N)).astype(np.uint64),
                sk_l=sk(), sk_h=sk(), keys=keys,
                task=bytes(rng.integers(0, 256, 32, dtype=np.uint8)))


def _run(eng, c, kem, **kw):
    import torch
    from janus_amd import hpke as G
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
    ls = G.HpkeSealer(c["keys"]["leader"][1], INFO_LEADER, device=0, kem_id=kem)
    hs = G.HpkeSealer(c["keys"]["helper"][1], INFO_HELPER, device=0, kem_id=kem)
    args = dict(leader_sealer=ls, helper_sealer=hs, task_id=c["task"], time_precision=PRECISION,
                measurements=t(c["m"]), report_ids=t(c["ids"]), times=t(c["times"]),
                rand=t(c["rand"]), sk_e_leader=t(c["sk_l"]), sk_e_helper=t(c["sk_h"]),
                leader_config_id=CFG_LEADER, helper_config_id=CFG_HELPER)
    args.update(kw)
    out = eng.prepare_reports_device(**args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_report(c, o, name, kem, i, raw):
    """Every field of report i against the restatements; returns the parsed report."""
    r = _parse_report(raw)
    pub, lshare, hshare = o.shard(int(c["m"][i, 0]), c["ids"][i].tobytes(), c["rand"][i].tobytes())
    t = int(c["times"][i])
    assert r["report_id"] == c["ids"][i].tobytes()
    assert r["time"] == t - t % PRECISION and r["time"] % PRECISION == 0
    assert r["public_share"] == pub and len(pub) == 32
    aad = H.input_share_aad(c["task"], r["report_id"], r["time"], pub)
    for who, cfgid, info, share, sk in (("leader", CFG_LEADER, INFO_LEADER, lshare, c["sk_l"]),
                                        ("helper", CFG_HELPER, INFO_HELPER, hshare, c["sk_h"])):
        skR, pkR = c["keys"][who]
        pt = H.plaintext_input_share(share)
        enc, ct = H.seal(pkR, sk[i].tobytes(), info, aad, pt, kem=kem)
        assert r[who]["config_id"] == cfgid
        assert r[who]["enc"] == enc, who
        assert r[who]["payload"] == ct, who
        opened = H.open_(skR, pkR, r[who]["enc"], info, aad, r[who]["payload"], kem=kem)
        assert opened == b"\x00\x00" + len(share).to_bytes(4, "big") + share, who
    return r


@pytest.mark.parametrize("kem", [H.KEM_X25519, H.KEM_P256])
@pytest.mark.parametrize("name", ["hist_10_c3", "sum8"])
def test_one_call_parity(name, kem):
    eng, o = _engine(CONFIGS[name]), _oracle(CONFIGS[name])
    c = _case(name, kem)
    out = _run(eng, c, kem)
    assert not out["status"].any()
    assert (c["times"] % PRECISION != 0).any()  # the rounding is exercised
    parsed = [_check_report(c, o, name, kem, i, out["reports"][i, :out["report_len"][i]].tobytes())
              for i in range(N)]
    for i in range(N):
        assert not out["reports"][i, out["report_len"][i]:].any()
    # the helper's one-call init on the emitted helper ciphertexts, with the leader's prepare
    # shares from the emitted leader shares
    from janus_amd import hpke as G
    sz = eng.sz
    ids = np.stack([np.frombuffer(p["report_id"], np.uint8) for p in parsed])
    times = np.array([p["time"] for p in parsed], np.uint64)
    pub = np.stack([np.frombuffer(p["public_share"], np.uint8) for p in parsed]) \
        if sz.public_share_len else None
    lsk, lpk = c["keys"]["leader"]
    lshares = np.stack([np.frombuffer(H.open_(
        lsk, lpk, p["leader"]["enc"], INFO_LEADER,
        H.input_share_aad(c["task"], p["report_id"], p["time"], p["public_share"]),
        p["leader"]["payload"], kem=kem)[6:], np.uint8) for p in parsed])
    lps, lst, lbatch = eng.leader_prepare_init_batch(ids, pub, lshares)
    lbatch.free()
    assert not lst.any()
    cl = np.array([len(p["helper"]["payload"]) for p in parsed], np.uint32)
    stride = -(-int(cl.max()) // 16) * 16
    ct = np.zeros((N, stride), np.uint8)
    for i, p in enumerate(parsed):
        ct[i, :cl[i]] = np.frombuffer(p["helper"]["payload"], np.uint8)
    enc = np.stack([np.frombuffer(p["helper"]["enc"], np.uint8) for p in parsed])
    hsk, hpk = c["keys"]["helper"]
    opener = G.HpkeOpener(hsk, hpk, device=0, kem_id=kem)
    msgs, st, agg, cnt = eng.aggregate_init_batch(opener, c["task"], ids, times, pub, enc, ct, cl,
                                                  lps)
    assert not st.any() and int(cnt[0]) == N


@pytest.mark.parametrize("name", ["hist_10_c3", "sum8"])
def test_invalid_measurements_are_left_out(name):
    kem = H.KEM_X25519
    eng, o = _engine(CONFIGS[name]), _oracle(CONFIGS[name])
    bad = (3, 64)
    c = _case(name, kem, bad)
    out = _run(eng, c, kem)
    want = np.zeros(N, np.uint8)
    want[list(bad)] = 1
    assert np.array_equal(out["status"], want)
    good = _run(eng, _case(name, kem), kem)
    for i in range(N):
        if i in bad:
            assert out["report_len"][i] == 0 and not out["reports"][i].any()
        else:
            assert np.array_equal(out["reports"][i], good["reports"][i])
            assert out["report_len"][i] == good["report_len"][i]
    for i in (0, 63, 65, N - 1):
        _check_report(c, o, name, kem, i, out["reports"][i, :out["report_len"][i]].tobytes())


def test_argument_errors_raise():
    from janus_amd import hpke as G
    name, kem = "sum8", H.KEM_X25519
    eng = _engine(CONFIGS[name])
    c = _case(name, kem)
    with pytest.raises(ValueError):
        _run(eng, c, kem, time_precision=0)
    other = G.HpkeSealer(c["keys"]["helper"][1], INFO_HELPER, device=1, kem_id=kem)
    with pytest.raises(ValueError):
        _run(eng, c, kem, helper_sealer=other)
    with pytest.raises(ValueError):
        _run(eng, c, kem, report_stride=64)
    # the C entry point refuses a zero precision too (PRIO3_EINVAL)
    import ctypes as C
    from janus_amd import prio3 as J
    ls = G.HpkeSealer(c["keys"]["leader"][1], INFO_LEADER, device=0, kem_id=kem)
    tid = (C.c_uint8 * 32).from_buffer_copy(c["task"])
    rc = J.load_library().prio3_client_prepare_reports_device(
        eng.handle, ls.handle, ls.handle, N, tid, 0, None, None, None, None, None, None, 1, 2, 0,
        None, 1 << 20, None, None, None)
    assert rc == -1

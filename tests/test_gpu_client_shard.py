"""The client role on the device: prio3_client_shard_device / _batch (k_shard) against both CPU
restatements of prio's Prio3::shard, bit for bit -- caller-supplied measurements, nonces and
randomness, exact sampling (a real rejection included), invalid measurements, and the shares fed
through the leader and helper engines end to end."""
import functools
import json
import os

import numpy as np
import pytest

from tests.conftest import CONFIGS, ROOT
from tests.test_gpu_parity import VK, _engine, _oracle

pytestmark = pytest.mark.gpu

NAMES = ["count", "sum1", "sum8", "sum64", "sumvec_1x1_c1", "sumvec_8x10_c9", "hist_1_c1",
         "hist_10_c3", "hist_256_c16"]
SIZES = [1, 67, 130]


def _mstride(cfg):
    return cfg["length"] if cfg["kind"] == "sumvec" else 1


def _bound(cfg):
    """Exclusive upper bound of a valid measurement entry."""
    return {"count": 2, "histogram": cfg.get("length", 0)}.get(cfg["kind"], 1 << cfg.get("bits", 0))


def _rand_len(cfg):
    """prio 0.16's Sum, SumVec and Histogram circuits all take joint randomness; Count does not."""
    return 16 * (3 if cfg["kind"] == "count" else 5)


@functools.lru_cache(maxsize=None)
def _inputs(name, n, seed=7):
    """Random valid measurements [n, mstride] (uint64), nonces [n, 16], rand [n, rand_len]."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng([seed, n, sorted(CONFIGS).index(name)])
    hi = _bound(cfg)
    m = rng.integers(0, hi, (n, _mstride(cfg)), dtype=np.uint64, endpoint=False) if hi <= 1 << 63 \
        else rng.integers(0, 1 << 64, (n, _mstride(cfg)), dtype=np.uint64, endpoint=False)
    return (m, rng.integers(0, 256, (n, 16), dtype=np.uint8),
            rng.integers(0, 256, (n, _rand_len(cfg)), dtype=np.uint8))


def _meas_arg(cfg, row):
    return [int(x) for x in row] if cfg["kind"] == "sumvec" else int(row[0])


def _oracle_rows(name, m, nonces, rand):
    """Oracle.shard (the C restatement) of every report: (public, leader, helper) uint8 arrays."""
    cfg = CONFIGS[name]
    o = _oracle(cfg)
    rows = [o.shard(_meas_arg(cfg, m[i]), nonces[i].tobytes(), rand[i].tobytes())
            for i in range(len(m))]
    cat = lambda k: np.frombuffer(b"".join(r[k] for r in rows), np.uint8).reshape(  # noqa: E731
        len(rows), len(rows[0][k]))
    return cat(0), cat(1), cat(2)


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    return _oracle_rows(name, *_inputs(name, n))


def _shard_device(eng, m, nonces, rand):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = eng.shard_device(t(m.view(np.int64)), t(nonces), t(rand))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_rows(out, ref, rows=None):
    sel = slice(None) if rows is None else rows
    for k, r in zip(("public_shares", "leader_input_shares", "helper_shares"), ref):
        assert np.array_equal(out[k][sel], r[sel]), k


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_parity(name, n):
    from oracle.prio3_py import Prio3, Prio3Type
    cfg = CONFIGS[name]
    m, nonces, rand = _inputs(name, n)
    eng = _engine(cfg)
    out = _shard_device(eng, m, nonces, rand)
    assert not out["status"].any()
    _assert_rows(out, _reference(name, n))
    # the Python restatement on the first reports
    P = Prio3(Prio3Type(**cfg))
    for i in range(min(n, 8)):
        pub, leader, helper = P.shard(_meas_arg(cfg, m[i]), nonces[i].tobytes(), rand[i].tobytes())
        assert out["public_shares"][i].tobytes() == pub
        assert out["leader_input_shares"][i].tobytes() == leader
        assert out["helper_shares"][i].tobytes() == helper
    # the host-buffer form
    hb = eng.shard_batch(m, nonces, rand)
    for k in out:
        assert np.array_equal(hb[k], out[k]), k


@pytest.mark.parametrize("name", ["count", "hist_10_c3"])
def test_independent_of_the_verify_key(name):
    from janus_amd import prio3 as J
    cfg = CONFIGS[name]
    m, nonces, rand = _inputs(name, 67)
    a = _engine(cfg)
    b = J.HelperEngine(a.vdaf, bytes(range(0x90, 0xA0)), device=0)
    assert bytes(range(0x90, 0xA0)) != VK
    oa, ob = _shard_device(a, m, nonces, rand), _shard_device(b, m, nonces, rand)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k


BAD = [("count", 2), ("sum1", 2), ("sum8", 1 << 8), ("sumvec_8x10_c9", 1 << 8),
       ("sumvec_1x1_c1", 2), ("hist_10_c3", 10), ("hist_1_c1", 1), ("hist_256_c16", 256)]


@pytest.mark.parametrize("name,bad", BAD)
def test_invalid_measurements(name, bad):
    cfg = CONFIGS[name]
    n = 130
    m, nonces, rand = _inputs(name, n)
    eng = _engine(cfg)
    good = _shard_device(eng, m, nonces, rand)
    pos = [0, 63, 64, n - 1]
    m2 = m.copy()
    for j, i in enumerate(pos):
        m2[i, j % m2.shape[1]] = bad  # SumVec: one bad entry, a different one per report
    out = _shard_device(eng, m2, nonces, rand)
    want = np.zeros(n, np.uint8)
    want[pos] = 1
    assert np.array_equal(out["status"], want)
    keep = np.setdiff1d(np.arange(n), pos)
    for k in ("public_shares", "leader_input_shares", "helper_shares"):
        assert not out[k][pos].any(), k
        assert np.array_equal(out[k][keep], good[k][keep]), k
    _assert_rows(out, _reference(name, n), keep)


def test_sum64_takes_every_u64():
    """bits = 64: there is no invalid measurement; the extremes shard like any other."""
    cfg = CONFIGS["sum64"]
    m, nonces, rand = (a.copy() for a in _inputs("sum64", 67))
    m[0, 0], m[63, 0], m[66, 0] = (1 << 64) - 1, 1 << 63, 0
    out = _shard_device(_engine(cfg), m, nonces, rand)
    assert not out["status"].any()
    _assert_rows(out, _oracle_rows("sum64", m, nonces, rand))


@pytest.mark.parametrize("name", ["count", "sum8", "hist_10_c3", "sumvec_8x10_c9"])
def test_agrees_with_the_seeded_generator(name):
    """(nonce, rand, measurement) of (seed, i) derived as k_gen derives them, through shard_device:
    the generator's own outputs for every report it did not flag."""
    from oracle.oracle import turboshake128
    cfg = CONFIGS[name]
    n, seed, ms, rl = 67, 11, _mstride(cfg), _rand_len(cfg)
    eng = _engine(cfg)
    g = eng.generate_reports_device(n, seed=seed, with_checks=True, with_leader_inputs=True)
    g = {k: v.cpu().numpy() for k, v in g.items()}
    m = np.zeros((n, ms), np.uint64)
    nonces = np.zeros((n, 16), np.uint8)
    rand = np.zeros((n, rl), np.uint8)
    for i in range(n):
        s = turboshake128(b"janus-amd-gen" + seed.to_bytes(8, "little") + i.to_bytes(8, "little"),
                          1, 96 + 8 * ms)
        nonces[i] = np.frombuffer(s[:16], np.uint8)
        rand[i] = np.frombuffer(s[16:16 + rl], np.uint8)
        for e in range(ms):
            v = int.from_bytes(s[96 + 8 * e:104 + 8 * e], "little")
            if cfg["kind"] == "count":
                v &= 1
            elif cfg["kind"] == "histogram":
                v %= cfg["length"]
            else:
                v &= (1 << cfg["bits"]) - 1
            m[i, e] = v
    assert np.array_equal(m.view(np.int64), g["measurements"])
    out = _shard_device(eng, m, nonces, rand)
    ok = g["flags"] == 0
    assert ok.any()
    assert np.array_equal(nonces[ok], g["nonces"][ok])
    for k in ("public_shares", "helper_shares", "leader_input_shares"):
        assert np.array_equal(out[k][ok], g[k][ok]), k


@pytest.mark.parametrize("name", ["count", "sum8", "hist_10_c3", "sumvec_8x10_c9"])
def test_forced_slow_path(name):
    cfg = CONFIGS[name]
    m, nonces, rand = _inputs(name, 67)
    eng = _engine(cfg)
    eng.set_option("force_slow_path", 1)
    out = _shard_device(eng, m, nonces, rand)
    assert not out["status"].any()
    _assert_rows(out, _reference(name, 67))


def test_a_real_rejection():
    """tests/golden/client_reject_count.json: the helper measurement share's first candidate is
    >= p, so the fast block-wise expansion is wrong for this report and the lane must redo it
    through the rejection sampler."""
    from oracle.prio3_py import Prio3, Prio3Type, Xof
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "client_reject_count.json")))
    f_nonce, f_rand = bytes.fromhex(fx["nonce"]), bytes.fromhex(fx["rand"])
    P = Prio3(Prio3Type("count"))
    first = int.from_bytes(Xof(f_rand[:16], P.dst("meas"), b"\x01").next(8), "little")
    assert first >= 2**64 - 2**32 + 1  # the fixture really rejects
    m, nonces, rand = (a.copy() for a in _inputs("count", 67))
    m[5, 0] = fx["measurement"]
    nonces[5] = np.frombuffer(f_nonce, np.uint8)
    rand[5] = np.frombuffer(f_rand, np.uint8)
    out = _shard_device(_engine(CONFIGS["count"]), m, nonces, rand)
    assert not out["status"].any()
    ref = _oracle_rows("count", m, nonces, rand)
    _assert_rows(out, ref)
    assert out["leader_input_shares"][5].tobytes() == P.shard(fx["measurement"], f_nonce, f_rand)[1]


@pytest.mark.parametrize("name", ["count", "sum8", "sumvec_8x10_c9", "hist_10_c3"])
def test_end_to_end(name):
    """Device shares through the leader's prepare_init, the helper's prepare + aggregate and the
    leader's prepare_next + aggregate: every report verifies and the two aggregate shares
    unshard to the plaintext sum."""
    from oracle.oracle import decode_elems, field_modulus
    cfg = CONFIGS[name]
    n = 130
    m, nonces, rand = _inputs(name, n)
    eng = _engine(cfg)
    out = _shard_device(eng, m, nonces, rand)
    pub = out["public_shares"] if eng.sz.public_share_len else None
    lps, lst, lbatch = eng.leader_prepare_init_batch(nonces, pub, out["leader_input_shares"])
    assert not lst.any()
    msgs, hst, hagg, hcnt = eng.prepare_aggregate_batch(nonces, pub, out["helper_shares"], lps)
    assert not hst.any() and int(hcnt[0]) == n
    lst2, lagg, lcnt = lbatch.leader_prepare_next_aggregate(msgs, lst)
    lbatch.free()
    assert not lst2.any() and int(lcnt[0]) == n
    p = field_modulus(cfg["kind"])
    es = eng.sz.field_bytes
    got = [(a + b) % p for a, b in zip(decode_elems(lagg[0], es), decode_elems(hagg[0], es))]
    if cfg["kind"] == "histogram":
        want = np.bincount(m[:, 0].astype(np.int64), minlength=cfg["length"]).tolist()
    else:
        want = [int(x) for x in m.astype(object).sum(axis=0)]
    assert got == want

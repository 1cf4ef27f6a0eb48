"""The client role of Prio3SumVecField64MultiproofHmacSha256Aes128 on the device
(prio3_client_shard_device / _batch, k_shard_mp64): caller-supplied measurements, nonces and 160
bytes of randomness, bit for bit against the Python restatement of prio's Prio3::shard
(oracle/prio3_py.py; the C restatement's shard does not take 32-byte seeds) -- exact sampling with a
real rejection, invalid measurements, the 65,536-report chunk boundary -- and the shares through the
device's own leader and helper engines (which tests/test_mp64.py pins to both restatements)."""
import functools
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

VK = bytes(range(0x40, 0x60))
P64 = 2**64 - 2**32 + 1
# (proofs, bits, length, chunk): one element and one gadget call; 80 elements in 27 calls, so a
# padded last call; three proofs with calls dividing exactly; the reference's own instance, whose
# calls + 1 equal the 16-point domain
SHAPES = [(2, 1, 1, 1), (2, 8, 10, 3), (3, 4, 9, 4), (2, 16, 15, 16)]
NMAX = 130
FIXTURE = os.path.join(ROOT, "tests", "golden", "client_reject_mp64.json")


@functools.lru_cache(maxsize=None)
def _vdaf(shape):
    from oracle.prio3_py import Prio3, Prio3Type
    proofs, bits, length, chunk = shape
    return Prio3(Prio3Type("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk,
                           num_proofs=proofs))


@functools.lru_cache(maxsize=None)
def _engine(shape, vk=VK):
    from janus_amd import prio3 as J
    return J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(*shape), vk, device=0)


@functools.lru_cache(maxsize=None)
def _all_inputs(shape):
    """NMAX random valid reports of a shape, read-only: measurements [NMAX, length] (uint64),
    nonces [NMAX, 16], rand [NMAX, 160].  Every batch of n is their first n rows, so one Python
    shard per row serves all the tests (this file's and tests/test_gpu_client_reports_mp64.py's)."""
    _, bits, length, _ = shape
    rng = np.random.default_rng([7, *shape])
    out = (rng.integers(0, 1 << bits, (NMAX, length), dtype=np.uint64),
           rng.integers(0, 256, (NMAX, 16), dtype=np.uint8),
           rng.integers(0, 256, (NMAX, 160), dtype=np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


def _inputs(shape, n):
    return tuple(a[:n] for a in _all_inputs(shape))


def _py_shard(shape, m, nonce, rand):
    return _vdaf(shape).shard([int(x) for x in m], nonce.tobytes(), rand.tobytes())


@functools.lru_cache(maxsize=None)
def _ref_row(shape, i):
    """(public, leader, helper) of row i of _all_inputs: the Python restatement's shard."""
    m, nonces, rand = _all_inputs(shape)
    return _py_shard(shape, m[i], nonces[i], rand[i])


def _shard_device(eng, m, nonces, rand):
    import torch
    t = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731 (a copy: inputs are read-only)
    out = eng.shard_device(t(m.view(np.int64)), t(nonces), t(rand))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


KEYS = ("public_shares", "leader_input_shares", "helper_shares")


def _assert_row(out, i, ref):
    for k, want in zip(KEYS, ref):
        assert out[k][i].tobytes() == want, (i, k)


@pytest.mark.parametrize("shape,n", [(s, n) for s in SHAPES[:2] for n in (1, 67, NMAX)] +
                         [(s, 67) for s in SHAPES[2:]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_parity(shape, n):
    m, nonces, rand = _inputs(shape, n)
    eng = _engine(shape)
    sz = eng.sz
    assert eng.rand_len == 160 and sz.public_share_len == 64 and sz.helper_share_len == 96
    out = _shard_device(eng, m, nonces, rand)
    assert not out["status"].any()
    for i in range(n):
        _assert_row(out, i, _ref_row(shape, i))
    hb = eng.shard_batch(m, nonces, rand)  # the host-buffer form
    for k in out:
        assert np.array_equal(hb[k], out[k]), k


def test_invalid_measurements():
    """An entry >= 2^bits (SumVec::encode_measurement's check; the Python restatement's encode
    does not make it): status 1 and three zero rows, the other lanes of both waves untouched."""
    shape = SHAPES[1]
    bits, n = shape[1], 67
    m, nonces, rand = _inputs(shape, n)
    bad = {0: (0, 1 << bits), 31: (3, (1 << 64) - 1), 63: (9, 1 << bits), 64: (5, (1 << 64) - 1),
           66: (7, 1 << bits)}
    m2 = m.copy()
    for i, (pos, v) in bad.items():
        m2[i, pos] = v
    out = _shard_device(_engine(shape), m2, nonces, rand)
    want = np.zeros(n, np.uint8)
    want[list(bad)] = 1
    assert np.array_equal(out["status"], want)
    for i in range(n):
        if i in bad:
            for k in KEYS:
                assert not out[k][i].any(), (i, k)
        else:
            _assert_row(out, i, _ref_row(shape, i))


def test_a_real_rejection():
    """tests/golden/client_reject_mp64.json (tools/find_reject_mp64.py): a candidate of the helper
    measurement share's stream is >= p, so every later element of that share moves up one
    candidate.  The rejecting report sits between two ordinary ones of the same wave."""
    from oracle.prio3_py import XofHmacSha256Aes128
    fx = json.load(open(FIXTURE))
    shape = (fx["num_proofs"], fx["bits"], fx["length"], fx["chunk_length"])
    v = _vdaf(shape)
    f_rand = bytes.fromhex(fx["rand"])
    assert f_rand[:32] == bytes.fromhex(fx["seed"])
    idx = fx["element_index"]
    stream = XofHmacSha256Aes128(f_rand[:32], v.dst("meas"), b"\x01").next(8 * (idx + 1))
    assert int.from_bytes(stream[8 * idx:], "little") >= P64  # the fixture really rejects
    rng = np.random.default_rng(23)
    m = rng.integers(0, 1 << shape[1], (3, shape[2]), dtype=np.uint64)
    nonces = rng.integers(0, 256, (3, 16), dtype=np.uint8)
    rand = rng.integers(0, 256, (3, 160), dtype=np.uint8)
    m[1] = np.array(fx["measurement"], np.uint64)
    nonces[1] = np.frombuffer(bytes.fromhex(fx["nonce"]), np.uint8)
    rand[1] = np.frombuffer(f_rand, np.uint8)
    out = _shard_device(_engine(shape), m, nonces, rand)
    assert not out["status"].any()
    for i in range(3):
        _assert_row(out, i, _py_shard(shape, m[i], nonces[i], rand[i]))


def test_chunk_boundary():
    """65,600 reports: one launch of 65,536 and one of 64 on the same scratch columns."""
    shape = SHAPES[0]
    n, C = 65_600, 65_536
    rng = np.random.default_rng(41)
    m = rng.integers(0, 2, (n, 1), dtype=np.uint64)
    nonces = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    rand = rng.integers(0, 256, (n, 160), dtype=np.uint8)
    eng = _engine(shape)
    out = _shard_device(eng, m, nonces, rand)
    assert not out["status"].any()
    for i in list(range(8)) + list(range(C - 8, n)):
        _assert_row(out, i, _py_shard(shape, m[i], nonces[i], rand[i]))
    tail = _shard_device(eng, m[C:], nonces[C:], rand[C:])
    for k in out:
        assert np.array_equal(out[k][C:], tail[k]), k


def test_end_to_end():
    """Device shares through the leader's prepare_init, the helper's prepare, then prepare_next
    and aggregate on both sides: every report is accepted and the two aggregate shares unshard to
    the measurements' column sums."""
    shape = SHAPES[3]
    n, length = 67, shape[2]
    m, nonces, rand = _inputs(shape, n)
    eng = _engine(shape)
    out = _shard_device(eng, m, nonces, rand)
    assert not out["status"].any()
    pub = out["public_shares"]
    lps, lst, lbatch = eng.leader_prepare_init_batch(nonces, pub, out["leader_input_shares"])
    assert not lst.any()
    msgs, hst, hagg, hcnt = eng.prepare_aggregate_batch(nonces, pub, out["helper_shares"], lps)
    assert not hst.any() and int(hcnt[0]) == n
    lst2, lagg, lcnt = lbatch.leader_prepare_next_aggregate(msgs, lst)
    lbatch.free()
    assert not lst2.any() and int(lcnt[0]) == n
    dec = lambda a: [int.from_bytes(a[0, 8 * e:8 * e + 8].tobytes(), "little")  # noqa: E731
                     for e in range(length)]
    got = [(a + b) % P64 for a, b in zip(dec(lagg), dec(hagg))]
    assert got == [int(x) for x in m.astype(object).sum(axis=0)]


def test_independent_of_the_verify_key():
    shape = SHAPES[1]
    other = bytes(range(0x90, 0xB0))
    assert other != VK and len(other) == 32
    m, nonces, rand = _inputs(shape, 67)
    oa = _shard_device(_engine(shape), m, nonces, rand)
    ob = _shard_device(_engine(shape, other), m, nonces, rand)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k

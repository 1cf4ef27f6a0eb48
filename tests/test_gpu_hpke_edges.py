"""The HPKE openers' device arithmetic at its edges, on the GPU:

* GF(2^255 - 19) (janus_hpke_selftest_field, field 0): the five generated asm routines bit-equal
  to the CPU model of tests/asm_model.py on the edge x edge cross product (which takes every
  conditional second fold) and random pairs, and fe_inv / fe_freeze / one ladder step against
  Python integers;
* X448 and P-521 products on the limbs that add / sub / mul_small leave (ops 6..9);
* open at edge ephemeral points (low-order, non-canonical, bit 255 set, j G for edge j, x >= p),
  ciphertexts from the oracle's recipient-side seal, through `open` and `open_input_shares`;
* edge private keys for P-521, X25519 and X448;
* the plaintext / AAD length grid through the generic open.

Everything is bit-exact; there are no tolerances."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import hpke as H
from tests import asm_model as M
from tests import test_hpke_edges as E
from tests import test_limb_bounds as LB
from tests.test_gpu_hpke_seal import AAD_LENS, PT_LENS

pytestmark = pytest.mark.gpu

P = M.P25519
INFO = H.INFO_INPUT_SHARE_HELPER


def _field(field, op, a, b, nw):
    from janus_amd import hpke as G
    enc = lambda xs: np.frombuffer(b"".join(x.to_bytes(4 * nw, "little") for x in xs),  # noqa
                                   np.uint32).copy()
    A, B = enc(a), enc(b)
    out = np.zeros_like(A)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert len(a) == len(b) <= 1 << 15
    assert G._lib().janus_hpke_selftest_field(field, op, len(a), ptr(A), ptr(B), ptr(out)) == 0
    raw = out.tobytes()
    return [int.from_bytes(raw[4 * nw * i:4 * nw * (i + 1)], "little") for i in range(len(a))]


# ---- B. GF(2^255 - 19) ---------------------------------------------------------------------
@pytest.mark.parametrize("op", range(5), ids=M.FE_OPS)
def test_gpu_fe25519_asm_is_bit_equal_to_the_model(op):
    """Ops 0..4 on the edge x edge cross product and 4,096 random pairs: the device's eight raw
    words equal the model's (which also validates the model against the hardware), are below
    2^256 and congruent to the Python integer result mod p."""
    a, b, ne = M.operands_25519()
    got = _field(0, op, a, b, 8)
    model = M.model_25519(op)
    assert sum(f for _, f in model[:ne]) > 0   # these operands do take the second fold
    diff = [i for i in range(len(a)) if got[i] != model[i][0]]
    assert not diff, (f"{M.FE_OPS[op]}: device and model differ on {len(diff)} operands, first "
                      f"a={a[diff[0]]:#x} b={b[diff[0]]:#x}: device {got[diff[0]]:#x} model "
                      f"{model[diff[0]][0]:#x}")
    fn = M.FE_PY[op]
    bad = [i for i in range(len(a)) if got[i] >= 2**256 or (got[i] - fn(a[i], b[i])) % P]
    assert not bad, f"{M.FE_OPS[op]}: {len(bad)} wrong, first a={a[bad[0]]:#x} b={b[bad[0]]:#x}"


def _unary_operands(n, seed):
    e = M.edge_25519()
    rnd = random.Random(seed)
    return e + [rnd.randrange(2**256) for _ in range(n - len(e))]


def test_gpu_fe25519_inv():
    a = _unary_operands(2048, 5)
    got = _field(0, 5, a, a, 8)
    bad = [i for i in range(len(a)) if got[i] >= 2**256 or (got[i] - pow(a[i], P - 2, P)) % P]
    assert not bad, f"fe_inv: {len(bad)} wrong, first a={a[bad[0]]:#x} got {got[bad[0]]:#x}"
    assert a[0] == 0 and got[0] == 0
    assert all(got[i] % P == 0 for i in range(len(a)) if a[i] % P == 0)


def test_gpu_fe25519_freeze():
    a = _unary_operands(4096, 6)
    subs = [sum(1 for x in a if x // P == k) for k in range(3)]   # 2^256 - 1 < 3p
    assert all(s > 0 for s in subs), f"zero / one / two subtractions: {subs}"
    for x in (P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 2**256 - 1):
        assert x in a
    got = _field(0, 6, a, a, 8)
    bad = [i for i in range(len(a)) if got[i] != a[i] % P]
    assert not bad, f"fe_freeze: {len(bad)} wrong, first a={a[bad[0]]:#x} got {got[bad[0]]:#x}"


def _ladder_step(a, b):
    x1, x2, z2, x3, z3 = a, a, b, b, a
    A, B = x2 + z2, x2 - z2
    AA, BB = A * A, B * B
    Ee = AA - BB
    Cc, D = x3 + z3, x3 - z3
    DA, CB = D * A, Cc * B
    x3 = (DA + CB) ** 2
    z3 = x1 * (DA - CB) ** 2
    x2 = AA * BB
    z2 = Ee * (AA + 121665 * Ee)
    return (x2 * z3 + x3 * z2) % P


def test_gpu_fe25519_ladder_step():
    a, b, _ = M.operands_25519()
    got = _field(0, 7, a, b, 8)
    bad = [i for i in range(len(a)) if got[i] != _ladder_step(a[i], b[i])]
    assert not bad, f"ladder step: {len(bad)} wrong, first a={a[bad[0]]:#x} b={b[bad[0]]:#x}"


def test_selftest_field_rejects_ops_out_of_range():
    from janus_amd import hpke as G
    z = np.zeros(17, np.uint32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for field, op in ((0, 8), (1, 10), (2, 10), (3, 6), (4, 0), (-1, 0), (0, -1)):
        assert G._lib().janus_hpke_selftest_field(field, op, 1, ptr(z), ptr(z), ptr(z)) == -1


# ---- C. X448 / P-521 products on the limbs they meet in use -----------------------------------
@pytest.mark.parametrize("op", LB.CHAINED_OPS)
@pytest.mark.parametrize("field", [1, 2])
def test_gpu_x448_p521_chained_products(field, op):
    """mul / sqr of what add, sub and mul_small leave (limbs 0 and 8, or limb 0, above their
    nominal width; tests/test_limb_bounds.py checks the headers' bounds on the same operands),
    against Python integers: results canonical."""
    a, b = LB.chained_operands(field)
    got = _field(field, op, a, b, 14 if field == 1 else 17)
    bad = [i for i in range(len(a)) if got[i] != LB.chained_int(field, op, a[i], b[i])]
    assert not bad, (f"field {field} op {op}: {len(bad)} wrong, first a={a[bad[0]]:x} "
                     f"b={b[bad[0]]:x}")


# ---- D. open at edge ephemeral points ---------------------------------------------------------
def _open_rows(kem, skR, pkR, rows, seed, aead=1):
    """Generic-open rows: (encs, cts, aads, expected plaintexts (None where refused))."""
    rng = np.random.default_rng(seed)
    kdf = E.KEM_KDF[kem]
    encs, cts, aads, want = [], [], [], []
    for i, (enc, refused) in enumerate(rows):
        pt = rng.integers(0, 256, PT_LENS[i % len(PT_LENS)], dtype=np.uint8).tobytes()
        aad = rng.integers(0, 256, AAD_LENS[i % len(AAD_LENS)], dtype=np.uint8).tobytes()
        ct = H.seal_to_enc(skR, pkR, enc, INFO, aad, pt, aead=aead, kem=kem, kdf=kdf)
        assert (ct is None) == refused
        if refused:
            ct = rng.integers(0, 256, len(pt) + 16, dtype=np.uint8).tobytes()
        encs.append(enc), cts.append(ct), aads.append(aad)
        want.append(None if refused else pt)
    return encs, cts, aads, want


def _input_share_rows(kem, skR, pkR, rows, seed):
    """Janus-shaped rows (InputShareAad, PlaintextInputShare) sealed to the given enc values."""
    rng = np.random.default_rng(seed)
    kdf = E.KEM_KDF[kem]
    n, share_len = len(rows), 48
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = (1_700_000_000 + rng.integers(0, 3600, n)).astype(np.uint64)
    pubs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    shares = rng.integers(0, 256, (n, share_len), dtype=np.uint8)
    stride = 6 + share_len + 16
    enc = np.zeros((n, H.NENC[kem]), np.uint8)
    ct = rng.integers(0, 256, (n, stride), dtype=np.uint8)   # any bytes for the refused points
    cl = np.full(n, stride, np.uint32)
    for r, (e, refused) in enumerate(rows):
        enc[r] = np.frombuffer(e, np.uint8)
        aad = H.input_share_aad(task, ids[r].tobytes(), int(times[r]), pubs[r].tobytes())
        c = H.seal_to_enc(skR, pkR, e, INFO, aad, H.plaintext_input_share(shares[r].tobytes()),
                          kem=kem, kdf=kdf)
        assert (c is None) == refused
        if not refused:
            ct[r] = np.frombuffer(c, np.uint8)
    return dict(task_id=task, enc=enc, ct=ct, ct_len=cl, report_ids=ids, times=times, pubs=pubs,
                shares=shares, share_len=share_len)


def _check_both_entry_points(kem, skR, rows, seed, pair_max=None):
    from janus_amd import hpke as G
    pkR = H.kem_public(skR, kem)
    kdf = E.KEM_KDF[kem]
    refused = np.array([r for _, r in rows])
    assert refused.any() and not refused.all()
    op = G.HpkeOpener(skR, pkR, info=INFO, kem_id=kem, kdf_id=kdf)
    if pair_max is not None:
        op.executor_control("pair_max", pair_max)
    # janus_hpke_open
    encs, cts, aads, want = _open_rows(kem, skR, pkR, rows, seed)
    got = op.open(encs, cts, aads)
    for i in range(len(rows)):
        assert got[i] == want[i], (i, encs[i].hex(), "refused" if refused[i] else "accepted")
    # janus_hpke_open_input_shares: statuses as the restatement gives them for the same rows
    d = _input_share_rows(kem, skR, pkR, rows, seed + 1)
    ref_sh, ref_st = H.open_input_shares(skR, pkR, d["task_id"], d["enc"], d["ct"], d["ct_len"],
                                         d["report_ids"], d["times"], d["pubs"], d["share_len"],
                                         kem=kem, kdf=kdf)
    assert ((ref_st != 0) == refused).all()
    np.testing.assert_array_equal(ref_sh[~refused], d["shares"][~refused])
    sh, st = op.open_input_shares(d["task_id"], d["enc"], d["ct"], d["ct_len"], d["report_ids"],
                                  d["times"], d["pubs"], d["share_len"])
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(sh, ref_sh)
    op.close()


@pytest.mark.parametrize("pair_max", [65536, 0], ids=["lane_pair", "one_lane"])
def test_gpu_x25519_open_at_edge_points(pair_max):
    """The 14 low-order encodings fail their own row only; p + k (2 <= k <= 18), 2^255 + 9,
    2^256 - 1 and ordinary points open, on both ladders and through both entry points."""
    rows = E.xdh_points(H.KEM_X25519)
    assert len(rows) == 14 + 22
    for seed, skR in enumerate([H.kem_private(np.random.default_rng(1), H.KEM_X25519),
                                b"\xff" * 32]):
        _check_both_entry_points(H.KEM_X25519, skR, rows, 10 + 2 * seed, pair_max)


def test_gpu_x448_open_at_edge_points():
    rows = E.xdh_points(H.KEM_X448)
    skR = H.kem_private(np.random.default_rng(2), H.KEM_X448)
    _check_both_entry_points(H.KEM_X448, skR, rows, 20)


P256_EDGE_KEYS = [1, 2, 3, 6, 14, 15, 16, 18, 30, E.P256_N - 1, E.P256_N - 2, E.P256_N - 6,
                  E.P256_N - 14, E.P256_N - 15, E.P256_N - 18, E.P256_N - 30, E.P256_N - 31,
                  2**255, 0x1234567 << 200]
P384_EDGE_KEYS = [1, 2, 3, 6, 15, 16, 30, E.P384_N - 1, E.P384_N - 2, E.P384_N - 6, E.P384_N - 30,
                  E.P384_N - 31, 2**383, 0x1234567 << 300]
P521_EDGE_KEYS = [1, 2, 3, 6, 15, 16, 30, E.P521_N - 1, E.P521_N - 2, E.P521_N - 6, E.P521_N - 30,
                  E.P521_N - 31, 2**520, 0x1234567 << 400]
NIST_EDGE_KEYS = {H.KEM_P256: P256_EDGE_KEYS, H.KEM_P384: P384_EDGE_KEYS,
                  H.KEM_P521: P521_EDGE_KEYS}


def _key_id(kem, sk):
    n = E.KEM_ORDER[kem]
    return f"kem{kem:#x}-" + (f"n-{n - sk}" if n - sk < 64 else str(sk) if sk < 64 else
                              f"2^{sk.bit_length() - 1}" if sk & (sk - 1) == 0 else f"{sk:#x}"[:12])


@pytest.mark.parametrize("kem,sk", [pytest.param(k, s, id=_key_id(k, s))
                                    for k in NIST_EDGE_KEYS for s in NIST_EDGE_KEYS[k]])
def test_gpu_nist_open_at_edge_points_and_keys(kem, sk):
    """enc = j G for j in {1, 2, 3, 15, 16, 17, n - 1, n - 2} under each edge private key: the
    window's table entries and the running point coincide or are opposite somewhere in the
    walk.  A point with x >= p is refused, for its row only."""
    rows = E.nist_points(kem)
    _check_both_entry_points(kem, sk.to_bytes(H.NSK[kem], "big"), rows, sk % 1009)


# ---- F. edge private keys ------------------------------------------------------------------
def _open_batch_as_oracle(kem, skR, seed):
    from janus_amd import hpke as G
    kdf = E.KEM_KDF[kem]
    d = H.make_batch(8, 48, 32, seed=seed, skR=skR, kem=kem, kdf=kdf)
    ref_sh, ref_st = H.open_input_shares(d["skR"], d["pkR"], d["task_id"], d["enc"], d["ct"],
                                         d["ct_len"], d["report_ids"], d["times"], d["pubs"], 48,
                                         kem=kem, kdf=kdf)
    assert (ref_st == 0).all()
    op = G.HpkeOpener(d["skR"], d["pkR"], kem_id=kem, kdf_id=kdf)
    sh, st = op.open_input_shares(d["task_id"], d["enc"], d["ct"], d["ct_len"], d["report_ids"],
                                  d["times"], d["pubs"], 48)
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(sh, ref_sh)
    op.close()


@pytest.mark.parametrize("sk", [pytest.param(s, id=_key_id(H.KEM_P521, s))
                                for s in P521_EDGE_KEYS])
def test_gpu_p521_edge_private_keys(sk):
    """DHKEM(P-521, HKDF-SHA512): ecdh_a3.h's fixed signed window over the host recoding (131
    digits) for even keys (run as n - sk), keys whose last window meets the doubling case, tiny
    and near-n keys, against the OpenSSL oracle."""
    n1 = H.kem_public((E.P521_N - 1).to_bytes(66, "big"), H.KEM_P521)
    assert n1[:67] == H.kem_public((1).to_bytes(66, "big"), H.KEM_P521)[:67]   # n is the order
    _open_batch_as_oracle(H.KEM_P521, sk.to_bytes(66, "big"), sk % 983)


X25519_EDGE_KEYS = {"zero": bytes(32), "ones": b"\xff" * 32,
                    "low3": bytes([0x57]) + bytes(range(1, 31)) + bytes([0x40]),
                    "bit254_clear": bytes(range(8, 39)) + bytes([0x3f]),
                    "bit255_set": bytes(range(16, 47)) + bytes([0xc5])}
X448_EDGE_KEYS = {"zero": bytes(56), "ones": b"\xff" * 56,
                  "low2": bytes([0x53]) + bytes(range(1, 55)) + bytes([0x80]),
                  "bit447_clear": bytes(range(8, 63)) + bytes([0x7f])}


@pytest.mark.parametrize("name", X25519_EDGE_KEYS)
def test_gpu_x25519_private_keys_are_clamped(name):
    """decodeScalar25519 on the host (the low three bits, bit 255, bit 254): each key opens as
    OpenSSL, which clamps it."""
    _open_batch_as_oracle(H.KEM_X25519, X25519_EDGE_KEYS[name], 31)


@pytest.mark.parametrize("name", X448_EDGE_KEYS)
def test_gpu_x448_private_keys_are_clamped(name):
    """decodeScalar448 on the host (the low two bits, bit 447)."""
    _open_batch_as_oracle(H.KEM_X448, X448_EDGE_KEYS[name], 37)


# ---- G. the length grid through the generic open -------------------------------------------
@pytest.mark.parametrize("kem,aead", [(H.KEM_X25519, 1), (H.KEM_X25519, 2), (H.KEM_X25519, 3),
                                      (H.KEM_P256, 1)])
def test_gpu_open_length_grid(kem, aead):
    """Every plaintext x AAD length pair of the seal test, sealed by the oracle: the device open
    returns the plaintext; the same row with the last tag byte flipped fails; rows with ct_len
    0, 1 and 15 fail and leave their neighbours intact."""
    from janus_amd import hpke as G
    rng = np.random.default_rng(1000 * kem + aead)
    skR = H.kem_private(rng, kem)
    pkR = H.kem_public(skR, kem)
    encs, cts, aads, want = [], [], [], []
    short = {3: 0, 20: 1, 50: 15}   # length pair -> a ciphertext of this many bytes before it
    pairs = [(pl, al) for pl in PT_LENS for al in AAD_LENS]
    for j, (pl, al) in enumerate(pairs):
        pt = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
        aad = rng.integers(0, 256, al, dtype=np.uint8).tobytes()
        enc, ct = H.seal(pkR, H.kem_private(rng, kem), INFO, aad, pt, aead=aead, kem=kem)
        if j in short:
            encs.append(enc), aads.append(aad), want.append(None)
            cts.append(rng.integers(0, 256, short.pop(j), dtype=np.uint8).tobytes())
        bad = bytearray(ct)
        bad[-1] ^= 1
        encs += [enc, enc]
        cts += [ct, bytes(bad)]
        aads += [aad, aad]
        want += [pt, None]
    assert not short and len(cts) == 2 * len(PT_LENS) * len(AAD_LENS) + 3
    op = G.HpkeOpener(skR, pkR, info=INFO, kem_id=kem, aead_id=aead)
    got = op.open(encs, cts, aads)
    bad = [i for i in range(len(cts)) if got[i] != want[i]]
    assert not bad, (f"{len(bad)} rows wrong, first row {bad[0]}: ct_len {len(cts[bad[0]])} "
                     f"aad_len {len(aads[bad[0]])}")
    op.close()

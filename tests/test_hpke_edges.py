"""Edge ephemeral points for the HPKE openers, without a GPU: the point lists the device tests
(tests/test_gpu_hpke_edges.py, tests/test_gpu_hpke_seal.py) walk, a plain RFC 7748 ladder on
Python integers as the arbiter of which X25519 / X448 points Decap must refuse (an all-zero
output), and the oracle's recipient-side seal (oracle/hpke.py seal_to_enc), which produces a
valid ciphertext for a chosen enc -- nobody knows the ephemeral private key of a low-order or
non-canonical point, so the sender-side seal cannot."""
import numpy as np
import pytest

from oracle import hpke as H

P25519 = 2**255 - 19
P448 = 2**448 - 2**224 - 1
P256_N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
P384_N = int("ff" * 24 + "c7634d81f4372ddf581a0db248b0a77aecec196accc52973", 16)
P521_N = int("01" + "ff" * 32 + "fa51868783bf2f966b7fcc0148f709a5d03bb5c9b8899c47aebb6fb71e913864"
             "09", 16)
KEM_ORDER = {H.KEM_P256: P256_N, H.KEM_P384: P384_N, H.KEM_P521: P521_N}
KEM_KDF = {H.KEM_X25519: 1, H.KEM_P256: 1, H.KEM_X448: 3, H.KEM_P521: 3, H.KEM_P384: 2}
ALL_KEMS = (H.KEM_X25519, H.KEM_X448, H.KEM_P256, H.KEM_P384, H.KEM_P521)


# ---- RFC 7748 section 5 on Python integers ---------------------------------------------------
def _ladder(k, u, p, bits, a24):
    x1, x2, z2, x3, z3, swap = u, 1, 0, u, 1, 0
    for t in reversed(range(bits)):
        kt = k >> t & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        A, B = (x2 + z2) % p, (x2 - z2) % p
        AA, BB = A * A % p, B * B % p
        E = (AA - BB) % p
        C, D = (x3 + z3) % p, (x3 - z3) % p
        DA, CB = D * A % p, C * B % p
        x3 = (DA + CB) ** 2 % p
        z3 = x1 * (DA - CB) ** 2 % p
        x2 = AA * BB % p
        z2 = E * (AA + a24 * E) % p
    if swap:
        x2, z2 = x3, z3
    return x2 * pow(z2, p - 2, p) % p


def x25519(k: bytes, u: bytes) -> bytes:
    ki = int.from_bytes(k, "little") & ~7 & (2**255 - 1) | 2**254   # decodeScalar25519
    ui = int.from_bytes(u, "little") & (2**255 - 1)                  # decodeUCoordinate
    return _ladder(ki, ui % P25519, P25519, 255, 121665).to_bytes(32, "little")


def x448(k: bytes, u: bytes) -> bytes:
    ki = int.from_bytes(k, "little") & ~3 | 2**447                   # decodeScalar448
    return _ladder(ki, int.from_bytes(u, "little") % P448, P448, 448, 39081).to_bytes(56, "little")


XDH = {H.KEM_X25519: x25519, H.KEM_X448: x448}

# ---- the points ------------------------------------------------------------------------------
X25519_LOW_ORDER_U = [
    0, 1, 325606250916557431795983626356110631294008115727848805560023387167927233504,
    39382357235489614581723060781553021112529911719440698176882885853963445705823,
    P25519 - 1, P25519, P25519 + 1]
# the seven low-order u, each with bit 255 clear and set: Decap refuses all 14
X25519_REFUSED = [u | hi << 255 for u in X25519_LOW_ORDER_U for hi in (0, 1)]
# non-canonical p + k up to 2^255 - 1, bit 255 set, and ordinary points: all accepted
X25519_ACCEPTED = [P25519 + k for k in range(2, 19)] + [2**255 + 9, 2**256 - 1, 2, 9, P25519 - 2]
X448_REFUSED = [0, 1, P448 - 1, P448, P448 + 1]
X448_ACCEPTED = [P448 + 2, 2**448 - 1, 2**448 - 2, 2**447, 2**224, 2**224 - 1, 5, P448 - 2]
NIST_ENC_SCALARS = lambda n: [1, 2, 3, 15, 16, 17, n - 1, n - 2]  # noqa: E731  enc = j G


def xdh_points(kem):
    """[(enc bytes, refused)] with ordinary rows interleaved between the refused ones."""
    nb = H.NENC[kem]
    bad, good = ((X25519_REFUSED, X25519_ACCEPTED) if kem == H.KEM_X25519
                 else (X448_REFUSED, X448_ACCEPTED))
    rows = []
    for i in range(max(len(bad), len(good))):
        if i < len(bad):
            rows.append((bad[i].to_bytes(nb, "little"), True))
        if i < len(good):
            rows.append((good[i].to_bytes(nb, "little"), False))
    return rows


def nist_points(kem):
    """[(enc bytes, refused)]: j G for the edge j, and one point with x >= p."""
    n = KEM_ORDER[kem]
    nsk = H.NSK[kem]
    rows = [(H.kem_public(j.to_bytes(nsk, "big"), kem), False) for j in NIST_ENC_SCALARS(n)]
    g = rows[0][0]
    big_x = {H.KEM_P256: b"\xff" * 32, H.KEM_P384: b"\xff" * 48,
             H.KEM_P521: b"\x01" + b"\xff" * 65}[kem]                # P-521: x = p itself
    rows.insert(4, (b"\x04" + big_x + g[1 + nsk:], True))
    return rows


def edge_points(kem):
    return xdh_points(kem) if kem in XDH else nist_points(kem)


# ---- tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kem", (H.KEM_X25519, H.KEM_X448))
def test_python_ladder_matches_openssl_public_keys(kem):
    rng = np.random.default_rng(kem)
    base = (9 if kem == H.KEM_X25519 else 5).to_bytes(H.NENC[kem], "little")
    edge = [bytes(H.NSK[kem]), b"\xff" * H.NSK[kem]]
    for sk in edge + [H.kem_private(rng, kem) for _ in range(6)]:
        assert XDH[kem](sk, base) == H.kem_public(sk, kem)


def test_low_order_points_are_low_order():
    for u in X25519_LOW_ORDER_U:
        assert _ladder(8, u % P25519, P25519, 4, 121665) == 0, u   # cofactor 8 kills them
    assert x25519(b"\x55" * 32, (2**255 + 9).to_bytes(32, "little")) == \
        x25519(b"\x55" * 32, (9).to_bytes(32, "little"))
    k = b"\x37" * 56  # 2^224 and 2^224 - 1 are inverses of each other: the same u-line output
    assert (2**224) * (2**224 - 1) % P448 == 1
    assert x448(k, (2**224).to_bytes(56, "little")) == x448(k, (2**224 - 1).to_bytes(56, "little"))


@pytest.mark.parametrize("kem", (H.KEM_X25519, H.KEM_X448))
def test_oracle_accepts_exactly_the_points_with_a_nonzero_ladder_output(kem):
    rng = np.random.default_rng(100 + kem)
    rows = xdh_points(kem)
    assert sum(r for _, r in rows) == (14 if kem == H.KEM_X25519 else 5)
    for skR in [H.kem_private(rng, kem) for _ in range(2)] + [bytes(H.NSK[kem])]:
        pkR = H.kem_public(skR, kem)
        for enc, refused in rows:
            dh = XDH[kem](skR, enc)
            assert (dh == bytes(len(dh))) == refused, enc.hex()
            ct = H.seal_to_enc(skR, pkR, enc, b"info", b"aad", b"plaintext", kem=kem,
                               kdf=KEM_KDF[kem])
            assert (ct is None) == refused, enc.hex()
            if refused:
                assert H.open_(skR, pkR, enc, b"info", b"aad", bytes(25), kem=kem,
                               kdf=KEM_KDF[kem]) is None


@pytest.mark.parametrize("aead", [1, 2, 3])
@pytest.mark.parametrize("kem", ALL_KEMS)
def test_recipient_side_seal_round_trip(kem, aead):
    """open_ of seal_to_enc's output returns the plaintext, for every KEM and every edge enc; for
    an enc whose ephemeral key is known it is the sender-side seal's ciphertext, byte for byte."""
    rng = np.random.default_rng(7 * kem + aead)
    skR = H.kem_private(rng, kem)
    pkR = H.kem_public(skR, kem)
    kdf = KEM_KDF[kem]
    for pt, aad in ((b"", b""), (b"x" * 33, b"a" * 17)):
        skE = H.kem_private(rng, kem)
        enc, ct = H.seal(pkR, skE, b"info", aad, pt, aead=aead, kem=kem, kdf=kdf)
        assert H.seal_to_enc(skR, pkR, enc, b"info", aad, pt, aead=aead, kem=kem, kdf=kdf) == ct
        for e, refused in edge_points(kem):
            c = H.seal_to_enc(skR, pkR, e, b"info", aad, pt, aead=aead, kem=kem, kdf=kdf)
            assert (c is None) == refused, e.hex()
            if not refused:
                assert len(c) == len(pt) + 16
                assert H.open_(skR, pkR, e, b"info", aad, c, aead=aead, kem=kem, kdf=kdf) == pt
                assert H.open_(skR, pkR, e, b"info", aad + b"!", c, aead=aead, kem=kem,
                               kdf=kdf) is None


def test_p521_opener_rejects_bad_keys():
    """DeserializePrivateKey (1 <= sk < n) and the public key's SEC 1 prefix for the P-521 KEM:
    creation fails with JANUS_HPKE_EINVAL before any device call (runs without a GPU)."""
    import ctypes as C
    from janus_amd import hpke as G
    lib = G._lib()
    out = C.c_void_p()
    pk = b"\x04" + bytes(132)
    for sk in (0, P521_N, P521_N + 1, 2**528 - 1):
        assert lib.janus_hpke_opener_create(0x12, 3, 1, sk.to_bytes(66, "big"), 66, pk, 133, None,
                                            0, 0, C.byref(out)) == -1, hex(sk)
    five = (5).to_bytes(66, "big")
    assert lib.janus_hpke_opener_create(0x12, 3, 1, five, 66, b"\x02" + bytes(132), 133, None, 0,
                                        0, C.byref(out)) == -1
    assert lib.janus_hpke_opener_create(0x12, 3, 1, five, 65, pk, 133, None, 0, 0,
                                        C.byref(out)) == -1


@pytest.mark.parametrize("kem", (H.KEM_P256, H.KEM_P384, H.KEM_P521))
def test_group_orders(kem):
    """(n - 1) G = -G has G's x-coordinate: the orders above are the curves' own."""
    n, nsk = KEM_ORDER[kem], H.NSK[kem]
    g = H.kem_public((1).to_bytes(nsk, "big"), kem)
    m = H.kem_public((n - 1).to_bytes(nsk, "big"), kem)
    assert g[:1 + nsk] == m[:1 + nsk] and g != m

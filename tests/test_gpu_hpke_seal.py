"""The batched HPKE seal on the GPU (include/janus_hpke.h "Seal", janus_amd.hpke.HpkeSealer) against
the OpenSSL-composed oracle (oracle/hpke.py): RFC 9180 SetupBaseS + Seal at sequence number 0,
bit for bit, for every suite, at the launch-shape boundaries, in DAP input-share mode (what the
existing openers read back), and at the edges of the ephemeral and the recipient key.

Out-of-range P-256 scalars are asserted by status only: OpenSSL reduces n + 1 where RFC 9180 7.1.2
refuses it."""
import ctypes as C

import numpy as np
import pytest

from oracle import hpke as H

pytestmark = pytest.mark.gpu

INFO = H.INFO_INPUT_SHARE_HELPER
P256_N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
PT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 102)
AAD_LENS = (0, 1, 15, 16, 17, 60, 92, 124)
KEMS = (H.KEM_X25519, H.KEM_P256)


def _recipient(kem, seed=7):
    skR = H.kem_private(np.random.default_rng(seed), kem)
    return skR, H.kem_public(skR, kem)


def _messages(n, seed):
    rng = np.random.default_rng(seed)
    pts = [rng.integers(0, 256, PT_LENS[i % len(PT_LENS)], dtype=np.uint8).tobytes()
           for i in range(n)]
    aads = [rng.integers(0, 256, AAD_LENS[i % len(AAD_LENS)], dtype=np.uint8).tobytes()
            for i in range(n)]
    return pts, aads


def _expect(pkR, sks, pts, aads, kem, kdf=1, aead=1):
    return [H.seal(pkR, sks[i], INFO, aads[i], pts[i], aead=aead, kem=kem, kdf=kdf)
            for i in range(len(sks))]


def _rows(pts, aads):
    """The padded row arrays of the device form (and their lengths)."""
    n = len(pts)
    ps = -(-max(len(p) for p in pts) // 16) * 16
    as_ = -(-max(len(a) for a in aads) // 16) * 16
    pt = np.zeros((n, max(ps, 16)), np.uint8)
    aad = np.zeros((n, max(as_, 16)), np.uint8)
    for i in range(n):
        pt[i, :len(pts[i])] = np.frombuffer(pts[i], np.uint8)
        aad[i, :len(aads[i])] = np.frombuffer(aads[i], np.uint8)
    pl = np.array([len(p) for p in pts], np.uint32)
    al = np.array([len(a) for a in aads], np.uint32)
    return pt, pl, aad, al


def _seal_device(sealer, sks, pts, aads, extra_rows=0, sentinel=0xA5, stream=None):
    """janus_hpke_seal_device on torch tensors; outputs carry extra_rows rows of sentinel bytes
    past the batch.  Returns numpy (enc, ct, ct_len, status) including those rows."""
    import torch
    from janus_amd import hpke as G
    from janus_amd.prio3 import _stream, _tptr
    n = len(pts)
    pt, pl, aad, al = _rows(pts, aads)
    cs = pt.shape[1] + 16
    dev = torch.device("cuda", sealer.device)
    T = lambda x: torch.from_numpy(np.array(x)).to(dev)  # noqa: E731  (a writable copy)
    d_sk = T(np.frombuffer(b"".join(sks), np.uint8).reshape(n, 32))
    d_pt, d_pl, d_aad, d_al = T(pt), T(pl.view(np.int32)), T(aad), T(al.view(np.int32))
    m = n + extra_rows
    enc = torch.full((m, sealer.nenc), sentinel, dtype=torch.uint8, device=dev)
    ct = torch.full((m, cs), sentinel, dtype=torch.uint8, device=dev)
    cl = torch.full((m,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    st = torch.full((m,), sentinel, dtype=torch.uint8, device=dev)
    rc = G._lib().janus_hpke_seal_device(
        sealer.handle, n, _tptr(d_sk), _tptr(d_pt), _tptr(d_pl), pt.shape[1], _tptr(d_aad),
        _tptr(d_al), aad.shape[1], _tptr(enc), _tptr(ct), _tptr(cl), cs, _tptr(st),
        _stream(stream, sealer.device))
    assert rc == 0
    torch.cuda.synchronize()
    return enc.cpu().numpy(), ct.cpu().numpy(), cl.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _check_rows(exp, enc, ct, cl, st):
    """Rows equal the oracle's (enc, ct || tag), with ct_len and a zero-filled rest of the row."""
    for i, (e, c) in enumerate(exp):
        assert st[i] == 0, i
        assert cl[i] == len(c), i
        assert enc[i].tobytes() == e, i
        assert ct[i, :cl[i]].tobytes() == c, i
        assert not ct[i, cl[i]:].any(), i


@pytest.mark.parametrize("aead", [1, 2, 3])
@pytest.mark.parametrize("kdf", [1, 2, 3])
@pytest.mark.parametrize("kem", KEMS)
def test_seal_matches_oracle_every_suite(kem, kdf, aead):
    from janus_amd import hpke as G
    n = 67
    rng = np.random.default_rng(1000 * kem + 10 * kdf + aead)
    _, pkR = _recipient(kem)
    sks = [H.kem_private(rng, kem) for _ in range(n)]
    pts, aads = _messages(n, kem + kdf + aead)
    exp = _expect(pkR, sks, pts, aads, kem, kdf, aead)
    s = G.HpkeSealer(pkR, INFO, kem_id=kem, kdf_id=kdf, aead_id=aead)
    # the host form
    enc, cts, st = s.seal(sks, pts, aads)
    assert not st.any()
    for i, (e, c) in enumerate(exp):
        assert enc[i].tobytes() == e and cts[i] == c, i
    # the device form
    _check_rows(exp, *_seal_device(s, sks, pts, aads))


_BOUNDARY = {}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("kem", KEMS)
def test_launch_shape_boundaries(kem, n):
    """Every n around the wave and block sizes: rows < n equal the oracle, the row past the batch
    keeps its sentinel bytes.  (One oracle run of 257 reports per KEM, shared by the sizes.)"""
    from janus_amd import hpke as G
    _, pkR = _recipient(kem)
    if kem not in _BOUNDARY:
        rng = np.random.default_rng(kem)
        sks = [H.kem_private(rng, kem) for _ in range(257)]
        pts, aads = _messages(257, 5)
        _BOUNDARY[kem] = (sks, pts, aads, _expect(pkR, sks, pts, aads, kem))
    sks, pts, aads, exp = _BOUNDARY[kem]
    s = G.HpkeSealer(pkR, INFO, kem_id=kem)
    enc, ct, cl, st = _seal_device(s, sks[:n], pts[:n], aads[:n], extra_rows=1)
    _check_rows(exp[:n], enc, ct, cl, st)
    assert (enc[n] == 0xA5).all() and (ct[n] == 0xA5).all() and st[n] == 0xA5
    assert cl[n] == 0x5A5A5A5A


@pytest.mark.parametrize("taskprov", [False, True])
@pytest.mark.parametrize("share_len", [32, 48, 96])
@pytest.mark.parametrize("pub_len", [0, 32, 64])
@pytest.mark.parametrize("kem", KEMS)
def test_input_share_mode(kem, pub_len, share_len, taskprov):
    """The PlaintextInputShare framing and the InputShareAad are built on the device: the first 16
    rows equal the oracle's seal of them, and every row opens to the original helper share through
    the device opener and through the oracle; an opener with the taskprov flag inverted reports
    INVALID_MESSAGE for every row."""
    import torch
    from janus_amd import hpke as G
    n = 129
    rng = np.random.default_rng(kem + pub_len + share_len + taskprov)
    skR, pkR = _recipient(kem)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = (1_700_000_000 + rng.integers(0, 3600, n)).astype(np.uint64)
    pubs = rng.integers(0, 256, (n, pub_len), dtype=np.uint8) if pub_len else None
    shares = rng.integers(0, 256, (n, share_len), dtype=np.uint8)
    sks = [H.kem_private(rng, kem) for _ in range(n)]
    sk = np.frombuffer(b"".join(sks), np.uint8).reshape(n, 32)
    s = G.HpkeSealer(pkR, INFO, kem_id=kem)
    enc, ct, cl, st = s.seal_input_shares(task, sk, ids, times, pubs, shares,
                                          with_taskprov_extension=taskprov)
    assert not st.any()
    ext = ((0xFF00, b""),) if taskprov else ()
    assert ct.shape[1] % 16 == 0
    for r in range(16):
        aad = H.input_share_aad(task, ids[r].tobytes(), int(times[r]),
                                b"" if pubs is None else pubs[r].tobytes())
        e, c = H.seal(pkR, sks[r], INFO, aad, H.plaintext_input_share(shares[r].tobytes(), ext),
                      kem=kem)
        assert enc[r].tobytes() == e and cl[r] == len(c), r
        assert ct[r, :cl[r]].tobytes() == c and not ct[r, cl[r]:].any(), r
    # back through the oracle
    got, ost = H.open_input_shares(skR, pkR, task, enc, ct, cl, ids, times, pubs, share_len,
                                   require_taskprov=taskprov, kem=kem)
    assert not ost.any()
    np.testing.assert_array_equal(got, shares)
    # and through the device opener, both ways round
    dev = torch.device("cuda", 0)
    T = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa
    op = G.HpkeOpener(skR, pkR, INFO, kem_id=kem)
    for require, want in ((taskprov, 0), (not taskprov, G.INVALID_MESSAGE)):
        out = torch.empty((n, share_len), dtype=torch.uint8, device=dev)
        ostat = torch.empty(n, dtype=torch.uint8, device=dev)
        op.open_input_shares_device(task, T(enc), T(ct), T(cl.view(np.int32)), T(ids),
                                    T(times.view(np.int64)), T(pubs), out, ostat,
                                    require_taskprov=require)
        torch.cuda.synchronize()
        assert (ostat.cpu().numpy() == want).all()
        if want == 0:
            np.testing.assert_array_equal(out.cpu().numpy(), shares)


def _be(x):
    return x.to_bytes(32, "big")


def test_p256_ephemeral_key_edges():
    """Small scalars, scalars next to the order (n-2, n-6, n-30: the last window's doubling case),
    even scalars (the y-negation after k' = n - sk), and out-of-range scalars between valid ones:
    0, n, n+1 and 2^256-1 give SEAL_KEY_ERROR, zero rows and ct_len 0, their neighbours the
    oracle's bytes."""
    from janus_amd import hpke as G
    kem = H.KEM_P256
    _, pkR = _recipient(kem)
    valid = [1, 2, 3, 15, 16, 17, P256_N - 1, P256_N - 2, P256_N - 6, P256_N - 30, P256_N - 31,
             (P256_N + 1) // 2]
    bad = [0, P256_N, P256_N + 1, 2**256 - 1]
    ks = valid[:3] + bad[:1] + valid[3:6] + bad[1:3] + valid[6:] + bad[3:]
    sks = [_be(k) for k in ks]
    pts, aads = _messages(len(ks), 3)
    s = G.HpkeSealer(pkR, INFO, kem_id=kem)
    enc, ct, cl, st = _seal_device(s, sks, pts, aads)
    enc_h, cts_h, st_h = s.seal(sks, pts, aads)
    for i, k in enumerate(ks):
        if k in bad:
            assert st[i] == st_h[i] == G.SEAL_KEY_ERROR, hex(k)
            assert cl[i] == 0 and not enc[i].any() and not ct[i].any(), hex(k)
            assert cts_h[i] is None and not enc_h[i].any(), hex(k)
        else:
            e, c = H.seal(pkR, sks[i], INFO, aads[i], pts[i], kem=kem)
            assert st[i] == st_h[i] == 0, hex(k)
            assert enc[i].tobytes() == enc_h[i].tobytes() == e, hex(k)
            assert ct[i, :cl[i]].tobytes() == cts_h[i] == c, hex(k)
            assert e == H.kem_public(sks[i], kem), hex(k)


def test_x25519_ephemeral_keys_are_clamped_on_the_device():
    from janus_amd import hpke as G
    kem = H.KEM_X25519
    _, pkR = _recipient(kem)
    rng = np.random.default_rng(25519)
    sks = [bytes(32), b"\xff" * 32, bytes([7]) + bytes(30) + bytes([0x80]),
           bytes([0xff]) + bytes(30) + bytes([0x3f])]
    sks += [bytes(rng.integers(0, 256, 32, dtype=np.uint8) | 0x87) for _ in range(4)]
    pts, aads = _messages(len(sks), 4)
    s = G.HpkeSealer(pkR, INFO, kem_id=kem)
    _check_rows(_expect(pkR, sks, pts, aads, kem), *_seal_device(s, sks, pts, aads))


def test_recipient_key_edges():
    from janus_amd import hpke as G
    n = 5
    pts, aads = _messages(n, 6)
    rng = np.random.default_rng(11)
    # X25519: pkR = 0 gives an all-zero shared secret
    sks = [H.kem_private(rng, H.KEM_X25519) for _ in range(n)]
    s = G.HpkeSealer(bytes(32), INFO, kem_id=H.KEM_X25519)
    enc, ct, cl, st = _seal_device(s, sks, pts, aads)
    assert (st == G.SEAL_KEY_ERROR).all() and not cl.any() and not enc.any() and not ct.any()
    # P-256: y off the curve, and a compressed-point prefix
    _, pkR = _recipient(H.KEM_P256)
    off = bytearray(pkR)
    off[64] ^= 1
    sks = [H.kem_private(rng, H.KEM_P256) for _ in range(n)]
    for pk in (bytes(off), b"\x02" + pkR[1:]):
        s = G.HpkeSealer(pk, INFO, kem_id=H.KEM_P256)
        enc, ct, cl, st = _seal_device(s, sks, pts, aads)
        assert (st == G.SEAL_KEY_ERROR).all() and not cl.any() and not enc.any() and not ct.any()
        _, cts, st = s.seal(sks, pts, aads)
        assert (st == G.SEAL_KEY_ERROR).all() and cts == [None] * n


def _u32le(u):
    return u.to_bytes(32, "little")


def test_x25519_recipient_key_edges_accepted():
    """A recipient key that is a non-canonical u (p + k up to 2^255 - 1), has bit 255 set, or is
    an ordinary small point: the device masks bit 255 and reduces as RFC 7748 says, so both
    forms give the oracle's bytes (kem_context carries pkR as given)."""
    from janus_amd import hpke as G
    from tests.test_hpke_edges import X25519_ACCEPTED
    kem = H.KEM_X25519
    n = 5
    rng = np.random.default_rng(12)
    sks = [H.kem_private(rng, kem) for _ in range(n)]
    pts, aads = _messages(n, 8)
    for u in X25519_ACCEPTED:
        pkR = _u32le(u)
        exp = _expect(pkR, sks, pts, aads, kem)
        s = G.HpkeSealer(pkR, INFO, kem_id=kem)
        _check_rows(exp, *_seal_device(s, sks, pts, aads))
        enc, cts, st = s.seal(sks, pts, aads)
        assert not st.any(), hex(u)
        for i, (e, c) in enumerate(exp):
            assert enc[i].tobytes() == e and cts[i] == c, (hex(u), i)
        s.close()


def test_x25519_recipient_key_edges_refused():
    """Each of the seven low-order u, with bit 255 clear and set, gives an all-zero shared
    secret: SEAL_KEY_ERROR for every row, zero rows and ct_len 0, in both forms."""
    from janus_amd import hpke as G
    from tests.test_hpke_edges import X25519_REFUSED
    kem = H.KEM_X25519
    n = 5
    rng = np.random.default_rng(13)
    sks = [H.kem_private(rng, kem) for _ in range(n)]
    pts, aads = _messages(n, 9)
    assert len(X25519_REFUSED) == 14
    for u in X25519_REFUSED:
        s = G.HpkeSealer(_u32le(u), INFO, kem_id=kem)
        enc, ct, cl, st = _seal_device(s, sks, pts, aads)
        assert (st == G.SEAL_KEY_ERROR).all(), hex(u)
        assert not cl.any() and not enc.any() and not ct.any(), hex(u)
        enc, cts, st = s.seal(sks, pts, aads)
        assert (st == G.SEAL_KEY_ERROR).all() and cts == [None] * n and not enc.any(), hex(u)
        s.close()


def test_create_errors():
    from janus_amd import hpke as G
    L = G._lib()

    def create(kem, kdf, aead, pk):
        h = C.c_void_p()
        rc = L.janus_hpke_sealer_create(kem, kdf, aead, G._b(pk), len(pk), G._b(INFO), len(INFO),
                                        0, C.byref(h))
        assert (rc == 0) == bool(h)
        if h:
            L.janus_hpke_sealer_destroy(h)
        return rc

    assert create(0x20, 1, 1, bytes(31)) == -1
    assert create(0x20, 1, 1, bytes(65)) == -1
    assert create(0x10, 1, 1, b"\x04" + bytes(31)) == -1
    assert create(0x10, 1, 1, b"\x04" + bytes(65)) == -1
    for kem, npk in ((0x21, 56), (0x12, 133), (0x11, 97)):
        assert create(kem, 1, 1, bytes(npk)) == -3
    assert create(0x20, 4, 1, bytes(32)) == -3
    assert create(0x20, 1, 4, bytes(32)) == -3
    assert create(0x20, 1, 1, bytes(range(32))) == 0
    with pytest.raises(NotImplementedError):
        G.HpkeSealer(bytes(56), kem_id=0x21).handle
    with pytest.raises(RuntimeError, match="rc=-1"):
        G.HpkeSealer(bytes(33)).handle
    # row-layout errors of the device entry points: EINVAL before any launch
    import torch
    from janus_amd.prio3 import _tptr
    s = G.HpkeSealer(bytes(range(32)))
    buf = [_tptr(torch.zeros(4096, dtype=torch.uint8, device="cuda:0")) for _ in range(9)]
    sk, ids, t, pub, hs, enc, ct, cl, st = buf

    def seal_one(pub_ptr, pub_len, ct_stride):
        return L.janus_hpke_seal_input_shares_device(s.handle, 1, G._b(bytes(32)), sk, ids, t,
                                                     pub_ptr, pub_len, hs, 48, 0, enc, ct, cl,
                                                     ct_stride, st, None)

    assert seal_one(None, 0, 64) == -1   # 6 + 48 + 16 > 64
    assert seal_one(None, 0, 72) == -1   # not a multiple of 16
    assert seal_one(pub, 16, 80) == -1   # a public share of 16 bytes
    assert seal_one(None, 32, 80) == -1  # public share bytes without a pointer
    assert seal_one(None, 0, 80) == 0
    torch.cuda.synchronize()


def test_callers_device_and_stream():
    """Every entry point leaves the calling thread's HIP device as it was (the sealer lives on the
    last GPU, the thread stays on GPU 0; on a one-GPU machine the two coincide), and the device form
    on a side stream followed by the device opener on the same stream needs no synchronisation in
    between."""
    import torch
    from janus_amd import hpke as G
    sd = torch.cuda.device_count() - 1
    torch.cuda.set_device(0)
    current = torch.cuda.current_device
    kem = H.KEM_X25519
    skR, pkR = _recipient(kem)
    n, share_len = 200, 48
    rng = np.random.default_rng(77)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    s = G.HpkeSealer(pkR, INFO, device=sd, kem_id=kem)
    s.handle
    assert current() == 0
    dev = torch.device("cuda", sd)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    times = (1_700_000_000 + rng.integers(0, 3600, n)).astype(np.int64)
    pubs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    shares = rng.integers(0, 256, (n, share_len), dtype=np.uint8)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_sk, d_ids, d_t, d_pub, d_sh = T(sk), T(ids), T(times), T(pubs), T(shares)
    cs = G.sealed_stride(share_len)
    enc = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    ct = torch.empty((n, cs), dtype=torch.uint8, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty((n, share_len), dtype=torch.uint8, device=dev)
    ost = torch.empty(n, dtype=torch.uint8, device=dev)
    op = G.HpkeOpener(skR, pkR, INFO, device=sd, kem_id=kem)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    # the side stream by its handle: the thread's current device stays GPU 0
    s.seal_input_shares_device(task, d_sk, d_ids, d_t, d_pub, d_sh, enc, ct, cl, st,
                               stream=side.cuda_stream)
    assert current() == 0
    op.open_input_shares_device(task, enc, ct, cl, d_ids, d_t, d_pub, out, ost,
                                stream=side.cuda_stream)
    side.synchronize()
    assert not st.cpu().numpy().any() and not ost.cpu().numpy().any()
    np.testing.assert_array_equal(out.cpu().numpy(), shares)
    # the generic device form and the host forms
    _seal_device(s, [bytes(sk[0])], [b"abc"], [b"xy"])
    assert current() == 0
    e2, c2, l2, s2 = s.seal_input_shares(task, sk, ids, times.view(np.uint64), pubs, shares)
    assert current() == 0
    np.testing.assert_array_equal(e2, enc.cpu().numpy())
    np.testing.assert_array_equal(c2, ct.cpu().numpy())
    s.seal([bytes(sk[0])], [b"abc"], [b""])
    assert current() == 0
    s.close()
    assert current() == 0

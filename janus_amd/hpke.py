"""Python mirror of the batched HPKE opener and sealer (include/janus_hpke.h), SURVEY 8(f) row 2.

``HpkeOpener`` corresponds to one Janus ``HpkeKeypair`` + ``HpkeApplicationInfo``
(/root/reference/core/src/hpke.rs:70-85, 186-203, 283-305); ``open_input_shares`` is the
decrypt + PlaintextInputShare decode + extension checks of the helper's aggregate-init loop
(aggregator.rs:1796-1990) for a whole batch, producing the helper input shares that
``HelperEngine.prepare_*`` consumes.  ``HpkeSealer`` is the other direction (``hpke::seal``,
hpke.rs:167-189): one recipient public key + application info, sealing a batch with ephemeral
private keys the caller supplies.  No CPU fallback: the HIP library must be built.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .prio3 import _np_ptr, _stream, _tptr, load_library

KEM_X25519_HKDF_SHA256 = 0x0020
KEM_P256_HKDF_SHA256 = 0x0010
KEM_X448_HKDF_SHA512 = 0x0021
KEM_P521_HKDF_SHA512 = 0x0012
KEM_P384_HKDF_SHA384 = 0x0011
KDF_HKDF_SHA256 = 0x0001
KDF_HKDF_SHA384 = 0x0002
KDF_HKDF_SHA512 = 0x0003
# Nenc (= Npk) per KEM (RFC 9180 7.1)
NENC = {KEM_X25519_HKDF_SHA256: 32, KEM_P256_HKDF_SHA256: 65, KEM_X448_HKDF_SHA512: 56,
        KEM_P521_HKDF_SHA512: 133, KEM_P384_HKDF_SHA384: 97}
AEAD_AES_128_GCM = 0x0001
AEAD_AES_256_GCM = 0x0002
AEAD_CHACHA20_POLY1305 = 0x0003
OK, DECRYPT_ERROR, INVALID_MESSAGE = 0, 4, 8
SEAL_KEY_ERROR, SEAL_LENGTH_ERROR = 0x40, 0x41
NSK_E = 32  # bytes of ephemeral private key per report (both seal KEMs)
INFO_INPUT_SHARE_HELPER = b"dap-09 input share" + bytes([1, 3])  # Label::InputShare, Client->Helper
INFO_INPUT_SHARE_LEADER = b"dap-09 input share" + bytes([1, 2])  # Label::InputShare, Client->Leader

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, u32 = C.c_void_p, C.c_uint32
        L.janus_hpke_opener_create.argtypes = [C.c_uint16, C.c_uint16, C.c_uint16, vp, C.c_size_t,
                                               vp, C.c_size_t, vp, C.c_size_t, C.c_int,
                                               C.POINTER(vp)]
        L.janus_hpke_opener_destroy.argtypes = [vp]
        L.janus_hpke_open_input_shares_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp,
                                                          u32, u32, C.c_int, vp, vp, vp]
        L.janus_hpke_open_input_shares.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, u32,
                                                   u32, C.c_int, vp, vp]
        L.janus_hpke_open_device.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp]
        L.janus_hpke_open.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp]
        L.janus_hpke_sealer_create.argtypes = [C.c_uint16, C.c_uint16, C.c_uint16, vp, C.c_size_t,
                                               vp, C.c_size_t, C.c_int, C.POINTER(vp)]
        L.janus_hpke_sealer_destroy.argtypes = [vp]
        L.janus_hpke_seal_device.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp,
                                             u32, vp, vp]
        L.janus_hpke_seal.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, u32, vp]
        L.janus_hpke_seal_input_shares_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, u32,
                                                          C.c_int, vp, vp, vp, u32, vp, vp]
        L.janus_hpke_seal_input_shares.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, u32,
                                                   C.c_int, vp, vp, vp, u32, vp]
        L.janus_hpke_set_timing.argtypes = [vp, C.c_int]
        L.janus_hpke_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        L.janus_hpke_executor_stats_get.argtypes = [vp, C.POINTER(C.c_uint64 * 5)]
        L.janus_hpke_executor_control.argtypes = [vp, C.c_char_p, C.c_int64]
        L.janus_hpke_selftest_p256.argtypes = [C.c_int, u32, vp, vp, vp]
        L.janus_hpke_selftest_field.argtypes = [C.c_int, C.c_int, u32, vp, vp, vp]
        _bound = True
    return L


def _b(x: bytes):
    return C.cast(C.c_char_p(bytes(x)), C.c_void_p)


class HpkeOpener:
    def __init__(self, private_key: bytes, public_key: bytes, info: bytes = INFO_INPUT_SHARE_HELPER,
                 device: int = 0, kem_id=KEM_X25519_HKDF_SHA256, kdf_id=KDF_HKDF_SHA256,
                 aead_id=AEAD_AES_128_GCM):
        self.device = device
        self.nenc = NENC.get(kem_id, 0)  # enc bytes per report
        self._keep = (bytes(private_key), bytes(public_key), bytes(info))
        h = C.c_void_p()
        rc = _lib().janus_hpke_opener_create(kem_id, kdf_id, aead_id, _b(private_key),
                                             len(private_key), _b(public_key), len(public_key),
                                             _b(info) if info else None, len(info), device,
                                             C.byref(h))
        if rc == -3:
            raise NotImplementedError("HPKE suite not supported by the GPU opener")
        if rc:
            raise RuntimeError(f"janus_hpke_opener_create failed (rc={rc})")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            _lib().janus_hpke_opener_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- DAP helper input shares ----------------------------------------------------
    def open_input_shares(self, task_id: bytes, enc, ct, ct_len, report_ids, times,
                          public_shares, helper_share_len: int, require_taskprov=False):
        """Host arrays -> (helper_shares [n, helper_share_len], status [n])."""
        enc = np.ascontiguousarray(enc, np.uint8)
        n = enc.shape[0]
        ct = np.ascontiguousarray(ct, np.uint8)
        if ct.shape[1] % 16:
            ct = np.pad(ct, ((0, 0), (0, 16 - ct.shape[1] % 16)))
        ct_len = np.ascontiguousarray(ct_len, np.uint32)
        ids = np.ascontiguousarray(report_ids, np.uint8)
        times = np.ascontiguousarray(times, np.uint64)
        pub = None if public_shares is None else np.ascontiguousarray(public_shares, np.uint8)
        publen = 0 if pub is None else pub.shape[1]
        shares = np.zeros((n, helper_share_len), np.uint8)
        status = np.zeros(n, np.uint8)
        rc = _lib().janus_hpke_open_input_shares(
            self.handle, n, _b(task_id), _np_ptr(enc), _np_ptr(ct), _np_ptr(ct_len), ct.shape[1],
            _np_ptr(ids), _np_ptr(times), _np_ptr(pub), publen, helper_share_len,
            int(require_taskprov), _np_ptr(shares), _np_ptr(status))
        if rc:
            raise RuntimeError(f"janus_hpke_open_input_shares failed (rc={rc})")
        return shares, status

    def open_input_shares_device(self, task_id: bytes, enc, ct, ct_len, report_ids, times,
                                 public_shares, helper_shares, status, require_taskprov=False,
                                 stream=None):
        """torch tensors on this opener's GPU; ct is [n, stride] with stride % 16 == 0."""
        rc = _lib().janus_hpke_open_input_shares_device(
            self.handle, enc.shape[0], _b(task_id), _tptr(enc), _tptr(ct), _tptr(ct_len),
            ct.shape[1], _tptr(report_ids), _tptr(times), _tptr(public_shares),
            0 if public_shares is None else public_shares.shape[1], helper_shares.shape[1],
            int(require_taskprov), _tptr(helper_shares), _tptr(status),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"janus_hpke_open_input_shares_device failed (rc={rc})")

    # ---- generic single-shot open ----------------------------------------------------
    def open(self, enc, ct_list, aad_list):
        """Lists of byte strings -> list of plaintexts (None where the open failed)."""
        n = len(ct_list)
        cs = max(16, -(-max(len(c) for c in ct_list) // 16) * 16)
        as_ = -(-max([len(a) for a in aad_list] + [1]) // 16) * 16
        encs = np.zeros((n, self.nenc), np.uint8)
        ct = np.zeros((n, cs), np.uint8)
        aad = np.zeros((n, as_), np.uint8)
        cl = np.zeros(n, np.uint32)
        al = np.zeros(n, np.uint32)
        for i in range(n):
            encs[i] = np.frombuffer(bytes(enc[i]), np.uint8)
            ct[i, :len(ct_list[i])] = np.frombuffer(ct_list[i], np.uint8)
            aad[i, :len(aad_list[i])] = np.frombuffer(aad_list[i], np.uint8)
            cl[i], al[i] = len(ct_list[i]), len(aad_list[i])
        pt = np.zeros((n, cs), np.uint8)
        st = np.zeros(n, np.uint8)
        rc = _lib().janus_hpke_open(self.handle, n, _np_ptr(encs), _np_ptr(ct), _np_ptr(cl), cs,
                                    _np_ptr(aad), _np_ptr(al), as_, _np_ptr(pt), _np_ptr(st))
        if rc:
            raise RuntimeError(f"janus_hpke_open failed (rc={rc})")
        return [None if st[i] else pt[i, :cl[i] - 16].tobytes() for i in range(n)]

    def executor_stats(self) -> dict:
        """Counters of the GPU's HPKE executor (janus_hpke_executor_stats_get)."""
        v = (C.c_uint64 * 5)()
        rc = _lib().janus_hpke_executor_stats_get(self.handle, C.byref(v))
        if rc:
            raise RuntimeError(f"janus_hpke_executor_stats_get failed (rc={rc})")
        return dict(zip(("jobs", "reports", "groups", "active_jobs", "active_reports"), v))

    def executor_control(self, key: str, value: int):
        """janus_hpke_executor_control: "hold", "heavy", "coalesce"."""
        rc = _lib().janus_hpke_executor_control(self.handle, key.encode(), int(value))
        if rc:
            raise ValueError(f"executor control {key} failed (rc={rc})")

    def set_timing(self, on: bool):
        _lib().janus_hpke_set_timing(self.handle, int(on))

    def timing(self):
        ms, k = C.c_double(), C.c_uint32()
        _lib().janus_hpke_timing(self.handle, C.byref(ms), C.byref(k))
        return ms.value, k.value


def sealed_stride(helper_share_len: int, with_taskprov_extension: bool = False) -> int:
    """ct_stride of sealed helper input shares: PlaintextInputShare framing (6 bytes, 10 with the
    taskprov extension) + share + tag, rounded up to 16."""
    return -(-((10 if with_taskprov_extension else 6) + helper_share_len + 16) // 16) * 16


class HpkeSealer:
    """One recipient public key + application info (janus_hpke_sealer).  The library draws no
    randomness: every call takes one 32-byte ephemeral private key per report from the caller's
    CSPRNG.  Arguments are checked here, before any library call (ValueError); the device sealer
    itself is created on first use, so the checks need no GPU."""

    def __init__(self, public_key: bytes, info: bytes = INFO_INPUT_SHARE_HELPER, device: int = 0,
                 kem_id=KEM_X25519_HKDF_SHA256, kdf_id=KDF_HKDF_SHA256, aead_id=AEAD_AES_128_GCM):
        self.device = device
        self.kem_id, self.kdf_id, self.aead_id = kem_id, kdf_id, aead_id
        self.nenc = NENC.get(kem_id, 0)  # enc bytes per report
        self._keep = (bytes(public_key), bytes(info))
        self._handle = None

    @property
    def handle(self):
        if self._handle is None:
            pk, info = self._keep
            h = C.c_void_p()
            rc = _lib().janus_hpke_sealer_create(self.kem_id, self.kdf_id, self.aead_id, _b(pk),
                                                 len(pk), _b(info) if info else None, len(info),
                                                 self.device, C.byref(h))
            if rc == -3:
                raise NotImplementedError("HPKE suite not supported by the GPU sealer")
            if rc:
                raise RuntimeError(f"janus_hpke_sealer_create failed (rc={rc})")
            self._handle = h
        return self._handle

    def close(self):
        if getattr(self, "_handle", None):
            _lib().janus_hpke_sealer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- generic single-shot seal ----------------------------------------------------
    def seal(self, sk_e, pt_list, aad_list):
        """Lists of byte strings (sk_e: n keys of 32 bytes, or an [n, 32] array) ->
        (enc [n, Nenc], list of ciphertexts (None where the seal failed), status [n])."""
        n = len(pt_list)
        if isinstance(sk_e, np.ndarray):
            sk = np.ascontiguousarray(sk_e, np.uint8)
        else:
            keys = [bytes(k) for k in sk_e]
            if any(len(k) != NSK_E for k in keys):
                raise ValueError(f"every ephemeral private key must be {NSK_E} bytes")
            sk = np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), NSK_E)
        if sk.shape != (n, NSK_E):
            raise ValueError(f"sk_e must be {n} keys of {NSK_E} bytes")
        if len(aad_list) != n:
            raise ValueError("pt_list and aad_list differ in length")
        if n == 0:
            return np.zeros((0, self.nenc), np.uint8), [], np.zeros(0, np.uint8)
        ps = -(-max(len(p) for p in pt_list) // 16) * 16
        as_ = -(-max(len(a) for a in aad_list) // 16) * 16
        cs = ps + 16
        pt = np.zeros((n, ps), np.uint8)
        aad = np.zeros((n, as_), np.uint8)
        pl = np.zeros(n, np.uint32)
        al = np.zeros(n, np.uint32)
        for i in range(n):
            pt[i, :len(pt_list[i])] = np.frombuffer(bytes(pt_list[i]), np.uint8)
            aad[i, :len(aad_list[i])] = np.frombuffer(bytes(aad_list[i]), np.uint8)
            pl[i], al[i] = len(pt_list[i]), len(aad_list[i])
        enc = np.zeros((n, self.nenc), np.uint8)
        ct = np.zeros((n, cs), np.uint8)
        cl = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        rc = _lib().janus_hpke_seal(self.handle, n, _np_ptr(sk), _np_ptr(pt) if ps else None,
                                    _np_ptr(pl), ps, _np_ptr(aad) if as_ else None,
                                    _np_ptr(al) if as_ else None, as_, _np_ptr(enc), _np_ptr(ct),
                                    _np_ptr(cl), cs, _np_ptr(st))
        if rc:
            raise RuntimeError(f"janus_hpke_seal failed (rc={rc})")
        return enc, [None if st[i] else ct[i, :cl[i]].tobytes() for i in range(n)], st

    # ---- DAP helper input shares ----------------------------------------------------
    @staticmethod
    def _check_input_shares(task_id, sk_e, report_ids, times, public_shares, helper_shares):
        """The shapes the C ABI reads, for numpy arrays and torch tensors alike; returns
        (n, public share length)."""
        def shape(x):
            return tuple(x.shape)
        n = shape(report_ids)[0] if len(shape(report_ids)) else -1
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        if shape(report_ids) != (n, 16):
            raise ValueError("report_ids must be [n, 16]")
        if shape(sk_e) != (n, NSK_E):
            raise ValueError(f"sk_e must be [n, {NSK_E}]: one ephemeral private key per report")
        if shape(times) != (n,):
            raise ValueError("times must be [n]")
        if len(shape(helper_shares)) != 2 or shape(helper_shares)[0] != n:
            raise ValueError("helper_shares must be [n, helper_share_len]")
        publen = 0
        if public_shares is not None and shape(public_shares)[-1] != 0:
            if len(shape(public_shares)) != 2 or shape(public_shares)[0] != n or \
                    shape(public_shares)[1] not in (32, 64):
                raise ValueError("public_shares must be None or [n, 32 | 64]")
            publen = shape(public_shares)[1]
        return n, publen

    def seal_input_shares(self, task_id: bytes, sk_e, report_ids, times, public_shares,
                          helper_shares, with_taskprov_extension=False, ct_stride=None):
        """Host arrays -> (enc [n, Nenc], ct [n, ct_stride], ct_len [n], status [n]): the rows
        ``HpkeOpener.open_input_shares`` and ``HelperEngine.aggregate_init_batch`` read."""
        sk = np.ascontiguousarray(sk_e, np.uint8)
        ids = np.ascontiguousarray(report_ids, np.uint8)
        t = np.ascontiguousarray(times, np.uint64)
        hs = np.ascontiguousarray(helper_shares, np.uint8)
        pub = None if public_shares is None else np.ascontiguousarray(public_shares, np.uint8)
        n, publen = self._check_input_shares(task_id, sk, ids, t, pub, hs)
        cs = sealed_stride(hs.shape[1], with_taskprov_extension) if ct_stride is None else ct_stride
        if cs % 16 or cs < sealed_stride(hs.shape[1], with_taskprov_extension):
            raise ValueError("ct_stride must be a multiple of 16 and >= plaintext length + 16")
        enc = np.zeros((n, self.nenc), np.uint8)
        ct = np.zeros((n, cs), np.uint8)
        cl = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        rc = _lib().janus_hpke_seal_input_shares(
            self.handle, n, _b(task_id), _np_ptr(sk), _np_ptr(ids), _np_ptr(t),
            _np_ptr(pub) if publen else None, publen, _np_ptr(hs), hs.shape[1],
            int(bool(with_taskprov_extension)), _np_ptr(enc), _np_ptr(ct), _np_ptr(cl), cs,
            _np_ptr(st))
        if rc:
            raise RuntimeError(f"janus_hpke_seal_input_shares failed (rc={rc})")
        return enc, ct, cl, st

    def seal_input_shares_device(self, task_id: bytes, sk_e, report_ids, times, public_shares,
                                 helper_shares, enc, ct, ct_len, status,
                                 with_taskprov_extension=False, stream=None):
        """torch tensors on this sealer's GPU (uint8; times 8-byte integers, ct_len int32 /
        uint32): writes enc [n, Nenc], ct [n, stride] (stride % 16 == 0), ct_len [n],
        status [n], stream-ordered."""
        n, publen = self._check_input_shares(task_id, sk_e, report_ids, times, public_shares,
                                             helper_shares)
        if tuple(enc.shape) != (n, self.nenc) or ct.dim() != 2 or ct.shape[0] != n or \
                tuple(ct_len.shape) != (n,) or tuple(status.shape) != (n,):
            raise ValueError("output shapes do not match the batch")
        if ct.shape[1] % 16 or \
                ct.shape[1] < sealed_stride(helper_shares.shape[1], with_taskprov_extension):
            raise ValueError("ct stride must be a multiple of 16 and >= plaintext length + 16")
        if times.element_size() != 8 or ct_len.element_size() != 4:
            raise ValueError("times must be 8-byte and ct_len 4-byte integers")
        for t in (sk_e, report_ids, times, helper_shares, enc, ct, ct_len, status) + \
                ((public_shares,) if publen else ()):
            if not t.is_contiguous() or t.device.index != self.device or t.device.type != "cuda":
                raise ValueError("tensors must be contiguous and on the sealer's GPU")
        rc = _lib().janus_hpke_seal_input_shares_device(
            self.handle, n, _b(task_id), _tptr(sk_e), _tptr(report_ids), _tptr(times),
            _tptr(public_shares) if publen else None, publen, _tptr(helper_shares),
            helper_shares.shape[1], int(bool(with_taskprov_extension)), _tptr(enc), _tptr(ct),
            _tptr(ct_len), ct.shape[1], _tptr(status), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"janus_hpke_seal_input_shares_device failed (rc={rc})")

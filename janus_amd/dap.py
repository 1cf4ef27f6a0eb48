"""Python mirror of the DAP-09 marshaling around the device calls (include/janus_dap.h),
SURVEY 8(f) row 3: AggregationJobInitializeReq body -> SoA buffers for the HPKE opener and the
prio3 engine, and their outputs -> the AggregationJobResp body (helper init step); and the
leader's two opposite directions: its SoA buffers -> the request body, the response body -> the
prepare messages and per-report errors its prepare_next reads."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .prio3 import _np_ptr, _stream, _tptr, load_library

DAP_EXPORTED_SYMBOLS = (
    "janus_dap_agg_init_scan", "janus_dap_agg_init_scan_ex", "janus_dap_agg_init_unpack_device",
    "janus_dap_agg_init_unpack_host", "janus_dap_agg_job_resp_max_len",
    "janus_dap_agg_job_resp_encode_device", "janus_dap_agg_job_resp_encode_host",
    # leader side
    "janus_dap_agg_init_req_max_len", "janus_dap_agg_init_req_encode_host",
    "janus_dap_agg_init_req_encode_device", "janus_dap_agg_job_resp_unpack_host",
    "janus_dap_agg_job_resp_unpack_device",
    # client side
    "janus_dap_report_max_len", "janus_dap_report_encode_device", "janus_dap_report_encode_host",
    # leader upload
    "janus_dap_report_decode_host", "janus_dap_report_decode_device",
)
NO_ERROR = 0xFF  # prepare_error value meaning "no DAP-level error for this report"


class Layout(C.Structure):
    _fields_ = [("n", C.c_uint32), ("query_type", C.c_uint8), ("batch_id", C.c_uint8 * 32),
                ("agg_param_off", C.c_uint64), ("agg_param_len", C.c_uint64),
                ("list_off", C.c_uint64), ("list_len", C.c_uint64), ("record_len", C.c_uint32),
                ("public_share_len", C.c_uint32), ("enc_len", C.c_uint32),
                ("payload_len", C.c_uint32), ("message_len", C.c_uint32),
                ("prep_share_len", C.c_uint32), ("uniform", C.c_int)]


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, u32 = C.c_void_p, C.c_uint32
        L.janus_dap_agg_init_scan.argtypes = [vp, C.c_size_t, C.POINTER(Layout)]
        L.janus_dap_agg_init_scan_ex.argtypes = [vp, C.c_size_t, u32, u32, u32, C.POINTER(Layout)]
        L.janus_dap_agg_init_unpack_device.argtypes = [C.POINTER(Layout), vp, vp, vp, vp, vp, vp,
                                                       vp, vp, u32, vp, vp, vp, vp]
        L.janus_dap_agg_init_unpack_host.argtypes = [vp, C.c_size_t, C.POINTER(Layout), u32, vp,
                                                     vp, vp, vp, vp, vp, vp, u32, vp, vp]
        L.janus_dap_agg_init_unpack_host.restype = C.c_int64
        L.janus_dap_agg_job_resp_max_len.argtypes = [u32, u32]
        L.janus_dap_agg_job_resp_max_len.restype = C.c_size_t
        L.janus_dap_agg_job_resp_encode_device.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp,
                                                           vp]
        L.janus_dap_agg_job_resp_encode_host.argtypes = [u32, vp, vp, vp, vp, u32, vp]
        L.janus_dap_agg_job_resp_encode_host.restype = C.c_int64
        u8 = C.c_uint8
        L.janus_dap_agg_init_req_max_len.argtypes = [u32, u32, u8, u32, u32, u32, u32]
        L.janus_dap_agg_init_req_max_len.restype = C.c_size_t
        req = [u32, vp, u32, u8, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, u32, vp, u32, vp]
        L.janus_dap_agg_init_req_encode_host.argtypes = req + [vp, vp, vp]
        L.janus_dap_agg_init_req_encode_host.restype = C.c_int64
        L.janus_dap_agg_init_req_encode_device.argtypes = req + [vp, vp, vp, vp, vp, vp, vp]
        L.janus_dap_agg_job_resp_unpack_host.argtypes = [u32, vp, vp, u32, vp, C.c_size_t, u32, vp,
                                                         vp]
        L.janus_dap_agg_job_resp_unpack_device.argtypes = [u32, vp, vp, u32, vp, C.c_size_t, u32,
                                                           vp, vp, vp, vp, vp]
        rep = [u32, vp, vp, vp, u32, u8, vp, u32, vp, vp, u32, u8, vp, u32, vp, vp, u32, vp, vp,
               u32, vp]
        L.janus_dap_report_max_len.argtypes = [u32] * 5
        L.janus_dap_report_max_len.restype = C.c_size_t
        L.janus_dap_report_encode_host.argtypes = rep
        L.janus_dap_report_encode_host.restype = C.c_int64
        L.janus_dap_report_encode_device.argtypes = rep + [vp]
        dec = [u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, vp]
        L.janus_dap_report_decode_host.argtypes = dec
        L.janus_dap_report_decode_host.restype = C.c_int64
        L.janus_dap_report_decode_device.argtypes = dec + [vp]
        _bound = True
    return L


LEN_ANY = 0xFFFFFFFF


def scan(body: bytes, public_share_len=None, enc_len=None, prep_share_len=None) -> Layout:
    """Layout of an AggregationJobInitializeReq body.  With the task's expected lengths (VDAF
    public share, KEM Nenc, VDAF leader prep share) every record is checked against those, so a
    malformed first record fails alone (janus_dap_agg_init_scan_ex); without them the first
    record's lengths are taken."""
    lay = Layout()
    buf = np.frombuffer(body, np.uint8)
    if public_share_len is None and enc_len is None and prep_share_len is None:
        rc = _lib().janus_dap_agg_init_scan(_np_ptr(buf), len(body), C.byref(lay))
    else:
        v = lambda x: LEN_ANY if x is None else int(x)
        rc = _lib().janus_dap_agg_init_scan_ex(_np_ptr(buf), len(body), v(public_share_len),
                                               v(enc_len), v(prep_share_len), C.byref(lay))
    if rc:
        raise ValueError("AggregationJobInitializeReq does not decode")
    return lay


INVALID_MESSAGE = 8  # DAP PrepareError::InvalidMessage


def prepare_error(hpke_status, msg_status):
    """Per-report DAP PrepareError for the response encoder: the HPKE opener's error first, then
    a public share that does not decode (msg_status 6 -> InvalidMessage, aggregator.rs:1985-1999),
    else NO_ERROR (the prio3 status decides).  numpy arrays or torch tensors."""
    try:
        import torch
        if isinstance(hpke_status, torch.Tensor):
            pe = torch.where(msg_status == 6, torch.full_like(hpke_status, INVALID_MESSAGE),
                             torch.full_like(hpke_status, NO_ERROR))
            return torch.where(hpke_status != 0, hpke_status, pe)
    except ImportError:
        pass
    hs = np.asarray(hpke_status, np.uint8)
    pe = np.where(np.asarray(msg_status) == 6, INVALID_MESSAGE, NO_ERROR).astype(np.uint8)
    return np.where(hs != 0, hs, pe).astype(np.uint8)


def ct_stride_for(lay: Layout, slack: int = 0) -> int:
    return max(16, -(-(lay.payload_len + slack) // 16) * 16)


def unpack_host(body: bytes, lay: Layout, cap: int, ct_stride: int):
    buf = np.frombuffer(body, np.uint8)
    out = dict(report_ids=np.zeros((cap, 16), np.uint8), times=np.zeros(cap, np.uint64),
               public_shares=np.zeros((cap, lay.public_share_len), np.uint8),
               config_ids=np.zeros(cap, np.uint8), enc=np.zeros((cap, lay.enc_len), np.uint8),
               ct=np.zeros((cap, ct_stride), np.uint8), ct_len=np.zeros(cap, np.uint32),
               prep_shares=np.zeros((cap, lay.prep_share_len), np.uint8),
               msg_status=np.zeros(cap, np.uint8))
    n = _lib().janus_dap_agg_init_unpack_host(
        _np_ptr(buf), len(body), C.byref(lay), cap, _np_ptr(out["report_ids"]),
        _np_ptr(out["times"]), _np_ptr(out["public_shares"]), _np_ptr(out["config_ids"]),
        _np_ptr(out["enc"]), _np_ptr(out["ct"]), _np_ptr(out["ct_len"]), ct_stride,
        _np_ptr(out["prep_shares"]), _np_ptr(out["msg_status"]))
    if n < 0:
        raise ValueError("AggregationJobInitializeReq does not decode")
    return {k: v[:n] for k, v in out.items()}


def unpack_device(lay: Layout, d_body, ct_stride: int, stream=None):
    """d_body: uint8 torch tensor (padded by >= 4 bytes) on the GPU. Returns (dict of tensors,
    mismatch count); mismatch > 0 means the body is not uniform -> use unpack_host."""
    import torch
    dev = d_body.device
    n = lay.n
    u8 = dict(dtype=torch.uint8, device=dev)
    out = dict(report_ids=torch.empty((n, 16), **u8),
               times=torch.empty(n, dtype=torch.int64, device=dev),
               public_shares=torch.empty((n, max(lay.public_share_len, 1)), **u8),
               config_ids=torch.empty(n, **u8), enc=torch.empty((n, max(lay.enc_len, 1)), **u8),
               ct=torch.zeros((n, ct_stride), **u8),
               ct_len=torch.empty(n, dtype=torch.int32, device=dev),
               prep_shares=torch.empty((n, max(lay.prep_share_len, 1)), **u8),
               msg_status=torch.empty(n, **u8))
    mism = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib().janus_dap_agg_init_unpack_device(
        C.byref(lay), _tptr(d_body), _tptr(out["report_ids"]), _tptr(out["times"]),
        _tptr(out["public_shares"]) if lay.public_share_len else None, _tptr(out["config_ids"]),
        _tptr(out["enc"]), _tptr(out["ct"]), _tptr(out["ct_len"]), ct_stride,
        _tptr(out["prep_shares"]), _tptr(out["msg_status"]), _tptr(mism),
        _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_agg_init_unpack_device failed (rc={rc})")
    return out, mism


def encode_resp_host(report_ids, prepare_error, prio3_status, prep_msgs, prep_msg_len: int):
    ids = np.ascontiguousarray(report_ids, np.uint8)
    n = ids.shape[0]
    pe = np.ascontiguousarray(prepare_error, np.uint8)
    st = np.ascontiguousarray(prio3_status, np.uint8)
    pm = np.ascontiguousarray(prep_msgs, np.uint8) if prep_msg_len else None
    out = np.zeros(_lib().janus_dap_agg_job_resp_max_len(n, prep_msg_len), np.uint8)
    ln = _lib().janus_dap_agg_job_resp_encode_host(n, _np_ptr(ids), _np_ptr(pe), _np_ptr(st),
                                                   _np_ptr(pm), prep_msg_len, _np_ptr(out))
    return out[:ln].tobytes()


def encode_resp_device(report_ids, prepare_error, prio3_status, prep_msgs, prep_msg_len: int,
                       stream=None):
    """torch tensors on the GPU -> (out tensor, length tensor)."""
    import torch
    dev = report_ids.device
    n = report_ids.shape[0]
    out = torch.empty(_lib().janus_dap_agg_job_resp_max_len(n, prep_msg_len), dtype=torch.uint8,
                      device=dev)
    ln = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(n // 256 + 2, dtype=torch.int32, device=dev)
    rc = _lib().janus_dap_agg_job_resp_encode_device(
        n, _tptr(report_ids), _tptr(prepare_error), _tptr(prio3_status),
        _tptr(prep_msgs) if prep_msg_len else None, prep_msg_len, _tptr(out), _tptr(ln),
        _tptr(scratch), _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_agg_job_resp_encode_device failed (rc={rc})")
    return out, ln


# ---- leader side: encode the request, decode the response ----------------------------------
INDEX_NONE = 0xFFFFFFFF  # index[r] of a report that is not in the request
VDAF_PREP_ERROR = 5      # DAP PrepareError::VdafPrepError
AGG_PARAM_MAX = 256      # device form (JANUS_DAP_AGG_PARAM_MAX)
RESP_IRREGULAR, RESP_LISTLEN, RESP_TRAILING, RESP_MALFORMED = 1, 2, 4, 8
RESP_REJECT_CODE, RESP_COUNT, RESP_ID = 16, 32, 64
RESP_ERRORS = {-3: "the list length runs past the body", -4: "bytes after the list",
               -5: "a PrepareResp or its PingPongMessage does not decode",
               -6: "Reject with a PrepareError code above 9",
               -7: "the record count is not the request's",
               -8: "a record's report ID is not the expected one"}


class RespError(ValueError):
    """The whole AggregationJobResp is rejected; ``code`` is the JANUS_DAP_RESP_E* value."""

    def __init__(self, code):
        super().__init__(f"AggregationJobResp rejected: {RESP_ERRORS.get(code, code)} (rc={code})")
        self.code = code


def leader_outcome(leader_status, prepare_error, next_status):
    """Per-report outcome of the leader's init step, as prepare_error() is for the helper:
    NO_ERROR for a report that finished (it is accumulated), else the DAP PrepareError it fails
    with -- VdafPrepError when leader_initialized failed (leader_status != 0,
    aggregation_job_driver.rs:430-437), the helper's error (prepare_error from the response
    decode, :735-751), VdafPrepError when leader_continued failed (next_status != 0, :708-710).
    numpy arrays or torch tensors."""
    try:
        import torch
        if isinstance(leader_status, torch.Tensor):
            fail = torch.full_like(prepare_error, VDAF_PREP_ERROR)
            out = torch.where((prepare_error == NO_ERROR) & (next_status != 0), fail,
                              prepare_error)
            return torch.where(leader_status != 0, fail, out)
    except ImportError:
        pass
    ls, ns = np.asarray(leader_status), np.asarray(next_status)
    pe = np.asarray(prepare_error, np.uint8)
    out = np.where((pe == NO_ERROR) & (ns != 0), VDAF_PREP_ERROR, pe)
    return np.where(ls != 0, VDAF_PREP_ERROR, out).astype(np.uint8)


def _req_header_check(agg_param, query_type, batch_id):
    if query_type not in (1, 2):
        raise ValueError("query_type must be 1 (TimeInterval) or 2 (FixedSize)")
    if (query_type == 2) != (batch_id is not None) or (batch_id is not None and
                                                       len(batch_id) != 32):
        raise ValueError("FixedSize takes a 32-byte batch_id, TimeInterval none")
    return np.frombuffer(bytes(agg_param), np.uint8), \
        None if batch_id is None else np.frombuffer(bytes(batch_id), np.uint8)


def _req_shapes(n, rows, vecs):
    """rows: name -> 2-D [n, w] array / tensor (None: width 0); vecs: name -> 1-D [n]."""
    for k, v in rows.items():
        if v is not None and (v.ndim != 2 or v.shape[0] != n):
            raise ValueError(f"{k} must be [{n}, width], not {tuple(v.shape)}")
    for k, v in vecs.items():
        if tuple(v.shape) != (n,):
            raise ValueError(f"{k} must be [{n}], not {tuple(v.shape)}")
    if rows["report_ids"].shape[1] != 16:
        raise ValueError("report_ids must be [n, 16]")
    if rows["enc"].shape[1] > 0xFFFF:
        raise ValueError("enc is u16-prefixed")


def encode_req_host(agg_param: bytes, query_type: int, batch_id, report_ids, times,
                    public_shares, config_ids, enc, ct, ct_len, prep_shares, leader_status):
    """AggregationJobInitializeReq of the reports with leader_status 0 (host buffers).
    Returns (body bytes, index uint32 [n], n_included)."""
    ap, bid = _req_header_check(agg_param, query_type, batch_id)
    c = lambda a, t: np.ascontiguousarray(a, t)  # noqa: E731
    ids, tm, cfg = c(report_ids, np.uint8), c(times, np.uint64), c(config_ids, np.uint8)
    pub = None if public_shares is None or np.shape(public_shares)[1] == 0 else \
        c(public_shares, np.uint8)
    e, t, cl = c(enc, np.uint8), c(ct, np.uint8), c(ct_len, np.uint32)
    ps, st = c(prep_shares, np.uint8), c(leader_status, np.uint8)
    n = ids.shape[0]
    _req_shapes(n, dict(report_ids=ids, public_shares=pub, enc=e, ct=t, prep_shares=ps),
                dict(times=tm, config_ids=cfg, ct_len=cl, leader_status=st))
    if ((st == 0) & (cl > t.shape[1])).any():
        raise ValueError("a ct_len is above the ct row length")
    psl = 0 if pub is None else pub.shape[1]
    L = _lib()
    out = np.zeros(L.janus_dap_agg_init_req_max_len(n, len(ap), query_type, psl, e.shape[1],
                                                    t.shape[1], ps.shape[1]), np.uint8)
    index = np.zeros(n, np.uint32)
    ninc = C.c_uint32(0)
    ln = L.janus_dap_agg_init_req_encode_host(
        n, _np_ptr(ap), len(ap), query_type, _np_ptr(bid), _np_ptr(ids), _np_ptr(tm), _np_ptr(pub),
        psl, _np_ptr(cfg), _np_ptr(e), e.shape[1], _np_ptr(t), _np_ptr(cl), t.shape[1], _np_ptr(ps),
        ps.shape[1], _np_ptr(st), _np_ptr(out), _np_ptr(index), C.byref(ninc))
    if ln == -3:
        raise OverflowError("the PrepareInit list does not fit its u32 length prefix")
    if ln < 0:
        raise ValueError(f"janus_dap_agg_init_req_encode_host failed (rc={ln})")
    return out[:ln].tobytes(), index, ninc.value


def _dev_tensor(name, t, esize, dev):
    import torch
    if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor on {dev}")
    if t.element_size() != esize:
        raise ValueError(f"{name} must have {esize}-byte elements")
    return t


def encode_req_device(agg_param: bytes, query_type: int, batch_id, report_ids, times,
                      public_shares, config_ids, enc, ct, ct_len, prep_shares, leader_status,
                      stream=None):
    """Device form on torch tensors of one GPU (times: 8-byte, ct_len: 4-byte integers; ct /
    ct_len as HpkeSealer.seal_input_shares_device writes them).  Returns a dict of tensors:
    out (uint8, the body in its first out_len bytes), out_len (int64 [1]), index (int32 [n],
    -1 = left out), n_included (int32 [1]), err (int32 [2]: reports left out for a ct_len above
    the row length; 1 if the list does not fit a u32).  No host synchronisation."""
    import torch
    ap, bid = _req_header_check(agg_param, query_type, batch_id)
    if len(ap) > AGG_PARAM_MAX:
        raise ValueError(f"the device form takes up to {AGG_PARAM_MAX} aggregation parameter bytes")
    dev = report_ids.device
    if dev.type != "cuda":
        raise ValueError("encode_req_device takes GPU tensors")
    n = report_ids.shape[0]
    pub = None if public_shares is None or public_shares.shape[1] == 0 else public_shares
    rows = dict(report_ids=report_ids, public_shares=pub, enc=enc, ct=ct, prep_shares=prep_shares)
    vecs = dict(times=times, config_ids=config_ids, ct_len=ct_len, leader_status=leader_status)
    for k, v in rows.items():
        if v is not None and v.shape[1]:
            _dev_tensor(k, v, 1, dev)
    for k, v in vecs.items():
        _dev_tensor(k, v, 8 if k == "times" else 4 if k == "ct_len" else 1, dev)
    _req_shapes(n, rows, vecs)
    psl = 0 if pub is None else pub.shape[1]
    L = _lib()
    cap = L.janus_dap_agg_init_req_max_len(n, len(ap), query_type, psl, enc.shape[1], ct.shape[1],
                                           prep_shares.shape[1])
    res = dict(out=torch.empty(cap, dtype=torch.uint8, device=dev),
               out_len=torch.zeros(1, dtype=torch.int64, device=dev),
               index=torch.empty(n, dtype=torch.int32, device=dev),
               n_included=torch.zeros(1, dtype=torch.int32, device=dev),
               err=torch.zeros(2, dtype=torch.int32, device=dev))
    scratch = torch.empty((n + 1) // 2 + 2 * (n // 256 + 2), dtype=torch.int64, device=dev)
    w = lambda t: _tptr(t) if t is not None and t.shape[-1] else None  # noqa: E731
    rc = L.janus_dap_agg_init_req_encode_device(
        n, _np_ptr(ap), len(ap), query_type, _np_ptr(bid), _tptr(report_ids), _tptr(times), w(pub),
        psl, _tptr(config_ids), w(enc), enc.shape[1], w(ct), _tptr(ct_len), ct.shape[1],
        w(prep_shares), prep_shares.shape[1], _tptr(leader_status), _tptr(res["out"]),
        _tptr(res["out_len"]), _tptr(res["index"]), _tptr(res["n_included"]), _tptr(res["err"]),
        _tptr(scratch), _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_agg_init_req_encode_device failed (rc={rc})")
    return res


def unpack_resp_host(body: bytes, index, report_ids, n_included: int, prep_msg_len: int):
    """The leader's decode of an AggregationJobResp body (host buffers): returns (prep_msgs
    uint8 [n, prep_msg_len], prepare_error uint8 [n]) in the engine's row order; raises
    RespError when the whole response is rejected."""
    ids = np.ascontiguousarray(report_ids, np.uint8)
    idx = np.ascontiguousarray(index).astype(np.int64).astype(np.uint32)
    n = ids.shape[0]
    if ids.shape != (n, 16) or idx.shape != (n,):
        raise ValueError("report_ids must be [n, 16] and index [n]")
    inc = idx[idx != INDEX_NONE]
    if not 0 <= n_included <= n or len(inc) != n_included or \
            sorted(inc.tolist()) != list(range(n_included)):
        raise ValueError("index must number the n_included reports of the request 0 .. "
                         "n_included - 1")
    buf = np.frombuffer(bytes(body) + b"\0", np.uint8)
    msgs = np.zeros((n, prep_msg_len), np.uint8)
    pe = np.zeros(n, np.uint8)
    rc = _lib().janus_dap_agg_job_resp_unpack_host(n, _np_ptr(idx), _np_ptr(ids), n_included,
                                                   _np_ptr(buf), len(body), prep_msg_len,
                                                   _np_ptr(msgs), _np_ptr(pe))
    if rc in RESP_ERRORS:
        raise RespError(rc)
    if rc:
        raise ValueError(f"janus_dap_agg_job_resp_unpack_host failed (rc={rc})")
    return msgs, pe


def unpack_resp_device(d_body, body_len: int, index, report_ids, n_included: int,
                       prep_msg_len: int, stream=None):
    """Device form: d_body is a uint8 tensor holding the body and at least 4 more bytes; index
    (int32 [n], as encode_req_device returns it) and report_ids (uint8 [n, 16]) are tensors on
    the same GPU.  Returns (prep_msgs [n, max(prep_msg_len, 1)], prepare_error [n], flags int32
    [1]); a non-zero flags (RESP_* bits) means the outputs are incomplete: RESP_IRREGULAR alone
    sends the body to unpack_resp_host, every other bit rejects the response."""
    import torch
    dev = d_body.device
    if dev.type != "cuda":
        raise ValueError("unpack_resp_device takes GPU tensors")
    n = report_ids.shape[0]
    _dev_tensor("d_body", d_body, 1, dev)
    _dev_tensor("index", index, 4, dev)
    _dev_tensor("report_ids", report_ids, 1, dev)
    if tuple(report_ids.shape) != (n, 16) or tuple(index.shape) != (n,):
        raise ValueError("report_ids must be [n, 16] and index [n]")
    if not 0 <= n_included <= n:
        raise ValueError("n_included must be within 0 .. n")
    if body_len < 0 or d_body.numel() < body_len + 4:
        raise ValueError("d_body must hold the body and 4 bytes of padding")
    msgs = torch.empty((n, max(prep_msg_len, 1)), dtype=torch.uint8, device=dev)
    pe = torch.empty(n, dtype=torch.uint8, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(2 * (n_included + 2), dtype=torch.int32, device=dev)
    rc = _lib().janus_dap_agg_job_resp_unpack_device(
        n, _tptr(index), _tptr(report_ids), n_included, _tptr(d_body), body_len, prep_msg_len,
        _tptr(msgs) if prep_msg_len else None, _tptr(pe), _tptr(flags), _tptr(scratch),
        _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_agg_job_resp_unpack_device failed (rc={rc})")
    return msgs, pe, flags


# ---- client side: the upload body ---------------------------------------------------------
def report_max_len(public_share_len: int, leader_enc_len: int, leader_ct_stride: int,
                   helper_enc_len: int, helper_ct_stride: int) -> int:
    """Row length that holds any Report of these field lengths (janus_dap_report_max_len)."""
    return _lib().janus_dap_report_max_len(public_share_len, leader_enc_len, leader_ct_stride,
                                           helper_enc_len, helper_ct_stride)


def _report_shapes(n, public_shares, cts, out_stride):
    """Argument rules shared by both Report encoders; returns (public share length, stride)."""
    psl = 0 if public_shares is None else public_shares.shape[1]
    if public_shares is not None and (len(public_shares.shape) != 2 or public_shares.shape[0] != n):
        raise ValueError("public_shares must be None or [n, public_share_len]")
    for who, (cfg, enc, ct, ct_len) in cts.items():
        if not 0 <= int(cfg) <= 0xFF:
            raise ValueError(f"{who}_config_id is one byte")
        if len(enc.shape) != 2 or enc.shape[0] != n or enc.shape[1] > 0xFFFF:
            raise ValueError(f"{who}_enc must be [n, enc_len] with a u16-prefixed enc_len")
        if len(ct.shape) != 2 or ct.shape[0] != n or tuple(ct_len.shape) != (n,):
            raise ValueError(f"{who}_ct must be [n, ct_stride] and {who}_ct_len [n]")
    need = report_max_len(psl, cts["leader"][1].shape[1], cts["leader"][2].shape[1],
                          cts["helper"][1].shape[1], cts["helper"][2].shape[1])
    stride = need if out_stride is None else int(out_stride)
    if stride < need:
        raise ValueError(f"out_stride must be >= report_max_len(...) = {need}")
    return psl, stride


def report_encode_host(report_ids, times, public_shares, leader_config_id: int, leader_enc,
                       leader_ct, leader_ct_len, helper_config_id: int, helper_enc, helper_ct,
                       helper_ct_len, skip=None, out_stride=None):
    """DAP ``Report`` rows from host SoA buffers: returns (out uint8 [n, out_stride], out_len
    uint32 [n]).  A report whose skip byte is non-zero, or one of whose ct_len is 0 or above its
    row, is left out (length 0, zero row)."""
    c = lambda a, t: np.ascontiguousarray(a, t)  # noqa: E731
    ids, tm = c(report_ids, np.uint8), c(times, np.uint64)
    n = ids.shape[0]
    if ids.shape != (n, 16) or tm.shape != (n,):
        raise ValueError("report_ids must be [n, 16] and times [n]")
    pub = None if public_shares is None or np.shape(public_shares)[1] == 0 else \
        c(public_shares, np.uint8)
    le, lc, ll = c(leader_enc, np.uint8), c(leader_ct, np.uint8), c(leader_ct_len, np.uint32)
    he, hc, hl = c(helper_enc, np.uint8), c(helper_ct, np.uint8), c(helper_ct_len, np.uint32)
    sk = None if skip is None else c(skip, np.uint8)
    if sk is not None and sk.shape != (n,):
        raise ValueError("skip must be [n]")
    psl, stride = _report_shapes(n, pub, dict(leader=(leader_config_id, le, lc, ll),
                                              helper=(helper_config_id, he, hc, hl)), out_stride)
    out = np.zeros((n, stride), np.uint8)
    out_len = np.zeros(n, np.uint32)
    w = lambda a: _np_ptr(a) if a is not None and a.size else None  # noqa: E731
    rc = _lib().janus_dap_report_encode_host(
        n, _np_ptr(ids), _np_ptr(tm), w(pub), psl, leader_config_id, w(le), le.shape[1], w(lc),
        _np_ptr(ll), lc.shape[1], helper_config_id, w(he), he.shape[1], w(hc), _np_ptr(hl),
        hc.shape[1], _np_ptr(sk), _np_ptr(out), stride, _np_ptr(out_len))
    if rc < 0:
        raise ValueError(f"janus_dap_report_encode_host failed (rc={rc})")
    return out, out_len


def report_encode_device(report_ids, times, public_shares, leader_config_id: int, leader_enc,
                         leader_ct, leader_ct_len, helper_config_id: int, helper_enc, helper_ct,
                         helper_ct_len, skip=None, out_stride=None, stream=None):
    """Device form on torch tensors of one GPU (times 8-byte, ct_len 4-byte integers, the rows as
    HpkeSealer.seal_input_shares_device writes them).  Returns (out uint8 [n, out_stride],
    out_len int32 [n]); no host synchronisation."""
    import torch
    dev = report_ids.device
    if dev.type != "cuda":
        raise ValueError("report_encode_device takes GPU tensors")
    n = report_ids.shape[0]
    if tuple(report_ids.shape) != (n, 16) or tuple(times.shape) != (n,):
        raise ValueError("report_ids must be [n, 16] and times [n]")
    pub = None if public_shares is None or public_shares.shape[1] == 0 else public_shares
    psl, stride = _report_shapes(n, pub, dict(
        leader=(leader_config_id, leader_enc, leader_ct, leader_ct_len),
        helper=(helper_config_id, helper_enc, helper_ct, helper_ct_len)), out_stride)
    for k, v, es in (("report_ids", report_ids, 1), ("times", times, 8), ("public_shares", pub, 1),
                     ("leader_enc", leader_enc, 1), ("leader_ct", leader_ct, 1),
                     ("leader_ct_len", leader_ct_len, 4), ("helper_enc", helper_enc, 1),
                     ("helper_ct", helper_ct, 1), ("helper_ct_len", helper_ct_len, 4),
                     ("skip", skip, 1)):
        if v is not None:
            _dev_tensor(k, v, es, dev)
    if skip is not None and tuple(skip.shape) != (n,):
        raise ValueError("skip must be [n]")
    out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    w = lambda t: _tptr(t) if t is not None and t.numel() else None  # noqa: E731
    rc = _lib().janus_dap_report_encode_device(
        n, _tptr(report_ids), _tptr(times), w(pub), psl, leader_config_id, w(leader_enc),
        leader_enc.shape[1], w(leader_ct), _tptr(leader_ct_len), leader_ct.shape[1],
        helper_config_id, w(helper_enc), helper_enc.shape[1], w(helper_ct), _tptr(helper_ct_len),
        helper_ct.shape[1], _tptr(skip), _tptr(out), stride, _tptr(out_len),
        _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_report_encode_device failed (rc={rc})")
    return out, out_len


# ---- leader upload: the Report rows, decoded -------------------------------------------------
REPORT_FIELDS = 10  # JANUS_DAP_REPORT_FIELDS
(F_PUBLIC_SHARE_OFF, F_PUBLIC_SHARE_LEN, F_LEADER_ENC_OFF, F_LEADER_ENC_LEN, F_LEADER_PAYLOAD_OFF,
 F_LEADER_PAYLOAD_LEN, F_HELPER_ENC_OFF, F_HELPER_ENC_LEN, F_HELPER_PAYLOAD_OFF,
 F_HELPER_PAYLOAD_LEN) = range(REPORT_FIELDS)


def _decode_shapes(reports, report_len, helper_enc_len, helper_ct_stride):
    if len(reports.shape) != 2 or tuple(report_len.shape) != (reports.shape[0],):
        raise ValueError("reports must be [n, report_stride] and report_len [n]")
    if not 0 <= int(helper_enc_len) <= 0xFFFF:
        raise ValueError("helper_enc_len is u16-prefixed")
    if reports.shape[1] >= 1 << 31 or not 0 <= int(helper_ct_stride) < 1 << 32:
        raise ValueError("report_stride must be below 2^31 and helper_ct_stride fit a u32")
    return reports.shape[0], reports.shape[1]


def report_decode_host(reports, report_len, helper_enc_len: int, helper_ct_stride: int):
    """The inverse of report_encode_host (janus_dap_report_decode_host, no GPU): reports uint8
    [n, report_stride] with report_len [n] -> dict of report_ids [n, 16], times uint64 [n], fields
    uint32 [n, REPORT_FIELDS] (offset and length of the public share and of both ciphertexts' enc
    and payload within the row, at the F_* indices), leader_config_ids, helper_config_ids, the
    helper ciphertext rows helper_enc [n, helper_enc_len] / helper_ct [n, helper_ct_stride] /
    helper_ct_len [n], and malformed uint8 [n] (1: the Report does not decode; its outputs are
    zero)."""
    rows = np.ascontiguousarray(reports, np.uint8)
    ln = np.ascontiguousarray(report_len, np.uint32)
    n, stride = _decode_shapes(rows, ln, helper_enc_len, helper_ct_stride)
    out = dict(report_ids=np.empty((n, 16), np.uint8), times=np.empty(n, np.uint64),
               fields=np.empty((n, REPORT_FIELDS), np.uint32),
               leader_config_ids=np.empty(n, np.uint8), helper_config_ids=np.empty(n, np.uint8),
               helper_enc=np.empty((n, helper_enc_len), np.uint8),
               helper_ct=np.empty((n, helper_ct_stride), np.uint8),
               helper_ct_len=np.empty(n, np.uint32), malformed=np.empty(n, np.uint8))
    w = lambda a: _np_ptr(a) if a.size else None  # noqa: E731
    rc = _lib().janus_dap_report_decode_host(
        n, w(rows), stride, _np_ptr(ln), _np_ptr(out["report_ids"]), _np_ptr(out["times"]),
        _np_ptr(out["fields"]), _np_ptr(out["leader_config_ids"]),
        _np_ptr(out["helper_config_ids"]), w(out["helper_enc"]), helper_enc_len,
        w(out["helper_ct"]), _np_ptr(out["helper_ct_len"]), helper_ct_stride,
        _np_ptr(out["malformed"]))
    if rc < 0:
        raise ValueError(f"janus_dap_report_decode_host failed (rc={rc})")
    return out


def report_decode_device(reports, report_len, helper_enc_len: int, helper_ct_stride: int,
                         stream=None):
    """Device form on torch tensors of one GPU (reports uint8 [n, report_stride], report_len int32
    [n], as prepare_reports_device returns them): the same dict as report_decode_host, as tensors
    (times int64, fields / helper_ct_len int32); no host synchronisation."""
    import torch
    dev = reports.device
    if dev.type != "cuda":
        raise ValueError("report_decode_device takes GPU tensors")
    _dev_tensor("reports", reports, 1, dev)
    _dev_tensor("report_len", report_len, 4, dev)
    n, stride = _decode_shapes(reports, report_len, helper_enc_len, helper_ct_stride)
    u8 = dict(dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(report_ids=torch.empty((n, 16), **u8),
               times=torch.empty(n, dtype=torch.int64, device=dev),
               fields=torch.empty((n, REPORT_FIELDS), **i32),
               leader_config_ids=torch.empty(n, **u8), helper_config_ids=torch.empty(n, **u8),
               helper_enc=torch.empty((n, helper_enc_len), **u8),
               helper_ct=torch.empty((n, helper_ct_stride), **u8),
               helper_ct_len=torch.empty(n, **i32), malformed=torch.empty(n, **u8))
    if n == 0:
        return out
    w = lambda t: _tptr(t) if t.numel() else None  # noqa: E731
    rc = _lib().janus_dap_report_decode_device(
        n, w(reports), stride, _tptr(report_len), _tptr(out["report_ids"]), _tptr(out["times"]),
        _tptr(out["fields"]), _tptr(out["leader_config_ids"]), _tptr(out["helper_config_ids"]),
        w(out["helper_enc"]), helper_enc_len, w(out["helper_ct"]), _tptr(out["helper_ct_len"]),
        helper_ct_stride, _tptr(out["malformed"]), _stream(stream, dev.index or 0))
    if rc:
        raise RuntimeError(f"janus_dap_report_decode_device failed (rc={rc})")
    return out

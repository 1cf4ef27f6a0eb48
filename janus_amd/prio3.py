"""Host-side mirror of the prio 0.16.2 ``Prio3`` aggregator surface that Janus uses on the
helper's aggregate-init hot path, backed by the gfx950 HIP engine (``libjanus_prio3.so``).

Reference surface being mirrored:
  * instance constructors ``Prio3::new_count / new_sum / new_sum_vec_multithreaded /
    new_histogram`` as dispatched by ``vdaf_dispatch!`` (/root/reference/core/src/vdaf.rs:198-300);
  * the per-report ``helper_initialized(..) + evaluate(..)`` call inside
    ``handle_aggregate_init_generic`` (/root/reference/aggregator/src/aggregator.rs:2020-2042),
    here batched over the whole job;
  * ``AggregateShare::merge`` accumulation performed by ``AggregationJobWriter``
    (/root/reference/aggregator/src/aggregator/aggregation_job_writer.rs:591-695).

There is no CPU fallback: if the HIP library is missing or no GPU is present, engine
creation raises.  (The CPU restatement under ``oracle/`` is test infrastructure only.)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# JANUS_PRIO3_LIB selects an alternative build of the same sources (A/B experiments,
# tools/build_variant.sh); the default is the in-tree library built by `make -C janus_amd`.
LIB_PATH = os.environ.get("JANUS_PRIO3_LIB") or os.path.join(_HERE, "libjanus_prio3.so")

PRIO3_COUNT, PRIO3_SUM, PRIO3_SUMVEC, PRIO3_HISTOGRAM, PRIO3_SUMVEC_F64_MP = 0, 1, 2, 3, 4
PRIO3_FPVEC_BOUNDED_L2 = 5

STATUS_FINISHED = 0
STATUS_PREP_INIT = 1
STATUS_PREP_SHARE_DECODE = 2
STATUS_PREP_MSG = 3
# leader upload (prio3_leader_upload_batch): per-report status, Janus's ReportRejectionReason from 1
(UPLOAD_OK, UPLOAD_INTERVAL_COLLECTED, UPLOAD_DECRYPT_FAILURE, UPLOAD_DECODE_FAILURE,
 UPLOAD_TASK_EXPIRED, UPLOAD_EXPIRED, UPLOAD_TOO_EARLY, UPLOAD_OUTDATED_HPKE_CONFIG) = range(8)
UPLOAD_MALFORMED, UPLOAD_HOST = 0x40, 0x41
UINT64_MAX = (1 << 64) - 1
STATUS_PREP_NEXT = 4
STATUS_PEER_MISMATCH = 5
STATUS_INPUT_SHARE_DECODE = 6
#: merged statuses of prio3_helper_aggregate_init_batch[_ex]: 0x80 | the DAP PrepareError of a
#: report the helper rejected before its VDAF ran (aggregator.rs:1847-2015): the input-share open
#: and decode first, then the report deadline
STATUS_HPKE_DECRYPT = 0x84
STATUS_INVALID_MESSAGE = 0x88
STATUS_REPORT_TOO_EARLY = 0x89

#: prio ``PingPongError`` variant for each status (error.rs:365-428 maps these to labels).
STATUS_PINGPONG_ERROR = {
    STATUS_PREP_INIT: "VdafPrepareInit",
    STATUS_PREP_SHARE_DECODE: "CodecPrepShare",
    STATUS_PREP_MSG: "VdafPrepareSharesToPrepareMessage",
    STATUS_PREP_NEXT: "VdafPrepareNext",
    STATUS_PEER_MISMATCH: "PeerMessageMismatch",
    STATUS_INPUT_SHARE_DECODE: "InvalidMessage",
}

#: ``janus_step_failures{type=...}`` metric label per status, helper role
#: (handle_ping_pong_error, /root/reference/aggregator/src/aggregator/error.rs:379-411).
STATUS_METRIC_LABEL = {
    STATUS_PREP_INIT: "prepare_init_failure",
    STATUS_PREP_SHARE_DECODE: "leader_prep_share_decode_failure",
    STATUS_PREP_MSG: "prepare_message_failure",
    STATUS_PREP_NEXT: "prepare_next_failure",
    STATUS_PEER_MISMATCH: "leader_ping_pong_message_mismatch",
}


class Prio3Params(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("bits", C.c_uint32), ("length", C.c_uint32),
                ("chunk_length", C.c_uint32), ("num_proofs", C.c_uint32)]


class Prio3MemberInfo(C.Structure):
    _fields_ = [("device", C.c_int32), ("lane", C.c_uint32), ("jobs", C.c_uint64),
                ("reports", C.c_uint64), ("exec_jobs", C.c_uint64), ("exec_groups", C.c_uint64)]


class Prio3ExecutorStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("jobs", "reports", "groups", "active_jobs",
                                          "active_reports")]


#: executor kinds of prio3_executor_stats_get
EXEC_PREPARE, EXEC_ACCUMULATE, EXEC_LEADER_INIT, EXEC_LEADER_NEXT = 0, 1, 2, 3
EXEC_UPLOAD = 5  # the leader upload's (4 is the HPKE open's, janus_amd/hpke.py)


class Prio3Sizes(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "field_bytes", "meas_len", "out_len", "proof_len", "verifier_len", "joint_rand_len",
        "nonce_len", "public_share_len", "helper_share_len", "prep_share_len", "prep_msg_len",
        "agg_share_len", "leader_input_share_len")]


class Prio3JobIndexInfo(C.Structure):
    """prio3_job_index_info (include/janus_prio3.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("n_segments", "overflow", "n_duplicates",
                                          "first_duplicate", "n_closed", "n_time_errors")]


#: d_reject of a report in a closed batch: 0x80 | PrepareError::BatchCollected
REJECT_BATCH_COLLECTED = 0x80

#: the limits of prio3_helper_aggregate_job's in-group path (PRIO3_JOB_GROUP_MAX_REPORTS /
#: PRIO3_JOB_GROUP_MAX_SEGMENTS); a larger job runs the three calls inside the entry point
JOB_GROUP_MAX_REPORTS = 4096
JOB_GROUP_MAX_SEGMENTS = 64


class Prio3HelperJobIn(C.Structure):
    """prio3_helper_job_in (include/janus_prio3.h)."""
    _fields_ = [("opener", C.c_void_p), ("fallback_opener", C.c_void_p),
                ("report_deadline", C.c_uint64), ("n", C.c_uint32),
                ("require_taskprov", C.c_int32), ("task_id", C.c_void_p),
                ("report_ids", C.c_void_p), ("times", C.c_void_p), ("public_shares", C.c_void_p),
                ("enc", C.c_void_p), ("ct", C.c_void_p), ("ct_len", C.c_void_p),
                ("leader_prep_shares", C.c_void_p), ("ct_stride", C.c_uint32), ("k", C.c_uint32),
                ("time_precision", C.c_uint64), ("closed_intervals", C.c_void_p),
                ("accept_mask", C.c_void_p), ("max_segments", C.c_uint32),
                ("reserved", C.c_uint32)]


class Prio3HelperJobOut(C.Structure):
    """prio3_helper_job_out (include/janus_prio3.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "segment_ids", "segment_starts", "reject", "duplicate", "info", "prep_msgs", "status",
        "agg_shares", "counts", "checksums", "intervals")]


#: the report limit of prio3_leader_upload_job's in-group path (PRIO3_UPLOAD_JOB_MAX_REPORTS); a
#: larger job runs prio3_leader_upload_batch inside the entry point
UPLOAD_JOB_MAX_REPORTS = 4096


class Prio3UploadJobIn(C.Structure):
    """prio3_upload_job_in (include/janus_prio3.h)."""
    _fields_ = [("task_opener", C.c_void_p), ("global_opener", C.c_void_p),
                ("task_config_id", C.c_uint8), ("global_config_id", C.c_uint8),
                ("reserved", C.c_uint8 * 2), ("n", C.c_uint32), ("task_id", C.c_uint8 * 32),
                ("now", C.c_uint64), ("report_deadline", C.c_uint64),
                ("task_expiration", C.c_uint64), ("report_expiry_age", C.c_uint64),
                ("reports", C.c_void_p), ("report_len", C.c_void_p),
                ("report_stride", C.c_uint32), ("ext_stride", C.c_uint32),
                ("helper_enc_len", C.c_uint32), ("helper_ct_stride", C.c_uint32)]


class Prio3UploadJobOut(C.Structure):
    """prio3_upload_job_out (include/janus_prio3.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "report_ids", "times", "public_shares", "leader_input_shares", "extensions", "ext_len",
        "helper_config_ids", "helper_enc", "helper_ct", "helper_ct_len", "leader_config_ids",
        "status")]


class Prio3LeaderJobIn(C.Structure):
    """prio3_leader_job_in (include/janus_prio3.h)."""
    _fields_ = [("report_ids", C.c_void_p), ("times", C.c_void_p),
                ("leader_status", C.c_void_p), ("prepare_error", C.c_void_p),
                ("prep_msgs", C.c_void_p), ("time_precision", C.c_uint64),
                ("closed_intervals", C.c_void_p), ("accept_mask", C.c_void_p),
                ("k", C.c_uint32), ("max_segments", C.c_uint32)]


class Prio3LeaderJobOut(C.Structure):
    """prio3_leader_job_out (include/janus_prio3.h)."""
    _fields_ = [(n, C.c_void_p) for n in (
        "segment_ids", "segment_starts", "reject", "duplicate", "info", "status", "outcome",
        "agg_shares", "counts", "checksums", "intervals")]


#: Every symbol include/janus_prio3.h declares.
EXPORTED_SYMBOLS = (
    "prio3_sizes", "prio3_engine_create", "prio3_engine_destroy", "prio3_helper_prepare_batch",
    "prio3_helper_prepare_aggregate_batch",
    "prio3_accumulate", "prio3_debug_output_shares", "prio3_batch_free", "prio3_device_prepare",
    "prio3_device_accumulate", "prio3_device_output_shares", "prio3_device_combine",
    "prio3_engine_set_option", "prio3_engine_timing", "prio3_engine_timing_reset",
    "prio3_client_generate_device", "prio3_selftest_field", "prio3_trace_enabled", "prio3_device_prepare_aggregate",
    "prio3_device_trim",
    "prio3_device_aggregate_finish", "prio3_leader_prepare_init_batch",
    "prio3_leader_prepare_next_batch", "prio3_device_leader_prepare_init",
    "prio3_device_leader_prepare_next", "prio3_device_batch_metadata", "prio3_batch_metadata",
    "prio3_device_combine_metadata", "prio3_engine_create_ex", "prio3_engine_create_mask",
    "prio3_engine_create_devices", "prio3_engine_members", "prio3_executor_control",
    "prio3_executor_stats_get", "prio3_helper_aggregate_init_batch",
    "prio3_helper_aggregate_init_batch_ex",
    "prio3_leader_prepare_next_aggregate_batch",
    "prio3_client_shard_device", "prio3_client_shard_batch", "prio3_client_prepare_reports_device",
    "prio3_client_rand_len", "prio3_client_report_stride", "prio3_selftest_tile",
    "prio3_selftest_field64",
    "prio3_device_leader_upload", "prio3_leader_upload_batch",
    "prio3_device_job_index", "prio3_job_index", "prio3_helper_aggregate_job",
    "prio3_leader_finish_job",
    "prio3_helper_prepare_aggregate_batch_submit", "prio3_helper_aggregate_init_batch_ex_submit",
    "prio3_helper_aggregate_job_submit", "prio3_leader_prepare_init_batch_submit",
    "prio3_leader_finish_job_submit", "prio3_ticket_poll", "prio3_ticket_wait",
    "prio3_leader_upload_job", "prio3_leader_upload_job_submit",
)
# include/janus_hpke.h (the batched HPKE opener, janus_amd/hpke.py)
HPKE_EXPORTED_SYMBOLS = (
    "janus_hpke_opener_create", "janus_hpke_opener_destroy",
    "janus_hpke_open_input_shares_device", "janus_hpke_open_input_shares",
    "janus_hpke_open_device", "janus_hpke_open", "janus_hpke_set_timing", "janus_hpke_timing",
    "janus_hpke_selftest_p256", "janus_hpke_selftest_field", "janus_hpke_executor_stats_get",
    "janus_hpke_executor_control",
    "janus_hpke_sealer_create", "janus_hpke_sealer_destroy", "janus_hpke_seal_device",
    "janus_hpke_seal", "janus_hpke_seal_input_shares_device", "janus_hpke_seal_input_shares",
)

_lib = None


def load_library() -> C.CDLL:
    """Load the in-tree HIP engine; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"janus_amd HIP engine not built: {LIB_PATH} is missing "
                          "(run `make -C janus_amd` or __graft_entry__.build())")
    # One HIP runtime per process: when PyTorch-ROCm is present its bundled libamdhip64
    # (SONAME libamdhip64.so.7) must be the copy our NEEDED entry binds to, otherwise two HSA
    # runtimes coexist and the second one sees no GPU.  Importing torch first makes the
    # dynamic linker reuse torch's runtime for libjanus_prio3.so.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # RTLD_GLOBAL: the native jobs harness (libjanus_jobs.so, linked against libjanus_prio3.so)
    # then binds to this same copy, also when JANUS_PRIO3_LIB selects an A/B build -- one engine
    # library (one set of executors) per process
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    P, u8p, vp = C.POINTER, C.POINTER(C.c_uint8), C.c_void_p
    L.prio3_sizes.argtypes = [P(Prio3Params), P(Prio3Sizes)]
    L.prio3_engine_create.argtypes = [P(Prio3Params), u8p, C.c_int, P(vp)]
    L.prio3_engine_create_ex.argtypes = [P(Prio3Params), u8p, C.c_size_t, C.c_int, P(vp)]
    L.prio3_engine_create_mask.argtypes = [P(Prio3Params), u8p, C.c_size_t, C.c_int, P(vp)]
    L.prio3_engine_create_devices.argtypes = [P(Prio3Params), u8p, C.c_size_t, P(C.c_int),
                                              C.c_uint32, P(vp)]
    L.prio3_engine_members.argtypes = [vp, P(Prio3MemberInfo), C.c_uint32]
    L.prio3_executor_control.argtypes = [vp, C.c_int, C.c_char_p, C.c_int64]
    L.prio3_executor_stats_get.argtypes = [vp, C.c_uint32, C.c_int, P(Prio3ExecutorStats)]
    L.prio3_engine_destroy.argtypes = [vp]
    L.prio3_engine_destroy.restype = None
    L.prio3_helper_prepare_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, P(vp)]
    L.prio3_accumulate.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
    L.prio3_helper_prepare_aggregate_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                                       C.c_uint32, vp, vp, vp, vp]
    u32 = C.c_uint32
    L.prio3_helper_aggregate_init_batch.argtypes = [vp, vp, u32, vp, C.c_int, vp, vp, vp, vp, vp,
                                                    vp, u32, vp, vp, vp, u32, vp, vp, vp, vp]
    L.prio3_helper_aggregate_init_batch_ex.argtypes = [vp, vp, vp, C.c_uint64, u32, vp, C.c_int, vp,
                                                       vp, vp, vp, vp, vp, u32, vp, vp, vp, u32,
                                                       vp, vp, vp, vp]
    L.prio3_helper_aggregate_job.argtypes = [vp, P(Prio3HelperJobIn), P(Prio3HelperJobOut)]
    L.prio3_leader_finish_job.argtypes = [vp, P(Prio3LeaderJobIn), P(Prio3LeaderJobOut)]
    L.prio3_leader_upload_job.argtypes = [vp, P(Prio3UploadJobIn), P(Prio3UploadJobOut)]
    # the ticketed twins: the same arguments, then notify_fd and ticket_out
    for name in ("prio3_helper_prepare_aggregate_batch", "prio3_helper_aggregate_init_batch_ex",
                 "prio3_helper_aggregate_job", "prio3_leader_finish_job",
                 "prio3_leader_upload_job"):
        getattr(L, name + "_submit").argtypes = getattr(L, name).argtypes + [C.c_int, P(vp)]
    L.prio3_leader_prepare_init_batch_submit.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, P(vp),
                                                         C.c_int, P(vp)]
    L.prio3_ticket_poll.argtypes = [vp]
    L.prio3_ticket_wait.argtypes = [vp]
    L.prio3_debug_output_shares.argtypes = [vp, vp]
    L.prio3_batch_free.argtypes = [vp]
    L.prio3_batch_free.restype = None
    L.prio3_device_prepare.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.prio3_device_accumulate.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.prio3_device_output_shares.argtypes = [vp, C.c_uint32, vp]
    L.prio3_device_combine.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.prio3_client_generate_device.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp,
                                               vp, vp, vp, vp, vp, vp, vp]
    L.prio3_engine_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.prio3_engine_timing.argtypes = [vp, C.c_char_p, C.c_size_t, P(C.c_double),
                                      P(C.c_uint64), C.c_int]
    L.prio3_engine_timing_reset.argtypes = [vp]
    L.prio3_engine_timing_reset.restype = None
    L.prio3_selftest_field.argtypes = [C.c_int, C.c_uint32, vp, vp, vp]
    L.prio3_selftest_tile.argtypes = [C.c_uint32, vp, vp]
    L.prio3_selftest_field64.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.prio3_trace_enabled.argtypes = []
    L.prio3_device_trim.argtypes = [C.c_int]
    L.prio3_device_prepare_aggregate.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32,
                                                 vp, vp, vp]
    L.prio3_device_aggregate_finish.argtypes = [vp, vp, vp, vp, vp, vp]
    L.prio3_leader_prepare_init_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, P(vp)]
    L.prio3_leader_prepare_next_batch.argtypes = [vp, vp, vp]
    L.prio3_leader_prepare_next_aggregate_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp,
                                                            vp]
    L.prio3_device_leader_prepare_init.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.prio3_device_leader_prepare_next.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.prio3_device_batch_metadata.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, vp,
                                              vp, vp]
    L.prio3_batch_metadata.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, vp, vp]
    L.prio3_device_combine_metadata.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    jix = [vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.prio3_device_job_index.argtypes = jix + [vp, vp]
    L.prio3_job_index.argtypes = jix + [P(Prio3JobIndexInfo)]
    L.prio3_client_rand_len.argtypes = [P(Prio3Params)]
    L.prio3_client_shard_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.prio3_client_shard_batch.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.prio3_client_report_stride.argtypes = [P(Prio3Params), vp, vp, C.c_int]
    L.prio3_client_prepare_reports_device.argtypes = [vp, vp, vp, u32, vp, C.c_uint64, vp, vp, vp,
                                                      vp, vp, vp, C.c_uint8, C.c_uint8, C.c_int,
                                                      vp, u32, vp, vp, vp]
    u8, u64 = C.c_uint8, C.c_uint64
    up = [vp, vp, u8, vp, u8, u32, vp, u64, u64, u64, u64, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32,
          vp, vp, u32, vp, vp, u32, vp, vp]
    L.prio3_leader_upload_batch.argtypes = up
    L.prio3_device_leader_upload.argtypes = up + [vp]
    _lib = L
    return L


def trim_device_pool(device: int = 0) -> None:
    """Free the idle scratch slabs the engine keeps on `device` (prio3_device_trim)."""
    rc = load_library().prio3_device_trim(device)
    if rc:
        raise RuntimeError(f"prio3_device_trim failed (rc={rc})")


def selftest_field(op: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Test hook: device Field128 primitive ``op`` over uint8 [m, 16] operands (see header)."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    n = a.shape[0] // (16 if op >= 4 else 1)
    out = np.zeros((n, 16), np.uint8)
    rc = load_library().prio3_selftest_field(op, n, _np_ptr(a), _np_ptr(b), _np_ptr(out))
    if rc:
        raise RuntimeError(f"prio3_selftest_field failed (rc={rc})")
    return out


def selftest_field64(op: int, n: int, k: int, a: np.ndarray,
                     b: Optional[np.ndarray] = None) -> np.ndarray:
    """Test hook: Field64 primitives and the limit-operand pieces of Field128 (ops of
    prio3_selftest_field64 in the header) over uint8 operand rows; returns uint8 [n, 8]
    (op 7: [n, 16]; op 8: [2, n, 16])."""
    a = np.ascontiguousarray(a, np.uint8)
    b = None if b is None else np.ascontiguousarray(b, np.uint8)
    per = k if op == 4 else 2 * k if op == 8 else 1
    es = 16 if op >= 6 else 8
    assert a.size == per * n * es and (b is None or b.size == a.size)
    out = np.zeros((2, n, 16) if op == 8 else (n, 16 if op == 7 else 8), np.uint8)
    rc = load_library().prio3_selftest_field64(op, n, k, _np_ptr(a),
                                               None if b is None else _np_ptr(b), _np_ptr(out))
    if rc:
        raise RuntimeError(f"prio3_selftest_field64 failed (rc={rc})")
    return out


def selftest_tile(values: np.ndarray, n_elems: int) -> np.ndarray:
    """Test hook: the fused accumulate's tile reduction over uint8 [8, 64, 16] (slot, lane, LE
    bytes); returns uint32 [n_elems, 8], the 16-bit-weighted addends of each slot's wave sum."""
    values = np.ascontiguousarray(values, np.uint8)
    assert values.shape == (8, 64, 16)
    out = np.zeros((n_elems, 8), np.uint32)
    rc = load_library().prio3_selftest_tile(n_elems, _np_ptr(values), _np_ptr(out))
    if rc:
        raise RuntimeError(f"prio3_selftest_tile failed (rc={rc})")
    return out


# ------------------------------------------------------------------------------------
# VDAF instances (mirrors of prio's constructors; names follow core/src/vdaf.rs)
# ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Prio3:
    kind: int
    bits: int = 0
    length: int = 0
    chunk_length: int = 0
    num_proofs: int = 1

    def params(self) -> Prio3Params:
        return Prio3Params(self.kind, self.bits, self.length, self.chunk_length, self.num_proofs)

    def sizes(self) -> Prio3Sizes:
        s = Prio3Sizes()
        rc = load_library().prio3_sizes(C.byref(self.params()), C.byref(s))
        if rc:
            raise ValueError(f"unsupported Prio3 parameters (rc={rc})")
        return s


def Prio3Count() -> Prio3:
    return Prio3(PRIO3_COUNT)


def Prio3Sum(bits: int) -> Prio3:
    return Prio3(PRIO3_SUM, bits=bits)


def Prio3SumVec(bits: int, length: int, chunk_length: int) -> Prio3:
    return Prio3(PRIO3_SUMVEC, bits=bits, length=length, chunk_length=chunk_length)


def Prio3SumVecField64MultiproofHmacSha256Aes128(proofs: int, bits: int, length: int,
                                                 chunk_length: int) -> Prio3:
    """janus_core::vdaf::new_prio3_sum_vec_field64_multiproof_hmacsha256_aes128
    (core/src/vdaf.rs:173-195): 32-byte verify key and seeds, proofs >= 2."""
    if proofs < 2:
        raise ValueError("Must use at least two proofs with Field64")
    return Prio3(PRIO3_SUMVEC_F64_MP, bits, length, chunk_length, proofs)


def Prio3Histogram(length: int, chunk_length: int) -> Prio3:
    return Prio3(PRIO3_HISTOGRAM, length=length, chunk_length=chunk_length)


def Prio3FixedPointBoundedL2VecSum(length: int, bitsize: int = 16) -> Prio3:
    """Prio3::new_fixedpoint_boundedl2_vec_sum_multithreaded(2, length) with FixedI16<U15>
    (bitsize 16) or FixedI32<U31> (bitsize 32) (core/src/vdaf.rs:292-335).  Helper role; the
    circuit is the reconstruction in oracle/fpvec_py.py."""
    if bitsize not in (16, 32):
        raise ValueError("bitsize must be 16 or 32 (Prio3FixedPointBoundedL2VecSumBitSize)")
    return Prio3(PRIO3_FPVEC_BOUNDED_L2, bits=bitsize, length=length)


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream, device):
    """Device-resident calls default to torch's current stream on the engine's device, so they
    are ordered after the torch ops that produced their inputs (a handle of 0 is HIP's null
    stream, which the C-ABI takes as such)."""
    if stream:
        return C.c_void_p(stream)
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream or None)


def _seg_accept(n, segment_ids, accept_mask, n_segments):
    """The C ABI reads n segment ids and n accept bytes (janus_prio3.h): a shorter array would be
    a host over-read inside the library, so the length contract is checked here."""
    seg = None if segment_ids is None else np.ascontiguousarray(segment_ids, np.uint32)
    acc = None if accept_mask is None else np.ascontiguousarray(accept_mask, np.uint8)
    if seg is not None and seg.shape != (n,):
        raise ValueError(f"segment_ids must have shape ({n},), got {seg.shape}")
    if acc is not None and acc.shape != (n,):
        raise ValueError(f"accept_mask must have shape ({n},), got {acc.shape}")
    if n_segments < 1:
        raise ValueError("n_segments must be >= 1")
    return seg, acc


class Ticket:
    """One submitted job (prio3_ticket*): ``poll()`` tells whether it is done without blocking,
    ``wait()`` blocks until it is, and returns exactly what the blocking method returns.  The
    ticket keeps every buffer the library was given alive until it has been waited: ``inputs``
    (read by the library inside submit only) and ``outputs`` (written inside ``wait`` only, on the
    waiting thread).  A ticket that is dropped without a wait is waited by ``__del__``: a done
    ticket keeps its group's pinned staging (96 MB) until then."""

    def __init__(self, name: str, handle: C.c_void_p, inputs: list, outputs: list, result):
        self.name, self.handle = name, handle
        self.inputs, self.outputs, self._result = inputs, outputs, result

    def poll(self) -> bool:
        if not self.handle:
            return True
        return bool(load_library().prio3_ticket_poll(self.handle))

    def wait(self):
        if not self.handle:
            raise RuntimeError(f"{self.name}: the ticket has been waited already")
        h, self.handle = self.handle, None
        rc = load_library().prio3_ticket_wait(h)
        result, self._result = self._result, None
        self.inputs = []
        if rc:
            raise RuntimeError(f"{self.name} failed (rc={rc})")
        return result()

    def __del__(self):
        try:
            if self.handle:
                h, self.handle = self.handle, None
                load_library().prio3_ticket_wait(h)
        except Exception:
            pass


def _job_call(name: str, args: tuple, inputs: list, outputs: list, result, ticket: bool,
              notify_fd):
    """The blocking call `name`, or (ticket) its ``_submit`` twin: `args` are the blocking form's,
    `result` makes the method's return value from the output buffers once they are written."""
    L = load_library()
    if not ticket:
        rc = getattr(L, name)(*args)
        if rc:
            raise RuntimeError(f"{name} failed (rc={rc})")
        return result()
    h = C.c_void_p()
    rc = getattr(L, name + "_submit")(*args, -1 if notify_fd is None else int(notify_fd),
                                      C.byref(h))
    if rc:
        raise RuntimeError(f"{name}_submit failed (rc={rc})")
    return Ticket(name, h, [x for x in inputs if x is not None], outputs, result)


class PreparedBatch:
    """Device-resident output shares of one ``prepare_batch`` call (prio3_batch*)."""

    def __init__(self, engine: "HelperEngine", handle: C.c_void_p, n: int):
        self.engine, self.handle, self.n = engine, handle, n

    def accumulate(self, segment_ids=None, accept_mask=None, n_segments: int = 1):
        sz = self.engine.sz
        agg = np.zeros((n_segments, sz.agg_share_len), np.uint8)
        cnt = np.zeros(n_segments, np.uint64)
        seg, acc = _seg_accept(self.n, segment_ids, accept_mask, n_segments)
        rc = load_library().prio3_accumulate(self.handle, _np_ptr(seg), _np_ptr(acc), n_segments,
                                             _np_ptr(agg), _np_ptr(cnt))
        if rc:
            raise RuntimeError(f"prio3_accumulate failed (rc={rc})")
        return agg, cnt

    def leader_prepare_next(self, prep_msgs, status) -> np.ndarray:
        """Leader ``prepare_next`` on the helper's prepare messages (leader_continued,
        aggregation_job_driver.rs:677-691); returns the updated per-report status."""
        st = np.array(status, np.uint8, copy=True)
        msgs = None
        if self.engine.sz.prep_msg_len:
            msgs = np.ascontiguousarray(prep_msgs, np.uint8)
            if msgs.shape != (self.n, self.engine.sz.prep_msg_len):
                raise ValueError("prepare message shape does not match the VDAF instance")
        rc = load_library().prio3_leader_prepare_next_batch(self.handle, _np_ptr(msgs),
                                                            _np_ptr(st))
        if rc:
            raise RuntimeError(f"prio3_leader_prepare_next_batch failed (rc={rc})")
        return st

    def leader_prepare_next_aggregate(self, prep_msgs, status, segment_ids=None,
                                      accept_mask=None, n_segments: int = 1):
        """``leader_prepare_next`` + ``accumulate`` in one launch of the prepare_next executor
        (prio3_leader_prepare_next_aggregate_batch).  Returns (status, agg [S, agg_len],
        counts [S])."""
        st = np.array(status, np.uint8, copy=True)
        msgs = None
        if self.engine.sz.prep_msg_len:
            msgs = np.ascontiguousarray(prep_msgs, np.uint8)
            if msgs.shape != (self.n, self.engine.sz.prep_msg_len):
                raise ValueError("prepare message shape does not match the VDAF instance")
        seg, acc = _seg_accept(self.n, segment_ids, accept_mask, n_segments)
        agg = np.zeros((n_segments, self.engine.sz.agg_share_len), np.uint8)
        cnt = np.zeros(n_segments, np.uint64)
        rc = load_library().prio3_leader_prepare_next_aggregate_batch(
            self.handle, _np_ptr(msgs), _np_ptr(st), _np_ptr(seg), _np_ptr(acc), n_segments,
            _np_ptr(agg), _np_ptr(cnt))
        if rc:
            raise RuntimeError(f"prio3_leader_prepare_next_aggregate_batch failed (rc={rc})")
        return st, agg, cnt

    def submit_leader_finish_job(self, report_ids, times, leader_status, prep_msgs,
                                 time_precision: int, max_segments: int, prepare_error=None,
                                 closed_intervals=None, accept_mask=None,
                                 notify_fd=None) -> Ticket:
        """``leader_finish_job`` as a ticket (prio3_leader_finish_job_submit): the inputs are
        consumed when this returns, ``wait()`` returns the blocking method's dict.  The batch must
        outlive the ticket."""
        return self.leader_finish_job(report_ids, times, leader_status, prep_msgs, time_precision,
                                      max_segments, prepare_error, closed_intervals, accept_mask,
                                      _ticket=True, _notify_fd=notify_fd)

    def leader_finish_job(self, report_ids, times, leader_status, prep_msgs,
                          time_precision: int, max_segments: int, prepare_error=None,
                          closed_intervals=None, accept_mask=None, _ticket=False,
                          _notify_fd=None) -> dict:
        """The rest of a leader aggregation job in one call (prio3_leader_finish_job), once the
        helper's response is decoded: the helper's ``prepare_error`` laid over the init
        ``leader_status``, the job index (``job_index``), ``leader_prepare_next_aggregate`` over
        the index's segment ids and its accept bytes ANDed with ``accept_mask``, the batch
        metadata (``batch_metadata``) and the per-report outcome (``dap.leader_outcome``, then
        BatchCollected for a report of a closed batch that had not failed), byte for byte what
        those calls give.  Returns a dict: segment_ids [n], segment_starts [S], reject [n],
        duplicate [n], the fields of Prio3JobIndexInfo, status [n], outcome [n], agg [S, agg_len],
        counts [S], checksums [S, 32] and intervals [S, 2], with S = max_segments."""
        sz, n = self.engine.sz, self.n
        ids = np.ascontiguousarray(report_ids, np.uint8).reshape(-1, 16)
        t = np.ascontiguousarray(times, np.uint64)
        ls = np.ascontiguousarray(leader_status, np.uint8)
        if ids.shape[0] != n or t.shape != (n,) or ls.shape != (n,):
            raise ValueError("input shapes do not match the batch")
        msgs = None
        if sz.prep_msg_len:
            msgs = np.ascontiguousarray(prep_msgs, np.uint8)
            if msgs.shape != (n, sz.prep_msg_len):
                raise ValueError("prepare message shape does not match the VDAF instance")
        pe = m = None
        if prepare_error is not None:
            pe = np.ascontiguousarray(prepare_error, np.uint8)
            if pe.shape != (n,):
                raise ValueError("prepare_error must have one byte per report")
        if accept_mask is not None:
            m = np.ascontiguousarray(accept_mask, np.uint8)
            if m.shape != (n,):
                raise ValueError("accept_mask must have one byte per report")
        cz, k = self.engine._closed(closed_intervals)
        S = max(0, min(int(max_segments), 4096))
        seg = np.zeros(n, np.uint32)
        starts = np.zeros(S, np.uint64)
        rej = np.zeros(n, np.uint8)
        dup = np.zeros(n, np.uint8)
        info = Prio3JobIndexInfo()
        status = np.zeros(n, np.uint8)
        outcome = np.zeros(n, np.uint8)
        agg = np.zeros((S, sz.agg_share_len), np.uint8)
        cnt = np.zeros(S, np.uint64)
        ck = np.zeros((S, 32), np.uint8)
        iv = np.zeros((S, 2), np.uint64)
        a = lambda x: None if x is None else x.ctypes.data
        jin = Prio3LeaderJobIn(
            report_ids=a(ids), times=a(t), leader_status=a(ls), prepare_error=a(pe),
            prep_msgs=a(msgs), time_precision=int(time_precision), closed_intervals=a(cz),
            accept_mask=a(m), k=k, max_segments=int(max_segments))
        jout = Prio3LeaderJobOut(
            segment_ids=a(seg), segment_starts=a(starts), reject=a(rej), duplicate=a(dup),
            info=C.addressof(info), status=a(status), outcome=a(outcome), agg_shares=a(agg),
            counts=a(cnt), checksums=a(ck), intervals=a(iv))

        def result():
            out = dict(segment_ids=seg, segment_starts=starts, reject=rej, duplicate=dup,
                       status=status, outcome=outcome, agg=agg, counts=cnt, checksums=ck,
                       intervals=iv)
            out.update({f: int(getattr(info, f)) for f, _ in Prio3JobIndexInfo._fields_})
            return out

        return _job_call("prio3_leader_finish_job", (self.handle, C.byref(jin), C.byref(jout)),
                         [self, ids, t, ls, pe, msgs, cz, m],
                         [seg, starts, rej, dup, status, outcome, agg, cnt, ck, iv, info], result,
                         _ticket, _notify_fd)

    def output_shares(self) -> np.ndarray:
        out = np.zeros((self.n, self.engine.sz.agg_share_len), np.uint8)
        rc = load_library().prio3_debug_output_shares(self.handle, _np_ptr(out))
        if rc:
            raise RuntimeError(f"prio3_debug_output_shares failed (rc={rc})")
        return out

    def free(self):
        if self.handle:
            load_library().prio3_batch_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HelperEngine:
    """One engine per (Prio3 instance, verify key) -- created where Janus builds ``VdafOps`` for
    a task (aggregator.rs:880-988) -- on one GPU (``device``), on the GPUs of ``device_mask``
    (bit d = GPU d; jobs placed whole on the least-loaded GPU, prio3_engine_create_mask), or on
    an explicit ``devices`` list (a GPU listed k times gets k executors: the one-GPU rehearsal
    of that placement)."""

    def __init__(self, vdaf: Prio3, verify_key: bytes, device: int = 0,
                 allow_unpinned: bool = False, device_mask: Optional[int] = None,
                 devices: Optional[list] = None):
        """allow_unpinned: required for Prio3FixedPointBoundedL2VecSum, whose circuit is a
        reconstruction with parity against prio unpinned (engine option experimental_fpvec)."""
        vk_len = 32 if vdaf.kind == PRIO3_SUMVEC_F64_MP else 16
        if len(verify_key) != vk_len:
            raise ValueError(f"verify key must be {vk_len} bytes (VERIFY_KEY_LENGTH[_HMACSHA256_"
                             "AES128], core/src/vdaf.rs)")
        L = load_library()
        self.sz = vdaf.sizes()
        h = C.c_void_p()
        vk = (C.c_uint8 * vk_len).from_buffer_copy(verify_key)
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            device = devices[0]
            rc = L.prio3_engine_create_devices(C.byref(vdaf.params()), vk, vk_len, arr,
                                               len(devices), C.byref(h))
        elif device_mask is not None:
            device = (device_mask & -device_mask).bit_length() - 1
            rc = L.prio3_engine_create_mask(C.byref(vdaf.params()), vk, vk_len, device_mask,
                                            C.byref(h))
        else:
            rc = L.prio3_engine_create_ex(C.byref(vdaf.params()), vk, vk_len, device, C.byref(h))
        self.vdaf, self.device = vdaf, device
        if rc:
            raise RuntimeError(f"prio3_engine_create failed (rc={rc}); a GPU is required")
        self.handle = h
        if vdaf.kind == PRIO3_FPVEC_BOUNDED_L2 and allow_unpinned:
            self.set_option("experimental_fpvec", 1)

    def close(self):
        if getattr(self, "handle", None):
            load_library().prio3_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key: str, value: int):
        rc = load_library().prio3_engine_set_option(self.handle, key.encode(), int(value))
        if rc:
            raise ValueError(f"unknown option {key}")

    def members(self) -> list:
        """Per-GPU placement of this engine's host-buffer jobs (prio3_engine_members): one dict
        per member with device, lane, jobs, reports, and its executor's exec_jobs / exec_groups."""
        L = load_library()
        k = L.prio3_engine_members(self.handle, None, 0)
        if k < 0:
            raise RuntimeError(f"prio3_engine_members failed (rc={k})")
        arr = (Prio3MemberInfo * k)()
        L.prio3_engine_members(self.handle, arr, k)
        return [{f: getattr(m, f) for f, _ in Prio3MemberInfo._fields_} for m in arr]

    def executor_stats(self, kind: int = EXEC_PREPARE, member: int = 0) -> dict:
        """Counters of the executor of `kind` that member `member`'s jobs use."""
        st = Prio3ExecutorStats()
        rc = load_library().prio3_executor_stats_get(self.handle, member, kind, C.byref(st))
        if rc:
            raise RuntimeError(f"prio3_executor_stats_get failed (rc={rc})")
        return {f: getattr(st, f) for f, _ in Prio3ExecutorStats._fields_}

    def executor_control(self, key: str, value: int, kind: int = -1):
        """prio3_executor_control on the executors of `kind` (-1: all): "hold" (tests queue jobs
        behind it), "heavy" (load switch)."""
        rc = load_library().prio3_executor_control(self.handle, kind, key.encode(), int(value))
        if rc:
            raise ValueError(f"executor control {key} failed (rc={rc})")

    # ---- host-buffer path -----------------------------------------------------------
    def prepare_batch(self, nonces, public_shares, helper_shares, leader_prep_shares):
        """Batched helper prepare_init -> prepare_shares_to_prepare_message -> prepare_next.

        Arrays are uint8 [n, len].  Returns (prep_msgs [n, prep_msg_len], status [n], batch).
        """
        sz = self.sz
        nonces = np.ascontiguousarray(nonces, np.uint8)
        n = nonces.shape[0]
        helper_shares = np.ascontiguousarray(helper_shares, np.uint8)
        leader_prep_shares = np.ascontiguousarray(leader_prep_shares, np.uint8)
        if helper_shares.shape != (n, sz.helper_share_len) or \
                leader_prep_shares.shape != (n, sz.prep_share_len):
            raise ValueError("input share shapes do not match the VDAF instance")
        pub = None
        if sz.public_share_len:
            pub = np.ascontiguousarray(public_shares, np.uint8)
            if pub.shape != (n, sz.public_share_len):
                raise ValueError("public share shape does not match the VDAF instance")
        msgs = np.zeros((n, max(sz.prep_msg_len, 1)), np.uint8)
        status = np.zeros(n, np.uint8)
        bh = C.c_void_p()
        rc = load_library().prio3_helper_prepare_batch(
            self.handle, n, _np_ptr(nonces), _np_ptr(pub), _np_ptr(helper_shares),
            _np_ptr(leader_prep_shares), _np_ptr(msgs), _np_ptr(status), C.byref(bh))
        if rc:
            raise RuntimeError(f"prio3_helper_prepare_batch failed (rc={rc})")
        return msgs[:, :sz.prep_msg_len], status, PreparedBatch(self, bh, n)

    def submit_prepare_aggregate_batch(self, nonces, public_shares, helper_shares,
                                       leader_prep_shares, segment_ids=None, accept_mask=None,
                                       n_segments: int = 1, notify_fd=None) -> Ticket:
        """``prepare_aggregate_batch`` as a ticket (prio3_helper_prepare_aggregate_batch_submit)."""
        return self.prepare_aggregate_batch(nonces, public_shares, helper_shares,
                                            leader_prep_shares, segment_ids, accept_mask,
                                            n_segments, _ticket=True, _notify_fd=notify_fd)

    def prepare_aggregate_batch(self, nonces, public_shares, helper_shares, leader_prep_shares,
                                segment_ids=None, accept_mask=None, n_segments: int = 1,
                                _ticket=False, _notify_fd=None):
        """prepare_batch + accumulate of the same reports in one coalesced launch
        (prio3_helper_prepare_aggregate_batch).  Returns (prep_msgs, status, agg [S, agg_len],
        counts [S])."""
        sz = self.sz
        nonces = np.ascontiguousarray(nonces, np.uint8)
        n = nonces.shape[0]
        helper_shares = np.ascontiguousarray(helper_shares, np.uint8)
        leader_prep_shares = np.ascontiguousarray(leader_prep_shares, np.uint8)
        if helper_shares.shape != (n, sz.helper_share_len) or \
                leader_prep_shares.shape != (n, sz.prep_share_len):
            raise ValueError("input share shapes do not match the VDAF instance")
        pub = None
        if sz.public_share_len:
            pub = np.ascontiguousarray(public_shares, np.uint8)
            if pub.shape != (n, sz.public_share_len):
                raise ValueError("public share shape does not match the VDAF instance")
        seg, acc = _seg_accept(n, segment_ids, accept_mask, n_segments)
        msgs = np.zeros((n, max(sz.prep_msg_len, 1)), np.uint8)
        status = np.zeros(n, np.uint8)
        agg = np.zeros((n_segments, sz.agg_share_len), np.uint8)
        cnt = np.zeros(n_segments, np.uint64)
        return _job_call(
            "prio3_helper_prepare_aggregate_batch",
            (self.handle, n, _np_ptr(nonces), _np_ptr(pub), _np_ptr(helper_shares),
             _np_ptr(leader_prep_shares), _np_ptr(seg), _np_ptr(acc), n_segments, _np_ptr(msgs),
             _np_ptr(status), _np_ptr(agg), _np_ptr(cnt)),
            [self, nonces, pub, helper_shares, leader_prep_shares, seg, acc],
            [msgs, status, agg, cnt], lambda: (msgs[:, :sz.prep_msg_len], status, agg, cnt),
            _ticket, _notify_fd)

    def submit_aggregate_init_batch(self, opener, task_id: bytes, report_ids, times,
                                    public_shares, enc, ct, ct_len, leader_prep_shares,
                                    segment_ids=None, accept_mask=None, n_segments: int = 1,
                                    require_taskprov=False, fallback_opener=None,
                                    report_deadline=None, notify_fd=None) -> Ticket:
        """``aggregate_init_batch`` as a ticket: always the _ex entry point
        (prio3_helper_aggregate_init_batch_ex_submit; without a fallback keypair and a deadline it
        is the plain call for every instance the plain call admits)."""
        return self.aggregate_init_batch(opener, task_id, report_ids, times, public_shares, enc,
                                         ct, ct_len, leader_prep_shares, segment_ids, accept_mask,
                                         n_segments, require_taskprov, fallback_opener,
                                         report_deadline, _ticket=True, _notify_fd=notify_fd)

    def aggregate_init_batch(self, opener, task_id: bytes, report_ids, times, public_shares,
                             enc, ct, ct_len, leader_prep_shares, segment_ids=None,
                             accept_mask=None, n_segments: int = 1, require_taskprov=False,
                             fallback_opener=None, report_deadline=None, _ticket=False,
                             _notify_fd=None):
        """The helper's whole loop body for one job from the sealed input shares
        (prio3_helper_aggregate_init_batch; aggregator.rs:1794-2096): HPKE open with ``opener``
        (janus_amd.hpke.HpkeOpener), decode, prepare and accumulate in one coalesced launch.
        enc [n, Nenc], ct [n, ct_stride] (stride a multiple of 16), ct_len [n].  Returns
        (prep_msgs, status [merged: STATUS_* or STATUS_HPKE_DECRYPT / STATUS_INVALID_MESSAGE /
        STATUS_REPORT_TOO_EARLY], agg [S, agg_len], counts [S]).

        With ``fallback_opener`` (the global keypair of the same config id and KEM) and / or
        ``report_deadline`` (seconds; a report with a later time gets STATUS_REPORT_TOO_EARLY) the
        call is prio3_helper_aggregate_init_batch_ex: the reports ``opener`` cannot decrypt are
        opened again with the fallback inside the same launch.  With both left at None it is the
        plain entry point."""
        sz = self.sz
        ids = np.ascontiguousarray(report_ids, np.uint8)
        n = ids.shape[0]
        t = np.ascontiguousarray(times, np.uint64)
        e = np.ascontiguousarray(enc, np.uint8)
        c = np.ascontiguousarray(ct, np.uint8)
        cl = np.ascontiguousarray(ct_len, np.uint32)
        lps = np.ascontiguousarray(leader_prep_shares, np.uint8)
        if ids.shape != (n, 16) or t.shape != (n,) or cl.shape != (n,) or c.ndim != 2 or \
                c.shape[0] != n or e.shape[0] != n or lps.shape != (n, sz.prep_share_len):
            raise ValueError("input shapes do not match the job")
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        pub = None
        if sz.public_share_len:
            pub = np.ascontiguousarray(public_shares, np.uint8)
            if pub.shape != (n, sz.public_share_len):
                raise ValueError("public share shape does not match the VDAF instance")
        seg, acc = _seg_accept(n, segment_ids, accept_mask, n_segments)
        msgs = np.zeros((n, max(sz.prep_msg_len, 1)), np.uint8)
        status = np.zeros(n, np.uint8)
        agg = np.zeros((n_segments, sz.agg_share_len), np.uint8)
        cnt = np.zeros(n_segments, np.uint64)
        tid = (C.c_uint8 * 32).from_buffer_copy(task_id)
        if _ticket or fallback_opener is not None or report_deadline is not None:
            deadline = (1 << 64) - 1 if report_deadline is None else int(report_deadline)
            return _job_call(
                "prio3_helper_aggregate_init_batch_ex",
                (self.handle, None if opener is None else opener.handle,
                 None if fallback_opener is None else fallback_opener.handle, deadline, n, tid,
                 int(bool(require_taskprov)), _np_ptr(ids), _np_ptr(t), _np_ptr(pub), _np_ptr(e),
                 _np_ptr(c), _np_ptr(cl), c.shape[1], _np_ptr(lps), _np_ptr(seg), _np_ptr(acc),
                 n_segments, _np_ptr(msgs), _np_ptr(status), _np_ptr(agg), _np_ptr(cnt)),
                [self, opener, fallback_opener, tid, ids, t, pub, e, c, cl, lps, seg, acc],
                [msgs, status, agg, cnt], lambda: (msgs[:, :sz.prep_msg_len], status, agg, cnt),
                _ticket, _notify_fd)
        rc = load_library().prio3_helper_aggregate_init_batch(
            self.handle, opener.handle, n, tid, int(bool(require_taskprov)), _np_ptr(ids),
            _np_ptr(t), _np_ptr(pub), _np_ptr(e), _np_ptr(c), _np_ptr(cl), c.shape[1],
            _np_ptr(lps), _np_ptr(seg), _np_ptr(acc), n_segments, _np_ptr(msgs), _np_ptr(status),
            _np_ptr(agg), _np_ptr(cnt))
        if rc:
            raise RuntimeError(f"prio3_helper_aggregate_init_batch failed (rc={rc})")
        return msgs[:, :sz.prep_msg_len], status, agg, cnt

    def submit_aggregate_job(self, opener, task_id: bytes, report_ids, times, public_shares, enc,
                             ct, ct_len, leader_prep_shares, time_precision: int,
                             max_segments: int, closed_intervals=None, accept_mask=None,
                             require_taskprov=False, fallback_opener=None, report_deadline=None,
                             notify_fd=None) -> Ticket:
        """``aggregate_job`` as a ticket (prio3_helper_aggregate_job_submit): the inputs are
        consumed when this returns, ``wait()`` returns the blocking method's dict."""
        return self.aggregate_job(opener, task_id, report_ids, times, public_shares, enc, ct,
                                  ct_len, leader_prep_shares, time_precision, max_segments,
                                  closed_intervals, accept_mask, require_taskprov, fallback_opener,
                                  report_deadline, _ticket=True, _notify_fd=notify_fd)

    def aggregate_job(self, opener, task_id: bytes, report_ids, times, public_shares, enc, ct,
                      ct_len, leader_prep_shares, time_precision: int, max_segments: int,
                      closed_intervals=None, accept_mask=None, require_taskprov=False,
                      fallback_opener=None, report_deadline=None, _ticket=False,
                      _notify_fd=None) -> dict:
        """A whole helper aggregation job in one call (prio3_helper_aggregate_job): the job index
        (``job_index``), the loop body (``aggregate_init_batch`` with fallback keypair and report
        deadline) over the index's segment ids and its accept bytes ANDed with ``accept_mask``, and
        the batch metadata (``batch_metadata``), byte for byte what the three calls give.  Returns
        a dict: segment_ids [n], segment_starts [S], reject [n], duplicate [n], the fields of
        Prio3JobIndexInfo, prep_msgs, status [n], agg [S, agg_len], counts [S], checksums [S, 32]
        and intervals [S, 2], with S = max_segments."""
        sz = self.sz
        ids = np.ascontiguousarray(report_ids, np.uint8).reshape(-1, 16)
        n = ids.shape[0]
        t = np.ascontiguousarray(times, np.uint64)
        e = np.ascontiguousarray(enc, np.uint8)
        c = np.ascontiguousarray(ct, np.uint8)
        cl = np.ascontiguousarray(ct_len, np.uint32)
        lps = np.ascontiguousarray(leader_prep_shares, np.uint8)
        if t.shape != (n,) or cl.shape != (n,) or c.ndim != 2 or c.shape[0] != n or \
                e.shape[0] != n or lps.shape != (n, sz.prep_share_len):
            raise ValueError("input shapes do not match the job")
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        pub = None
        if sz.public_share_len:
            pub = np.ascontiguousarray(public_shares, np.uint8)
            if pub.shape != (n, sz.public_share_len):
                raise ValueError("public share shape does not match the VDAF instance")
        m = None
        if accept_mask is not None:
            m = np.ascontiguousarray(accept_mask, np.uint8)
            if m.shape != (n,):
                raise ValueError("accept_mask must have one byte per report")
        cz, k = self._closed(closed_intervals)
        S = max(0, min(int(max_segments), 4096))
        tid = (C.c_uint8 * 32).from_buffer_copy(task_id)
        seg = np.zeros(n, np.uint32)
        starts = np.zeros(S, np.uint64)
        rej = np.zeros(n, np.uint8)
        dup = np.zeros(n, np.uint8)
        info = Prio3JobIndexInfo()
        msgs = np.zeros((n, max(sz.prep_msg_len, 1)), np.uint8)
        status = np.zeros(n, np.uint8)
        agg = np.zeros((S, sz.agg_share_len), np.uint8)
        cnt = np.zeros(S, np.uint64)
        ck = np.zeros((S, 32), np.uint8)
        iv = np.zeros((S, 2), np.uint64)
        a = lambda x: None if x is None else x.ctypes.data
        jin = Prio3HelperJobIn(
            opener=None if opener is None else opener.handle.value,
            fallback_opener=None if fallback_opener is None else fallback_opener.handle.value,
            report_deadline=(1 << 64) - 1 if report_deadline is None else int(report_deadline),
            n=n, require_taskprov=int(bool(require_taskprov)), task_id=C.addressof(tid),
            report_ids=a(ids), times=a(t), public_shares=a(pub), enc=a(e), ct=a(c), ct_len=a(cl),
            leader_prep_shares=a(lps), ct_stride=c.shape[1], k=k,
            time_precision=int(time_precision), closed_intervals=a(cz), accept_mask=a(m),
            max_segments=int(max_segments), reserved=0)
        jout = Prio3HelperJobOut(
            segment_ids=a(seg), segment_starts=a(starts), reject=a(rej), duplicate=a(dup),
            info=C.addressof(info), prep_msgs=a(msgs), status=a(status), agg_shares=a(agg),
            counts=a(cnt), checksums=a(ck), intervals=a(iv))

        def result():
            out = dict(segment_ids=seg, segment_starts=starts, reject=rej, duplicate=dup,
                       prep_msgs=msgs[:, :sz.prep_msg_len], status=status, agg=agg, counts=cnt,
                       checksums=ck, intervals=iv)
            out.update({f: int(getattr(info, f)) for f, _ in Prio3JobIndexInfo._fields_})
            return out

        return _job_call("prio3_helper_aggregate_job", (self.handle, C.byref(jin), C.byref(jout)),
                         [self, opener, fallback_opener, tid, ids, t, pub, e, c, cl, lps, cz, m],
                         [seg, starts, rej, dup, msgs, status, agg, cnt, ck, iv, info], result,
                         _ticket, _notify_fd)

    # ---- leader side (same instance, agg_id 0) -----------------------------------
    def submit_leader_prepare_init_batch(self, nonces, public_shares, leader_input_shares,
                                         notify_fd=None) -> Ticket:
        """``leader_prepare_init_batch`` as a ticket (prio3_leader_prepare_init_batch_submit);
        the batch handle is made by ``wait()``."""
        return self.leader_prepare_init_batch(nonces, public_shares, leader_input_shares,
                                              _ticket=True, _notify_fd=notify_fd)

    def leader_prepare_init_batch(self, nonces, public_shares, leader_input_shares,
                                  _ticket=False, _notify_fd=None):
        """Batched leader prepare_init (leader_initialized, aggregation_job_driver.rs:397-415).

        Returns (prep_shares [n, prep_share_len], status [n], batch); the batch's
        ``leader_prepare_next`` then takes the helper's prepare messages."""
        sz = self.sz
        nonces = np.ascontiguousarray(nonces, np.uint8)
        n = nonces.shape[0]
        ls = np.ascontiguousarray(leader_input_shares, np.uint8)
        if ls.shape != (n, sz.leader_input_share_len):
            raise ValueError("leader input share shape does not match the VDAF instance")
        pub = None
        if sz.public_share_len:
            pub = np.ascontiguousarray(public_shares, np.uint8)
            if pub.shape != (n, sz.public_share_len):
                raise ValueError("public share shape does not match the VDAF instance")
        ps = np.zeros((n, sz.prep_share_len), np.uint8)
        status = np.zeros(n, np.uint8)
        bh = C.c_void_p()
        return _job_call(
            "prio3_leader_prepare_init_batch",
            (self.handle, n, _np_ptr(nonces), _np_ptr(pub), _np_ptr(ls), _np_ptr(ps),
             _np_ptr(status), C.byref(bh)),
            [self, nonces, pub, ls], [ps, status, bh],
            lambda: (ps, status, PreparedBatch(self, bh, n)), _ticket, _notify_fd)

    def leader_prepare_init_device(self, nonces, public_shares, leader_input_shares, prep_shares,
                                   status, stream=None) -> None:
        rc = load_library().prio3_device_leader_prepare_init(
            self.handle, nonces.shape[0], _tptr(nonces), _tptr(public_shares),
            _tptr(leader_input_shares), _tptr(prep_shares), _tptr(status),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_leader_prepare_init failed (rc={rc})")

    def leader_prepare_next_device(self, n, prep_msgs, status, stream=None) -> None:
        rc = load_library().prio3_device_leader_prepare_next(
            self.handle, n, _tptr(prep_msgs), _tptr(status), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_leader_prepare_next failed (rc={rc})")

    # ---- device-resident path (torch tensors on this engine's GPU) ------------------
    def prepare_device(self, nonces, public_shares, helper_shares, leader_prep_shares,
                       prep_msgs, status, stream=None) -> None:
        rc = load_library().prio3_device_prepare(
            self.handle, nonces.shape[0], _tptr(nonces), _tptr(public_shares),
            _tptr(helper_shares), _tptr(leader_prep_shares), _tptr(prep_msgs), _tptr(status),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_prepare failed (rc={rc})")

    def prepare_aggregate_device(self, nonces, public_shares, helper_shares, leader_prep_shares,
                                 segment_ids, n_segments, prep_msgs, status, stream=None) -> None:
        """Prepare and aggregate in one pass (torch tensors on this engine's GPU)."""
        rc = load_library().prio3_device_prepare_aggregate(
            self.handle, nonces.shape[0], _tptr(nonces), _tptr(public_shares),
            _tptr(helper_shares), _tptr(leader_prep_shares), _tptr(segment_ids), n_segments,
            _tptr(prep_msgs), _tptr(status), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_prepare_aggregate failed (rc={rc})")

    def aggregate_finish_device(self, status, accept_mask, agg, counts, stream=None) -> None:
        rc = load_library().prio3_device_aggregate_finish(
            self.handle, _tptr(status), _tptr(accept_mask), _tptr(agg), _tptr(counts),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_aggregate_finish failed (rc={rc})")

    def accumulate_device(self, n, status, segment_ids, accept_mask, n_segments, agg, counts,
                          stream=None) -> None:
        rc = load_library().prio3_device_accumulate(
            self.handle, n, _tptr(status), _tptr(segment_ids), _tptr(accept_mask), n_segments,
            _tptr(agg), _tptr(counts), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_accumulate failed (rc={rc})")

    def combine_device(self, k, n_segments, parts, part_counts, out, out_counts,
                       stream=None) -> None:
        rc = load_library().prio3_device_combine(
            self.handle, k, n_segments, _tptr(parts), _tptr(part_counts), _tptr(out),
            _tptr(out_counts), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_combine failed (rc={rc})")

    def batch_metadata_device(self, report_ids, times, status, accept_mask, segment_ids,
                              n_segments, checksums, intervals, stream=None) -> None:
        """Per-segment ReportIdChecksum [n_segments, 32] (uint8) and client-timestamp interval
        [n_segments, 2] (int64 start, duration) of the batch (torch tensors on this GPU)."""
        rc = load_library().prio3_device_batch_metadata(
            self.handle, status.shape[0], _tptr(report_ids), _tptr(times), _tptr(status),
            _tptr(accept_mask), _tptr(segment_ids), n_segments, _tptr(checksums),
            _tptr(intervals), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_batch_metadata failed (rc={rc})")

    def combine_metadata_device(self, k, n_segments, checksums_in, intervals_in, checksums,
                                intervals, stream=None) -> None:
        rc = load_library().prio3_device_combine_metadata(
            self.handle, k, n_segments, _tptr(checksums_in), _tptr(intervals_in),
            _tptr(checksums), _tptr(intervals), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_combine_metadata failed (rc={rc})")

    def batch_metadata(self, report_ids, times, status, accept_mask=None, segment_ids=None,
                       n_segments: int = 1):
        """Host-buffer form: returns (checksums uint8 [S, 32], intervals uint64 [S, 2])."""
        ids = np.ascontiguousarray(report_ids, np.uint8)
        n = ids.shape[0]
        st = np.ascontiguousarray(status, np.uint8)
        if ids.shape != (n, 16) or st.shape != (n,):
            raise ValueError("report_ids must be [n, 16] and status [n]")
        t = None if times is None else np.ascontiguousarray(times, np.uint64)
        m = None if accept_mask is None else np.ascontiguousarray(accept_mask, np.uint8)
        sg = None if segment_ids is None else np.ascontiguousarray(segment_ids, np.uint32)
        ck = np.zeros((n_segments, 32), np.uint8)
        iv = np.zeros((n_segments, 2), np.uint64)
        rc = load_library().prio3_batch_metadata(
            self.handle, n, _np_ptr(ids), _np_ptr(t), _np_ptr(st), _np_ptr(m), _np_ptr(sg),
            n_segments, _np_ptr(ck), _np_ptr(iv))
        if rc:
            raise RuntimeError(f"prio3_batch_metadata failed (rc={rc})")
        return ck, iv

    @staticmethod
    def _closed(closed_intervals):
        """[k, 2] uint64 (start, duration) host array of the closed batch intervals, or None."""
        if closed_intervals is None:
            return None, 0
        c = np.ascontiguousarray(closed_intervals, np.uint64).reshape(-1, 2)
        return (c, c.shape[0]) if c.shape[0] else (None, 0)

    def job_index_device(self, report_ids, times, time_precision: int, max_segments: int,
                         segment_ids, accept_mask, info, closed_intervals=None,
                         segment_starts=None, reject=None, duplicate=None, stream=None) -> None:
        """prio3_device_job_index on torch tensors of this engine's GPU: report_ids [n, 16] uint8
        and times [n] (64-bit; None for time_precision 0) in; segment_ids [n] (32-bit), accept_mask
        [n] uint8, info [6] (32-bit: the fields of Prio3JobIndexInfo in order) and the optional
        segment_starts [max_segments] (64-bit), reject [n] and duplicate [n] uint8 out.
        closed_intervals is a host array [k, 2] of (start, duration).  Stream-ordered; nothing is
        waited for."""
        c, k = self._closed(closed_intervals)
        rc = load_library().prio3_device_job_index(
            self.handle, report_ids.shape[0], _tptr(report_ids), _tptr(times), time_precision,
            _np_ptr(c), k, max_segments, _tptr(segment_ids), _tptr(segment_starts),
            _tptr(accept_mask), _tptr(reject), _tptr(duplicate), _tptr(info),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_device_job_index failed (rc={rc})")

    def job_index(self, report_ids, times, time_precision: int, max_segments: int,
                  closed_intervals=None, with_starts: bool = True, with_reject: bool = True,
                  with_duplicate: bool = True) -> dict:
        """Host-buffer form (blocking): returns segment_ids, segment_starts, accept_mask, reject,
        duplicate (None for an output switched off; segment_starts also for time_precision 0) and
        the fields of Prio3JobIndexInfo."""
        ids = np.ascontiguousarray(report_ids, np.uint8).reshape(-1, 16)
        n = ids.shape[0]
        t = None if times is None else np.ascontiguousarray(times, np.uint64)
        if t is not None and t.shape != (n,):
            raise ValueError(f"times must have shape ({n},), got {t.shape}")
        c, k = self._closed(closed_intervals)
        seg = np.zeros(n, np.uint32)
        acc = np.zeros(n, np.uint8)
        cap = max(0, min(int(max_segments), 4096))
        starts = np.zeros(cap, np.uint64) if with_starts and time_precision else None
        rej = np.zeros(n, np.uint8) if with_reject else None
        dup = np.zeros(n, np.uint8) if with_duplicate else None
        info = Prio3JobIndexInfo()
        rc = load_library().prio3_job_index(
            self.handle, n, _np_ptr(ids), _np_ptr(t), time_precision, _np_ptr(c), k, max_segments,
            _np_ptr(seg), _np_ptr(starts), _np_ptr(acc), _np_ptr(rej), _np_ptr(dup),
            C.byref(info))
        if rc:
            raise RuntimeError(f"prio3_job_index failed (rc={rc})")
        out = dict(segment_ids=seg, segment_starts=starts, accept_mask=acc, reject=rej,
                   duplicate=dup)
        out.update({f: int(getattr(info, f)) for f, _ in Prio3JobIndexInfo._fields_})
        return out

    def device_output_shares(self, n: int) -> np.ndarray:
        out = np.zeros((n, self.sz.agg_share_len), np.uint8)
        rc = load_library().prio3_device_output_shares(self.handle, n, _np_ptr(out))
        if rc:
            raise RuntimeError("prio3_device_output_shares failed")
        return out

    # ---- synthetic client ------------------------------------------------------------
    def generate_reports_device(self, n: int, seed: int = 1, first_index: int = 0,
                                with_checks: bool = False, with_leader_inputs: bool = False,
                                stream=None) -> dict:
        """Honest synthetic reports generated on the GPU (shard + leader prepare_init).

        Returns torch uint8 tensors on this engine's device (plus measurements / leader
        output shares / flags when ``with_checks``).  Every TurboSHAKE instance, including
        FixedPointBoundedL2VecSum (its prover runs on the device too; the engine needs the
        allow_unpinned opt-in), and the HMAC-SHA256/AES-128 multiproof VDAF.  Report i is
        derived from (seed, first_index + i) exactly as oracle's generators derive it."""
        import torch
        sz = self.sz
        dev = torch.device("cuda", self.device)
        u8 = dict(dtype=torch.uint8, device=dev)
        out = dict(nonces=torch.empty((n, 16), **u8),
                   public_shares=torch.empty((n, max(sz.public_share_len, 1)), **u8),
                   helper_shares=torch.empty((n, sz.helper_share_len), **u8),
                   leader_prep_shares=torch.empty((n, sz.prep_share_len), **u8))
        if with_checks:
            # SumVec: the entries; FPVec: the signed fixed-point entries X (x = X / 2^(bits-1))
            mstride = (self.vdaf.length if self.vdaf.kind in (PRIO3_SUMVEC, PRIO3_FPVEC_BOUNDED_L2,
                                                              PRIO3_SUMVEC_F64_MP) else 1)
            out["measurements"] = torch.empty((n, mstride), dtype=torch.int64, device=dev)
            out["leader_out_shares"] = torch.empty((n, sz.agg_share_len), **u8)
            out["flags"] = torch.zeros(n, **u8)
        if with_leader_inputs:
            out["leader_input_shares"] = torch.empty((n, sz.leader_input_share_len), **u8)
        rc = load_library().prio3_client_generate_device(
            self.handle, n, seed, first_index, _tptr(out["nonces"]),
            _tptr(out["public_shares"]) if sz.public_share_len else None,
            _tptr(out["helper_shares"]), _tptr(out["leader_prep_shares"]),
            _tptr(out.get("measurements")), _tptr(out.get("leader_out_shares")),
            _tptr(out.get("flags")), _tptr(out.get("leader_input_shares")),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_client_generate_device failed (rc={rc})")
        if not sz.public_share_len:
            out["public_shares"] = out["public_shares"][:, :0]
        return out

    def generate_sealed_reports_device(self, sealer, task_id: bytes, n: int, times, sk_e,
                                       seed: int = 1, first_index: int = 0,
                                       with_taskprov_extension: bool = False, stream=None,
                                       with_checks: bool = False,
                                       with_leader_inputs: bool = False) -> dict:
        """``generate_reports_device`` followed, on the same stream, by
        ``sealer.seal_input_shares_device`` (janus_amd.hpke.HpkeSealer on this engine's GPU): what
        a helper actually receives.  The report IDs are the reports' nonces.  times [n] (8-byte
        integers) and sk_e [n, 32] (uint8, one ephemeral private key per report from the caller's
        CSPRNG) are torch tensors on the GPU.  Returns the client's dict plus enc [n, Nenc],
        ct [n, stride], ct_len [n] (int32) and seal_status [n]; with_checks / with_leader_inputs
        as for ``generate_reports_device`` (the measurements; the leader input shares a leader
        engine's ``leader_prepare_init_device`` reads)."""
        import torch
        from .hpke import NSK_E, sealed_stride
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        if sealer.device != self.device:
            raise ValueError("the sealer is bound to another GPU than the engine")
        if tuple(times.shape) != (n,) or tuple(sk_e.shape) != (n, NSK_E):
            raise ValueError(f"times must be [{n}] and sk_e [{n}, {NSK_E}]")
        if self.sz.public_share_len not in (0, 32, 64):
            raise ValueError("the sealer takes public shares of 0, 32 or 64 bytes")
        out = self.generate_reports_device(n, seed=seed, first_index=first_index, stream=stream,
                                           with_checks=with_checks,
                                           with_leader_inputs=with_leader_inputs)
        dev = torch.device("cuda", self.device)
        out["enc"] = torch.empty((n, sealer.nenc), dtype=torch.uint8, device=dev)
        out["ct"] = torch.empty((n, sealed_stride(self.sz.helper_share_len,
                                                  with_taskprov_extension)),
                                dtype=torch.uint8, device=dev)
        out["ct_len"] = torch.empty(n, dtype=torch.int32, device=dev)
        out["seal_status"] = torch.empty(n, dtype=torch.uint8, device=dev)
        sealer.seal_input_shares_device(
            task_id, sk_e, out["nonces"], times,
            out["public_shares"] if self.sz.public_share_len else None, out["helper_shares"],
            out["enc"], out["ct"], out["ct_len"], out["seal_status"],
            with_taskprov_extension=with_taskprov_extension, stream=stream)
        return out

    # ---- client role -------------------------------------------------------------------
    @property
    def rand_len(self) -> int:
        """Bytes of shard randomness per report (prio3_client_rand_len)."""
        return load_library().prio3_client_rand_len(C.byref(self.vdaf.params()))

    def _client_shapes(self, n, measurements, nonces, rand):
        if self.vdaf.kind not in (PRIO3_COUNT, PRIO3_SUM, PRIO3_SUMVEC, PRIO3_HISTOGRAM,
                                  PRIO3_SUMVEC_F64_MP):
            raise NotImplementedError(
                "the client role does not take FixedPointBoundedL2VecSum (it takes Count, Sum, "
                "SumVec, Histogram and SumVecField64MultiproofHmacSha256Aes128)")
        mstride = self.vdaf.length if self.vdaf.kind in (PRIO3_SUMVEC, PRIO3_SUMVEC_F64_MP) else 1
        if tuple(measurements.shape) not in ((n, mstride),) + (((n,),) if mstride == 1 else ()):
            raise ValueError(f"measurements must be [{n}, {mstride}]")
        if tuple(nonces.shape) != (n, 16):
            raise ValueError(f"nonces (the report IDs) must be [{n}, 16]")
        if tuple(rand.shape) != (n, self.rand_len):
            raise ValueError(f"rand must be [{n}, {self.rand_len}]")

    def shard_device(self, measurements, nonces, rand, stream=None) -> dict:
        """prio ``Prio3::shard`` of the caller's measurements on the GPU (prio3_client_shard_device).

        torch tensors on this engine's device: measurements [n, length] (SumVec) or [n] / [n, 1],
        8-byte integers; nonces [n, 16] uint8 (the report IDs); rand [n, rand_len] uint8 from the
        caller's CSPRNG (layout: janus_prio3.h).  Returns public_shares, leader_input_shares,
        helper_shares (uint8 rows) and status [n] (1 = invalid measurement, rows zero).
        Stream-ordered, no host synchronisation."""
        import torch
        n = nonces.shape[0] if len(nonces.shape) else -1
        self._client_shapes(n, measurements, nonces, rand)
        if measurements.element_size() != 8:
            raise ValueError("measurements must be 8-byte integers")
        for t in (measurements, nonces, rand):
            if not isinstance(t, torch.Tensor) or not t.is_contiguous() or \
                    t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("tensors must be contiguous and on the engine's GPU")
        sz = self.sz
        u8 = dict(dtype=torch.uint8, device=torch.device("cuda", self.device))
        out = dict(public_shares=torch.empty((n, sz.public_share_len), **u8),
                   leader_input_shares=torch.empty((n, sz.leader_input_share_len), **u8),
                   helper_shares=torch.empty((n, sz.helper_share_len), **u8),
                   status=torch.empty(n, **u8))
        rc = load_library().prio3_client_shard_device(
            self.handle, n, _tptr(measurements), _tptr(nonces), _tptr(rand),
            _tptr(out["public_shares"]) if sz.public_share_len else None,
            _tptr(out["leader_input_shares"]), _tptr(out["helper_shares"]), _tptr(out["status"]),
            _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_client_shard_device failed (rc={rc})")
        return out

    def shard_batch(self, measurements, nonces, rand) -> dict:
        """The numpy form of ``shard_device`` (prio3_client_shard_batch, blocking)."""
        m = np.ascontiguousarray(measurements, np.uint64)
        ids = np.ascontiguousarray(nonces, np.uint8)
        rnd = np.ascontiguousarray(rand, np.uint8)
        n = ids.shape[0] if ids.ndim else -1
        self._client_shapes(n, m, ids, rnd)
        sz = self.sz
        out = dict(public_shares=np.zeros((n, sz.public_share_len), np.uint8),
                   leader_input_shares=np.zeros((n, sz.leader_input_share_len), np.uint8),
                   helper_shares=np.zeros((n, sz.helper_share_len), np.uint8),
                   status=np.zeros(n, np.uint8))
        rc = load_library().prio3_client_shard_batch(
            self.handle, n, _np_ptr(m), _np_ptr(ids), _np_ptr(rnd),
            _np_ptr(out["public_shares"]) if sz.public_share_len else None,
            _np_ptr(out["leader_input_shares"]), _np_ptr(out["helper_shares"]),
            _np_ptr(out["status"]))
        if rc:
            raise RuntimeError(f"prio3_client_shard_batch failed (rc={rc})")
        return out

    def prepare_reports_device(self, leader_sealer, helper_sealer, task_id: bytes,
                               time_precision: int, measurements, report_ids, times, rand,
                               sk_e_leader, sk_e_helper, leader_config_id: int,
                               helper_config_id: int, with_taskprov_extension: bool = False,
                               report_stride=None, stream=None) -> dict:
        """``Client::prepare_report`` for a batch of one task in one call
        (prio3_client_prepare_reports_device): times rounded down to ``time_precision``, the shard,
        one input share sealed to each aggregator (janus_amd.hpke.HpkeSealer objects on this
        engine's GPU; sk_e_leader / sk_e_helper [n, 32] uint8, one fresh ephemeral key per report
        and aggregator) and the DAP ``Report`` encode.  torch tensors on the GPU; times are 8-byte
        integers.  Returns reports [n, stride] (uint8), report_len [n] (int32; 0 = left out) and
        status [n] (0, 1 = invalid measurement, 0x40 / 0x41 = the sealer's)."""
        import torch
        from .hpke import NSK_E
        n = report_ids.shape[0] if len(report_ids.shape) else -1
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        if int(time_precision) <= 0:
            raise ValueError("time_precision must be positive")
        if leader_sealer.device != self.device or helper_sealer.device != self.device:
            raise ValueError("a sealer is bound to another GPU than the engine")
        if not 0 <= leader_config_id <= 0xFF or not 0 <= helper_config_id <= 0xFF:
            raise ValueError("an HPKE config id is one byte")
        self._client_shapes(n, measurements, report_ids, rand)
        if tuple(times.shape) != (n,) or tuple(sk_e_leader.shape) != (n, NSK_E) or \
                tuple(sk_e_helper.shape) != (n, NSK_E):
            raise ValueError(f"times must be [{n}], sk_e_leader and sk_e_helper [{n}, {NSK_E}]")
        if times.element_size() != 8 or measurements.element_size() != 8:
            raise ValueError("times and measurements must be 8-byte integers")
        for t in (measurements, report_ids, times, rand, sk_e_leader, sk_e_helper):
            if not isinstance(t, torch.Tensor) or not t.is_contiguous() or \
                    t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("tensors must be contiguous and on the engine's GPU")
        L = load_library()
        need = L.prio3_client_report_stride(C.byref(self.vdaf.params()), leader_sealer.handle,
                                            helper_sealer.handle, int(bool(with_taskprov_extension)))
        stride = need if report_stride is None else int(report_stride)
        if need == 0 or stride < need:
            raise ValueError(f"report_stride must be >= {need}")
        dev = torch.device("cuda", self.device)
        out = dict(reports=torch.empty((n, stride), dtype=torch.uint8, device=dev),
                   report_len=torch.empty(n, dtype=torch.int32, device=dev),
                   status=torch.empty(n, dtype=torch.uint8, device=dev))
        tid = (C.c_uint8 * 32).from_buffer_copy(bytes(task_id))
        rc = L.prio3_client_prepare_reports_device(
            self.handle, leader_sealer.handle, helper_sealer.handle, n, tid, int(time_precision),
            _tptr(measurements), _tptr(report_ids), _tptr(times), _tptr(rand), _tptr(sk_e_leader),
            _tptr(sk_e_helper), leader_config_id, helper_config_id,
            int(bool(with_taskprov_extension)), _tptr(out["reports"]), stride,
            _tptr(out["report_len"]), _tptr(out["status"]), _stream(stream, self.device))
        if rc:
            raise RuntimeError(f"prio3_client_prepare_reports_device failed (rc={rc})")
        return out

    # ---- leader upload ----------------------------------------------------------------
    def _upload_args(self, task_opener, global_opener, task_config_id, global_config_id, task_id,
                     report_stride, ext_stride):
        if task_opener is None and global_opener is None:
            raise ValueError("the upload needs the task's opener, the global one, or both")
        for o in (task_opener, global_opener):
            if o is not None and o.device != self.device:
                raise ValueError("an opener is bound to another GPU than the engine")
        if len(task_id) != 32:
            raise ValueError("task_id must be 32 bytes")
        if not 0 <= int(task_config_id) <= 0xFF or not 0 <= int(global_config_id) <= 0xFF:
            raise ValueError("an HPKE config id is one byte")
        if report_stride % 4 or ext_stride % 4 or ext_stride < 0:
            raise ValueError("report_stride and ext_stride must be multiples of 4")
        return (None if task_opener is None else task_opener.handle, int(task_config_id),
                None if global_opener is None else global_opener.handle, int(global_config_id))

    def leader_upload_batch(self, reports, report_len, task_id: bytes, now: int,
                            report_deadline: int, task_opener=None, task_config_id: int = 0,
                            global_opener=None, global_config_id: int = 0,
                            task_expiration: int = UINT64_MAX, report_expiry_age: int = UINT64_MAX,
                            ext_stride: int = 64, helper_enc_len: int = 32,
                            helper_ct_stride: int = 0) -> dict:
        """The leader's upload handler for a batch of one task (prio3_leader_upload_batch; host
        buffers, blocking): reports uint8 [n, report_stride] with report_len [n] -> dict of
        report_ids, times, public_shares, leader_input_shares, extensions / ext_len, the helper
        ciphertext rows (helper_config_ids, helper_enc, helper_ct, helper_ct_len),
        leader_config_ids and status (0, UPLOAD_* = Janus's ReportRejectionReason from 1,
        UPLOAD_MALFORMED, UPLOAD_HOST).  Rows of a report with non-zero status are zero."""
        rows = np.ascontiguousarray(reports, np.uint8)
        ln = np.ascontiguousarray(report_len, np.uint32)
        if rows.ndim != 2 or ln.shape != (rows.shape[0],):
            raise ValueError("reports must be [n, report_stride] and report_len [n]")
        n, stride = rows.shape
        ho, hc, go, gc = self._upload_args(task_opener, global_opener, task_config_id,
                                           global_config_id, task_id, stride, ext_stride)
        sz = self.sz
        out = dict(report_ids=np.zeros((n, 16), np.uint8), times=np.zeros(n, np.uint64),
                   public_shares=np.zeros((n, sz.public_share_len), np.uint8),
                   leader_input_shares=np.zeros((n, sz.leader_input_share_len), np.uint8),
                   extensions=np.zeros((n, ext_stride), np.uint8), ext_len=np.zeros(n, np.uint32),
                   helper_config_ids=np.zeros(n, np.uint8),
                   helper_enc=np.zeros((n, helper_enc_len), np.uint8),
                   helper_ct=np.zeros((n, helper_ct_stride), np.uint8),
                   helper_ct_len=np.zeros(n, np.uint32), leader_config_ids=np.zeros(n, np.uint8),
                   status=np.zeros(n, np.uint8))
        w = lambda a: _np_ptr(a) if a.size else None  # noqa: E731
        tid = (C.c_uint8 * 32).from_buffer_copy(bytes(task_id))
        rc = load_library().prio3_leader_upload_batch(
            self.handle, ho, hc, go, gc, n, tid, int(now), int(report_deadline),
            int(task_expiration), int(report_expiry_age), w(rows), stride, _np_ptr(ln),
            _np_ptr(out["report_ids"]), _np_ptr(out["times"]), w(out["public_shares"]),
            _np_ptr(out["leader_input_shares"]), w(out["extensions"]), _np_ptr(out["ext_len"]),
            ext_stride, _np_ptr(out["helper_config_ids"]), w(out["helper_enc"]), helper_enc_len,
            w(out["helper_ct"]), _np_ptr(out["helper_ct_len"]), helper_ct_stride,
            _np_ptr(out["leader_config_ids"]), _np_ptr(out["status"]))
        if rc == -3:
            raise NotImplementedError("prio3_leader_upload_batch: unsupported instance")
        if rc:
            raise RuntimeError(f"prio3_leader_upload_batch failed (rc={rc})")
        return out

    def submit_leader_upload_job(self, reports, report_len, task_id: bytes, now: int,
                                 report_deadline: int, task_opener=None, task_config_id: int = 0,
                                 global_opener=None, global_config_id: int = 0,
                                 task_expiration: int = UINT64_MAX,
                                 report_expiry_age: int = UINT64_MAX, ext_stride: int = 64,
                                 helper_enc_len: int = 32, helper_ct_stride: int = 0,
                                 notify_fd=None) -> Ticket:
        """``leader_upload_job`` as a ticket (prio3_leader_upload_job_submit): the rows and
        lengths are consumed when this returns, ``wait()`` returns the blocking method's dict."""
        return self.leader_upload_job(reports, report_len, task_id, now, report_deadline,
                                      task_opener, task_config_id, global_opener,
                                      global_config_id, task_expiration, report_expiry_age,
                                      ext_stride, helper_enc_len, helper_ct_stride, _ticket=True,
                                      _notify_fd=notify_fd)

    def leader_upload_job(self, reports, report_len, task_id: bytes, now: int,
                          report_deadline: int, task_opener=None, task_config_id: int = 0,
                          global_opener=None, global_config_id: int = 0,
                          task_expiration: int = UINT64_MAX, report_expiry_age: int = UINT64_MAX,
                          ext_stride: int = 64, helper_enc_len: int = 32,
                          helper_ct_stride: int = 0, _ticket=False, _notify_fd=None) -> dict:
        """``leader_upload_batch`` through the upload executor (prio3_leader_upload_job): the
        same arguments and the same dict, byte for byte; concurrent jobs of every task that
        opens with the same keypairs share one launch chain."""
        rows = np.ascontiguousarray(reports, np.uint8)
        ln = np.ascontiguousarray(report_len, np.uint32)
        if rows.ndim != 2 or ln.shape != (rows.shape[0],):
            raise ValueError("reports must be [n, report_stride] and report_len [n]")
        n, stride = rows.shape
        ho, hc, go, gc = self._upload_args(task_opener, global_opener, task_config_id,
                                           global_config_id, task_id, stride, ext_stride)
        sz = self.sz
        out = dict(report_ids=np.zeros((n, 16), np.uint8), times=np.zeros(n, np.uint64),
                   public_shares=np.zeros((n, sz.public_share_len), np.uint8),
                   leader_input_shares=np.zeros((n, sz.leader_input_share_len), np.uint8),
                   extensions=np.zeros((n, ext_stride), np.uint8), ext_len=np.zeros(n, np.uint32),
                   helper_config_ids=np.zeros(n, np.uint8),
                   helper_enc=np.zeros((n, helper_enc_len), np.uint8),
                   helper_ct=np.zeros((n, helper_ct_stride), np.uint8),
                   helper_ct_len=np.zeros(n, np.uint32), leader_config_ids=np.zeros(n, np.uint8),
                   status=np.zeros(n, np.uint8))
        a = lambda x: x.ctypes.data if x.size else None  # noqa: E731
        h = lambda o: None if o is None else o.value  # noqa: E731
        jin = Prio3UploadJobIn(
            task_opener=h(ho), global_opener=h(go), task_config_id=hc, global_config_id=gc, n=n,
            task_id=(C.c_uint8 * 32).from_buffer_copy(bytes(task_id)), now=int(now),
            report_deadline=int(report_deadline), task_expiration=int(task_expiration),
            report_expiry_age=int(report_expiry_age), reports=a(rows), report_len=a(ln),
            report_stride=stride, ext_stride=ext_stride, helper_enc_len=helper_enc_len,
            helper_ct_stride=helper_ct_stride)
        jout = Prio3UploadJobOut(**{k: a(v) for k, v in out.items()})
        name = "prio3_leader_upload_job"
        try:
            return _job_call(name, (self.handle, C.byref(jin), C.byref(jout)),
                             [self, task_opener, global_opener, rows, ln], list(out.values()),
                             lambda: out, _ticket, _notify_fd)
        except RuntimeError as e:
            if "(rc=-3)" in str(e):
                raise NotImplementedError(f"{name}: unsupported instance") from None
            raise

    def leader_upload_device(self, reports, report_len, task_id: bytes, now: int,
                             report_deadline: int, task_opener=None, task_config_id: int = 0,
                             global_opener=None, global_config_id: int = 0,
                             task_expiration: int = UINT64_MAX,
                             report_expiry_age: int = UINT64_MAX, ext_stride: int = 64,
                             helper_enc_len: int = 32, helper_ct_stride: int = 0,
                             stream=None) -> dict:
        """Device form (prio3_device_leader_upload) on torch tensors of the engine's GPU: reports
        uint8 [n, report_stride], report_len int32 [n], as prepare_reports_device returns them.
        Returns the same dict as leader_upload_batch, as tensors (times int64, the lengths int32);
        no host synchronisation."""
        import torch
        for t, es in ((reports, 1), (report_len, 4)):
            if not isinstance(t, torch.Tensor) or not t.is_contiguous() or \
                    t.device.type != "cuda" or t.device.index != self.device or \
                    t.element_size() != es:
                raise ValueError("reports / report_len must be contiguous uint8 / 4-byte tensors "
                                 "on the engine's GPU")
        if reports.dim() != 2 or tuple(report_len.shape) != (reports.shape[0],):
            raise ValueError("reports must be [n, report_stride] and report_len [n]")
        n, stride = reports.shape
        ho, hc, go, gc = self._upload_args(task_opener, global_opener, task_config_id,
                                           global_config_id, task_id, stride, ext_stride)
        sz = self.sz
        dev = reports.device
        u8 = dict(dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = dict(report_ids=torch.empty((n, 16), **u8),
                   times=torch.empty(n, dtype=torch.int64, device=dev),
                   public_shares=torch.empty((n, sz.public_share_len), **u8),
                   leader_input_shares=torch.empty((n, sz.leader_input_share_len), **u8),
                   extensions=torch.empty((n, ext_stride), **u8), ext_len=torch.empty(n, **i32),
                   helper_config_ids=torch.empty(n, **u8),
                   helper_enc=torch.empty((n, helper_enc_len), **u8),
                   helper_ct=torch.empty((n, helper_ct_stride), **u8),
                   helper_ct_len=torch.empty(n, **i32), leader_config_ids=torch.empty(n, **u8),
                   status=torch.empty(n, **u8))
        w = lambda t: _tptr(t) if t.numel() else None  # noqa: E731
        tid = (C.c_uint8 * 32).from_buffer_copy(bytes(task_id))
        rc = load_library().prio3_device_leader_upload(
            self.handle, ho, hc, go, gc, n, tid, int(now), int(report_deadline),
            int(task_expiration), int(report_expiry_age), w(reports), stride, _tptr(report_len),
            _tptr(out["report_ids"]), _tptr(out["times"]), w(out["public_shares"]),
            _tptr(out["leader_input_shares"]), w(out["extensions"]), _tptr(out["ext_len"]),
            ext_stride, _tptr(out["helper_config_ids"]), w(out["helper_enc"]), helper_enc_len,
            w(out["helper_ct"]), _tptr(out["helper_ct_len"]), helper_ct_stride,
            _tptr(out["leader_config_ids"]), _tptr(out["status"]), _stream(stream, self.device))
        if rc == -3:
            raise NotImplementedError("prio3_device_leader_upload: unsupported instance")
        if rc:
            raise RuntimeError(f"prio3_device_leader_upload failed (rc={rc})")
        return out

    # ---- measurement ----------------------------------------------------------------
    def timing(self) -> dict:
        names = C.create_string_buffer(4096)
        ms = (C.c_double * 64)()
        launches = (C.c_uint64 * 64)()
        k = load_library().prio3_engine_timing(self.handle, names, 4096, ms, launches, 64)
        keys = names.value.decode().split(",") if k else []
        return {keys[i]: (ms[i], int(launches[i])) for i in range(min(k, 64))}

    def timing_reset(self):
        load_library().prio3_engine_timing_reset(self.handle)

"""The declarations of the one-call leader job (no GPU): the header's entry point and its two
structs; the Python binding and its ctypes mirrors; the jobs driver's worker; the Rust block of
INTEGRATION.md."""
import inspect
import os
import re
import sys

from tests.conftest import ROOT

IN_FIELDS = ("report_ids", "times", "leader_status", "prepare_error", "prep_msgs", "time_precision",
             "closed_intervals", "accept_mask", "k", "max_segments")
OUT_FIELDS = ("segment_ids", "segment_starts", "reject", "duplicate", "info", "status", "outcome",
              "agg_shares", "counts", "checksums", "intervals")


def _header():
    return open(os.path.join(ROOT, "include", "janus_prio3.h")).read()


def _ffi():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ffi_rs as F
    return F


def test_header_declares_the_entry_point():
    hdr = _header()
    m = re.search(r"int\s+prio3_leader_finish_job\s*\(([^;]*)\)\s*;", hdr)
    assert m, "prio3_leader_finish_job is missing from the header"
    assert " ".join(m.group(1).split()) == ("prio3_batch* batch, const prio3_leader_job_in* job, "
                                            "const prio3_leader_job_out* out")
    # beside the leader entry points, after prepare_next + aggregate
    assert hdr.index("int prio3_leader_prepare_next_aggregate_batch(") < m.start() < \
        hdr.index("int prio3_device_leader_prepare_init(")
    structs = _ffi().parse_header(os.path.join(ROOT, "include", "janus_prio3.h"))["structs"]
    assert tuple(f for f, _ in structs["prio3_leader_job_in"]) == IN_FIELDS
    assert tuple(f for f, _ in structs["prio3_leader_job_out"]) == OUT_FIELDS
    types = dict(structs["prio3_leader_job_in"])
    assert types["time_precision"] == "u64" and types["k"] == types["max_segments"] == "u32"
    assert types["prepare_error"] == "*const u8" and types["times"] == "*const u64"
    out = dict(structs["prio3_leader_job_out"])
    assert out["info"] == "*mut prio3_job_index_info" and out["outcome"] == "*mut u8"
    assert out["segment_ids"] == "*mut u32" and out["intervals"] == "*mut u64"


def test_python_binds_it():
    import ctypes as C

    from janus_amd import prio3 as J
    assert "prio3_leader_finish_job" in J.EXPORTED_SYMBOLS
    sig = inspect.signature(J.PreparedBatch.leader_finish_job)
    for p in ("report_ids", "times", "leader_status", "prep_msgs", "time_precision",
              "max_segments", "prepare_error", "closed_intervals", "accept_mask"):
        assert p in sig.parameters, p
    # the ctypes mirrors carry the header's fields in the header's order
    structs = _ffi().parse_header(os.path.join(ROOT, "include", "janus_prio3.h"))["structs"]
    for cls, name in ((J.Prio3LeaderJobIn, "prio3_leader_job_in"),
                      (J.Prio3LeaderJobOut, "prio3_leader_job_out")):
        assert [f for f, _ in cls._fields_] == [f for f, _ in structs[name]], name
        for (f, ct), (_, rt) in zip(cls._fields_, structs[name]):
            assert (ct is C.c_void_p) == rt.startswith("*"), (name, f, rt)
    assert C.sizeof(J.Prio3LeaderJobIn) == 72 and C.sizeof(J.Prio3LeaderJobOut) == 88
    assert J.Prio3LeaderJobIn.time_precision.offset == 40 and J.Prio3LeaderJobIn.k.offset == 64


def test_jobs_library_exports_the_worker():
    import ctypes as C
    lib = os.path.join(ROOT, "janus_amd", "libjanus_jobs.so")
    fn = C.CDLL(lib).janus_jobs_run_leader_job  # AttributeError: the symbol is not exported
    assert fn is not None
    src = open(os.path.join(ROOT, "janus_amd", "csrc", "jobs_driver.cpp")).read()
    assert "prio3_leader_finish_job(" in src
    # form 0 is the four moves: overlay, index, prepare_next + aggregate, metadata
    body = src[src.index("double janus_jobs_run_leader_job("):]
    for call in ("prio3_job_index(", "prio3_leader_prepare_next_aggregate_batch(",
                 "prio3_batch_metadata(", "prio3_leader_prepare_init_batch("):
        assert call in body, call


def test_engine_library_exports_the_entry_point():
    import ctypes as C
    lib = os.path.join(ROOT, "janus_amd", "libjanus_prio3.so")
    assert C.CDLL(lib).prio3_leader_finish_job is not None


def test_rust_block_declares_it():
    F = _ffi()
    rs = F.parse_rust(F.integration_block())
    fn = rs["funcs"]["prio3_leader_finish_job"]
    assert fn["ret"] == "c_int"
    assert [t for _, t in fn["params"]] == ["*mut prio3_batch", "*const prio3_leader_job_in",
                                            "*const prio3_leader_job_out"]
    assert tuple(f for f, _ in rs["structs"]["prio3_leader_job_in"]) == IN_FIELDS
    assert tuple(f for f, _ in rs["structs"]["prio3_leader_job_out"]) == OUT_FIELDS

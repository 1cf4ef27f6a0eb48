"""The declarations of the one-call helper job (no GPU): the header's entry point, its two structs
and the in-group limits; the Python binding; the jobs driver's worker."""
import inspect
import os
import re

from tests.conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "janus_prio3.h")).read()


def test_header_declares_the_entry_point_and_the_limits():
    hdr = _header()
    m = re.search(r"int\s+prio3_helper_aggregate_job\s*\(([^;]*)\)\s*;", hdr)
    assert m, "prio3_helper_aggregate_job is missing from the header"
    assert " ".join(m.group(1).split()) == ("prio3_engine* engine, const prio3_helper_job_in* job, "
                                            "const prio3_helper_job_out* out")
    assert re.search(r"PRIO3_JOB_GROUP_MAX_REPORTS\s*=\s*4096\b", hdr)
    assert re.search(r"PRIO3_JOB_GROUP_MAX_SEGMENTS\s*=\s*64\b", hdr)
    # in the host-buffer section, after the _ex form and ahead of the device-resident section
    assert hdr.index("prio3_helper_aggregate_init_batch_ex(") < m.start() < \
        hdr.index("/* ---- Device-resident entry points")
    for field in ("time_precision", "closed_intervals", "max_segments", "accept_mask",
                  "report_deadline", "fallback_opener"):
        assert re.search(r"\b%s;" % field, hdr), field
    for field in ("segment_ids", "segment_starts", "reject", "duplicate", "info", "prep_msgs",
                  "status", "agg_shares", "counts", "checksums", "intervals"):
        assert re.search(r"\*\s*%s;" % field, hdr), field


def test_python_binds_it():
    import ctypes as C
    import sys

    from janus_amd import prio3 as J
    assert "prio3_helper_aggregate_job" in J.EXPORTED_SYMBOLS
    assert (J.JOB_GROUP_MAX_REPORTS, J.JOB_GROUP_MAX_SEGMENTS) == (4096, 64)
    sig = inspect.signature(J.HelperEngine.aggregate_job)
    for p in ("time_precision", "max_segments", "closed_intervals", "accept_mask",
              "fallback_opener", "report_deadline"):
        assert p in sig.parameters, p
    # the ctypes mirrors carry the header's fields in the header's order
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ffi_rs as F
    structs = F.parse_header(os.path.join(ROOT, "include", "janus_prio3.h"))["structs"]
    for cls, name in ((J.Prio3HelperJobIn, "prio3_helper_job_in"),
                      (J.Prio3HelperJobOut, "prio3_helper_job_out")):
        assert [f for f, _ in cls._fields_] == [f for f, _ in structs[name]], name
        for (f, ct), (_, rt) in zip(cls._fields_, structs[name]):
            assert (ct is C.c_void_p) == rt.startswith("*"), (name, f, rt)
    assert C.sizeof(J.Prio3HelperJobIn) == 136 and C.sizeof(J.Prio3HelperJobOut) == 88


def test_jobs_library_exports_the_worker():
    lib = os.path.join(ROOT, "janus_amd", "libjanus_jobs.so")
    import ctypes as C
    fn = C.CDLL(lib).janus_jobs_run_job  # AttributeError: the symbol is not exported
    assert fn is not None
    src = open(os.path.join(ROOT, "janus_amd", "csrc", "jobs_driver.cpp")).read()
    assert "prio3_helper_aggregate_job(" in src and "call_mu" in src

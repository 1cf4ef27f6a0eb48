"""The declarations of the leader's upload job (no GPU): the ctypes structs of the Python binding
against the header's field order and sizes, the submit form against its blocking twin, and the
two entry points in the Rust crate of INTEGRATION.md section 2."""
import ctypes as C
import inspect
import os
import sys

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffi_rs as F  # noqa: E402

HEADER = os.path.join(ROOT, "include", "janus_prio3.h")
RUST = {"u8": C.c_uint8, "u32": C.c_uint32, "u64": C.c_uint64, "[u8; 2]": C.c_uint8 * 2,
        "[u8; 32]": C.c_uint8 * 32}


def _ctype(rust: str):
    return C.c_void_p if rust.startswith("*") else RUST[rust]


def test_ctypes_structs_match_the_header():
    from janus_amd import prio3 as J
    structs = F.parse_header(HEADER)["structs"]
    for name, cls, size in (("prio3_upload_job_in", J.Prio3UploadJobIn, 120),
                            ("prio3_upload_job_out", J.Prio3UploadJobOut, 96)):
        fields = structs[name]
        assert [n for n, _ in cls._fields_] == [n for n, _ in fields], name
        for (n, ct), (_, rt) in zip(cls._fields_, fields):
            assert ct is _ctype(rt) or C.sizeof(ct) == C.sizeof(_ctype(rt)), (name, n)
        # the size a C compiler gives the header's struct: the fields in order, each aligned to
        # its own size (arrays to their element's)
        off = 0
        for fname, rt in fields:
            t = _ctype(rt)
            al = C.alignment(t)
            off = -(-off // al) * al
            assert getattr(cls, fname).offset == off, (name, fname)
            off += C.sizeof(t)
        off = -(-off // 8) * 8
        assert off == C.sizeof(cls) == size, name
    # no implicit padding in the input struct: every field sits where the one before it ends
    end = 0
    for n, t in J.Prio3UploadJobIn._fields_:
        assert getattr(J.Prio3UploadJobIn, n).offset == end, n
        end += C.sizeof(t)
    consts = F.parse_header(HEADER)["consts"]
    assert consts["PRIO3_UPLOAD_JOB_MAX_REPORTS"] == J.UPLOAD_JOB_MAX_REPORTS == 4096
    assert J.EXEC_UPLOAD == 5


def test_submit_is_the_blocking_call_plus_fd_and_ticket():
    from janus_amd import prio3 as J
    funcs = F.parse_header(HEADER)["funcs"]
    blocking, submit = funcs["prio3_leader_upload_job"], funcs["prio3_leader_upload_job_submit"]
    assert blocking["params"] == [("engine", "*mut prio3_engine"),
                                  ("job", "*const prio3_upload_job_in"),
                                  ("out", "*const prio3_upload_job_out")]
    assert submit["params"] == blocking["params"] + [("notify_fd", "c_int"),
                                                     ("ticket_out", "*mut *mut prio3_ticket")]
    assert blocking["ret"] == submit["ret"] == "c_int"
    hdr = open(HEADER).read()
    upload = hdr[hdr.index("/* ---- Leader upload ---- */"):hdr.index("/* ---- Client ---- */")]
    for name in ("prio3_leader_upload_job(", "prio3_leader_upload_job_submit(",
                 "PRIO3_UPLOAD_JOB_MAX_REPORTS = 4096", "96 MB"):
        assert name in upload, name
    for name in ("prio3_leader_upload_job", "prio3_leader_upload_job_submit"):
        assert name in J.EXPORTED_SYMBOLS
    b = inspect.signature(J.HelperEngine.leader_upload_job).parameters
    s = inspect.signature(J.HelperEngine.submit_leader_upload_job).parameters
    assert list(s) == [p for p in b if not p.startswith("_")] + ["notify_fd"]
    batch = inspect.signature(J.HelperEngine.leader_upload_batch).parameters
    assert [p for p in b if not p.startswith("_")] == list(batch)  # the batch form's arguments
    L = J.load_library()
    assert len(L.prio3_leader_upload_job_submit.argtypes) == \
        len(L.prio3_leader_upload_job.argtypes) + 2


def test_integration_declares_the_entry_points():
    r = F.parse_rust(F.integration_block())
    c = F.parse_header(HEADER)
    for name in ("prio3_leader_upload_job", "prio3_leader_upload_job_submit"):
        assert r["funcs"][name] == c["funcs"][name], name
    for name in ("prio3_upload_job_in", "prio3_upload_job_out"):
        assert r["structs"][name] == c["structs"][name], name
    assert r["consts"]["PRIO3_UPLOAD_JOB_MAX_REPORTS"] == 4096

"""The declarations of ticketed job submission (no GPU): the header's five submit forms and the
two ticket calls, the Python binding's twins, and the jobs driver's ticketed workers."""
import inspect
import os
import re
import sys

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "janus_prio3.h")
TWINS = ("prio3_helper_prepare_aggregate_batch", "prio3_helper_aggregate_init_batch_ex",
         "prio3_helper_aggregate_job", "prio3_leader_prepare_init_batch",
         "prio3_leader_finish_job")


def _funcs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ffi_rs as F
    assert "prio3_ticket" in F.OPAQUE
    return F.parse_header(HEADER)["funcs"]


def test_header_declares_the_seven_functions():
    funcs = _funcs()
    for name in TWINS:
        blocking, submit = funcs[name], funcs[name + "_submit"]
        # the blocking twin's arguments, then the eventfd and the ticket
        assert submit["params"] == blocking["params"] + [("notify_fd", "c_int"),
                                                         ("ticket_out", "*mut *mut prio3_ticket")]
        assert submit["ret"] == "c_int"
    assert funcs["prio3_ticket_poll"] == dict(ret="c_int",
                                              params=[("ticket", "*const prio3_ticket")])
    assert funcs["prio3_ticket_wait"] == dict(ret="c_int", params=[("ticket", "*mut prio3_ticket")])


def test_header_section_and_contract():
    hdr = open(HEADER).read()
    a = hdr.index("/* ---- Ticketed job submission ---- */")
    # a section of its own: after the leader's device entry points, ahead of the upload
    assert hdr.index("int prio3_device_leader_prepare_next(") < a < \
        hdr.index("/* ---- Leader upload ---- */")
    section = hdr[a:hdr.index("/* ---- Leader upload ---- */")]
    assert "typedef struct prio3_ticket prio3_ticket;" in section
    for name in [t + "_submit" for t in TWINS] + ["prio3_ticket_poll", "prio3_ticket_wait"]:
        assert hdr.count(name + "(") == 1 and name + "(" in section, name
    text = " ".join(re.sub(r"\n \*", "\n", section).split())  # without the comment leaders
    for words in ("read only inside the submit call", "written only inside prio3_ticket_wait",
                  "exactly once per ticket", "*ticket_out = NULL", "waited exactly once",
                  "96 MB", "no cancel"):
        assert words in text, words


def test_python_binds_the_twins():
    from janus_amd import prio3 as J
    for name in [t + "_submit" for t in TWINS] + ["prio3_ticket_poll", "prio3_ticket_wait"]:
        assert name in J.EXPORTED_SYMBOLS, name
    pairs = ((J.HelperEngine, "prepare_aggregate_batch"), (J.HelperEngine, "aggregate_init_batch"),
             (J.HelperEngine, "aggregate_job"), (J.HelperEngine, "leader_prepare_init_batch"),
             (J.PreparedBatch, "leader_finish_job"))
    for cls, name in pairs:
        blocking = inspect.signature(getattr(cls, name)).parameters
        submit = inspect.signature(getattr(cls, "submit_" + name)).parameters
        public = [p for p in blocking if not p.startswith("_")]
        assert list(submit) == public + ["notify_fd"], name
        assert submit["notify_fd"].default is None
    for m in ("poll", "wait", "__del__"):
        assert callable(getattr(J.Ticket, m))
    L = J.load_library()
    for name in TWINS:
        assert len(getattr(L, name + "_submit").argtypes) == len(getattr(L, name).argtypes) + 2
    assert J.Ticket("x", None, [], [], lambda: 1).poll() is True  # a waited ticket never blocks


def test_jobs_library_exports_the_ticket_workers():
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, "janus_amd", "libjanus_jobs.so"))
    for fn in ("janus_jobs_run_tickets", "janus_jobs_run_job_tickets"):
        assert getattr(lib, fn) is not None  # AttributeError: the symbol is not exported
    src = open(os.path.join(ROOT, "janus_amd", "csrc", "jobs_driver.cpp")).read()
    assert "prio3_helper_prepare_aggregate_batch_submit(" in src
    assert "prio3_helper_aggregate_job_submit(" in src and "prio3_ticket_wait(" in src


def test_executor_template_has_no_hip():
    """The executor template lives in a header a CPU program can include."""
    src = open(os.path.join(ROOT, "janus_amd", "csrc", "prio3_exec.h")).read()
    assert "struct Exec" in src and "#include <hip" not in src and '#include "prio3_runtime.h"' not in src
    for fn in ("begin(", "done(", "complete(", "submit("):
        assert fn in src, fn
    rt = open(os.path.join(ROOT, "janus_amd", "csrc", "prio3_runtime.hip")).read()
    assert "struct Exec {" not in rt and '#include "prio3_exec.h"' in rt

"""GPU: reports with real XOF rejections, byte for byte against the C restatement.

The pytest process holds the default library, so every group of cases runs in a fresh child
process on the test-rejection build (janus_amd/libjanus_prio3_rej.so, option test_reject_bits;
tests/real_rejections.py has the cases and the rates).  The restatement carries the same
acceptance predicate, so statuses, prepare messages, output shares, aggregate shares and counts
must be equal, with no tolerance.  The reference conditions -- enough flagged reports but at most
half, flagged and unflagged reports in one wave, a tampered flagged report, and over the module
every stream, the element that straddles two squeeze blocks, first and last elements, repeated
rejections -- are computed from the restatement alone and asserted here, so no case passes
vacuously.  A child runs once; if it ends by a signal, at its time limit or with any other failure
status, the tests of its group fail from the record and the rest of the module skips instead of
starting more GPU work.
"""
import json
import os
import subprocess
import sys

import pytest

from tests import real_rejections as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

REJ_LIB = os.path.join(ROOT, "janus_amd", "libjanus_prio3_rej.so")
TIMEOUT = {"helper": 240, "fused": 120, "leader": 120, "client": 120, "executor": 120,
           "semantic": 90}
_state = {"dead": None, "cases": {}, "failed": {}, "seen": []}


def _group(group):
    """The cases of one group, run once in a child process: {case id: result}."""
    if group in _state["failed"]:
        raise AssertionError(_state["failed"][group])
    if group in _state["cases"]:
        return _state["cases"][group]
    if _state["dead"]:
        pytest.skip(f"an earlier child process {_state['dead']}; no further GPU work")
    assert os.path.exists(REJ_LIB), "the test-rejection library is not built (make -C janus_amd)"
    env = dict(os.environ, JANUS_PRIO3_LIB=REJ_LIB, PYTHONPATH=ROOT)
    p = subprocess.Popen([sys.executable, "-m", "tests.real_rejections", group], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        out = p.communicate(timeout=TIMEOUT[group])[0].decode(errors="replace")
    except subprocess.TimeoutExpired:
        p.kill()
        out = p.communicate()[0].decode(errors="replace")
        _state["dead"] = f"({group}) ran into its time limit"
        _state["failed"][group] = f"group {group} timed out:\n{out[-3000:]}"
        raise AssertionError(_state["failed"][group])
    res = {}
    for ln in out.splitlines():
        if ln.startswith("CASE "):
            r = json.loads(ln[5:])
            res[r["case"]] = r
            print(ln)
    # a child runs once: its cases, or its failure, are what every later test of the group sees,
    # and a child that did not end cleanly (exit status, signal) is the last GPU child started
    _state["cases"][group] = res
    if p.returncode != 0 or f"GROUP-DONE {group}" not in out:
        _state["dead"] = f"({group}) ended with status {p.returncode}"
        _state["failed"][group] = f"group {group} exit {p.returncode}:\n{out[-3000:]}"
        raise AssertionError(_state["failed"][group])
    _state["seen"] += [c for r in res.values() for c in r["cond"].get("jobs", [r["cond"]])
                       if "flagged" in c]
    return res


def _check(r, tampered=True):
    """The per-case reference conditions, then the device comparison."""
    c = r["cond"]
    assert 8 <= c["flagged"] <= c["n"] // 2, c
    assert c["mixed64"] and c["mixed32"], c
    if tampered:
        assert c["tampered_flagged"], c
    assert r["ok"], r["err"]


@pytest.mark.parametrize("case", [c[0] for c in R.HELPER_CASES])
def test_helper_prepare_accumulate(case):
    _check(_group("helper")[case])


def test_decode_checks_keep_lt_p():
    """A prep-share element with all its top bits set but < p decodes under the variant (it
    fails decide); an element >= p does not decode."""
    r = _group("helper")["decode_top_bits"]
    assert r["cond"]["top_bits_status"] != r["cond"]["ge_p_status"] and r["cond"]["ge_p_status"]
    assert r["ok"], r["err"]


@pytest.mark.parametrize("case", [c[0] for c in R.FUSED_CASES])
def test_fused_one_pass(case):
    r = _group("fused")[case]
    assert r["cond"]["unfused_by_flag"] and r["cond"]["flag_free"], r["cond"]
    _check(r)


@pytest.mark.parametrize("name", [c[0] for c in R.LEADER_CASES])
def test_leader(name):
    _check(_group("leader")["leader-" + name])


@pytest.mark.parametrize("name", [c[0] for c in R.CLIENT_CASES])
def test_client_shard(name):
    _check(_group("client")["shard-" + name], tampered=False)


def test_client_generator_marks_rejections():
    r = _group("client")["generate-" + R.GEN_CASE[0]]
    c = r["cond"]
    assert 8 <= c["flagged"] <= c["n"] // 2 and c["mixed64"] and c["mixed32"], c
    assert r["ok"], r["err"]


def test_executor_concurrent_jobs():
    r = _group("executor")["executor-4x500"]
    for c in r["cond"]["jobs"]:  # the conditions hold for each of the four jobs
        _check(dict(r, cond=c))


def test_semantic_end_to_end():
    r = _group("semantic")["semantic-" + R.SEMANTIC_CASE[0]]
    assert r["ok"], r["err"]


def test_default_build_has_no_reject_option():
    """The predicate is a build variant, not a runtime hook of the product library."""
    from tests.conftest import CONFIGS
    from tests.test_gpu_parity import _engine
    with pytest.raises(ValueError):
        _engine(CONFIGS["count"]).set_option("test_reject_bits", 10)


def test_module_wide_coverage():
    """Over all the cases: every stream, the straddling Field128 measurement-share element,
    first and last elements of a stream, and a stream with two or more rejections."""
    for g in ("helper", "fused", "leader", "client", "executor"):
        _group(g)
    seen = _state["seen"]
    assert {s for c in seen for s in c["streams"]} >= {"query", "meas", "proofs", "jr"}
    for k in ("straddle", "first", "last", "multi"):
        assert any(c[k] for c in seen), k

"""Host form of the DAP `Report` encoder (janus_dap_report_encode_host) against the reference's
own codec fixtures (messages/src/tests/upload.rs roundtrip_report, extracted as data by
tests/golden/gen_dap_report_fixtures.py), and its argument rules.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT

FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "dap_report_fixtures.json")))["reports"]


def _rows(reps, ct_pad=0):
    """SoA rows of fixture reports with one public share length; ct rows padded by ct_pad."""
    b = bytes.fromhex
    u8 = lambda xs: np.frombuffer(b"".join(xs), np.uint8).reshape(len(xs), len(xs[0])).copy()  # noqa: E731
    n = len(reps)
    out = dict(report_ids=u8([b(r["report_id"]) for r in reps]),
               times=np.array([r["time"] for r in reps], np.uint64),
               public_shares=u8([b(r["public_share"]) for r in reps]))
    for who in ("leader", "helper"):
        ct = u8([b(r[who]["payload"]) for r in reps])
        out[who + "_config_id"] = reps[0][who]["config_id"]
        out[who + "_enc"] = u8([b(r[who]["enc"]) for r in reps])
        out[who + "_ct_len"] = np.full(n, ct.shape[1], np.uint32)
        # poison past ct_len: the encoder must not copy it
        out[who + "_ct"] = np.concatenate([ct, np.full((n, ct_pad), 0xEE, np.uint8)], axis=1)
    return out


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("ct_pad", [0, 10])
def test_host_encode_reproduces_the_reference_fixture(i, ct_pad):
    from janus_amd import dap
    r = FIX[i]
    out, out_len = dap.report_encode_host(**_rows([r], ct_pad))
    want = bytes.fromhex(r["hex"])
    assert int(out_len[0]) == len(want)
    assert out[0, :len(want)].tobytes() == want
    assert not out[0, len(want):].any()
    assert out.shape[1] == dap.report_max_len(len(r["public_share"]) // 2, 6, 6 + ct_pad, 4,
                                              4 + ct_pad)


def test_fixture_lengths_are_the_ones_the_issue_names():
    assert [len(r["public_share"]) // 2 for r in FIX] == [0, 4]
    assert {(len(r["leader"]["enc"]) // 2, len(r["helper"]["enc"]) // 2) for r in FIX} == {(6, 4)}
    assert {(len(r["leader"]["payload"]) // 2, len(r["helper"]["payload"]) // 2)
            for r in FIX} == {(6, 4)}


def test_out_stride_too_small_is_earg():
    from janus_amd import dap
    rows = _rows([FIX[1]])
    need = dap.report_max_len(4, 6, 6, 4, 4)
    assert need == len(FIX[1]["hex"]) // 2
    with pytest.raises(ValueError):
        dap.report_encode_host(**rows, out_stride=need - 1)
    # the C entry point itself
    L = dap._lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    out = np.full(need, 0x55, np.uint8)
    out_len = np.full(1, 77, np.uint32)
    args = lambda stride: (1, p(rows["report_ids"]), p(rows["times"]), p(rows["public_shares"]), 4,  # noqa: E731
                           42, p(rows["leader_enc"]), 6, p(rows["leader_ct"]),
                           p(rows["leader_ct_len"]), 6, 13, p(rows["helper_enc"]), 4,
                           p(rows["helper_ct"]), p(rows["helper_ct_len"]), 4, None, p(out), stride,
                           p(out_len))
    assert L.janus_dap_report_encode_host(*args(need - 1)) == -1  # JANUS_DAP_EARG
    assert (out == 0x55).all() and out_len[0] == 77  # nothing written
    assert L.janus_dap_report_encode_host(*args(need)) == 1
    assert out.tobytes() == bytes.fromhex(FIX[1]["hex"])


def test_skipped_and_bad_length_reports_are_left_out():
    from janus_amd import dap
    reps = [FIX[1]] * 5
    rows = _rows(reps, ct_pad=2)
    rows["leader_ct_len"][2] = 0          # failed seal
    rows["helper_ct_len"][3] = 4 + 2 + 1  # above the row
    skip = np.array([0, 1, 0, 0, 0], np.uint8)
    out, out_len = dap.report_encode_host(**rows, skip=skip)
    want = bytes.fromhex(FIX[1]["hex"])
    assert out_len.tolist() == [len(want), 0, 0, 0, len(want)]
    for i in (1, 2, 3):
        assert not out[i].any()
    for i in (0, 4):
        assert out[i, :len(want)].tobytes() == want and not out[i, len(want):].any()

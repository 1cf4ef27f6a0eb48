"""Device form of the DAP `Report` decoder (k_rep_decode) against the host form: ragged batch
sizes, odd row strides, reports that do not decode next to honest ones, a helper `enc` of another
length, and a row's bytes past its report never reaching an output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("report_ids", "times", "fields", "leader_config_ids", "helper_config_ids", "helper_enc",
        "helper_ct", "helper_ct_len", "malformed")


def _reports(n, psl, seed, pad):
    from janus_amd import dap
    rng = np.random.default_rng([seed, n, psl])
    r = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)  # noqa: E731
    lstride, hstride = 208, 64
    rows, ln = dap.report_encode_host(
        report_ids=r(n, 16), times=rng.integers(0, 1 << 64, n, dtype=np.uint64),
        public_shares=r(n, psl), leader_config_id=42, leader_enc=r(n, 65), leader_ct=r(n, lstride),
        leader_ct_len=rng.integers(1, lstride + 1, n).astype(np.uint32), helper_config_id=13,
        helper_enc=r(n, 32), helper_ct=r(n, hstride),
        helper_ct_len=rng.integers(1, hstride + 1, n).astype(np.uint32),
        out_stride=dap.report_max_len(psl, 65, lstride, 32, hstride) + pad)
    # poison past each report: must not reach any output
    for i in range(n):
        rows[i, ln[i]:] = 0xEE
    return rows, ln


def _device(rows, ln, enc_len, ct_stride):
    import torch
    from janus_amd import dap
    d = dap.report_decode_device(torch.from_numpy(rows).cuda(),
                                 torch.from_numpy(ln.view(np.int32)).cuda(), enc_len, ct_stride)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    out["times"] = out["times"].view(np.uint64)
    out["fields"] = out["fields"].view(np.uint32)
    out["helper_ct_len"] = out["helper_ct_len"].view(np.uint32)
    return out


def _same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("psl", [0, 32])
@pytest.mark.parametrize("n", [1, 67, 259])
def test_device_equals_host(n, psl):
    from janus_amd import dap
    rows, ln = _reports(n, psl, 3, pad=3)  # an odd stride: rows start at every byte alignment
    want = dap.report_decode_host(rows, ln, 32, 64)
    assert not want["malformed"].any() and (want["helper_ct_len"] > 0).all()
    _same(_device(rows, ln, 32, 64), want)


def test_malformed_reports_next_to_honest_ones():
    from janus_amd import dap
    n = 67
    rows, ln = _reports(n, 32, 5, pad=1)
    honest = dap.report_decode_host(rows, ln, 32, 64)
    f = honest["fields"]
    rows, ln = rows.copy(), ln.copy()
    ln[3] -= 1                                    # truncated by one byte
    ln[4] += 1                                    # a trailing byte
    ln[5] = rows.shape[1] + 1                     # above the row
    ln[6] = 0                                     # empty
    ln[7] = 27                                    # inside the public share's prefix
    rows[8, 24:28] = 0xFF                         # the public share runs past the report
    rows[9, f[9, dap.F_LEADER_PAYLOAD_OFF] - 4] = 0x80   # the leader payload does
    rows[10, f[10, dap.F_HELPER_ENC_OFF] - 2] = 0xFF     # the helper enc does
    rows[63, f[63, dap.F_HELPER_PAYLOAD_OFF] - 1] ^= 1   # helper payload length off by one
    rows[64, 24:28] = (0, 0, 0, 31)               # public share one byte short: trailing byte
    rows[66, 0] ^= 1                              # an honest change
    bad = [3, 4, 5, 6, 7, 8, 9, 10, 63, 64]
    want = dap.report_decode_host(rows, ln, 32, 64)
    assert np.flatnonzero(want["malformed"]).tolist() == bad
    got = _device(rows, ln, 32, 64)
    _same(got, want)
    for k in KEYS[:-1]:
        assert not got[k][bad].any(), k
    ok = np.setdiff1d(np.arange(n), bad + [66])
    for k in KEYS:
        assert np.array_equal(got[k][ok], honest[k][ok]), k


@pytest.mark.parametrize("enc_len,ct_stride", [(31, 64), (32, 40), (0, 0), (32, 67)])
def test_helper_rows_of_another_shape(enc_len, ct_stride):
    from janus_amd import dap
    rows, ln = _reports(67, 32, 7, pad=0)
    want = dap.report_decode_host(rows, ln, enc_len, ct_stride)
    assert not want["malformed"].any()
    if enc_len == 32 and ct_stride == 40:  # some payloads fit, some do not
        assert (want["helper_ct_len"] == 0).any() and (want["helper_ct_len"] > 0).any()
    _same(_device(rows, ln, enc_len, ct_stride), want)


def test_device_argument_errors_raise():
    import torch
    from janus_amd import dap
    rows, ln = _reports(2, 0, 1, pad=0)
    with pytest.raises(ValueError):
        dap.report_decode_device(torch.from_numpy(rows), torch.from_numpy(ln.view(np.int32)), 32, 64)
    with pytest.raises(ValueError):
        dap.report_decode_device(torch.from_numpy(rows).cuda(),
                                 torch.from_numpy(ln.view(np.int32)[:1]).cuda(), 32, 64)
    with pytest.raises(ValueError):
        dap.report_decode_device(torch.from_numpy(rows).cuda(),
                                 torch.from_numpy(ln.view(np.int32)).cuda(), 0x10000, 64)

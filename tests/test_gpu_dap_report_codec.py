"""Device form of the DAP `Report` encoder (k_rep_write) against the host form: ragged batch
sizes, per-report ciphertext lengths that differ, reports left out, bytes past ct_len unread."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _batch(n, psl, seed):
    rng = np.random.default_rng([seed, n, psl])
    r = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)  # noqa: E731
    lstride, hstride = 208, 64
    return dict(report_ids=r(n, 16), times=rng.integers(0, 1 << 62, n, dtype=np.uint64),
                public_shares=r(n, psl), leader_config_id=42, leader_enc=r(n, 65),
                leader_ct=r(n, lstride),  # random past ct_len too: must not reach the output
                leader_ct_len=rng.integers(17, lstride + 1, n).astype(np.uint32),
                helper_config_id=13, helper_enc=r(n, 32), helper_ct=r(n, hstride),
                helper_ct_len=rng.integers(17, hstride + 1, n).astype(np.uint32))


def _device(rows, skip=None, out_stride=None):
    import torch
    from janus_amd import dap
    t = lambda a: a if isinstance(a, int) else torch.from_numpy(  # noqa: E731
        a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32
        else a).cuda()
    out, out_len = dap.report_encode_device(**{k: t(v) for k, v in rows.items()},
                                            skip=None if skip is None else t(skip),
                                            out_stride=out_stride)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("psl", [0, 32])
@pytest.mark.parametrize("n", [1, 67, 130])
def test_device_equals_host(n, psl):
    from janus_amd import dap
    rows = _batch(n, psl, 3)
    skip = (np.arange(n) % 11 == 7).astype(np.uint8)
    # an odd row stride: rows start at every byte alignment
    stride = dap.report_max_len(psl, 65, 208, 32, 64) + 3
    want, want_len = dap.report_encode_host(**rows, skip=skip, out_stride=stride)
    got, got_len = _device(rows, skip, stride)
    assert np.array_equal(got_len, want_len)
    assert np.array_equal(got, want)
    assert (want_len[skip == 0] == 42 + psl + 65 + 32 + rows["leader_ct_len"][skip == 0]
            + rows["helper_ct_len"][skip == 0]).all()
    assert not want_len[skip == 1].any()


def test_ct_len_above_the_stride_is_left_out():
    from janus_amd import dap
    n = 67
    rows = _batch(n, 32, 5)
    rows["leader_ct_len"][10] = 209       # above the leader row
    rows["helper_ct_len"][64] = 1 << 31   # far above the helper row
    rows["helper_ct_len"][65] = 0         # a failed seal
    want, want_len = dap.report_encode_host(**rows)
    got, got_len = _device(rows)
    assert np.array_equal(got_len, want_len) and np.array_equal(got, want)
    for i in (10, 64, 65):
        assert got_len[i] == 0 and not got[i].any()
    ok = np.setdiff1d(np.arange(n), [10, 64, 65])
    assert (got_len[ok] > 0).all()
    ref, ref_len = dap.report_encode_host(**_batch(n, 32, 5))
    assert np.array_equal(got[ok], ref[ok]) and np.array_equal(got_len[ok], ref_len[ok])


def test_device_out_stride_too_small_raises():
    from janus_amd import dap
    rows = _batch(1, 0, 1)
    with pytest.raises(ValueError):
        _device(rows, out_stride=dap.report_max_len(0, 65, 208, 32, 64) - 1)

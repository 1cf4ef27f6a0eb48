"""The leader's DAP marshaling on the GPU (janus_dap_agg_init_req_encode_device,
janus_dap_agg_job_resp_unpack_device) against the host forms, which tests/test_dap_leader_codec.py
pins to the oracle and the reference fixtures: at the wave, block and scan-chunk edges, with
sentinels behind every output and input, on every regular record mix of the response, on each
irregular shape and each whole-response error (asserted by their flag bits: every body read is
bounds-checked, nothing here is meant to fault), and on a side stream of another GPU than the
thread's."""
import struct

import numpy as np
import pytest

from tests.test_dap_leader_codec import (NONE, expected_index, host_decode, index_with_holes,
                                         job_args, make_job, make_resp)

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 1025]
SENT = 0xA5
WIDTH = 1024  # records the response index speculates per step (RUNP_WIDTH)


def _dev(x, dev, extra_rows=0):
    """numpy -> tensor on dev (uint64 / uint32 as int64 / int32), with sentinel rows appended."""
    import torch
    x = np.ascontiguousarray(x)
    if extra_rows:
        ext = np.zeros((extra_rows,) + x.shape[1:], x.dtype)
        ext.view(np.uint8)[...] = SENT
        x = np.concatenate([x, ext])
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(dev)


def _encode_raw(j, agg_param, qt, bid, dev="cuda:0", stream=None):
    """The C entry point on buffers with a sentinel row behind every input, sentinel bytes behind
    the body's capacity and a sentinel entry behind index.  Returns (body, index, n_included, err)
    after checking every sentinel."""
    import torch
    from janus_amd import dap as J
    from janus_amd.prio3 import _np_ptr, _stream, _tptr
    dev = torch.device(dev)
    n = len(j["times"])
    t = [_dev(x, dev, extra_rows=1) for x in job_args(j)]
    ids, times, pub, cfg, enc, ct, cl, ps, st = t
    psl, enc_len, stride, ps_len = (x.shape[1] for x in (pub, enc, ct, ps))
    L = J._lib()
    cap = L.janus_dap_agg_init_req_max_len(n, len(agg_param), qt, psl, enc_len, stride, ps_len)
    out = torch.full((cap + 64,), SENT, dtype=torch.uint8, device=dev)
    out_len = torch.full((2,), -1, dtype=torch.int64, device=dev)
    index = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ninc = torch.full((2,), -1, dtype=torch.int32, device=dev)
    err = torch.full((3,), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty((n + 1) // 2 + 2 * (n // 256 + 2), dtype=torch.int64, device=dev)
    ap = np.frombuffer(agg_param, np.uint8)
    b = None if bid is None else np.frombuffer(bid, np.uint8)
    w = lambda x: _tptr(x) if x.shape[1] else None  # noqa: E731
    rc = L.janus_dap_agg_init_req_encode_device(
        n, _np_ptr(ap), len(ap), qt, _np_ptr(b), _tptr(ids), _tptr(times), w(pub), psl, _tptr(cfg),
        w(enc), enc_len, w(ct), _tptr(cl), stride, w(ps), ps_len, _tptr(st), _tptr(out),
        _tptr(out_len), _tptr(index), _tptr(ninc), _tptr(err), _tptr(scratch),
        _stream(stream, dev.index or 0))
    assert rc == 0
    torch.cuda.synchronize(dev)
    ln = int(out_len[0])
    o = out.cpu().numpy()
    assert 0 <= ln <= cap and (o[cap:] == SENT).all()
    assert (o[ln:] == SENT).all()  # nothing behind the body, not even the rest of a dword
    assert int(out_len[1]) == -1 and int(ninc[1]) == -1 and int(err[2]) == -1
    assert int(index[n]) == 0x5A5A5A5A
    for x, src in zip(t, job_args(j)):  # the inputs, their sentinel rows included, are as before
        back = x.cpu().numpy()
        assert (back[n:].view(np.uint8) == SENT).all()
        np.testing.assert_array_equal(back[:n].view(np.uint8).reshape(n, -1),
                                      np.ascontiguousarray(src).view(np.uint8).reshape(n, -1))
    return (o[:ln].tobytes(), index[:n].cpu().numpy().view(np.uint32), int(ninc[0]),
            err[:2].cpu().numpy().tolist())


def _edges(n):
    return sorted({r for r in (0, 63, 64, 255, 256, 257, 1023, 1024, n - 1) if 0 <= r < n})


@pytest.mark.parametrize("n", NS)
def test_device_req_encode_equals_host(n):
    from janus_amd import dap as J
    for psl in (0, 16, 64):
        for mixed in (False, True):
            for excl in ((), _edges(n)):
                if excl and len(excl) == n and n > 1:
                    continue
                qt = 2 if mixed else 1
                bid = bytes(range(32)) if qt == 2 else None
                ap = b"" if psl else b"agg-param"
                j = make_job(n, psl, 32, 80, 48 if psl != 16 else 50, seed=n + psl, mixed_ct=mixed,
                             excluded=excl)
                want, windex, wninc = J.encode_req_host(ap, qt, bid, *job_args(j))
                body, index, ninc, err = _encode_raw(j, ap, qt, bid)
                assert body == want, (n, psl, mixed, excl)
                np.testing.assert_array_equal(index, windex)
                assert ninc == wninc and err == [0, 0]


def test_device_req_encode_leaves_out_a_report_with_ct_len_above_the_row():
    from janus_amd import dap as J
    n = 300
    j = make_job(n, 32, 32, 80, 48, seed=3)
    j["ct_len"][[0, 255, 299]] = [81, 0xFFFFFFFF, 1 << 31]
    body, index, ninc, err = _encode_raw(j, b"", 1, None)
    j["leader_status"][[0, 255, 299]] = 1
    want, windex, wninc = J.encode_req_host(b"", 1, None, *job_args(j))
    assert body == want and ninc == wninc == n - 3 and err == [3, 0]
    np.testing.assert_array_equal(index, windex)


def test_encode_req_device_wrapper():
    import torch
    from janus_amd import dap as J
    j = make_job(70, 0, 32, 64, 16, seed=5, excluded=(3, 4))
    t = [_dev(x, "cuda:0") for x in job_args(j)]
    res = J.encode_req_device(b"", 1, None, *t)
    torch.cuda.synchronize()
    want, windex, wninc = J.encode_req_host(b"", 1, None, *job_args(j))
    assert res["out"][:int(res["out_len"][0])].cpu().numpy().tobytes() == want
    np.testing.assert_array_equal(res["index"].cpu().numpy().view(np.uint32), windex)
    assert int(res["n_included"][0]) == wninc and not res["err"].any()


# ---- response decode --------------------------------------------------------------------------
def _decode_raw(body, index, ids, pml, n_included=None, dev="cuda:0", stream=None):
    """The C entry point with a sentinel row behind prep_msgs and prepare_error.  Returns
    (msgs, perr, flags)."""
    import torch
    from janus_amd import dap as J
    from janus_amd.prio3 import _stream, _tptr
    dev = torch.device(dev)
    n = len(ids)
    index = np.asarray(index, np.uint32)
    ninc = int((index != NONE).sum()) if n_included is None else n_included
    d_body = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
    if body:
        d_body[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    d_index, d_ids = _dev(index, dev), _dev(ids, dev)
    msgs = torch.full((n + 1, max(pml, 1)), SENT, dtype=torch.uint8, device=dev)
    pe = torch.full((n + 1,), SENT, dtype=torch.uint8, device=dev)
    flags = torch.full((2,), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(2 * (ninc + 2), dtype=torch.int32, device=dev)
    rc = J._lib().janus_dap_agg_job_resp_unpack_device(
        n, _tptr(d_index), _tptr(d_ids), ninc, _tptr(d_body), len(body), pml,
        _tptr(msgs) if pml else None, _tptr(pe), _tptr(flags), _tptr(scratch),
        _stream(stream, dev.index or 0))
    assert rc == 0
    torch.cuda.synchronize(dev)
    m, p = msgs.cpu().numpy(), pe.cpu().numpy()
    assert (m[n] == SENT).all() and p[n] == SENT and int(flags[1]) == -1
    if not pml:
        assert (m == SENT).all()
    return m[:n, :pml], p[:n], int(flags[0])


def _patterns(n):
    """Regular record mixes over n records ('c' Continue-Finish, 'f' Finished, int Reject)."""
    rng = np.random.default_rng(n)
    yield "no short", ["c"] * n
    yield "all reject", [int(x) for x in rng.integers(0, 10, n)]
    yield "all finished", ["f"] * n
    k = ["c"] * n
    k[0], k[-1] = 7, "f"
    yield "short first and last", k
    k = ["c"] * n
    for i in range(n // 3, min(n, n // 3 + 4)):
        k[i] = "f" if i & 1 else 4
    yield "adjacent short", k
    yield "random", [("c" if x < 0.8 else "f" if x < 0.85 else int(9 * x)) for x in rng.random(n)]
    if n > WIDTH:  # a short record as the last of a speculation window and as the first of the next
        for at in (WIDTH - 1, WIDTH):
            k = ["c"] * n
            k[at] = 2
            yield f"short at {at}", k


@pytest.mark.parametrize("n", NS)
def test_device_resp_decode_equals_host_on_regular_bodies(n):
    rng = np.random.default_rng(1000 + n)
    for pml in ((16, 0, 5) if n in (65, 257) else (16,)):
        for holes in (False, True):
            rows = n + (n // 4 + 2 if holes else 0)
            ids = rng.integers(0, 256, (rows, 16), dtype=np.uint8)
            index = index_with_holes(rows, rng.choice(rows, rows - n, replace=False)) if holes \
                else np.arange(n, dtype=np.uint32)
            inc = np.nonzero(index != NONE)[0]
            for name, kinds in _patterns(n):
                body = make_resp(ids[inc], kinds, pml, seed=n)
                want = host_decode(body, index, ids, pml)
                assert not isinstance(want, int), (name, want)
                msgs, pe, flags = _decode_raw(body, index, ids, pml)
                assert flags == 0, (name, pml, holes)
                np.testing.assert_array_equal(pe, want[1], err_msg=name)
                np.testing.assert_array_equal(msgs, want[0], err_msg=name)


def test_device_resp_decode_permuted_index_and_wrapper():
    import torch
    from janus_amd import dap as J
    rng = np.random.default_rng(4)
    n, pml = 200, 16
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.uint32)
    index = perm.copy()
    index[perm >= 150] = NONE
    order = np.argsort(np.where(index == NONE, n + 1, index))[:150]
    kinds = [("c" if x < 0.7 else 3) for x in rng.random(150)]
    body = make_resp(ids[order], kinds, pml, seed=4)
    want = host_decode(body, index, ids, pml)
    d_body = torch.zeros(len(body) + 4, dtype=torch.uint8, device="cuda")
    d_body[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
    msgs, pe, flags = J.unpack_resp_device(d_body, len(body), _dev(index, "cuda:0"),
                                           _dev(ids, "cuda:0"), 150, pml)
    torch.cuda.synchronize()
    assert int(flags[0]) == 0
    np.testing.assert_array_equal(pe.cpu().numpy(), want[1])
    np.testing.assert_array_equal(msgs.cpu().numpy(), want[0])


def test_device_resp_decode_flags():
    from janus_amd import dap as J
    pml, n = 16, 70
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    index = np.arange(n, dtype=np.uint32)
    base = ["c"] * n
    base[5], base[40] = 4, "f"
    good = make_resp(ids, base, pml, seed=1)
    assert _decode_raw(good, index, ids, pml)[2] == 0
    # each irregular shape: well-formed, so the host form decides (5 for that report)
    for msg in (dict(type="initialize", prep_share=b"s" * 16),
                dict(type="continue", prep_msg=b"m" * 16, prep_share=b"s" * 3),
                dict(type="finish", prep_msg=b"m" * 15), dict(type="finish", prep_msg=b"m" * 17)):
        for at in (0, 33, n - 1):
            kinds = list(base)
            kinds[at] = msg
            body = make_resp(ids, kinds, pml, seed=1)
            assert _decode_raw(body, index, ids, pml)[2] == J.RESP_IRREGULAR, (msg["type"], at)
            assert host_decode(body, index, ids, pml)[1][at] == 5
    # records that cannot decode: irregular and malformed
    rec6 = 4 + 5 * 42 + 18  # offset of record 6 (a Continue)
    for pos, val in ((rec6 + 16, 3), (rec6 + 21, 3), (rec6 + 25, 15), (rec6 + 20, 4)):
        bad = bytearray(good)
        bad[pos] = val
        fl = _decode_raw(bytes(bad), index, ids, pml)[2]
        assert fl == J.RESP_IRREGULAR | J.RESP_MALFORMED, (pos, fl)
        assert host_decode(bytes(bad), index, ids, pml) == -5
    # whole-response errors, each with its own bit
    bad = bytearray(good)
    bad[4 + 5 * 42 + 17] = 10
    assert _decode_raw(bytes(bad), index, ids, pml)[2] == J.RESP_REJECT_CODE
    bad = bytearray(good)
    bad[4 + 30 * 42 + 18 + 15] ^= 0x80  # the last ID byte of record 31
    assert _decode_raw(bytes(bad), index, ids, pml)[2] == J.RESP_ID
    few = make_resp(ids[:-1], base[:-1], pml, seed=1)
    assert _decode_raw(few, index, ids, pml)[2] & J.RESP_COUNT
    assert _decode_raw(few, index, ids, pml)[2] & ~J.RESP_COUNT == 0
    many = make_resp(np.vstack([ids, ids[:1]]), base + ["c"], pml, seed=1)
    assert _decode_raw(many, index, ids, pml)[2] == J.RESP_COUNT
    many = make_resp(np.vstack([ids, ids[:1]]), base + [3], pml, seed=1)
    assert _decode_raw(many, index, ids, pml)[2] == J.RESP_COUNT
    assert _decode_raw(good + b"\0", index, ids, pml)[2] == J.RESP_TRAILING
    assert _decode_raw(good[:-1], index, ids, pml)[2] == J.RESP_LISTLEN
    assert _decode_raw(good[:3], index, ids, pml)[2] == J.RESP_LISTLEN
    assert _decode_raw(b"", index, ids, pml)[2] == J.RESP_LISTLEN
    longer = struct.pack(">I", len(good) - 4 + 9) + good[4:]
    assert _decode_raw(longer, index, ids, pml)[2] == J.RESP_LISTLEN
    # a list cut inside its last record, with a consistent length: the record cannot decode
    cut = struct.pack(">I", len(good) - 4 - 7) + good[4:-7]
    assert _decode_raw(cut, index, ids, pml)[2] == J.RESP_IRREGULAR | J.RESP_MALFORMED
    # an empty response to an empty request
    assert _decode_raw(b"\0\0\0\0", np.full(3, NONE, np.uint32), ids[:3], pml)[2] == 0


def test_callers_device_and_stream():
    """Both device forms run on a side stream of the last GPU while the thread stays on GPU 0 (on
    a one-GPU machine the two coincide), back to back without synchronisation in between."""
    import torch
    from janus_amd import dap as J
    sd = torch.cuda.device_count() - 1
    torch.cuda.set_device(0)
    dev = torch.device("cuda", sd)
    n, pml = 300, 16
    j = make_job(n, 32, 32, 80, 48, seed=11, excluded=(0, 17, 299))
    t = [_dev(x, dev) for x in job_args(j)]
    index = expected_index(j["leader_status"])
    inc = np.nonzero(index != NONE)[0]
    kinds = ["c"] * len(inc)
    kinds[3], kinds[100] = 4, "f"
    body = make_resp(j["report_ids"][inc], kinds, pml, seed=2)
    d_body = torch.zeros(len(body) + 4, dtype=torch.uint8, device=dev)
    d_body[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    res = J.encode_req_device(b"", 1, None, *t, stream=side.cuda_stream)
    assert torch.cuda.current_device() == 0
    msgs, pe, flags = J.unpack_resp_device(d_body, len(body), res["index"], t[0], len(inc), pml,
                                           stream=side.cuda_stream)
    assert torch.cuda.current_device() == 0
    side.synchronize()
    want, windex, wninc = J.encode_req_host(b"", 1, None, *job_args(j))
    assert res["out"][:int(res["out_len"][0])].cpu().numpy().tobytes() == want
    assert int(res["n_included"][0]) == wninc == len(inc)
    hm, hp = host_decode(body, index, j["report_ids"], pml)
    assert int(flags[0]) == 0
    np.testing.assert_array_equal(pe.cpu().numpy(), hp)
    np.testing.assert_array_equal(msgs.cpu().numpy(), hm)

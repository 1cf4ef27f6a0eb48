"""The wire loop of query_h_body (prio3_prepare.hip) loads a gadget call's operands a trip ahead
of their use, over two register sets in a loop unrolled by two, and issues a sweep's finish
operands in two batches.  Every edge of that loop is put on the path here and the helper's
outputs -- statuses, prepare messages, aggregate, count -- must equal the CPU oracle's bit for
bit; there is no tolerance.

All shapes have P = 32 (16..31 gadget calls), the wire-polynomial length the fused k_prep_h and
k_slow_redo<32> take:

  length chunk calls
    64     4    16    fewest calls
    93     3    31    most calls; odd chunk, so the last sweep has one wire
    31     1    31    every sweep has an idle second wire
    50     3    17    last call two-thirds padding; odd trip count (one leading trip)
    61     2    31    last call half padding
   256    16    16    the flagship shape

200 reports are three full waves and a ragged one.  Small runs normally go to the lane-pair
kernel (k_prep_hp), so the tests turn that off (pair_max = 0) to reach k_prep_h.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_leader import _reports
from tests.test_gpu_parity import VK

pytestmark = pytest.mark.gpu

N = 200
SHAPES = [(64, 4), (93, 3), (31, 1), (50, 3), (61, 2), (256, 16)]
OOB_REPORT = 77  # the report whose segment id is out of range in the un-fused mode


def _cfg(length, chunk):
    return dict(kind="histogram", length=length, chunk_length=chunk)


@functools.lru_cache(maxsize=None)
def _case(length, chunk):
    """Reports of one shape with a few tampered ones, and the oracle's results for the two
    accept masks the modes use; computed once per shape and not modified afterwards."""
    from oracle.oracle import Oracle
    o = Oracle(**_cfg(length, chunk))
    d = o.gen_reports(VK, N, seed=1000 + 7 * length + chunk, n_threads=8)
    es = o.es
    lps, hs = d["leader_prep_shares"], d["helper_shares"]
    last = 2 * chunk  # the last wire's second verifier element: the last sweep's finish
    hs[11, 0] ^= 0x01            # a flipped share byte
    hs[139, hs.shape[1] - 1] ^= 0x40
    lps[3, 2 * es:3 * es] = 0xFF  # non-canonical leader elements: first sweep, second batch ...
    if chunk > 1:
        lps[66, 3 * es:4 * es] = 0xFF
    lps[130, last * es:(last + 1) * es] = 0xFF  # ... and the last sweep
    lps[197, :es] = 0xFF         # ... and the verifier's first element, in the ragged wave
    lps[5, -1] ^= 0x80           # a wrong joint-rand part
    lps[195, -16] ^= 0x01
    lps[20, es] ^= 0x01          # decide failures: a wire element of the first and last sweep
    lps[150, (last - 1) * es + 3] ^= 0x10
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    refs = {}
    for oob in (False, True):
        accept = np.ones(N, np.uint8)
        if oob:
            accept[OOB_REPORT] = 0
        refs[oob] = o.helper_batch(VK, d["nonces"], d["public_shares"], hs, lps,
                                   segment_ids=np.zeros(N, np.uint32), accept_mask=accept,
                                   n_segments=1, n_threads=8)
    st = refs[False][1]
    assert {0, 2, 3, 4} <= set(np.unique(st).tolist()), np.unique(st)
    return d, refs


def _run(length, chunk, opts, oob=False):
    import torch
    from janus_amd import prio3 as J
    d, refs = _case(length, chunk)
    ref_msgs, ref_status, ref_agg, ref_cnt = refs[oob]
    eng = J.HelperEngine(J.Prio3Histogram(length, chunk), VK, device=0)
    eng.set_option("pair_max", 0)
    for k, v in opts.items():
        eng.set_option(k, v)
    seg = np.zeros(N, np.uint32)
    if oob:
        seg[OOB_REPORT] = 4  # out of range: excluded from the aggregate and the count
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731 (a writable copy)
    sz = eng.sz
    msgs = torch.zeros((N, sz.prep_msg_len), dtype=torch.uint8, device=dev)
    status = torch.zeros(N, dtype=torch.uint8, device=dev)
    agg = torch.zeros((1, sz.agg_share_len), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    eng.prepare_aggregate_device(t(d["nonces"]), t(d["public_shares"]), t(d["helper_shares"]),
                                 t(d["leader_prep_shares"]), t(seg), 1, msgs, status)
    eng.aggregate_finish_device(status, t(np.ones(N, np.uint8)), agg, cnt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    np.testing.assert_array_equal(msgs.cpu().numpy()[:, :sz.prep_msg_len], ref_msgs)
    np.testing.assert_array_equal(cnt.cpu().numpy().astype(np.uint64), ref_cnt)
    np.testing.assert_array_equal(agg.cpu().numpy(), ref_agg)


@pytest.mark.parametrize("length,chunk", SHAPES)
def test_fused(length, chunk):
    """k_prep_h<true>: XOF, query and the fused accumulate in one launch."""
    _run(length, chunk, {"fuse_acc": 1})


@pytest.mark.parametrize("length,chunk", SHAPES)
def test_unfused_with_out_of_range_segment(length, chunk):
    """k_prep_h<false>: the specialised query (force_generic_query = 0) without the fused
    accumulate, one report's segment id out of range."""
    _run(length, chunk, {"fuse_acc": 0, "force_generic_query": 0}, oob=True)


@pytest.mark.parametrize("length,chunk", SHAPES)
def test_slow_redo(length, chunk):
    """Every report flagged: k_slow_redo<32> runs the same query body lane by lane."""
    _run(length, chunk, {"fuse_acc": 1, "force_slow_path": 1})


def test_leader_prepare_init():
    """k_leader_prep<32> (the LEADER form: no leader verifier loads) at (64, 4): prepare shares
    and statuses against the oracle's prepare_init."""
    from oracle.oracle import Oracle
    from janus_amd import prio3 as J
    cfg = _cfg(64, 4)
    o = Oracle(**cfg)
    d = _reports(o, cfg, N, seed=64)
    d["leader_shares"][9, :o.es] = 0xFF  # a non-canonical measurement-share element
    eng = J.HelperEngine(J.Prio3Histogram(64, 4), VK, device=0)
    ps, st, _ = eng.leader_prepare_init_batch(d["nonces"], d["public_shares"], d["leader_shares"])
    for i in range(N):
        rc, _, lps = o.prepare_init(VK, 0, d["nonces"][i].tobytes(),
                                    d["public_shares"][i].tobytes(), d["leader_shares"][i].tobytes())
        assert (st[i] == 0) == (rc == 0), i
        if rc == 0:
            assert ps[i].tobytes() == lps, i
    assert st[9] == 6 and int((st != 0).sum()) == 1

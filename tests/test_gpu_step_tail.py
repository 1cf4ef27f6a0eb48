"""GPU parity of the helper step's tail: the fused aggregate's finish (k_agg_parts: the wave
partials and the status scan in one grid; k_agg_final, which leaves the run's accumulators clean
for its next finish), the one-launch batch metadata (k_meta with a last-arriver reduction) and
the redo launch that strides over k_prep_h's list of flagged reports and zeroes the accumulators.

Every result is compared bit for bit with the CPU restatement (oracle.Oracle.helper_batch,
oracle.batch_metadata); the finish also with prio3_device_accumulate on the same statuses.
Shapes: Histogram(256, 16) and Histogram(100, 10) (M % 32 != 0: ragged slot range of the waves
role), n from {1, 63, 65, 1023, 1025, 2049 + 17} -- below / at / above one wave, one metadata
tile and one 32-wave chunk.
"""
import numpy as np
import pytest

from tests.conftest import CONFIGS
from tests.test_gpu_parity import VK, _engine, _oracle, _tamper

pytestmark = pytest.mark.gpu

NS = [1, 63, 65, 1023, 1025, 2049 + 17]
# the launches of one fused Histogram step (prepare_aggregate, aggregate_finish, batch_metadata)
STEP_LAUNCHES = [("k_prep_h", 1), ("k_slow_redo", 1), ("k_agg_parts", 1), ("k_agg_final", 1),
                 ("k_meta", 1)]
META_FAST_SEGS = 8  # launch_batch_metadata's one-launch bound (prio3_accumulate.hip)

_REPORTS = {}


def _reports(name, n, seed, tamper):
    """Generated (and tampered) reports, made once per shape and shared."""
    key = (name, n, seed, tamper)
    if key not in _REPORTS:
        o = _oracle(CONFIGS[name])
        d = o.gen_reports(VK, n, seed=seed, n_threads=8)
        if tamper:  # decide / decode failures, wrong joint-rand parts and public shares, bad seeds
            d = _tamper(o, d, np.random.default_rng(seed))
        _REPORTS[key] = d
    return _REPORTS[key]


def _segments(layout, n, rng):
    """(device segment ids, n_segments).  Ids >= n_segments exclude the report."""
    if layout == "one" or n < 8:
        return np.zeros(n, np.uint32), 1
    if layout == "runs":  # boundaries inside waves and inside 32-wave chunks
        S = 7
        seg = np.zeros(n, np.uint32)
        for c in np.sort(rng.choice(np.arange(1, n), S - 1, replace=False)):
            seg[c:] += 1
        return seg, S
    if layout == "random":  # no wave fuses: every report goes through the fix-up list
        return rng.integers(0, 4, n).astype(np.uint32), 4
    if layout == "oob":  # ids past n_segments, scattered and over whole waves
        seg = (np.arange(n) * 3 // n).astype(np.uint32)
        oob = rng.random(n) < 0.1
        oob[64:128] = True
        return np.where(oob, 3 + 5 + (np.arange(n) % 3), seg).astype(np.uint32), 3
    assert layout == "empty"  # segment 1 of 3 has no report
    return np.where(np.arange(n) < n // 2, 0, 2).astype(np.uint32), 3


def _masks(n, rng):
    return [np.ones(n, np.uint8), (rng.random(n) < 0.5).astype(np.uint8), np.zeros(n, np.uint8)]


def _finish_case(name, n, layout, seed, opts=None, force_slow=False, prepares=1, tamper=True):
    """prepare_aggregate once (or `prepares` times), then one finish per accept mask on the same
    run: all ones, a random half, all zeros."""
    import torch
    cfg = CONFIGS[name]
    o, eng = _oracle(cfg), _engine(cfg)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    if force_slow:
        eng.set_option("force_slow_path", 1)
    d = _reports(name, n, seed, tamper and n >= 63)
    rng = np.random.default_rng(seed + 1000)
    seg, S = _segments(layout, n, rng)
    oob = seg >= S
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sz = eng.sz
    msgs = torch.zeros((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    ins = (t(d["nonces"]), t(d["public_shares"]) if sz.public_share_len else None,
           t(d["helper_shares"]), t(d["leader_prep_shares"]), t(seg))
    for _ in range(prepares):
        eng.prepare_aggregate_device(*ins, S, msgs, status)
    any_rejected = False
    for accept in _masks(n, rng):
        ref_msgs, ref_status, ref_agg, ref_cnt = o.helper_batch(
            VK, d["nonces"], d["public_shares"], d["helper_shares"], d["leader_prep_shares"],
            segment_ids=np.where(oob, 0, seg).astype(np.uint32),
            accept_mask=np.where(oob, 0, accept).astype(np.uint8), n_segments=S, n_threads=8)
        # poisoned outputs: the finish must write every word, zero shares and counts included
        agg = torch.full((S, sz.agg_share_len), 0xA5, dtype=torch.uint8, device=dev)
        cnt = torch.full((S,), -1, dtype=torch.int64, device=dev)
        eng.aggregate_finish_device(status, t(accept), agg, cnt)
        agg2 = torch.full((S, sz.agg_share_len), 0x5A, dtype=torch.uint8, device=dev)
        cnt2 = torch.full((S,), -1, dtype=torch.int64, device=dev)
        eng.accumulate_device(n, status, ins[4], t(accept), S, agg2, cnt2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
        np.testing.assert_array_equal(msgs.cpu().numpy()[:, :sz.prep_msg_len], ref_msgs)
        np.testing.assert_array_equal(cnt.cpu().numpy().astype(np.uint64), ref_cnt)
        np.testing.assert_array_equal(agg.cpu().numpy(), ref_agg)
        np.testing.assert_array_equal(cnt2.cpu().numpy(), cnt.cpu().numpy())
        np.testing.assert_array_equal(agg2.cpu().numpy(), agg.cpu().numpy())
        any_rejected |= bool((ref_status != 0).any())
        if layout == "empty":
            assert ref_cnt[1] == 0 and not agg.cpu().numpy()[1].any()
    return any_rejected


@pytest.mark.parametrize("n", NS)
def test_finish_thrice_on_one_run(n):
    """Three finishes of one run with different accept masks: the final kernels leave agg64 and
    the count row clean, and the two fix-up counters alternate.  Tampered reports (decide and
    joint-rand failures) are in the fused wave sums and are subtracted."""
    rej = _finish_case("hist_256_c16", n, "runs", seed=100 + n)
    assert rej or n < 63


@pytest.mark.parametrize("n", [65, 2049 + 17])
def test_finish_thrice_short_histogram(n):
    """M = 100: M * 8 slots are no multiple of a waves-role block's 1024."""
    assert _finish_case("hist_100_c10", n, "runs", seed=200 + n)


@pytest.mark.parametrize("pair_max", [196608, 0])
@pytest.mark.parametrize("layout", ["one", "runs", "random", "oob", "empty"])
def test_finish_segment_layouts(layout, pair_max):
    """Every segment layout on both Histogram kernels: k_prep_hp (32-report waves, wshift 5, and
    k_agg_final_s for several segments) and k_prep_h (64-report waves, wshift 6)."""
    _finish_case("hist_256_c16", 2049 + 17, layout, seed=300, opts={"pair_max": pair_max})


@pytest.mark.parametrize("pair_max", [196608, 0])
def test_redo_launch_every_report_flagged(pair_max):
    """force_slow: every report is flagged -- on k_prep_h (pair_max 0) all 200 are appended to the
    redo list, more than one entry per lane of a wave and a ragged last wave; on k_prep_hp the
    redo launch scans the flags.  Either launch also zeroes the run's accumulators before its
    first finish."""
    _finish_case("hist_256_c16", 200, "runs", seed=400, force_slow=True,
                 opts={"pair_max": pair_max})


def test_redo_launch_none_flagged_and_prepared_twice():
    """An honest run (no report flagged), the same inputs prepared twice on one engine before the
    finishes, and a run with every report listed prepared twice and followed by a smaller honest
    run on the same stream: the redo launch put the list's counter back, or the later prepares
    would redo stale entries past their own reports."""
    _finish_case("hist_256_c16", 1025, "one", seed=410, tamper=False, opts={"pair_max": 0})
    _finish_case("hist_256_c16", 1025, "runs", seed=411, prepares=2, opts={"pair_max": 0})
    _finish_case("hist_256_c16", 200, "runs", seed=400, force_slow=True, prepares=2,
                 opts={"pair_max": 0})
    _finish_case("hist_256_c16", 63, "one", seed=163, opts={"pair_max": 0})


def test_redo_list_across_chunks():
    """Stream-overlapped chunks of k_prep_h append run-absolute columns to one list."""
    _finish_case("hist_256_c16", 1025, "runs", seed=411, force_slow=True,
                 opts={"pair_max": 0, "chunks": 3})


def test_finish_without_redo_launch():
    """A fused run whose prepare chain has no redo launch (the generic query) keeps its zeroing
    launch ahead of the first finish."""
    _finish_case("hist_256_c16", 1025, "runs", seed=420, opts={"force_generic_query": 1})


def test_step_launch_list():
    """One fused Histogram step is five launches (engine option timing = 2 counts them)."""
    import torch
    cfg = CONFIGS["hist_256_c16"]
    n = 1025
    eng = _engine(cfg)
    eng.set_option("pair_max", 0)  # k_prep_h, as the 1 Mi-report step
    d = _reports("hist_256_c16", n, 411, True)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sz = eng.sz
    msgs = torch.zeros((n, sz.prep_msg_len), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    agg = torch.zeros((1, sz.agg_share_len), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ck = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    iv = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    times = t(np.arange(n, dtype=np.int64) + 1_700_000_000)
    ins = (t(d["nonces"]), t(d["public_shares"]), t(d["helper_shares"]),
           t(d["leader_prep_shares"]), t(np.zeros(n, np.uint32)))
    accept = t(np.ones(n, np.uint8))
    for step in range(2):  # the first step may pay once-per-stream set-up; count the second
        eng.set_option("timing", 2)
        eng.timing_reset()
        eng.prepare_aggregate_device(*ins, 1, msgs, status)
        eng.aggregate_finish_device(status, accept, agg, cnt)
        eng.batch_metadata_device(ins[0], times, status, accept, ins[4], 1, ck, iv)
        torch.cuda.synchronize()
        got = [(k, v[1]) for k, v in eng.timing().items()]
    assert got == STEP_LAUNCHES


def _meta_case(n, S, seed, seg_mode, with_times=True, with_ck=True, streams=1):
    import torch
    from oracle.oracle import batch_metadata
    eng = _engine(CONFIGS["hist_256_c16"])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    calls = []
    for k in range(streams):
        rng = np.random.default_rng(seed + k)
        ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        times = rng.integers(1_600_000_000, 1_800_000_000, n).astype(np.int64)
        status = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), 0).astype(np.uint8)
        mask = (rng.random(n) < 0.8).astype(np.uint8)
        if seg_mode == "runs":  # whole tiles of one segment, tiles that mix two
            seg = (np.arange(n, dtype=np.uint64) * S // n).astype(np.uint32)
        else:  # every tile mixes segments; some ids out of range; segment 1 stays empty
            seg = rng.integers(0, S + 2, n).astype(np.uint32)
            if S > 2:
                seg[seg == 1] = 0
        ref_ck, ref_iv = batch_metadata(ids, times if with_times else None, status, mask, seg, S)
        ck = torch.full((S, 32), 0xA5, dtype=torch.uint8, device=dev) if with_ck else None
        iv = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        calls.append((t(ids), t(times) if with_times else None, t(status), t(mask), t(seg), ck, iv,
                      ref_ck, ref_iv))
    torch.cuda.synchronize()
    sts = [torch.cuda.Stream(device=dev) for _ in range(streams)] if streams > 1 else [None]
    for rep in range(2):  # twice: the ticket was put back
        for c, s in zip(calls, sts):
            eng.batch_metadata_device(c[0], c[1], c[2], c[3], c[4], S, c[5], c[6],
                                      stream=s.cuda_stream if s else None)
        torch.cuda.synchronize()
        for c in calls:
            if with_ck:
                np.testing.assert_array_equal(c[5].cpu().numpy(), c[7])
                c[5].fill_(0x3C)
            np.testing.assert_array_equal(c[6].cpu().numpy().astype(np.uint64), c[8])
            c[6].fill_(-1)
            if seg_mode == "random" and S > 2:
                assert not c[7][1].any() and not c[8][1].any()  # the empty segment: zero, (0, 0)


@pytest.mark.parametrize("n", NS)
def test_metadata_one_segment(n):
    _meta_case(n, 1, seed=500 + n, seg_mode="runs")


@pytest.mark.parametrize("S", [META_FAST_SEGS, META_FAST_SEGS + 1])
@pytest.mark.parametrize("seg_mode", ["runs", "random"])
def test_metadata_at_and_above_the_bound(S, seg_mode):
    """n_segments at the one-launch bound and one above it (the three-launch path); tiles of
    one segment, tiles that mix segments, ids out of range, a segment with no report."""
    _meta_case(2049 + 17, S, seed=600 + S, seg_mode=seg_mode)


def test_metadata_times_or_checksums_absent():
    _meta_case(1025, 3, seed=700, seg_mode="random", with_times=False)
    _meta_case(1025, 3, seed=701, seg_mode="random", with_ck=False)
    _meta_case(1025, META_FAST_SEGS + 1, seed=702, seg_mode="random", with_times=False)


def test_metadata_rows_from_many_blocks():
    """More blocks than the six sizes above give (40 tiles; the chip has 8 dies): the last
    block reads rows written on other dies, behind the release fence and the ticket."""
    _meta_case(40 * 1024 + 17, 2, seed=710, seg_mode="runs")
    _meta_case(40 * 1024 + 17, 5, seed=711, seg_mode="random")


def test_metadata_two_streams_back_to_back():
    """Two calls issued on two streams before either is synchronised: each stream has a ticket
    and rows of its own."""
    _meta_case(40 * 1024 + 17, 2, seed=720, seg_mode="runs", streams=2)
    _meta_case(2049 + 17, META_FAST_SEGS, seed=722, seg_mode="random", streams=2)

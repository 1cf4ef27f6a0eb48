"""prio3_job_index / prio3_device_job_index (include/janus_prio3.h, "Job index") against the
restatement of tests/job_index_ref.py: every output array and every info field, in the host form
and in the device form.  The device form runs on a side stream behind torch kernels that produce
its inputs on that stream, with no synchronisation before the call."""
import numpy as np
import pytest

from tests.job_index_ref import NO_SEGMENT, U64_MAX, job_index

pytestmark = pytest.mark.gpu

INFO = ("n_segments", "overflow", "n_duplicates", "first_duplicate", "n_closed", "n_time_errors")
ARRAYS = ("segment_ids", "segment_starts", "accept_mask", "reject", "duplicate")
FILL = 0x77  # the value every element of the device outputs holds before the call


@pytest.fixture(scope="module")
def eng():
    from janus_amd import prio3 as J
    e = J.HelperEngine(J.Prio3Count(), bytes(16), device=0)
    yield e
    e.close()


def _ids(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 16), dtype=np.uint8)


def _device_form(eng, ids, times, precision, max_segments, closed):
    import torch
    dev = torch.device("cuda", 0)
    n = ids.shape[0]
    new = lambda shape, dt: torch.full(shape, FILL, dtype=dt, device=dev)  # noqa: E731
    seg, acc, rej, dup = (new((n,), torch.int32), new((n,), torch.uint8), new((n,), torch.uint8),
                          new((n,), torch.uint8))
    starts = new((max_segments,), torch.int64)
    info = new((6,), torch.int32)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        # the inputs come out of kernels on this stream; nothing waits for them before the call
        d_ids = torch.from_numpy(ids ^ np.uint8(0x5A)).to(dev) ^ 0x5A
        d_t = None
        if times is not None:
            d_t = torch.from_numpy((times - np.uint64(1)).view(np.int64)).to(dev) + 1
        eng.job_index_device(d_ids, d_t, precision, max_segments, seg, acc, info,
                             closed_intervals=closed, segment_starts=starts, reject=rej,
                             duplicate=dup)
    torch.cuda.synchronize()
    out = dict(segment_ids=seg.cpu().numpy().view(np.uint32),
               segment_starts=starts.cpu().numpy().view(np.uint64), accept_mask=acc.cpu().numpy(),
               reject=rej.cpu().numpy(), duplicate=dup.cpu().numpy())
    out.update(zip(INFO, (int(v) for v in info.cpu().numpy().view(np.uint32))))
    return out


def _check(got, ref, what):
    for f in INFO:
        assert got[f] == ref[f], (what, f, got[f], ref[f])
    for a in ARRAYS:
        if ref[a] is None:  # time_precision 0: segment_starts is not written
            assert got[a] is None or (got[a] == np.uint64(FILL)).all(), what
        else:
            np.testing.assert_array_equal(got[a], ref[a], err_msg=f"{what}: {a}")


def _both(eng, ids, times, precision, max_segments, closed=None):
    """Runs the host and the device form, checks both against the restatement, returns the three."""
    ids = np.ascontiguousarray(ids, np.uint8)
    times = None if times is None else np.ascontiguousarray(times, np.uint64)
    ref = job_index(ids, times, precision, max_segments, closed)
    host = eng.job_index(ids, times, precision, max_segments, closed_intervals=closed)
    _check(host, ref, "host form")
    devf = _device_form(eng, ids, times, precision, max_segments, closed)
    _check(devf, ref, "device form")
    return ref, host, devf


# ---- sizes ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 4097, 20000])
def test_sizes(eng, n):
    """Wave edge, workgroup edge, many workgroups on the same slots: five buckets (one closed),
    a time error and duplicates at both ends."""
    rng = np.random.default_rng(n)
    times = (rng.integers(3, 8, n) * 300 + rng.integers(0, 300, n)).astype(np.uint64)
    ids = _ids(n, n)
    if n >= 2:
        ids[n - 1] = ids[0]
    if n >= 65:
        ids[33] = ids[32]
        times[n // 2] = U64_MAX
    ref, _, _ = _both(eng, ids, times, 300, 8, [(1500, 300)])
    if n >= 255:
        assert ref["n_segments"] == 5 and ref["n_closed"] > 0
    if n >= 65:
        assert ref["n_duplicates"] == 2 and ref["n_time_errors"] == 1


# ---- buckets ----
def _bucket_cases():
    rng = np.random.default_rng(11)
    c = {}
    c["one_bucket"] = ((90_000 + rng.integers(0, 300, 257)).astype(np.uint64), 300, 4)
    c["two_alternating"] = ((np.arange(257) % 2 * 300 + 600).astype(np.uint64), 300, 4)
    c["all_distinct_4096"] = (rng.permutation(4096).astype(np.uint64) * 300 + 7, 300, 4096)
    eight = (rng.integers(0, 8, 300) * 300).astype(np.uint64)
    eight[:8] = np.arange(8, dtype=np.uint64)[::-1] * 300
    c["max_segments_reached"] = (eight, 300, 8)
    nine = eight.copy()
    nine[150] = 8 * 300
    c["max_segments_exceeded"] = (nine, 300, 8)
    c["exceeded_by_far"] = (np.arange(20000, dtype=np.uint64) * 300, 300, 5)
    # precision 1: start = t, so the starts differ exactly where the times do
    hi = np.array([5, 5 + (1 << 32), 5 + (1 << 33), 5 + (1 << 63), 5 + (1 << 32) + (1 << 33)],
                  np.uint64)
    c["differ_above_bit_32"] = (hi[rng.integers(0, 5, 300)], 1, 8)
    q = np.uint64(123_456_789_012)
    c["differ_in_quotient_bit_0"] = (np.where(np.arange(300) % 3 == 0, q, q ^ np.uint64(1)) *
                                     np.uint64(300) + np.uint64(299), 300, 2)
    c["precision_300"] = (rng.integers(0, 3000, 500).astype(np.uint64), 300, 16)
    c["precision_1"] = (rng.integers(0, 40, 500).astype(np.uint64), 1, 64)
    c["precision_2_64_minus_1"] = (np.array([0, 5, U64_MAX - 1, U64_MAX], np.uint64), U64_MAX, 2)
    # 2^64 - 1 = 300 q + 15: the bucket at 300 q overflows, the one at 300 (q - 1) is the last
    edge = np.array([0, 299, U64_MAX, 300, U64_MAX - 15, U64_MAX - 16, 0], np.uint64)
    c["edge_times"] = (edge, 300, 4)
    c["fixed_size"] = (None, 0, 3)
    c["fixed_size_with_times"] = (rng.integers(0, 3000, 70).astype(np.uint64), 0, 1)
    return c


BUCKETS = _bucket_cases()


@pytest.mark.parametrize("name", list(BUCKETS))
def test_buckets(eng, name):
    times, precision, max_segments = BUCKETS[name]
    n = 70 if times is None else len(times)
    ref, host, devf = _both(eng, _ids(n, 3), times, precision, max_segments,
                            [(600, 300)] if precision == 300 else None)
    if "exceeded" in name:
        assert ref["overflow"] == 1 and ref["n_segments"] == max_segments + 1
        for got in (host, devf):  # in bounds for the calls queued behind this one
            s = got["segment_ids"]
            assert ((s < max_segments) | (s == NO_SEGMENT)).all()
            assert not got["accept_mask"][s == NO_SEGMENT].any()
    elif name == "all_distinct_4096":
        assert ref["n_segments"] == 4096 and ref["overflow"] == 0
    elif name == "edge_times":
        assert ref["n_time_errors"] == 2 and ref["segment_starts"][2] == U64_MAX - 315


# ---- closed batches ----
def _closed_cases():
    rng = np.random.default_rng(12)
    many = np.stack([rng.integers(10_000, 1 << 40, 1024), rng.integers(1, 1000, 1024)], 1)
    many[700] = (900, 1)  # one of the 1024 matches the bucket at 900
    return {
        "k0": [],
        "null": None,
        "one_bucket": [(600, 300)],
        "ends_at_a_start": [(300, 300)],       # [300, 600): bucket 300 closed, 600 open
        "ends_before_a_start": [(0, 300)],     # no report below 300
        "all": [(0, 1 << 20)],
        "all_to_the_end": [(1, U64_MAX)],      # an end past 2^64 - 1 does not wrap around
        "k1024": many.astype(np.uint64),
        "no_match": [(301, 299), (1500, 10**6)],
    }


CLOSED = _closed_cases()


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed(eng, name):
    rng = np.random.default_rng(13)
    times = (rng.integers(1, 5, 300) * 300 + rng.integers(0, 300, 300)).astype(np.uint64)
    ref, _, _ = _both(eng, _ids(300, 4), times, 300, 8, CLOSED[name])
    closed_buckets = {"k0": 0, "null": 0, "one_bucket": 1, "ends_at_a_start": 1,
                      "ends_before_a_start": 0, "all": 4, "all_to_the_end": 4, "k1024": 1,
                      "no_match": 0}[name]
    seg_closed = np.unique(ref["segment_ids"][ref["reject"] != 0])
    assert len(seg_closed) == closed_buckets and ref["n_segments"] == 4


# ---- report IDs ----
def _id_cases():
    c = {}
    n = 20000
    c["no_duplicates"] = _ids(n, 20)

    def pair(a, b, size=n):
        ids = _ids(size, 21)
        ids[b] = ids[a]
        return ids
    c["pair_in_one_wave"] = pair(130, 150)
    c["pair_across_two_waves"] = pair(60, 70)
    c["pair_across_two_workgroups"] = pair(200, 19000)
    c["pair_first_and_last"] = pair(0, n - 1)
    three = _ids(300, 22)
    three[7] = three[9] = three[3]
    c["three_copies"] = three
    sixty_four = _ids(n, 23)
    at = np.random.default_rng(24).choice(n, 64, replace=False)
    sixty_four[at] = sixty_four[at[0]]
    c["64_copies"] = sixty_four
    c["all_equal"] = np.tile(_ids(1, 25), (4097, 1))
    half = np.tile(_ids(1, 26), (600, 1))
    half[:, 8:12] = np.arange(600, dtype=np.uint32).view(np.uint8).reshape(600, 4)
    half[300:, 8:] = half[:300, 8:]  # rows r and r + 300 are equal
    half[450:, 15] ^= 0x80           # ... except those from 450 on
    c["same_first_8_bytes"] = half
    c["same_last_8_bytes"] = np.ascontiguousarray(np.roll(half, 8, axis=1))
    # 4,096 IDs that differ from one base ID in one byte only: byte i // 256 XOR i % 256 (the 16
    # rows with i % 256 == 0 are the base ID itself, so 15 of them are duplicates)
    one_byte = np.tile(_ids(1, 27), (4096, 1))
    one_byte[np.arange(4096), np.arange(4096) // 256] ^= (np.arange(4096) % 256).astype(np.uint8)
    c["one_byte_apart"] = one_byte
    ends = _ids(200, 28)
    ends[[3, 77, 140]] = 0
    ends[[4, 78, 199]] = 0xFF
    c["all_zero_and_all_ff"] = ends
    return c


IDS = _id_cases()


@pytest.mark.parametrize("name", list(IDS))
def test_ids(eng, name):
    ids = IDS[name]
    n = ids.shape[0]
    times = (np.arange(n) % 3 * 300).astype(np.uint64)
    runs = [_both(eng, ids, times, 300, 4, [(300, 300)]) for _ in range(2)]
    ref = runs[0][0]
    for form in (1, 2):  # two runs give byte-identical outputs
        for f in INFO:
            assert runs[0][form][f] == runs[1][form][f]
        for a in ARRAYS:
            assert runs[0][form][a].tobytes() == runs[1][form][a].tobytes(), (name, a)
    expect = {"no_duplicates": (0, 0xFFFFFFFF), "pair_in_one_wave": (1, 150),
              "pair_across_two_waves": (1, 70), "pair_across_two_workgroups": (1, 19000),
              "pair_first_and_last": (1, n - 1), "three_copies": (2, 7), "all_equal": (4096, 1),
              "same_first_8_bytes": (150, 300), "same_last_8_bytes": (150, 300),
              "one_byte_apart": (15, 256), "all_zero_and_all_ff": (4, 77)}
    if name in expect:
        assert (ref["n_duplicates"], ref["first_duplicate"]) == expect[name]
    if name == "64_copies":
        assert ref["n_duplicates"] == 63
    # the accept mask does not depend on the duplicates
    np.testing.assert_array_equal(ref["accept_mask"], (times != 300).astype(np.uint8))


# ---- arguments ----
def test_arguments(eng):
    ids, times = _ids(10, 30), np.arange(10, dtype=np.uint64) * 100
    for max_segments, closed in ((0, None), (4097, None), (4, np.zeros((1025, 2), np.uint64))):
        with pytest.raises(RuntimeError, match="rc=-1"):
            eng.job_index(ids, times, 300, max_segments, closed_intervals=closed)
    ref = job_index(ids, times, 300, 4, [(0, 300)])
    got = eng.job_index(ids, times, 300, 4, closed_intervals=[(0, 300)], with_starts=False,
                        with_reject=False, with_duplicate=False)  # NULL optional outputs
    assert got["segment_starts"] is None and got["reject"] is None and got["duplicate"] is None
    for f in INFO:
        assert got[f] == ref[f], f
    np.testing.assert_array_equal(got["segment_ids"], ref["segment_ids"])
    np.testing.assert_array_equal(got["accept_mask"], ref["accept_mask"])


def test_device_form_without_optional_outputs(eng):
    import torch
    dev = torch.device("cuda", 0)
    ids, times = _ids(300, 31), (np.arange(300) % 4 * 300).astype(np.uint64)
    ids[200] = ids[100]
    ref = job_index(ids, times, 300, 4, [(600, 300)])
    seg = torch.zeros(300, dtype=torch.int32, device=dev)
    acc = torch.zeros(300, dtype=torch.uint8, device=dev)
    info = torch.zeros(6, dtype=torch.int32, device=dev)
    eng.job_index_device(torch.from_numpy(ids).to(dev),
                         torch.from_numpy(times.view(np.int64)).to(dev), 300, 4, seg, acc, info,
                         closed_intervals=[(600, 300)])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(seg.cpu().numpy().view(np.uint32), ref["segment_ids"])
    np.testing.assert_array_equal(acc.cpu().numpy(), ref["accept_mask"])
    assert info.cpu().numpy().view(np.uint32).tolist() == [ref[f] for f in INFO]


# ---- the device-resident chain ----
def test_chain_into_prepare_aggregate(oracle_lib):
    """Histogram(10, 3), 300 reports in 3 buckets, one closed, one report ID duplicated:
    job_index_device -> prepare_aggregate_device (n_segments = max_segments = 8) ->
    aggregate_finish_device -> batch_metadata_device, all on one stream without a host round trip,
    against the same three calls fed the restatement's segment ids and accept mask.  Segments 3-7
    are empty (count 0, checksum 0, Interval::EMPTY).
    Path: Histogram(10, 3) is below the fused accumulate's size (PrepPlan::fusable wants a measurement
    of at least 19 elements), so prio3_device_prepare_aggregate defers the sum to the finish call's
    one-pass segmented reduction (run_accumulate, k_acc_seg); with 8 segments that is its
    8-segments-per-block instance, where 2-4 segments take the 4-segment one.  The existing
    multi-segment device tests (tests/test_gpu_fused_tiles.py) run Histogram(256, 16) through the
    fused path (k_agg_waves / k_agg_fix / k_agg_final_s) instead."""
    import torch
    from janus_amd import prio3 as J
    vk = bytes(range(16))
    n, S = 300, 8
    o = oracle_lib.Oracle("histogram", length=10, chunk_length=3)
    d = o.gen_reports(vk, n, seed=9, n_threads=4)
    d = {k: np.array(d[k]) for k in ("nonces", "public_shares", "helper_shares",
                                     "leader_prep_shares")}
    for a in d.values():
        a[250] = a[40]  # the same report twice: one duplicated ID
    d["leader_prep_shares"][17, 16] ^= 1  # and one report that fails its VDAF
    rng = np.random.default_rng(14)
    times = ((rng.integers(0, 3, n) * 2 + 5) * 300 + rng.integers(0, 300, n)).astype(np.uint64)
    closed = [(2100, 300)]  # the middle bucket
    ref = job_index(d["nonces"], times, 300, S, closed)
    assert ref["n_segments"] == 3 and ref["n_closed"] > 50 and ref["n_duplicates"] == 1
    eng = J.HelperEngine(J.Prio3Histogram(10, 3), vk, device=0)
    dev = torch.device("cuda", 0)
    sz = eng.sz
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ins = [t(d[k]) for k in ("nonces", "public_shares", "helper_shares", "leader_prep_shares")]
    d_times = t(times.view(np.int64))

    def chain(index):
        msgs = torch.zeros((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        agg = torch.full((S, sz.agg_share_len), FILL, dtype=torch.uint8, device=dev)
        cnt = torch.full((S,), FILL, dtype=torch.int64, device=dev)
        cks = torch.full((S, 32), FILL, dtype=torch.uint8, device=dev)
        ivs = torch.full((S, 2), FILL, dtype=torch.int64, device=dev)
        seg, acc = index()
        eng.prepare_aggregate_device(*ins, seg, S, msgs, status)
        eng.aggregate_finish_device(status, acc, agg, cnt)
        eng.batch_metadata_device(ins[0], d_times, status, acc, seg, S, cks, ivs)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (agg, cnt, cks, ivs, status, seg, acc)]

    dup = torch.zeros(n, dtype=torch.uint8, device=dev)
    info = torch.zeros(6, dtype=torch.int32, device=dev)

    def on_device():
        seg = torch.full((n,), FILL, dtype=torch.int32, device=dev)
        acc = torch.full((n,), FILL, dtype=torch.uint8, device=dev)
        eng.job_index_device(ins[0], d_times, 300, S, seg, acc, info, closed_intervals=closed,
                             duplicate=dup)
        return seg, acc

    got = chain(on_device)
    want = chain(lambda: (t(ref["segment_ids"].view(np.int32)), t(ref["accept_mask"])))
    for g, w, what in zip(got, want, ("aggregate shares", "counts", "checksums", "intervals",
                                      "status", "segment ids", "accept mask")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    agg, cnt, cks, ivs, status = got[:5]
    counted = (status == 0) & (ref["accept_mask"] == 1)
    assert status[17] != 0 and int(cnt.sum()) == int(counted.sum())
    assert cnt[1] == 0 and cnt[0] > 0 and cnt[2] > 0  # the closed bucket counts nothing
    assert not cnt[3:].any() and not agg[3:].any() and not cks[3:].any() and not ivs[3:].any()
    np.testing.assert_array_equal(dup.cpu().numpy(), ref["duplicate"])
    assert info.cpu().numpy().view(np.uint32).tolist() == [ref[f] for f in INFO]
    eng.close()

"""The job index restatement (tests/job_index_ref.py) against hand-written cases: it is the
expected value of every GPU test of prio3_job_index (tests/test_gpu_job_index.py), so its own
reading of the contract (include/janus_prio3.h, "Job index") is pinned here without the library."""
import numpy as np

from tests.job_index_ref import NO_SEGMENT, REJECT_BATCH_COLLECTED, U64_MAX, job_index


def _ids(n):
    ids = np.zeros((n, 16), np.uint8)
    ids[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    ids[:, 15] = 0xA5
    return ids


def test_three_copies_mark_the_later_two():
    ids = _ids(12)
    ids[7] = ids[3]
    ids[9] = ids[3]
    r = job_index(ids, np.full(12, 1000, np.uint64), 300, 4)
    assert r["duplicate"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0]
    assert (r["n_duplicates"], r["first_duplicate"]) == (2, 7)
    assert r["accept_mask"].tolist() == [1] * 12  # the mask does not depend on duplicates
    assert job_index(_ids(5), np.zeros(5, np.uint64), 300, 4)["first_duplicate"] == 0xFFFFFFFF


def test_closed_interval_end_is_exclusive():
    times = np.array([300, 600, 899, 900, 1200], np.uint64)
    r = job_index(_ids(5), times, 300, 8, closed_intervals=[(600, 300)])  # [600, 900)
    assert r["segment_starts"].tolist() == [300, 600, 900, 1200, 0, 0, 0, 0]
    assert r["segment_ids"].tolist() == [0, 1, 1, 2, 3]
    assert r["accept_mask"].tolist() == [1, 0, 0, 1, 1]
    assert r["reject"].tolist() == [0, REJECT_BATCH_COLLECTED, REJECT_BATCH_COLLECTED, 0, 0]
    assert REJECT_BATCH_COLLECTED == 0x80
    assert (r["n_segments"], r["n_closed"], r["overflow"]) == (4, 2, 0)
    # an interval that ends exactly at a bucket's start does not close it
    r = job_index(_ids(5), times, 300, 8, closed_intervals=[(0, 300)])
    assert r["accept_mask"].tolist() == [1] * 5 and r["n_closed"] == 0


def test_time_below_precision_starts_at_zero():
    r = job_index(_ids(3), np.array([0, 1, 299], np.uint64), 300, 2)
    assert r["segment_ids"].tolist() == [0, 0, 0]
    assert r["segment_starts"].tolist() == [0, 0] and r["n_segments"] == 1


def test_last_second_is_a_time_error():
    # 2^64 - 1 = 300 * q + 15: start = 2^64 - 16, and start + 300 overflows (Interval::new)
    r = job_index(_ids(2), np.array([U64_MAX, 600], np.uint64), 300, 2)
    assert r["segment_ids"].tolist() == [NO_SEGMENT, 0]
    assert r["accept_mask"].tolist() == [0, 1] and r["reject"].tolist() == [0, 0]
    assert (r["n_time_errors"], r["n_segments"]) == (1, 1)
    assert r["segment_starts"].tolist() == [600, 0]


def test_precision_one():
    times = np.array([5, 3, 5, U64_MAX - 1, U64_MAX], np.uint64)
    r = job_index(_ids(5), times, 1, 4)
    assert r["segment_starts"].tolist() == [3, 5, U64_MAX - 1, 0]
    assert r["segment_ids"].tolist() == [1, 0, 1, 2, NO_SEGMENT]  # 2^64 - 1 + 1 overflows
    assert (r["n_segments"], r["n_time_errors"]) == (3, 1)


def test_overflow_at_max_segments_plus_one():
    times = np.arange(5, dtype=np.uint64) * 300
    r = job_index(_ids(5), times, 300, 5)
    assert (r["n_segments"], r["overflow"]) == (5, 0)
    assert r["segment_ids"].tolist() == [0, 1, 2, 3, 4]
    r = job_index(_ids(5), times, 300, 4, closed_intervals=[(0, 300)])
    assert (r["n_segments"], r["overflow"], r["n_closed"]) == (5, 1, 0)
    assert r["segment_ids"].tolist() == [NO_SEGMENT] * 5  # in bounds for the calls queued behind
    assert r["accept_mask"].tolist() == [0] * 5 and r["reject"].tolist() == [0] * 5
    assert r["segment_starts"].tolist() == [0] * 4


def test_segments_ascend_on_shuffled_times():
    rng = np.random.default_rng(5)
    buckets = np.array([9000, 300, 300 << 32, 0, 600], np.uint64)
    which = rng.integers(0, 5, 200)
    times = buckets[which] + rng.integers(0, 300, 200).astype(np.uint64)
    r = job_index(_ids(200), times, 300, 8)
    assert r["segment_starts"].tolist() == [0, 300, 600, 9000, 300 << 32, 0, 0, 0]
    assert r["segment_ids"].tolist() == [[3, 1, 4, 0, 2][w] for w in which]


def test_fixed_size_task():
    r = job_index(_ids(4), None, 0, 3, closed_intervals=[(0, 1000)])
    assert r["segment_ids"].tolist() == [0] * 4 and r["accept_mask"].tolist() == [1] * 4
    assert r["segment_starts"] is None and (r["n_segments"], r["n_closed"]) == (1, 0)
    r = job_index(_ids(0), np.zeros(0, np.uint64), 300, 3)
    assert (r["n_segments"], r["n_duplicates"], r["first_duplicate"]) == (0, 0, 0xFFFFFFFF)
    assert r["segment_starts"].tolist() == [0, 0, 0]

"""A numpy / Python-set restatement of the job index (prio3_job_index, include/janus_prio3.h),
written from the reference and independent of the library:

  - batch identifier: TimeInterval::to_batch_identifier (aggregator_core/src/query_type.rs:72-82)
    = Interval::new(time.to_batch_interval_start(precision), precision), with
    to_batch_interval_start = t - t % precision (core/src/time.rs:207-224); Interval::new fails
    when start + duration overflows a u64.  The writer indexes the distinct identifiers
    (by_batch_identifier_index, aggregator/src/aggregator/aggregation_job_writer.rs:598); the
    index used here is the ascending one, numpy.unique's;
  - closed batches: fail_report_aggregations_for_collected_batches (aggregation_job_writer.rs:
    540-588) fails the reports of a batch that no longer accepts aggregations with
    PrepareError::BatchCollected = 0 (messages/src/lib.rs:2186), here 0x80 | 0;
  - duplicate report IDs: the HashSet over every PrepareInit of the request
    (aggregator/src/aggregator.rs:1765-1773); here per report: an earlier index has the same ID.
"""
import numpy as np

U64_MAX = (1 << 64) - 1
NO_SEGMENT = 0xFFFFFFFF
REJECT_BATCH_COLLECTED = 0x80 | 0


def job_index(report_ids, times, time_precision, max_segments, closed_intervals=None):
    """Returns the dict HelperEngine.job_index returns (segment_starts: None for precision 0)."""
    ids = np.ascontiguousarray(report_ids, np.uint8).reshape(-1, 16)
    n = ids.shape[0]
    closed_intervals = [] if closed_intervals is None else [
        (int(a), int(d)) for a, d in np.asarray(closed_intervals, np.uint64).reshape(-1, 2)]
    seg = np.full(n, NO_SEGMENT, np.uint32)
    accept = np.zeros(n, np.uint8)
    reject = np.zeros(n, np.uint8)
    info = dict(n_segments=0, overflow=0, n_closed=0, n_time_errors=0)
    starts_out = None
    if time_precision == 0:  # fixed size: one batch, nothing closed here
        seg[:] = 0
        accept[:] = 1
        info["n_segments"] = 1 if n else 0
    else:
        t = np.ascontiguousarray(times, np.uint64)
        assert t.shape == (n,)
        start = t - t % np.uint64(time_precision)
        err = start > np.uint64(U64_MAX - time_precision)  # Interval::new: start + precision
        info["n_time_errors"] = int(err.sum())
        uniq, inverse = np.unique(start[~err], return_inverse=True)
        starts_out = np.zeros(max_segments, np.uint64)
        if len(uniq) > max_segments:
            info["overflow"] = 1
            info["n_segments"] = max_segments + 1
        else:
            info["n_segments"] = len(uniq)
            starts_out[:len(uniq)] = uniq
            seg[~err] = inverse.astype(np.uint32)
            closed_seg = np.array([any(a <= int(s) < a + d for a, d in closed_intervals)
                                   for s in uniq], bool)
            closed = np.zeros(n, bool)
            closed[~err] = closed_seg[inverse] if len(uniq) else False
            accept[~err & ~closed] = 1
            reject[closed] = REJECT_BATCH_COLLECTED
            info["n_closed"] = int(closed.sum())
    seen = set()
    duplicate = np.zeros(n, np.uint8)
    for i in range(n):
        key = ids[i].tobytes()
        if key in seen:
            duplicate[i] = 1
        seen.add(key)
    dup_at = np.flatnonzero(duplicate)
    info["n_duplicates"] = len(dup_at)
    info["first_duplicate"] = int(dup_at[0]) if len(dup_at) else 0xFFFFFFFF
    return dict(segment_ids=seg, segment_starts=starts_out, accept_mask=accept, reject=reject,
                duplicate=duplicate, **info)

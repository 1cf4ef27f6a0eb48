// jobs_driver.cpp -- measurement harness for the production call shape (bench.py --role jobs):
// C host threads, each playing one Janus rayon worker that runs whole aggregation jobs
// (/root/reference/aggregator/src/aggregator.rs:2100-2123) of `job_size` reports
// (binaries/aggregation_job_creator.rs:63-64, default 100-500), calling the C ABI exactly as the
// FFI crate of INTEGRATION.md would: prio3_helper_prepare_batch (host buffers, PCIe included),
// then prio3_accumulate into the job's batch aggregation, then prio3_batch_free.  The leader and
// HPKE forms do the same for the leader's prepare_init / prepare_next
// (aggregation_job_driver.rs:397-415, 677-691, spawned per job at :449-462) and the helper's
// input-share open (aggregator.rs:1847-1890).
// Not part of the engine: a separate library (libjanus_jobs.so) that links libjanus_prio3.so.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/janus_hpke.h"
#include "../../include/janus_prio3.h"

namespace {
// A persistent pool, as Janus's rayon pool is (aggregator/src/binary_utils.rs:514-518): its
// threads are created by the first call that needs them (the lines' warmup run) and parked on a
// condition variable between calls, so a timed call neither creates threads nor pays each new
// thread's first HIP calls.  r06 timed 128 fresh threads per call: their creation added 4-9 ms to
// a ~55 ms region (r06o), and spinning while parked burnt CPU quota (r06v).
struct Pool {
  std::mutex mu;
  std::condition_variable cv, done;
  std::function<void()> work;
  uint64_t gen = 0;
  int threads = 0, want = 0, active = 0;
};
Pool& pool() {
  static Pool* p = new Pool();  // never destroyed: its threads stay parked until exit
  return *p;
}

// `work` once on each of `threads` pool threads; returns elapsed seconds
double run_threads(int threads, const std::function<void()>& work) {
  Pool& P = pool();
  // one caller at a time: the pool has one work slot, and a second caller arriving inside a run
  // would replace the work its threads are still picking up
  static std::mutex call_mu;
  std::lock_guard<std::mutex> call(call_mu);
  std::unique_lock<std::mutex> lk(P.mu);
  while (P.threads < threads) {
    const int idx = P.threads++;
    std::thread([&P, idx] {
      uint64_t seen = 0;
      std::unique_lock<std::mutex> l(P.mu);
      for (;;) {
        P.cv.wait(l, [&] { return P.gen != seen; });
        seen = P.gen;
        if (idx >= P.want) continue;
        const std::function<void()> w = P.work;
        l.unlock();
        w();
        l.lock();
        if (--P.active == 0) P.done.notify_all();
      }
    }).detach();
  }
  P.work = work;
  P.want = threads;
  P.active = threads;
  P.gen++;
  const auto t0 = std::chrono::steady_clock::now();
  P.cv.notify_all();
  P.done.wait(lk, [&] { return P.active == 0; });
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  P.work = nullptr;
  return dt;
}

// `threads` workers taking jobs 0..jobs-1 in order; returns elapsed seconds (< 0: a call failed)
template <class F>
double run_pool(int threads, int jobs, F job) {
  std::atomic<int> next{0}, failed{0};
  const double dt = run_threads(threads, [&] {
    for (;;) {
      const int j = next.fetch_add(1);
      if (j >= jobs) return;
      if (!job(j)) failed = 1;
    }
  });
  return failed ? -1.0 : dt;
}

// The same with tickets: each worker keeps up to K jobs outstanding -- it submits until it holds
// K tickets, then waits the oldest and submits the next.  submit(j, slot, &ticket) starts job j
// with the worker's output slot `slot` (0..K-1, free again once its ticket is waited).
template <class F>
double run_pool_tickets(int threads, int jobs, int K, F submit) {
  std::atomic<int> next{0}, failed{0};
  if (K < 1) K = 1;
  const double dt = run_threads(threads, [&] {
    std::vector<prio3_ticket*> ring((size_t)K, nullptr);
    size_t head = 0, held = 0;  // the oldest ticket's slot, tickets held
    auto wait_oldest = [&] {
      if (prio3_ticket_wait(ring[head]) != PRIO3_OK) failed = 1;
      ring[head] = nullptr;
      head = (head + 1) % (size_t)K;
      held--;
    };
    for (;;) {
      const int j = next.fetch_add(1);
      if (j >= jobs) break;
      if (held == (size_t)K) wait_oldest();
      const size_t slot = (head + held) % (size_t)K;
      prio3_ticket* t = nullptr;
      if (!submit(j, (int)slot, &t) || !t) {
        failed = 1;
        continue;
      }
      ring[slot] = t;
      held++;
    }
    while (held) wait_oldest();
  });
  return failed ? -1.0 : dt;
}
}  // namespace

extern "C" {

// engines[n_engines] (tasks of one VDAF instance, sizes *szp); one report pool per engine (its
// own verify key): nonces[n_engines * pool][16], pub[..][psl], helper[..][hsl], lps[..][L].  Job j
// runs on engine t = j % n_engines over `job_size` consecutive reports of pool t starting at
// ((j / n_engines) * job_size) % (pool - job_size + 1).  status_out[jobs * job_size],
// counts_out[jobs] and agg_out[jobs][agg_len] receive every job's verdicts, count and aggregate
// share.  combined = 0: prio3_helper_prepare_batch + prio3_accumulate + prio3_batch_free per job
// (two round trips through the executor); 1: prio3_helper_prepare_aggregate_batch (one).
// Returns elapsed seconds (< 0: a call failed).
double janus_jobs_run(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                      int threads, int jobs, int job_size,
                      uint32_t pool, const uint8_t* nonces, const uint8_t* pub,
                      const uint8_t* helper, const uint8_t* lps, uint8_t* status_out,
                      uint64_t* counts_out, uint8_t* agg_out, int combined) {
  const prio3_sizes_t sz = *szp;  // the instance's sizes (prio3_sizes; all engines share it)
  const uint32_t span = pool - (uint32_t)job_size + 1;
  return run_pool(threads, jobs, [&](int j) {
    thread_local std::vector<uint8_t> msgs;
    msgs.resize((size_t)job_size * (sz.prep_msg_len ? sz.prep_msg_len : 1));
    const uint32_t t = (uint32_t)(j % n_engines);
    const uint32_t r0 = t * pool + (uint32_t)(((uint64_t)(j / n_engines) * job_size) % span);
    const uint8_t* jp = sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr;
    uint8_t* agg = agg_out + (size_t)sz.agg_share_len * j;
    uint64_t cnt = 0;
    int rc;
    if (combined) {
      rc = prio3_helper_prepare_aggregate_batch(
          engines[t], (uint32_t)job_size, nonces + 16 * (size_t)r0, jp,
          helper + (size_t)sz.helper_share_len * r0, lps + (size_t)sz.prep_share_len * r0,
          nullptr, nullptr, 1, msgs.data(), status_out + (size_t)j * job_size, agg, &cnt);
    } else {
      prio3_batch* b = nullptr;
      rc = prio3_helper_prepare_batch(
          engines[t], (uint32_t)job_size, nonces + 16 * (size_t)r0, jp,
          helper + (size_t)sz.helper_share_len * r0, lps + (size_t)sz.prep_share_len * r0,
          msgs.data(), status_out + (size_t)j * job_size, &b);
      if (rc == PRIO3_OK) rc = prio3_accumulate(b, nullptr, nullptr, 1, agg, &cnt);
      if (b) prio3_batch_free(b);
    }
    counts_out[j] = cnt;
    return rc == PRIO3_OK;
  });
}

// janus_jobs_run's combined form through prio3_helper_prepare_aggregate_batch_submit: every
// worker keeps K tickets outstanding (K = 1: a blocking call in two halves).
double janus_jobs_run_tickets(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                              int threads, int jobs, int job_size, uint32_t pool,
                              const uint8_t* nonces, const uint8_t* pub, const uint8_t* helper,
                              const uint8_t* lps, uint8_t* status_out, uint64_t* counts_out,
                              uint8_t* agg_out, int K) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  const size_t msg_bytes = (size_t)job_size * (sz.prep_msg_len ? sz.prep_msg_len : 1);
  return run_pool_tickets(threads, jobs, K, [&](int j, int slot, prio3_ticket** tk) {
    thread_local std::vector<uint8_t> msgs;  // one prepare-message buffer per outstanding ticket
    msgs.resize(msg_bytes * (size_t)(K < 1 ? 1 : K));
    const uint32_t t = (uint32_t)(j % n_engines);
    const uint32_t r0 = t * pool + (uint32_t)(((uint64_t)(j / n_engines) * job_size) % span);
    const uint8_t* jp = sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr;
    counts_out[j] = 0;
    return prio3_helper_prepare_aggregate_batch_submit(
               engines[t], (uint32_t)job_size, nonces + 16 * (size_t)r0, jp,
               helper + (size_t)sz.helper_share_len * r0, lps + (size_t)sz.prep_share_len * r0,
               nullptr, nullptr, 1, msgs.data() + msg_bytes * (size_t)slot,
               status_out + (size_t)j * job_size, agg_out + (size_t)sz.agg_share_len * j,
               counts_out + j, -1, tk) == PRIO3_OK;
  });
}

// The leader's side of the same jobs: per job prio3_leader_prepare_init_batch on the explicit
// leader input shares lin[..][leader_input_share_len], prio3_leader_prepare_next_batch on the
// helper's prepare messages msgs[..][prep_msg_len], prio3_accumulate, prio3_batch_free.  Job j's
// reports are chosen as in janus_jobs_run; ps_out[jobs * job_size][prep_share_len].
// combined = 1: prio3_leader_prepare_next_aggregate_batch instead of the last two calls.
double janus_jobs_run_leader(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                             int threads, int jobs, int job_size, uint32_t pool,
                             const uint8_t* nonces, const uint8_t* pub, const uint8_t* lin,
                             const uint8_t* msgs, uint8_t* ps_out, uint8_t* status_out,
                             uint64_t* counts_out, uint8_t* agg_out, int combined) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  return run_pool(threads, jobs, [&](int j) {
    const uint32_t t = (uint32_t)(j % n_engines);
    const uint32_t r0 = t * pool + (uint32_t)(((uint64_t)(j / n_engines) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    prio3_batch* b = nullptr;
    int rc = prio3_leader_prepare_init_batch(
        engines[t], (uint32_t)job_size, nonces + 16 * (size_t)r0,
        sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr,
        lin + (size_t)sz.leader_input_share_len * r0, ps_out + (size_t)sz.prep_share_len * o,
        status_out + o, &b);
    const uint8_t* m = sz.prep_msg_len ? msgs + (size_t)sz.prep_msg_len * r0 : nullptr;
    uint8_t* agg = agg_out + (size_t)sz.agg_share_len * j;
    uint64_t cnt = 0;
    if (rc == PRIO3_OK && combined) {
      rc = prio3_leader_prepare_next_aggregate_batch(b, m, status_out + o, nullptr, nullptr, 1,
                                                     agg, &cnt);
    } else if (rc == PRIO3_OK) {
      rc = prio3_leader_prepare_next_batch(b, m, status_out + o);
      if (rc == PRIO3_OK) rc = prio3_accumulate(b, nullptr, nullptr, 1, agg, &cnt);
    }
    prio3_batch_free(b);
    counts_out[j] = cnt;
    return rc == PRIO3_OK;
  });
}

// The helper's input-share open per job: janus_hpke_open_input_shares over job j's reports of
// task t = j % n_tasks (task_ids[t][32]; per-task report pools as above, per-report rows of
// nenc / ct_stride / 4 / 16 / 8 / pub_len bytes).  shares_out[jobs * job_size][share_len].
double janus_jobs_run_hpke(janus_hpke_opener* op, int n_tasks, const uint8_t* task_ids,
                           int threads, int jobs, int job_size, uint32_t pool, uint32_t nenc,
                           const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len,
                           uint32_t ct_stride, const uint8_t* ids, const uint64_t* times,
                           const uint8_t* pubs, uint32_t pub_len, uint32_t share_len,
                           uint8_t* shares_out, uint8_t* status_out) {
  const uint32_t span = pool - (uint32_t)job_size + 1;
  return run_pool(threads, jobs, [&](int j) {
    const uint32_t t = (uint32_t)(j % n_tasks);
    const size_t r0 = t * (size_t)pool + (((uint64_t)(j / n_tasks) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    return janus_hpke_open_input_shares(
               op, (uint32_t)job_size, task_ids + 32 * (size_t)t, enc + nenc * r0,
               ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride, ids + 16 * r0, times + r0,
               pub_len ? pubs + pub_len * r0 : nullptr, pub_len, share_len,
               0, shares_out + (size_t)share_len * o, status_out + o) == JANUS_HPKE_SUCCESS;
  });
}

// The helper's whole loop body per job from the sealed input shares (aggregator.rs:1794-2096):
// job j of task t = j % n_engines over the same report windows as janus_jobs_run, whose input
// shares were sealed to `opener`'s keypair under task_ids[t][32] (enc[..][nenc], ct[..][ct_stride],
// ct_len, times).  one_call = 1: prio3_helper_aggregate_init_batch (the open, prepare and
// accumulate in one coalesced launch); 0: the two-call composition a caller of r05's ABI makes --
// janus_hpke_open_input_shares into host buffers, then prio3_helper_prepare_aggregate_batch with
// the open's rejections masked out and their statuses merged (0x80 | PrepareError).
double janus_jobs_run_init(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                           janus_hpke_opener* opener, const uint8_t* task_ids, int threads,
                           int jobs, int job_size, uint32_t pool, const uint8_t* nonces,
                           const uint8_t* pub, const uint64_t* times, const uint8_t* enc,
                           uint32_t nenc, const uint8_t* ct, const uint32_t* ct_len,
                           uint32_t ct_stride, const uint8_t* lps, uint8_t* status_out,
                           uint64_t* counts_out, uint8_t* agg_out, int one_call) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  return run_pool(threads, jobs, [&](int j) {
    thread_local std::vector<uint8_t> msgs, shares, hs, acc;
    msgs.resize((size_t)job_size * (sz.prep_msg_len ? sz.prep_msg_len : 1));
    const uint32_t t = (uint32_t)(j % n_engines);
    const size_t r0 = t * (size_t)pool + (((uint64_t)(j / n_engines) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    const uint8_t* jp = sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr;
    uint8_t* st = status_out + o;
    uint8_t* agg = agg_out + (size_t)sz.agg_share_len * j;
    uint64_t cnt = 0;
    int rc;
    if (one_call) {
      rc = prio3_helper_aggregate_init_batch(
          engines[t], opener, (uint32_t)job_size, task_ids + 32 * (size_t)t, 0,
          nonces + 16 * r0, times + r0, jp, enc + (size_t)nenc * r0,
          ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride, lps + (size_t)sz.prep_share_len * r0,
          nullptr, nullptr, 1, msgs.data(), st, agg, &cnt);
    } else {
      shares.resize((size_t)job_size * sz.helper_share_len);
      hs.resize(job_size);
      acc.resize(job_size);
      rc = janus_hpke_open_input_shares(
          opener, (uint32_t)job_size, task_ids + 32 * (size_t)t, enc + (size_t)nenc * r0,
          ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride, nonces + 16 * r0, times + r0, jp,
          sz.public_share_len, sz.helper_share_len, 0, shares.data(), hs.data());
      if (rc == 0) {
        for (int i = 0; i < job_size; i++) acc[i] = hs[i] == 0;
        rc = prio3_helper_prepare_aggregate_batch(
            engines[t], (uint32_t)job_size, nonces + 16 * r0, jp, shares.data(),
            lps + (size_t)sz.prep_share_len * r0, nullptr, acc.data(), 1, msgs.data(), st, agg,
            &cnt);
        for (int i = 0; i < job_size; i++)
          if (hs[i]) st[i] = (uint8_t)(0x80u | hs[i]);
      }
    }
    counts_out[j] = cnt;
    return rc == 0;
  });
}

// A whole helper job as AggregationJobWriter needs it, per job of the same report windows as
// janus_jobs_run_init: batch-identifier index (time_precision, closed[k][2], max_segments), the
// loop body, and the per-batch checksums and intervals.  form 0: the three calls a host-buffer
// caller makes today -- prio3_job_index, prio3_helper_aggregate_init_batch_ex with the index's
// segment ids and accept bytes, prio3_batch_metadata; 1: prio3_helper_aggregate_job; 2: the _ex
// call alone with one segment and no index or metadata (what janus_jobs_run_init times); 3: the
// _ex call alone over the segment ids and reject bytes an earlier index of the same jobs left in
// seg_out / reject_out (inputs in this form), with max_segments rows: form 0 without its two
// blocking calls, which separates what the job's segments cost the accumulate from what the index
// and the metadata cost.
// Per job j: seg_out / status_out / reject_out / dup_out [jobs * job_size], counts_out
// [jobs][max_segments], agg_out [jobs][max_segments][agg_len], ck_out [jobs][max_segments][32],
// iv_out [jobs][max_segments][2], starts_out [jobs][max_segments], info_out [jobs] (form 2 fills
// status, and row 0 of counts and agg).
double janus_jobs_run_job(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                          janus_hpke_opener* opener, const uint8_t* task_ids, int threads,
                          int jobs, int job_size, uint32_t pool, const uint8_t* nonces,
                          const uint8_t* pub, const uint64_t* times, const uint8_t* enc,
                          uint32_t nenc, const uint8_t* ct, const uint32_t* ct_len,
                          uint32_t ct_stride, const uint8_t* lps, uint64_t time_precision,
                          const uint64_t* closed, uint32_t k, uint32_t max_segments,
                          uint32_t* seg_out, uint64_t* starts_out, uint8_t* reject_out,
                          uint8_t* dup_out, prio3_job_index_info* info_out, uint8_t* status_out,
                          uint64_t* counts_out, uint8_t* agg_out, uint8_t* ck_out,
                          uint64_t* iv_out, int form) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  const size_t S = max_segments;
  return run_pool(threads, jobs, [&](int j) {
    thread_local std::vector<uint8_t> msgs, acc;
    msgs.resize((size_t)job_size * (sz.prep_msg_len ? sz.prep_msg_len : 1));
    const uint32_t t = (uint32_t)(j % n_engines);
    const size_t r0 = t * (size_t)pool + (((uint64_t)(j / n_engines) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    const uint32_t n = (uint32_t)job_size;
    const uint8_t* jp = sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr;
    const uint8_t* tid = task_ids + 32 * (size_t)t;
    uint8_t* agg = agg_out + (size_t)sz.agg_share_len * S * j;
    uint64_t* cnt = counts_out + S * j;
    if (form == 3) {  // seg_out / reject_out are inputs here: a finished index of the same job
      acc.resize(n);
      for (uint32_t i = 0; i < n; i++)
        acc[i] = seg_out[o + i] != 0xFFFFFFFFu && reject_out[o + i] == 0;
      return prio3_helper_aggregate_init_batch_ex(
                 engines[t], opener, nullptr, UINT64_MAX, n, tid, 0, nonces + 16 * r0, times + r0,
                 jp, enc + (size_t)nenc * r0, ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride,
                 lps + (size_t)sz.prep_share_len * r0, seg_out + o, acc.data(), max_segments,
                 msgs.data(), status_out + o, agg, cnt) == PRIO3_OK;
    }
    if (form == 2)
      return prio3_helper_aggregate_init_batch_ex(
                 engines[t], opener, nullptr, UINT64_MAX, n, tid, 0, nonces + 16 * r0, times + r0,
                 jp, enc + (size_t)nenc * r0, ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride,
                 lps + (size_t)sz.prep_share_len * r0, nullptr, nullptr, 1, msgs.data(),
                 status_out + o, agg, cnt) == PRIO3_OK;
    if (form == 1) {
      prio3_helper_job_in in{};
      in.opener = opener;
      in.report_deadline = UINT64_MAX;
      in.n = n;
      in.task_id = tid;
      in.report_ids = nonces + 16 * r0;
      in.times = times + r0;
      in.public_shares = jp;
      in.enc = enc + (size_t)nenc * r0;
      in.ct = ct + (size_t)ct_stride * r0;
      in.ct_len = ct_len + r0;
      in.leader_prep_shares = lps + (size_t)sz.prep_share_len * r0;
      in.ct_stride = ct_stride;
      in.k = k;
      in.time_precision = time_precision;
      in.closed_intervals = closed;
      in.max_segments = max_segments;
      prio3_helper_job_out out{};
      out.segment_ids = seg_out + o;
      out.segment_starts = starts_out + S * j;
      out.reject = reject_out + o;
      out.duplicate = dup_out + o;
      out.info = info_out + j;
      out.prep_msgs = msgs.data();
      out.status = status_out + o;
      out.agg_shares = agg;
      out.counts = cnt;
      out.checksums = ck_out + 32 * S * j;
      out.intervals = iv_out + 2 * S * j;
      return prio3_helper_aggregate_job(engines[t], &in, &out) == PRIO3_OK;
    }
    acc.resize(n);
    int rc = prio3_job_index(engines[t], n, nonces + 16 * r0, times + r0, time_precision, closed,
                             k, max_segments, seg_out + o, starts_out + S * j, acc.data(),
                             reject_out + o, dup_out + o, info_out + j);
    if (rc == PRIO3_OK)
      rc = prio3_helper_aggregate_init_batch_ex(
          engines[t], opener, nullptr, UINT64_MAX, n, tid, 0, nonces + 16 * r0, times + r0, jp,
          enc + (size_t)nenc * r0, ct + (size_t)ct_stride * r0, ct_len + r0, ct_stride,
          lps + (size_t)sz.prep_share_len * r0, seg_out + o, acc.data(), max_segments,
          msgs.data(), status_out + o, agg, cnt);
    if (rc == PRIO3_OK)
      rc = prio3_batch_metadata(engines[t], n, nonces + 16 * r0, times + r0, status_out + o,
                                acc.data(), seg_out + o, max_segments, ck_out + 32 * S * j,
                                iv_out + 2 * S * j);
    return rc == PRIO3_OK;
  });
}

// janus_jobs_run_job's form 1 through prio3_helper_aggregate_job_submit: every worker keeps K
// tickets outstanding.  Same inputs and outputs per job.
double janus_jobs_run_job_tickets(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                                  janus_hpke_opener* opener, const uint8_t* task_ids, int threads,
                                  int jobs, int job_size, uint32_t pool, const uint8_t* nonces,
                                  const uint8_t* pub, const uint64_t* times, const uint8_t* enc,
                                  uint32_t nenc, const uint8_t* ct, const uint32_t* ct_len,
                                  uint32_t ct_stride, const uint8_t* lps, uint64_t time_precision,
                                  const uint64_t* closed, uint32_t k, uint32_t max_segments,
                                  uint32_t* seg_out, uint64_t* starts_out, uint8_t* reject_out,
                                  uint8_t* dup_out, prio3_job_index_info* info_out,
                                  uint8_t* status_out, uint64_t* counts_out, uint8_t* agg_out,
                                  uint8_t* ck_out, uint64_t* iv_out, int K) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  const size_t S = max_segments;
  const size_t msg_bytes = (size_t)job_size * (sz.prep_msg_len ? sz.prep_msg_len : 1);
  return run_pool_tickets(threads, jobs, K, [&](int j, int slot, prio3_ticket** tk) {
    thread_local std::vector<uint8_t> msgs;  // one prepare-message buffer per outstanding ticket
    msgs.resize(msg_bytes * (size_t)(K < 1 ? 1 : K));
    const uint32_t t = (uint32_t)(j % n_engines);
    const size_t r0 = t * (size_t)pool + (((uint64_t)(j / n_engines) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    prio3_helper_job_in in{};
    in.opener = opener;
    in.report_deadline = UINT64_MAX;
    in.n = (uint32_t)job_size;
    in.task_id = task_ids + 32 * (size_t)t;
    in.report_ids = nonces + 16 * r0;
    in.times = times + r0;
    in.public_shares = sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr;
    in.enc = enc + (size_t)nenc * r0;
    in.ct = ct + (size_t)ct_stride * r0;
    in.ct_len = ct_len + r0;
    in.leader_prep_shares = lps + (size_t)sz.prep_share_len * r0;
    in.ct_stride = ct_stride;
    in.k = k;
    in.time_precision = time_precision;
    in.closed_intervals = closed;
    in.max_segments = max_segments;
    prio3_helper_job_out out{};
    out.segment_ids = seg_out + o;
    out.segment_starts = starts_out + S * j;
    out.reject = reject_out + o;
    out.duplicate = dup_out + o;
    out.info = info_out + j;
    out.prep_msgs = msgs.data() + msg_bytes * (size_t)slot;
    out.status = status_out + o;
    out.agg_shares = agg_out + (size_t)sz.agg_share_len * S * j;
    out.counts = counts_out + S * j;
    out.checksums = ck_out + 32 * S * j;
    out.intervals = iv_out + 2 * S * j;
    return prio3_helper_aggregate_job_submit(engines[t], &in, &out, -1, tk) == PRIO3_OK;
  });
}

// A whole leader job as AggregationJobWriter needs it, over the report windows of
// janus_jobs_run_leader: prio3_leader_prepare_init_batch per job in every form alike, then on the
// helper's response (msgs[..][prep_msg_len], perr[..] = its prepare_error bytes, times[..]):
// form 0: the four moves a host-buffer leader makes today -- the per-report overlay of perr on the
// init status, prio3_job_index, prio3_leader_prepare_next_aggregate_batch over the index's segment
// ids and accept bytes, prio3_batch_metadata, and the per-report outcome pass; 1:
// prio3_leader_finish_job; 2: prio3_leader_prepare_next_aggregate_batch alone with one segment and
// no index, overlay, metadata or outcome (what janus_jobs_run_leader's combined form times).
// Per job j: seg_out / status_out / reject_out / dup_out / outcome_out [jobs * job_size],
// ps_out [jobs * job_size][prep_share_len], counts_out [jobs][max_segments], agg_out
// [jobs][max_segments][agg_len], ck_out [jobs][max_segments][32], iv_out [jobs][max_segments][2],
// starts_out [jobs][max_segments], info_out [jobs] (form 2 fills status, and row 0 of counts and
// agg).
double janus_jobs_run_leader_job(prio3_engine** engines, int n_engines, const prio3_sizes_t* szp,
                                 int threads, int jobs, int job_size, uint32_t pool,
                                 const uint8_t* nonces, const uint8_t* pub, const uint8_t* lin,
                                 const uint8_t* msgs, const uint64_t* times, const uint8_t* perr,
                                 uint64_t time_precision, const uint64_t* closed, uint32_t k,
                                 uint32_t max_segments, uint8_t* ps_out, uint32_t* seg_out,
                                 uint64_t* starts_out, uint8_t* reject_out, uint8_t* dup_out,
                                 prio3_job_index_info* info_out, uint8_t* status_out,
                                 uint8_t* outcome_out, uint64_t* counts_out, uint8_t* agg_out,
                                 uint8_t* ck_out, uint64_t* iv_out, int form) {
  const prio3_sizes_t sz = *szp;
  const uint32_t span = pool - (uint32_t)job_size + 1;
  const size_t S = max_segments;
  return run_pool(threads, jobs, [&](int j) {
    thread_local std::vector<uint8_t> acc, ls;
    const uint32_t t = (uint32_t)(j % n_engines);
    const size_t r0 = t * (size_t)pool + (((uint64_t)(j / n_engines) * job_size) % span);
    const size_t o = (size_t)j * job_size;
    const uint32_t n = (uint32_t)job_size;
    ls.resize(n);
    prio3_batch* b = nullptr;
    int rc = prio3_leader_prepare_init_batch(
        engines[t], n, nonces + 16 * r0,
        sz.public_share_len ? pub + (size_t)sz.public_share_len * r0 : nullptr,
        lin + (size_t)sz.leader_input_share_len * r0, ps_out + (size_t)sz.prep_share_len * o,
        ls.data(), &b);
    const uint8_t* m = sz.prep_msg_len ? msgs + (size_t)sz.prep_msg_len * r0 : nullptr;
    const uint8_t* pe = perr + r0;
    uint8_t* st = status_out + o;
    uint8_t* agg = agg_out + (size_t)sz.agg_share_len * S * j;
    uint64_t* cnt = counts_out + S * j;
    if (rc == PRIO3_OK && form == 2) {
      memcpy(st, ls.data(), n);
      rc = prio3_leader_prepare_next_aggregate_batch(b, m, st, nullptr, nullptr, 1, agg, cnt);
    } else if (rc == PRIO3_OK && form == 1) {
      prio3_leader_job_in in{};
      in.report_ids = nonces + 16 * r0;
      in.times = times + r0;
      in.leader_status = ls.data();
      in.prepare_error = pe;
      in.prep_msgs = m;
      in.time_precision = time_precision;
      in.closed_intervals = closed;
      in.k = k;
      in.max_segments = max_segments;
      prio3_leader_job_out out{};
      out.segment_ids = seg_out + o;
      out.segment_starts = starts_out + S * j;
      out.reject = reject_out + o;
      out.duplicate = dup_out + o;
      out.info = info_out + j;
      out.status = st;
      out.outcome = outcome_out + o;
      out.agg_shares = agg;
      out.counts = cnt;
      out.checksums = ck_out + 32 * S * j;
      out.intervals = iv_out + 2 * S * j;
      rc = prio3_leader_finish_job(b, &in, &out);
    } else if (rc == PRIO3_OK) {
      acc.resize(n);
      for (uint32_t i = 0; i < n; i++)  // the helper's prepare_error over the init status
        st[i] = ls[i] ? ls[i] : pe[i] != 0xFF ? (uint8_t)PRIO3_STATUS_PEER_MISMATCH : 0;
      rc = prio3_job_index(engines[t], n, nonces + 16 * r0, times + r0, time_precision, closed, k,
                           max_segments, seg_out + o, starts_out + S * j, acc.data(),
                           reject_out + o, dup_out + o, info_out + j);
      if (rc == PRIO3_OK)
        rc = prio3_leader_prepare_next_aggregate_batch(b, m, st, seg_out + o, acc.data(),
                                                       max_segments, agg, cnt);
      if (rc == PRIO3_OK)
        rc = prio3_batch_metadata(engines[t], n, nonces + 16 * r0, times + r0, st, acc.data(),
                                  seg_out + o, max_segments, ck_out + 32 * S * j,
                                  iv_out + 2 * S * j);
      for (uint32_t i = 0; rc == PRIO3_OK && i < n; i++) {  // the outcome byte
        uint8_t oc = pe[i];
        if (oc == 0xFF && st[i] != 0) oc = 5;
        if (ls[i] != 0) oc = 5;
        if (oc == 0xFF && reject_out[o + i]) oc = 0;
        outcome_out[o + i] = oc;
      }
    }
    if (b) prio3_batch_free(b);
    return rc == PRIO3_OK;
  });
}

}  // extern "C"

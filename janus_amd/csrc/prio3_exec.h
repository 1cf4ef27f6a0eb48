// prio3_exec.h -- the group-commit executor template of the host runtime (prio3_runtime.hip) and
// the few runtime functions it calls.  The header includes no HIP header: the executor's state
// machine (begin / done / complete, the two launchers, the hold and the light/heavy switch) is
// plain C++ over a policy class, so a CPU program can instantiate it over a fake policy and run it
// under ThreadSanitizer (tools/exec_ticket_harness.cpp).
#pragma once
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

#include "../../include/janus_prio3.h"

// Executor counters (prio3_executor_control / prio3_engine_members).
struct ExecStats {
  uint64_t jobs = 0, reports = 0, groups = 0;  // submitted jobs / their reports / launches
  // jobs begun and not yet completed (a blocking caller: inside submit; a ticket: until its wait)
  uint64_t active_jobs = 0, active_reports = 0;
};

struct Staging {
  uint8_t* p = nullptr;    // inputs and outputs, as the job threads see them (pinned host memory)
  uint8_t* dev = nullptr;  // the same bytes as the device addresses them (kernels read per-report
                           // inputs straight from here and write outputs back: engine_group_issue)
  size_t bytes = 0;
  void* map = nullptr;  // huge-page staging: the mapping (hipHostRegister'ed at p) and its length
  size_t map_bytes = 0;
};

// Defined in prio3_runtime.hip (a CPU harness of the template brings its own).
// Takes an idle staging of at least `bytes`, or allocates one; gives one back.
Staging staging_get(int dev, size_t bytes);
void staging_put(int dev, Staging s);
// pins the calling thread to the CPUs of `device`'s NUMA node that the process may use
void pin_to_gpu_node(int device);
// JANUS_COHORT_CAP=0 (A/B): no cap on a heavy-load group's share of the jobs (Exec::cohort_full)
bool cohort_cap();
// JANUS_EXEC_TRACE=<path>: one line per launched group (microseconds: created, taken by the
// launcher, writers done, launch returned; jobs; reports), for tuning the executor
// (profiles/r03/r03t .. r03ab)
FILE* exec_trace();
double exec_us(std::chrono::steady_clock::time_point t);
double ns_since(std::chrono::steady_clock::time_point t);
// JANUS_HOST_CPU=1: the job threads' CPU time in staging and unstaging per executor kind, printed
// to stderr at exit (where the jobs lines' host CPU goes)
bool host_cpu_on();
double host_cpu_ns();
void host_cpu_add(int kind, double stage_ns, double unstage_ns);

// an executor "hold" (tests queue jobs behind it) expires by itself: a caller that fails between
// hold = 1 and hold = 0 must not stall every engine sharing the executor forever
constexpr int64_t HOLD_MAX_MS = 30000;
// reports of the jobs begun and not completed at which the launcher leaves its light-load pipeline
// (the box's 16 rayon threads keep ~8 Ki in flight, 128 threads ~64 Ki)
constexpr uint64_t HEAVY_DEFAULT = 32768;
// the heavy-load launcher's streams: 0 the plain pool (r05i), 1 the light pipeline's CU-masked
// streams, whose hardware queues are already active when the load crosses HEAVY_DEFAULT (the
// first heavy groups on idle plain queues stalled 7-20 ms, r06b / r06c kernel traces; interleaved
// r06d: 35.5 / 35.7 / 36.2 against 34.5 / 35.7 / 33.6 M reports/s at 128 threads)
#ifndef JANUS_HEAVY_OWN_QUEUE
#define JANUS_HEAVY_OWN_QUEUE 1
#endif
constexpr bool HEAVY_OWN_QUEUE = JANUS_HEAVY_OWN_QUEUE != 0;

template <class P>
struct Exec {
  struct Ticket;
  struct Group {
    uint64_t key = 0;
    typename P::State st;
    Staging stg;
    int writers = 0, readers = 0;
    bool closed = false, done = false;
    int rc = PRIO3_OK;
    std::chrono::steady_clock::time_point created, t_take, t_staged;
    int njobs = 0;
    std::condition_variable cv;
    Ticket* notify = nullptr;  // its tickets that carry a completion fd (linked through next)
  };
  // One job between begin and complete.  The job is the ticket's own copy: P::reserve and
  // P::stage write the job's placement into it, and P::unstage reads that (and the caller's output
  // pointers) when the ticket is completed, on whichever thread that is.
  struct Ticket {
    Group* g = nullptr;
    typename P::Job job;
    int fd = -1;  // caller-owned eventfd (or -1): the value 1 is written once the group is done
    Ticket* next = nullptr;
    double stage_ns = 0;
  };
  int device = 0, id = 0;
  std::mutex mu;
  std::condition_variable cv;  // the launcher
  std::map<uint64_t, Group*> open;
  std::deque<Group*> order;  // groups not yet taken by the launcher, oldest first
  bool started = false;
  // under mu:
  bool hold = false;  // exec_control "hold": take no group until hold_until at the latest
  std::chrono::steady_clock::time_point hold_until;
  uint64_t heavy_at = P::heavy_default();  // exec_control "heavy"
  ExecStats stats;

  bool holding() const { return hold && std::chrono::steady_clock::now() < hold_until; }
  // the launcher's wait for work (caller holds mu): a hold wakes it when it expires
  void wait_work(std::unique_lock<std::mutex>& lk) {
    if (hold)
      cv.wait_until(lk, hold_until);
    else
      cv.wait(lk);
  }

  // (caller holds mu, and so does whoever reads g->done: a ticket's fd is written after its
  // group is done and before any later done() or complete() can look)
  void finish_locked(Group* g, int rc) {
    g->rc = rc;
    g->done = true;
    g->cv.notify_all();
    const uint64_t one = 1;
    for (Ticket* t = g->notify; t; t = t->next) (void)!write(t->fd, &one, sizeof one);
    g->notify = nullptr;
  }
  bool takeable() const { return !order.empty() && !holding(); }
  // the oldest group, closed to later jobs, once its writers are done (caller holds mu)
  Group* take_locked(std::unique_lock<std::mutex>& lk) {
    Group* g = order.front();
    order.pop_front();
    if (!g->closed) {  // take an open group: no later job joins it
      g->closed = true;
      auto it = open.find(g->key);
      if (it != open.end() && it->second == g) open.erase(it);
    }
    g->t_take = std::chrono::steady_clock::now();
    while (g->writers > 0) g->cv.wait(lk);
    g->t_staged = std::chrono::steady_clock::now();
    return g;
  }
  // issues g with mu released; on failure its callers are woken with the error (returns false)
  // own_queue: the group's kernels on a hardware queue of their own (ws_exec_stream_get) -- the
  // light-load pipeline, whose groups are meant to run concurrently, and since r06 the heavy-load
  // launcher too (HEAVY_OWN_QUEUE; r05 had put it on the plain stream pool, r05i: 38.5-39.8 M/s
  // at 128 threads against 30.2-36.0 with dedicated queues, interleaved)
  bool issue_unlocked(std::unique_lock<std::mutex>& lk, Group* g, typename P::Handle* h,
                      bool own_queue) {
    lk.unlock();
    const int rc = P::issue(device, g->st, g->stg, h, own_queue);
    lk.lock();
    if (rc != PRIO3_OK) {
      finish_locked(g, rc);
      return false;
    }
    stats.groups++;
    return true;
  }
  void trace(const Group* g) {
    if (FILE* f = exec_trace())
      fprintf(f, "%.1f %.1f %.1f %.1f %d %u\n", exec_us(g->created), exec_us(g->t_take),
              exec_us(g->t_staged), exec_us(std::chrono::steady_clock::now()), g->njobs,
              P::reports(g->st));
  }

  // Light load vs heavy load (reports of the jobs begun and not completed): launcher_pipe() below
  // heavy_at, launcher() from there; launcher() hands back only below a third of it (between two
  // cohorts the callers of the finished group leave submit for a moment, and a handover there
  // cost the 128-thread line 10 %, r04z6).
  bool light() const { return stats.active_reports < heavy_at; }
  // Heavy load runs two cohorts of callers in turn: while one group runs, the callers it released
  // last fill the next.  Their sizes are whatever the start-up or a late caller made them, and they
  // persist: 41 / 87 jobs of the 128-thread line ran at 33.5 M reports/s, 58 / 68 at 37.6 (r06r).
  // A group open under heavy load takes at most about half the jobs inside submit, so a cohort
  // that is too big spills into the next group, which the other cohort then joins.
  bool cohort_full(const Group* g) const {
    return cohort_cap() && !light() && 2 * (uint64_t)g->njobs >= stats.active_jobs + 4;
  }
  bool lighter() const { return stats.active_reports < heavy_at / 3; }

  // Heavy load: one group on the GPU at a time.  While it runs, the launcher polls it; once its
  // prepare kernels are done, the next group -- by then holding the callers released by the
  // group before, all staged -- is issued behind it on its own stream, so the GPU does not idle
  // while this group's completion is noticed and the next launch is set up (r03y trace: 124 us
  // between groups).  The launcher must notice a group's 'prepared' event within microseconds,
  // but spinning through the whole ~0.7 ms group kept a core busy beside the staging writers
  // (ADVICE r3): it learns the prepare time per report from groups it watched complete while
  // spinning, and sleeps through the first 70 % of each later group (per group key: instances
  // of very different cost share the executor).  A sleep that overshoots (the group was already
  // prepared at the first poll) tells only an upper bound, so it shrinks the estimate instead of
  // feeding it (r04a: feeding it made the estimate hold itself up, 5.4 M reports/s).  `preds` is
  // the launcher thread's own table.  Returns (with nothing in flight) when the load turns light.
  struct Pred {
    double ns_per_report = 0;
    int seen = 0;
  };
  void launcher(std::map<uint64_t, Pred>& preds) {
    std::unique_lock<std::mutex> lk(mu);
    Group* cur = nullptr;
    typename P::Handle hc{};
    auto t0 = std::chrono::steady_clock::now();  // when cur could start
    for (;;) {
      if (!cur) {
        if (lighter()) return;
        while (!takeable()) wait_work(lk);
        Group* g = take_locked(lk);
        t0 = std::chrono::steady_clock::now();
        if (!issue_unlocked(lk, g, &hc, HEAVY_OWN_QUEUE)) continue;
        cur = g;
      }
      lk.unlock();
      Group* nxt = nullptr;
      typename P::Handle hn{};
      bool looked = false;
      auto tn = t0;  // when nxt was issued
      auto tp = t0;  // when cur was seen prepared (nxt's kernels start then)
      const uint32_t nrep = P::reports(cur->st);
      Pred& pr = preds[cur->key];
      bool just_slept = false;
      {  // sleep to 70 % of the predicted prepare time, less the timer slack (~60 us), <= 2 ms
        const double ns = std::min(2e6, 0.7 * pr.ns_per_report * nrep - 60e3 - ns_since(t0));
        if (pr.seen >= 2 && ns > 20e3) {
          std::this_thread::sleep_for(std::chrono::nanoseconds((int64_t)ns));
          just_slept = true;
        }
      }
      while (!P::done(hc)) {
        if (!looked && P::prepared(hc)) {
          looked = true;
          tp = std::chrono::steady_clock::now();
          const double x = nrep ? ns_since(t0) / nrep : 0;
          if (just_slept) {
            pr.ns_per_report *= 0.8;  // overslept: the elapsed time is only an upper bound
          } else {
            pr.ns_per_report = pr.seen ? std::min(x, 0.8 * pr.ns_per_report + 0.2 * x) : x;
            pr.seen++;
          }
          lk.lock();
          if (takeable() && order.front()->writers == 0 && !lighter()) {
            nxt = take_locked(lk);
            tn = std::chrono::steady_clock::now();
            if (!issue_unlocked(lk, nxt, &hn, HEAVY_OWN_QUEUE)) nxt = nullptr;
          }
          lk.unlock();
        }
        just_slept = false;
        std::this_thread::yield();
      }
      const int rc = P::finish(&hc);
      trace(cur);
      lk.lock();
      finish_locked(cur, rc);
      cur = nullptr;
      if (nxt) {
        cur = nxt;
        hc = hn;
        t0 = std::max(tn, tp);  // its prepare time counts from when its kernels could start
      }
    }
  }

  // Light load (the box's 16 rayon threads make groups of a few jobs, each a latency-bound kernel
  // at well under a wave per SIMD): up to four groups whose kernels run concurrently (no group
  // waits for another's prepare), each issued as soon as it is staged and holds >= 2 Ki reports
  // (smaller ones wait for an empty pipeline), any finished group completed at once: 10-15 M
  // reports/s at 16 threads against 5.6-7.6 M/s for launcher() on the same boxes (r04z).  Under
  // heavy load (the 128-thread line) launcher()'s two-cohort rhythm stays ahead (38.6-39.6 M/s
  // against 28-35 M/s for this pipeline, r04z2-4).  The pipeline yields between polls (a sleep's
  // timer slack would be a fifth of a small group's time).
  void launcher_pipe() {
    struct Slot {
      Group* g;
      typename P::Handle h;
    };
    std::deque<Slot> q;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      if (q.empty() && !light()) return;  // heavy load: launcher() from here
      while (takeable()) {
        Group* g = order.front();
        if (!q.empty()) {
          // heavy load: let the pipeline drain (one bubble) and hand over to launcher()
          if (g->writers > 0 || !light() || q.size() >= 4) break;
          if (P::reports(g->st) < 2048u) break;  // a small group waits for a drained pipeline
        }
        take_locked(lk);
        Slot sl{g, typename P::Handle{}};
        if (issue_unlocked(lk, g, &sl.h, true)) q.push_back(sl);
      }
      if (q.empty()) {
        while (!takeable() && light()) wait_work(lk);
        continue;
      }
      lk.unlock();
      bool any = false;
      for (size_t i = 0; i < q.size();) {
        if (P::done(q[i].h)) {
          Slot sl = q[i];
          q.erase(q.begin() + (long)i);
          const int rc = P::finish(&sl.h);
          trace(sl.g);
          std::lock_guard<std::mutex> lg(mu);
          finish_locked(sl.g, rc);
          any = true;
        } else {
          i++;
        }
      }
      if (!any) std::this_thread::yield();
      lk.lock();
    }
  }

  // The first half of a job: reserves its place in the open group of its key, stages its inputs
  // on the calling thread and tells the launcher once the group's writers are done.  Every input
  // the job points at has been read when begin returns.  On success *out is the job's ticket (to
  // be completed exactly once); on failure nothing is outstanding and fd is not written.
  int begin(const typename P::Job& job_in, int fd, Ticket** out) {
    *out = nullptr;
    Ticket* t = new Ticket();
    t->job = job_in;
    t->fd = fd;
    typename P::Job* job = &t->job;
    std::unique_lock<std::mutex> lk(mu);
    stats.jobs++;
    stats.reports += job->n;
    stats.active_jobs++;
    stats.active_reports += job->n;
    // (runs with mu held: every return below holds lk)
    auto fail = [&](int rc) {
      stats.active_jobs--;
      stats.active_reports -= job->n;
      delete t;
      return rc;
    };
    if (!started) {  // one launcher thread per executor (never joined: see g_exec)
      started = true;
      std::thread([this] {
        pin_to_gpu_node(device);  // the launcher runs on its GPU's NUMA node
        std::map<uint64_t, Pred> preds;
        for (;;) {  // launcher() under heavy load, launcher_pipe() under light load
          launcher(preds);
          launcher_pipe();
        }
      }).detach();
    }
    // the load may have crossed heavy_at: a launcher waiting in light mode re-checks
    cv.notify_one();
    const uint64_t key = P::key(job);
    Group* g = nullptr;
    for (;;) {
      auto it = open.find(key);
      g = it == open.end() ? nullptr : it->second;
      if (g && !cohort_full(g) && P::reserve(g->st, job)) break;
      if (g) {  // full: it stays queued for the launcher as it is
        g->closed = true;
        open.erase(it);
      }
      g = new Group();
      g->key = key;
      size_t bytes = 0;
      if (!P::create(g->st, job, &bytes)) {
        delete g;
        return fail(PRIO3_EINVAL);
      }
      g->stg = staging_get(device, bytes);
      if (!g->stg.p) {
        delete g;
        return fail(PRIO3_EDEVICE);
      }
      g->created = std::chrono::steady_clock::now();
      open[key] = g;
      order.push_back(g);
      cv.notify_one();
      if (!P::reserve(g->st, job)) return fail(PRIO3_EINVAL);  // cannot happen: sized for the job
      break;
    }
    g->writers++;
    g->readers++;
    g->njobs++;
    t->g = g;
    if (fd >= 0) {
      t->next = g->notify;
      g->notify = t;
    }
    lk.unlock();
    const double c0 = host_cpu_ns();
    P::stage(g->st, g->stg, job);
    t->stage_ns = host_cpu_ns() - c0;
    lk.lock();
    if (--g->writers == 0) g->cv.notify_all();
    *out = t;
    return PRIO3_OK;
  }

  // whether the ticket's group has run (never blocks on the device or on another job)
  bool done(const Ticket* t) {
    std::lock_guard<std::mutex> lk(mu);
    return t->g->done;
  }

  // The second half: waits for the ticket's group, copies the job's outputs out on the calling
  // thread, leaves the group (the last job out returns its staging) and frees the ticket.
  // job_out (nullable) receives the job with its results (its run, its columns).
  int complete(Ticket* t, typename P::Job* job_out) {
    Group* g = t->g;
    std::unique_lock<std::mutex> lk(mu);
    while (!g->done) g->cv.wait(lk);
    const int rc = g->rc;
    lk.unlock();
    const double c2 = host_cpu_ns();
    if (rc == PRIO3_OK) P::unstage(g->st, g->stg, &t->job);
    if (host_cpu_on()) host_cpu_add(P::kind, t->stage_ns, host_cpu_ns() - c2);
    if (job_out) *job_out = t->job;
    lk.lock();
    stats.active_jobs--;
    stats.active_reports -= t->job.n;
    if (--g->readers == 0) {
      staging_put(device, g->stg);
      delete g;
    }
    lk.unlock();
    delete t;
    return rc;
  }

  // the blocking form: begin, then complete at once
  int submit(typename P::Job* job) {
    Ticket* t = nullptr;
    const int rc = begin(*job, -1, &t);
    if (rc != PRIO3_OK) return rc;
    return complete(t, job);
  }

  int control(const char* key, int64_t value) {
    std::lock_guard<std::mutex> lk(mu);
    if (!strcmp(key, "hold")) {  // 1: at most HOLD_MAX_MS; v > 1: at most v ms
      hold = value != 0;
      hold_until = std::chrono::steady_clock::now() +
                   std::chrono::milliseconds(value > 1 ? value : HOLD_MAX_MS);
    } else if (!strcmp(key, "heavy")) {
      heavy_at = value > 0 ? (uint64_t)value : P::heavy_default();
    } else {
      return PRIO3_EINVAL;
    }
    cv.notify_all();
    return PRIO3_OK;
  }
  ExecStats get_stats() {
    std::lock_guard<std::mutex> lk(mu);
    return stats;
  }
};

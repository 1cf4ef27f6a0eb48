// exec_ticket_harness.cpp -- the executor's begin / done / complete state machine
// (janus_amd/csrc/prio3_exec.h) over a fake policy, as a stand-alone CPU program meant to run
// under ThreadSanitizer (janus_amd/Makefile target `tsan_exec`).  No GPU, no HIP: the fake
// policy's staging is malloc, its launch a short timer, its stage / unstage copies of the job's
// bytes with a checksum.
//
// 8 threads x 64 jobs, each thread holding up to K tickets (K cycles 1..8 by thread); a quarter
// of the jobs go through the blocking submit; completion is randomly poll-then-wait or a straight
// wait; a ninth thread toggles the executor's hold; the `heavy` control is 1 for the first half
// of the run, so both launchers see tickets; one eventfd is shared by every ticket and its summed
// count must equal the number of ticketed jobs.
// Exit status 0: every job's bytes came back right, every notification arrived exactly once and
// no job took longer than 30 s.  (With TSAN_OPTIONS=halt_on_error=1 a race report ends the run.)
//
// libstdc++ waits on a steady_clock deadline (the launcher's wait under a hold) through
// pthread_cond_clockwait, which the ThreadSanitizer runtime of GCC 11 does not intercept: it then
// believes the mutex stayed locked across the wait and reports a "double lock".  Without the macro
// below the same wait goes through pthread_cond_timedwait, which it knows.
#if __has_include(<bits/c++config.h>)
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT
#endif
#include <sys/eventfd.h>

#include <atomic>
#include <cstdlib>
#include <random>
#include <vector>

#include "../janus_amd/csrc/prio3_exec.h"

// ---- the runtime functions the template calls ----
Staging staging_get(int, size_t bytes) {
  Staging s;
  s.p = (uint8_t*)malloc(bytes);
  s.dev = s.p;
  s.bytes = bytes;
  return s;
}
void staging_put(int, Staging s) { free(s.p); }
void pin_to_gpu_node(int) {}
bool cohort_cap() { return true; }
FILE* exec_trace() { return nullptr; }
double exec_us(std::chrono::steady_clock::time_point) { return 0; }
double ns_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t).count();
}
bool host_cpu_on() { return false; }
double host_cpu_ns() { return 0; }
void host_cpu_add(int, double, double) {}

namespace {

constexpr uint32_t ROW = 64;        // bytes per report
constexpr uint32_t GROUP_CAP = 96;  // reports per group: a few jobs, so groups spill

uint64_t checksum(const uint8_t* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

struct FakeJob {
  uint32_t n = 0;
  const uint8_t* in = nullptr;  // [n][ROW], read by stage only
  uint8_t* out = nullptr;       // [n][ROW], written by unstage only
  uint64_t* sum_out = nullptr;  // the checksum the "device" made of the staged bytes
  uint32_t c0 = 0, slot = 0;    // placement in the group
};

struct FakePolicy {
  static constexpr int kind = 0;
  typedef FakeJob Job;
  static uint64_t heavy_default() { return 1u << 20; }
  struct State {
    uint32_t n = 0, jobs = 0;
    uint32_t c0[GROUP_CAP], len[GROUP_CAP];
    uint64_t sums[GROUP_CAP];
    std::chrono::steady_clock::time_point ready, half;
  };
  struct Handle {
    State* s = nullptr;
  };
  static uint64_t key(Job* j) { return j->n & 1u; }  // two keys: two open groups at a time
  static uint32_t reports(const State& s) { return s.n; }
  static bool create(State&, Job* j, size_t* bytes) {
    if (j->n > GROUP_CAP) return false;
    *bytes = (size_t)GROUP_CAP * ROW;
    return true;
  }
  static bool reserve(State& s, Job* j) {
    if (s.n + j->n > GROUP_CAP) return false;
    j->c0 = s.n;
    j->slot = s.jobs;
    s.c0[s.jobs] = s.n;
    s.len[s.jobs] = j->n;
    s.n += j->n;
    s.jobs++;
    return true;
  }
  static void stage(State&, Staging& g, Job* j) {
    memcpy(g.p + (size_t)ROW * j->c0, j->in, (size_t)ROW * j->n);
  }
  // the "launch": checksums of every job's staged rows, each row then inverted in place; it
  // "runs" for 200 us
  static int issue(int, State& s, Staging& g, Handle* h, bool) {
    for (uint32_t k = 0; k < s.jobs; k++) {
      uint8_t* p = g.p + (size_t)ROW * s.c0[k];
      const size_t m = (size_t)ROW * s.len[k];
      s.sums[k] = checksum(p, m);
      for (size_t i = 0; i < m; i++) p[i] = (uint8_t)~p[i];
    }
    const auto now = std::chrono::steady_clock::now();
    s.half = now + std::chrono::microseconds(100);
    s.ready = now + std::chrono::microseconds(200);
    h->s = &s;
    return PRIO3_OK;
  }
  static bool prepared(const Handle& h) { return std::chrono::steady_clock::now() >= h.s->half; }
  static bool done(const Handle& h) { return std::chrono::steady_clock::now() >= h.s->ready; }
  static int finish(Handle*) { return PRIO3_OK; }
  static void unstage(State& s, Staging& g, Job* j) {
    memcpy(j->out, g.p + (size_t)ROW * j->c0, (size_t)ROW * j->n);
    *j->sum_out = s.sums[j->slot];
  }
};

typedef Exec<FakePolicy> Ex;
Ex* g_ex = new Ex();  // never destroyed: its launcher thread is detached

constexpr int THREADS = 8, JOBS = 64;
std::atomic<int> g_errors{0};
std::atomic<uint64_t> g_ticketed{0};
std::atomic<int> g_finished{0};

void fail(const char* what, int t, int j) {
  fprintf(stderr, "exec_ticket_harness: %s (thread %d, job %d)\n", what, t, j);
  g_errors++;
}

struct Pending {
  Ex::Ticket* t = nullptr;
  int j = 0;
  std::vector<uint8_t> want, out;  // the input's bytes inverted; where unstage writes
  uint64_t want_sum = 0, sum = 0;
  std::chrono::steady_clock::time_point t0;
};

void check(Pending& p, int rc, int tid) {
  if (rc != PRIO3_OK) fail("job failed", tid, p.j);
  if (p.sum != p.want_sum) fail("wrong checksum", tid, p.j);
  if (p.out != p.want) fail("wrong bytes", tid, p.j);
  if (std::chrono::steady_clock::now() - p.t0 > std::chrono::seconds(30))
    fail("not done within 30 s", tid, p.j);
}

void worker(int tid, int fd) {
  std::mt19937 rng(1234u + (unsigned)tid);
  const size_t K = 1 + (size_t)tid % 8;
  std::deque<Pending*> q;
  auto finish_oldest = [&] {
    Pending* p = q.front();
    q.pop_front();
    if (rng() & 1u)  // poll, then wait
      while (!g_ex->done(p->t)) {
        if (std::chrono::steady_clock::now() - p->t0 > std::chrono::seconds(30)) break;
        std::this_thread::yield();
      }
    const int rc = g_ex->complete(p->t, nullptr);
    check(*p, rc, tid);
    delete p;
  };
  for (int j = 0; j < JOBS; j++) {
    Pending* p = new Pending();
    p->j = j;
    const uint32_t n = 1 + rng() % 40;
    std::vector<uint8_t> in((size_t)ROW * n);
    for (auto& b : in) b = (uint8_t)rng();
    p->want.resize(in.size());
    for (size_t i = 0; i < in.size(); i++) p->want[i] = (uint8_t)~in[i];
    p->want_sum = checksum(in.data(), in.size());
    p->out.assign(in.size(), 0xA5);
    FakeJob job;
    job.n = n;
    job.in = in.data();
    job.out = p->out.data();
    job.sum_out = &p->sum;
    p->t0 = std::chrono::steady_clock::now();
    if (j % 4 == 3) {  // a blocking caller among the tickets
      const int rc = g_ex->submit(&job);
      check(*p, rc, tid);
      delete p;
      continue;
    }
    const int rc = g_ex->begin(job, fd, &p->t);
    if (rc != PRIO3_OK || !p->t) {
      fail("begin failed", tid, j);
      delete p;
      continue;
    }
    g_ticketed++;
    // the inputs are consumed: overwrite them at once
    for (auto& b : in) b = 0x5A;
    q.push_back(p);
    if (q.size() >= K) finish_oldest();
    if (j == JOBS / 2 && tid == 0) g_ex->control("heavy", 0);  // the second half: the default
  }
  while (!q.empty()) finish_oldest();
  g_finished++;
}

}  // namespace

int main() {
  const int fd = eventfd(0, EFD_NONBLOCK);
  if (fd < 0) {
    perror("eventfd");
    return 2;
  }
  g_ex->control("heavy", 1);  // the first half of the run on the heavy-load launcher
  std::vector<std::thread> th;
  for (int t = 0; t < THREADS; t++) th.emplace_back(worker, t, fd);
  std::thread holder([] {  // the ninth thread: short holds while jobs queue up
    std::mt19937 rng(99);
    const auto start = std::chrono::steady_clock::now();
    while (g_finished.load() < THREADS) {
      if (std::chrono::steady_clock::now() - start > std::chrono::seconds(60)) {
        fprintf(stderr, "exec_ticket_harness: still running after 60 s: a job is stuck\n");
        _exit(3);
      }
      g_ex->control("hold", 5);  // expires by itself after 5 ms
      std::this_thread::sleep_for(std::chrono::microseconds(300 + rng() % 700));
      g_ex->control("hold", 0);
      std::this_thread::sleep_for(std::chrono::microseconds(300 + rng() % 700));
    }
    g_ex->control("hold", 0);
  });
  for (auto& t : th) t.join();
  holder.join();
  uint64_t total = 0, v = 0;
  while (read(fd, &v, sizeof v) == (ssize_t)sizeof v) total += v;
  if (total != g_ticketed.load()) {
    fprintf(stderr, "exec_ticket_harness: %llu notifications for %llu ticketed jobs\n",
            (unsigned long long)total, (unsigned long long)g_ticketed.load());
    g_errors++;
  }
  const ExecStats s = g_ex->get_stats();
  if (s.active_jobs || s.active_reports) {
    fprintf(stderr, "exec_ticket_harness: %llu jobs / %llu reports still active\n",
            (unsigned long long)s.active_jobs, (unsigned long long)s.active_reports);
    g_errors++;
  }
  if (s.jobs != (uint64_t)THREADS * JOBS) {
    fprintf(stderr, "exec_ticket_harness: %llu jobs counted\n", (unsigned long long)s.jobs);
    g_errors++;
  }
  printf("exec_ticket_harness: %llu jobs (%llu ticketed) in %llu groups, %d errors\n",
         (unsigned long long)s.jobs, (unsigned long long)total, (unsigned long long)s.groups,
         g_errors.load());
  close(fd);
  return g_errors.load() ? 1 : 0;
}

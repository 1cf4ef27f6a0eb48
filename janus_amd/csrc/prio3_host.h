// prio3_host.h -- host-only declarations shared by the three engine translation units:
//   prio3_prepare.hip     helper / leader prepare kernels and their launch plans
//   prio3_accumulate.hip  accumulate, aggregate, combine and metadata kernels and launches
//   prio3_engine.hip      sizes, timing, runs, executor hooks and the C ABI
// (prio3_client.hip includes it for the leader launch declarations.)  Device-only headers and the
// kernel families with a launch_* function of their own (prio3_common.h) do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <mutex>
#include <vector>

#include "prio3_common.h"
#include "prio3_runtime.h"

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t _e = (x);                                                            \
    if (_e != hipSuccess) {                                                         \
      fprintf(stderr, "janus_prio3: HIP error %s at %s:%d\n", hipGetErrorString(_e), \
              __FILE__, __LINE__);                                                  \
      return PRIO3_EDEVICE;                                                         \
    }                                                                               \
  } while (0)

// ---- per-kernel timing (option "timing"): HIP events on the launch stream ----
// One list per thread for the whole library, defined in prio3_engine.hip: collect_times folds
// the events of every unit's launches.
struct Pending {
  prio3_engine* e;
  size_t idx;
  hipEvent_t a, b;
};
std::vector<Pending>& pending();
size_t time_slot(prio3_engine* e, const char* name);
// timing 2: launches are counted only (no events on the production launch path)
void count_launch(prio3_engine* e, const char* name);
// folds this thread's finished timing events of engine e into e->times.  wait = false (the
// executor's group finish): events still pending -- those of the group issued ahead behind the
// finishing one -- are left for a later call instead of blocking the launcher on them
void collect_times(prio3_engine* e, bool wait = true);
#define TIMED(e, st, name, launch)                                   \
  do {                                                               \
    hipEvent_t _a = nullptr, _b = nullptr;                           \
    const bool _t = (e)->timing == 1 && hipEventCreate(&_a) == hipSuccess && \
                    hipEventCreate(&_b) == hipSuccess;               \
    if (_t) (void)hipEventRecord(_a, st);                            \
    launch;                                                          \
    HIPCHK(hipGetLastError());                                       \
    if (_t) {                                                        \
      (void)hipEventRecord(_b, st);                                  \
      pending().push_back(Pending{(e), time_slot(e, name), _a, _b}); \
    } else if ((e)->timing == 2) {                                   \
      count_launch((e), name);                                       \
    }                                                                \
  } while (0)

// ---- runs: the device state of one prepare call, carved from one pooled slab ----
enum : unsigned {
  RUN_SCRATCH = 1,  // SoA prepare scratch
  RUN_IO = 2,       // device copies of host inputs / outputs (host-buffer entry points)
  RUN_LINPUT = 8,   // leader input shares (host-buffer leader entry point)
  RUN_FUSED = 16,   // fused-accumulate partials (prio3_device_prepare_aggregate, Histogram)
  RUN_AGG_IO = 32,  // group segment ids, accept bytes, aggregate shares + counts (executor)
  RUN_HPKE = 64,    // open statuses + plaintext scratch of a sealed-input group (executor)
  RUN_JIX = 128,    // checksum + interval rows of a group of prio3_helper_aggregate_job jobs
};

static inline bool own_out(const DevParams& d) {  // the output share is not the measurement share
  return d.kind == PRIO3_SUM || d.kind == PRIO3_SUMVEC || d.kind == PRIO3_SUMVEC_F64_MP ||
         d.kind == PRIO3_FPVEC_BOUNDED_L2;
}
// the run's output shares at column c0 (SoA [element][ld_out])
static inline const uint8_t* run_out_shares(const Run* R, uint32_t c0) {
  return (const uint8_t*)(own_out(R->dp) ? R->sc.out : R->sc.meas) + (size_t)R->dp.es * c0;
}

constexpr uint32_t WCH = 32;  // waves per fused-partial chunk (k_agg_parts, run_carve)

// Zero-fill of up to 4 ranges by the threads of a launch (4-byte aligned lengths and pointers:
// 16-byte stores for the aligned body, 4-byte stores at the ends).  k_zero is that launch; a
// fused run's k_slow_redo* launch takes the ranges along instead (fused_first_zero), so the run's
// accumulators are clean before its first fused_finish without a launch of their own.
struct ZeroRanges {
  uint8_t* dst[4];
  size_t bytes[4];
};
__device__ __forceinline__ void zero_ranges(const ZeroRanges& z, size_t tid, size_t nth) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint8_t* d = z.dst[k];
    const size_t n = z.bytes[k];
    if (!d || !n) continue;
    const size_t h0 = (16 - ((uintptr_t)d & 15)) & 15, head = n < h0 ? n : h0;
    const size_t n16 = (n - head) / 16;
    for (size_t i = tid; i < n16; i += nth) ((uint4*)(d + head))[i] = make_uint4(0, 0, 0, 0);
    for (size_t i = tid * 4; i < head; i += nth * 4) *(uint32_t*)(d + i) = 0u;
    for (size_t i = head + 16 * n16 + tid * 4; i < n; i += nth * 4) *(uint32_t*)(d + i) = 0u;
  }
}
// The accumulators fused_finish adds into and leaves clean again: the 64-bit sums of the mixed
// chunks, the two fix-up counters and the count row.  (Defined in prio3_accumulate.hip.)
ZeroRanges fused_first_zero(const Run* R);
// 64 words of device memory per (GPU, stream), zero at the stream's first call and put back to
// zero by the last block of every launch that counts in them -- [0] k_meta's ticket, [1] the
// redo list's length and [2] the list launch's ticket (Scratch::redo_cnt = words + 1) -- so the
// steady path needs no memset.  Calls on one stream follow each other and share the words;
// calls on two streams, which may run at once, do not.  k_meta's rows follow at byte 256.
// nullptr past STREAM_ZERO_MAX streams: the caller then takes its path without them.
// *mu (optional): the stream's mutex, for a caller that counts in the words over several launches
// (prepare_run: from k_prep_h's appends to the redo launch) and so must keep another thread's
// launches on the same stream from falling between them.
// (Defined in prio3_accumulate.hip.)
uint32_t* stream_zero_words(int device, hipStream_t st, std::mutex** mu = nullptr);

// a pooled stream for one blocking host-buffer call
struct PooledStream {
  int device;
  hipStream_t s;
  explicit PooledStream(int dev) : device(dev), s(ws_stream_get(dev)) {}
  ~PooledStream() { ws_stream_put(device, s); }
};

// Copies by the shader cores between device memory and mapped pinned memory (up to 4 ranges,
// 16-byte aligned; 16-byte accesses, the byte tails by lane).  Host -> device, this reads PCIe at
// ~55 GB/s where the SDMA copy of the same staging ran at ~32 GB/s beside the XOF's own host
// reads (profiles/r03/r03l trace); device -> host, one launch returns a group's four outputs
// where four SDMA copies each paid their own setup.
struct PullRanges {
  const uint8_t* src[4];
  uint8_t* dst[4];
  size_t bytes[4];
};
// k_pull (prio3_engine.hip) over `blocks` blocks; false if the launch failed
bool launch_pull(const PullRanges& pr, unsigned blocks, hipStream_t st);

// ---- prio3_prepare.hip (described at their definitions) ----
// What one helper prepare of n reports launches: decided once, in plan_prepare, and only read by
// prepare_run, launch_prepare and launch_slow_redo (tests/golden/launch_table.json pins it).
enum class PrepChain : uint8_t {
  MP64,       // k_mp64_prepare
  FPVEC,      // sub-batches of XOF, k_xof_slow and the FPVec query
  FUSED_H,    // k_prep_h (or k_prep_hp on lane pairs): XOF + k_query_h<2, 32> in one launch
  FUSED_SUM,  // k_prep_sum: XOF + k_query_sum in one launch
  XOF_QUERY,  // the XOF, then the query
  GEN64,      // Field64 (Prio3Count): k_prep_gen
};
// PAIR, WIDE and SUM have a launch_* of their own that may decline: then k_xofd, k_query_ps, k_query
enum class XofKernel : uint8_t { NONE, PAIR, XOFD, XOF, XOF_A_JRPART };
enum class QueryKernel : uint8_t { NONE, FPW, FP, WIDE, H, PS, SUM, GENERIC };
enum class RedoFamily : uint8_t { NONE, QH, SUM, GEN64 };  // the run's k_slow_redo* launch
struct PrepPlan {
  PrepChain chain;
  XofKernel xof;
  QueryKernel query;
  bool fusable;      // the accumulate can ride on this instance's XOF (what callers pass as fuse)
  bool dual;         // the share spans two joint-rand blocks: the dual-state XOF
  bool trunc_xof;    // the XOF's squeeze also truncates / decodes the output share
  bool slow_defer;   // the query skips flagged reports; the redo launch takes them
  RedoFamily redo;
  bool redo_list;    // k_prep_h lists its flagged reports and the redo launch walks the list
  bool pair;         // Histogram on lane pairs (k_prep_hp)
  bool pull_in_xof;  // the fused launch copies the leader prep shares itself (else k_pull)
  uint32_t chunks, chunk_cols;  // stream-overlapped column ranges (1: one launch chain)
};
// pulling: the caller hands over mapped host staging to copy from (executor groups)
PrepPlan plan_prepare(const prio3_engine* e, const DevParams& dp, uint32_t n, bool fuse,
                      bool pulling);
inline bool prepare_fuses(const prio3_engine* e) {
  return plan_prepare(e, e->dp, 0, false, false).fusable;
}
// The leader's prepare_init.  soa_staging and the K_LEADER_PREP chain differ by the former's
// leader_share_len term: both answers are kept as they were.
enum class LeaderChain : uint8_t { FPVEC, MP64, K_LEADER_PREP, SUM, GENERIC };
struct LeaderPlan {
  LeaderChain chain;
  bool soa_staging;  // k_leader_prep can read the input shares from SoA staging (InPtrs::lin_ld)
  bool fuse_acc;     // the accumulate rides on k_leader_prep (option leader_fuse_acc)
};
LeaderPlan plan_leader(const prio3_engine* e);
// the helper's kernel chain over the whole run
int prepare_run(prio3_engine* e, Run* R, InPtrs in, OutPtrs out, hipStream_t st, bool fuse,
                bool allow_chunks, const PullRanges* pull = nullptr);
// the leader's prepare_init (agg_id 0) over the run; lin_ld: InPtrs::lin_ld
int leader_init_run(prio3_engine* e, Run* R, const uint8_t* d_nonces,
                    const uint8_t* d_public_shares, const uint8_t* d_leader_input_shares,
                    uint8_t* d_prep_shares, uint8_t* d_status, hipStream_t st,
                    const uint16_t* vk_slot = nullptr, const uint4* vk_tab = nullptr,
                    uint32_t lin_ld = 0);

// ---- prio3_accumulate.hip ----
// One-pass segmented accumulate over columns [c0, c0 + n) of a run: d_status[n] (the run's
// verdicts for those columns), d_seg[n] (nullable: segment 0), d_accept[n] (nullable: all
// accepted); d_agg[nseg][out_len * es], d_counts[nseg].
int run_accumulate(prio3_engine* e, Run* R, uint32_t c0, uint32_t n, const uint8_t* d_status,
                   const uint32_t* d_seg, const uint8_t* d_accept, uint32_t nseg, uint8_t* d_agg,
                   uint64_t* d_counts, hipStream_t st);
int fused_finish(prio3_engine* e, Run* R, const uint8_t* d_status, const uint32_t* seg,
                 const uint32_t* fix_seg, const uint8_t* d_accept_mask, uint32_t S,
                 uint8_t* d_agg_shares, uint64_t* d_counts, hipStream_t st);
// The accumulate of a group of n_jobs jobs (descriptors, segment ids and accept bytes staged in
// `host` as AccLayout lays them out) enqueued on st: the staged inputs into a device area from
// the scratch pool, k_acc_multi, the first out_bytes of the outputs back into `host`.  Returns
// the area (the caller releases it after the stream), or nullptr with *rc set.
// area (optional): the device area, acquired by the caller and already holding the group's segment
// ids and accept bytes (an indexed prepare_next group: its index kernel wrote them) -- then only
// the descriptors are copied in, so the staging's unset ids never land on them.
Slab* acc_multi_enqueue(int device, uint32_t es, uint8_t* host, const AccLayout& L,
                        uint32_t n_jobs, size_t out_bytes, hipStream_t st, int* rc,
                        Slab* area = nullptr);
int launch_combine(prio3_engine* e, uint32_t k, uint32_t n_segments, const uint8_t* d_in,
                   const uint64_t* d_counts_in, uint8_t* d_out, uint64_t* d_counts_out,
                   hipStream_t st);
int launch_batch_metadata(prio3_engine* e, uint32_t n, const uint8_t* d_report_ids,
                          const uint64_t* d_times, const uint8_t* d_status,
                          const uint8_t* d_accept_mask, const uint32_t* d_segment_ids,
                          uint32_t n_segments, uint32_t* ck, unsigned long long* iv,
                          hipStream_t st);
int launch_combine_metadata(prio3_engine* e, uint32_t k, uint32_t n_segments,
                            const uint32_t* ck_in, const unsigned long long* iv_in,
                            uint32_t* ck_out, unsigned long long* iv_out, hipStream_t st);

// ---- prio3_jobindex.hip ----
// k_jix_group over the n_jobs descriptors of a group of prio3_helper_aggregate_job jobs, one
// workgroup per job: desc / closed / ids / times / accept are the staged inputs (mapped), ids_dev
// a device copy of the IDs it leaves for its own probes and the metadata launch, gseg / gaccept
// the run's group segment ids and accept bytes (every column of the group is written), and
// seg_out .. info_out the index outputs in the staging.
struct JixGroupArgs {
  const JixJobDesc* desc;
  const unsigned long long* closed;
  const uint8_t* ids;
  const unsigned long long* times;
  const uint8_t* accept;
  uint8_t* ids_dev;
  uint32_t* gseg;
  uint8_t* gaccept;
  uint32_t* seg_out;
  uint8_t *rej_out, *dup_out;
  unsigned long long* starts_out;
  prio3_job_index_info* info_out;
  // k_jix_lgroup (a group of prio3_leader_finish_job jobs, columns = the group's report offsets,
  // no pad columns): the job-local segment ids k_acc_multi reads and the reject bytes the check
  // reads for the outcome, both in device memory
  uint32_t* lseg = nullptr;
  uint8_t* drej = nullptr;
};
// leader: k_jix_lgroup (the same device body, plus lseg / drej)
int launch_jix_group(prio3_engine* e, uint32_t n_jobs, const JixGroupArgs& a, hipStream_t st,
                     bool leader = false);

// ---- prio3_client.hip: the generic leader kernels ----
extern "C" int launch_leader_init(const DevParams& dp, const uint8_t* d_nonces,
                                  const uint8_t* d_pub, const uint8_t* d_lshares,
                                  const Scratch& sc, uint8_t* d_prep_shares, uint8_t* d_status,
                                  hipStream_t st, const uint16_t* vk_slot, const uint4* vk_tab);
extern "C" int launch_leader_next(const DevParams& dp, const uint8_t* d_prep_msgs,
                                  const Scratch& sc, uint8_t* d_status, hipStream_t st);
// What the check of an indexed group (prio3_leader_finish_job) reads and writes beside the
// staging's statuses, per report of the group: perr the staged prepare_error bytes, drej the index
// kernel's reject bytes (device), mstatus the merged statuses for the metadata launch (device),
// outcome the staged outcome bytes.
struct LNextJixPtrs {
  const uint8_t* perr = nullptr;
  const uint8_t* drej = nullptr;
  uint8_t* mstatus = nullptr;
  uint8_t* outcome = nullptr;
};
extern "C" int launch_leader_next_multi(uint32_t es, const LNextDesc* d_desc,
                                        const uint8_t* d_msgs, uint8_t* d_status, uint32_t n_jobs,
                                        uint32_t max_n, hipStream_t st,
                                        const LNextJixPtrs* jix = nullptr);

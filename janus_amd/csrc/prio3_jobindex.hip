// prio3_jobindex.hip -- the job index: the per-report bookkeeping between the unpack / upload and
// the prepare of a device-resident aggregation job (prio3_device_job_index, janus_prio3.h):
//   segment ids     TimeInterval::to_batch_identifier (aggregator_core/src/query_type.rs:72-82,
//                   Time::to_batch_interval_start, core/src/time.rs:207-224) collected as the
//                   writer's by_batch_identifier_index (aggregation_job_writer.rs:598);
//   accept mask     fail_report_aggregations_for_collected_batches (aggregation_job_writer.rs:
//                   540-588): PrepareError::BatchCollected for a report of a closed batch;
//   duplicate IDs   the HashSet over every PrepareInit of an init request (aggregator.rs:
//                   1765-1773).
// The kernels run on the caller's stream, ordered by their launch boundaries only -- no kernel
// waits on another workgroup:
//   k_jix_init    empties the two hash tables and the counters (k_jix_closed_put: the host's
//                 closed intervals, carried as kernel arguments, into scratch);
//   k_jix_insert  one lane per report.  Starts: equal starts are collapsed inside the wave (ballot
//                 loop) and the lowest lane of each class inserts the start into an
//                 open-addressing table of 64-bit keys with a compare-and-swap, counting the keys
//                 found.  IDs: every lane inserts its index into a table of report indices, keyed
//                 by the 16 ID bytes (compared by plain loads of the never-written input); a slot
//                 keeps the lowest index of its ID (atomicMin);
//   k_jix_rank    one workgroup: the found starts sorted in LDS (bitonic), d_segment_starts, the
//                 closed flag of each segment from the k intervals, the rank of each table slot,
//                 and the info struct's first values;
//   k_jix_assign  one lane per report (grid-stride): rank and closed flag of its start, the slot
//                 of its ID, the per-report outputs, and the info counters with one atomic per
//                 block.
// Every probe loop is bounded by its table's capacity.  The outputs are a pure function of the
// inputs: the tables' contents after k_jix_insert do not depend on the order of arrival (the key
// set; per ID the lowest index), except which slot a key sits in, which no output shows.
#include <algorithm>

#include "prio3_host.h"

namespace {

// The "empty" marks.  A start of 2^64 - 1 is never inserted: start + precision then overflows
// for every precision >= 1, which makes the report a time error before the insert.  A report
// index of 2^32 - 1 cannot occur: n <= 2^30.
constexpr unsigned long long JIX_NO_KEY = ~0ull;
constexpr uint32_t JIX_NO_INDEX = 0xffffffffu;
constexpr uint32_t JIX_MAX_SEG = 4096, JIX_MAX_CLOSED = 1024;
constexpr uint32_t JIX_RANK_T = 1024;  // threads of k_jix_rank
constexpr uint32_t JIX_CLOSED_BIT = 0x80000000u;
constexpr uint32_t JIX_PUT = 128;  // intervals per k_jix_closed_put launch (2 KiB of arguments)
constexpr uint32_t JIX_ASSIGN_BLOCKS = 1024;  // k_jix_assign's grid: 4 blocks per CU

struct JixCtl {  // zeroed by k_jix_init
  uint32_t found;  // distinct starts inserted (may pass max_segments by the inserts in flight)
  uint32_t pad[3];
};

struct JixTables {
  unsigned long long* keys;  // [scap] starts, JIX_NO_KEY = empty
  uint32_t* rank;            // [scap] rank of the slot's start | JIX_CLOSED_BIT
  uint32_t* slots;           // [icap] lowest report index of the slot's ID, JIX_NO_INDEX = empty
  JixCtl* ctl;
  const unsigned long long* closed;  // [k][2] (start, duration)
  uint32_t smask, imask;     // capacities - 1 (powers of two)
};

struct JixClosedChunk {
  unsigned long long v[JIX_PUT][2];
};

DEV uint32_t jix_hash_start(unsigned long long x) {  // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return (uint32_t)x;
}

DEV uint32_t jix_hash_id(const uint4& v) {  // every byte of the ID reaches every bit of the hash
  uint32_t x = v.x * 0x9e3779b1u;
  x = (x ^ (x >> 15) ^ v.y) * 0x85ebca6bu;
  x = (x ^ (x >> 13) ^ v.z) * 0xc2b2ae35u;
  x = (x ^ (x >> 16) ^ v.w) * 0x27d4eb2fu;
  return x ^ (x >> 15);
}

DEV bool jix_same(const uint4& a, const uint4& b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

DEV uint4 jix_id(const uint8_t* ids, uint32_t i) { return *(const uint4*)(ids + 16 * (size_t)i); }

// start of the report's batch interval; false: start + precision overflows a u64 (Interval::new)
DEV bool jix_start(unsigned long long t, unsigned long long precision, unsigned long long* start) {
  *start = t - t % precision;
  return *start <= ~0ull - precision;
}

__global__ __launch_bounds__(256) void k_jix_init(JixTables T, size_t key_quads,
                                                  size_t slot_quads) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (size_t q = t0; q < slot_quads; q += stride) ((uint4*)T.slots)[q] = ones;
  for (size_t q = t0; q < key_quads; q += stride) ((uint4*)T.keys)[q] = ones;
  if (t0 == 0) *(uint4*)T.ctl = make_uint4(0, 0, 0, 0);
}

__global__ void k_jix_closed_put(unsigned long long* closed, uint32_t first, uint32_t count,
                                 JixClosedChunk c) {
  const uint32_t t = threadIdx.x;
  if (t < count) {
    closed[2 * (size_t)(first + t)] = c.v[t][0];
    closed[2 * (size_t)(first + t) + 1] = c.v[t][1];
  }
}

__global__ __launch_bounds__(256) void k_jix_insert(uint32_t n, const uint8_t* ids,
                                                    const unsigned long long* times,
                                                    unsigned long long precision,
                                                    uint32_t max_segments, JixTables T) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
  const bool valid = i < n;
  if (precision) {
    unsigned long long start = 0;
    bool pending = valid && jix_start(times[valid ? i : 0], precision, &start);
    bool first = false;  // the lowest lane of the wave with this start
    unsigned long long m;
    while ((m = __ballot(pending))) {  // wave-uniform: one trip per distinct start of the wave
      const int l = __ffsll((long long)m) - 1;
      const unsigned long long key = __shfl(start, l);
      if (pending && start == key) {
        first = lane == (uint32_t)l;
        pending = false;
      }
    }
    if (first) {
      uint32_t h = jix_hash_start(start) & T.smask;
      for (uint32_t p = 0; p <= T.smask; p++) {
        // at its limit: more than max_segments starts are known, the call ends in overflow.
        // (Reading the slot first and the count only on a miss was slower in an alternating A/B:
        // 176 / 258 / 194 us against 130 / 153 / 145 us at 1 Mi reports in 1 / 8 / 1,024 buckets.)
        if (__hip_atomic_load(&T.ctl->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >
            max_segments)
          break;
        unsigned long long cur =
            __hip_atomic_load(T.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == JIX_NO_KEY) {
          cur = atomicCAS(T.keys + h, JIX_NO_KEY, start);
          if (cur == JIX_NO_KEY) {
            atomicAdd(&T.ctl->found, 1u);
            break;
          }
        }
        if (cur == start) break;
        h = (h + 1) & T.smask;
      }
    }
  }
  if (valid) {
    const uint4 id = jix_id(ids, i);
    uint32_t h = jix_hash_id(id) & T.imask;
    for (uint32_t p = 0; p <= T.imask; p++) {
      uint32_t j = __hip_atomic_load(T.slots + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (j == JIX_NO_INDEX) {
        j = atomicCAS(T.slots + h, JIX_NO_INDEX, i);
        if (j == JIX_NO_INDEX) break;
      }
      // j < n: a slot only ever holds indices of reports
      if (jix_same(jix_id(ids, j), id)) {
        if (i < j) atomicMin(T.slots + h, i);
        break;
      }
      h = (h + 1) & T.imask;
    }
  }
}

// One workgroup.  fixed: a fixed-size task (time_precision 0) -- only the info struct is written.
__global__ __launch_bounds__(JIX_RANK_T) void k_jix_rank(uint32_t n, uint32_t fixed,
                                                         uint32_t max_segments, uint32_t k,
                                                         JixTables T,
                                                         unsigned long long* seg_starts,
                                                         prio3_job_index_info* info) {
  __shared__ unsigned long long s_key[JIX_MAX_SEG];
  __shared__ uint8_t s_closed[JIX_MAX_SEG];
  __shared__ uint32_t s_count;
  const uint32_t tid = threadIdx.x;
  const uint32_t found = fixed ? (n ? 1u : 0u) : T.ctl->found;
  const bool overflow = found > max_segments;
  if (tid == 0) {
    info->n_segments = overflow ? max_segments + 1 : found;
    info->overflow = overflow ? 1u : 0u;
    info->n_duplicates = 0;
    info->first_duplicate = 0xffffffffu;
    info->n_closed = 0;
    info->n_time_errors = 0;
    s_count = 0;
  }
  if (fixed) return;
  if (overflow) {  // block-uniform; which starts reached the table is not defined: none is used
    if (seg_starts)
      for (uint32_t s = tid; s < max_segments; s += JIX_RANK_T) seg_starts[s] = 0;
    return;
  }
  __syncthreads();
  // found <= max_segments <= JIX_MAX_SEG keys are in the table
  for (uint32_t h = tid; h <= T.smask; h += JIX_RANK_T) {
    const unsigned long long key = T.keys[h];
    if (key != JIX_NO_KEY) {
      const uint32_t at = atomicAdd(&s_count, 1u);
      if (at < JIX_MAX_SEG) s_key[at] = key;
    }
  }
  uint32_t P = 1;  // the sort's size: the keys padded with JIX_NO_KEY to a power of two
  while (P < found) P <<= 1;
  for (uint32_t s = found + tid; s < P; s += JIX_RANK_T) s_key[s] = JIX_NO_KEY;
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t step = size >> 1; step > 0; step >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += JIX_RANK_T) {
        const uint32_t lo = 2 * t - (t & (step - 1)), hi = lo + step;  // lo has bit `step` clear
        const bool up = (lo & size) == 0;
        const unsigned long long a = s_key[lo], b = s_key[hi];
        if ((a > b) == up) {
          s_key[lo] = b;
          s_key[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t s = tid; s < max_segments; s += JIX_RANK_T) {
    bool closed = false;
    if (s < found) {
      const unsigned long long start = s_key[s];
      for (uint32_t j = 0; j < k; j++) {
        const unsigned long long a = T.closed[2 * j], d = T.closed[2 * j + 1];
        closed |= start >= a && start - a < d;  // [a, a + d), no wrap-around
      }
    }
    if (s < JIX_MAX_SEG) s_closed[s] = closed;
    if (seg_starts) seg_starts[s] = s < found ? s_key[s] : 0;
  }
  __syncthreads();
  for (uint32_t h = tid; h <= T.smask; h += JIX_RANK_T) {
    const unsigned long long key = T.keys[h];
    if (key == JIX_NO_KEY) continue;
    uint32_t lo = 0, hi = found;  // the first s with s_key[s] >= key
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_key[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    T.rank[h] = lo | (s_closed[lo < JIX_MAX_SEG ? lo : 0] ? JIX_CLOSED_BIT : 0u);
  }
}

__global__ __launch_bounds__(256) void k_jix_assign(uint32_t n, const uint8_t* ids,
                                                    const unsigned long long* times,
                                                    unsigned long long precision,
                                                    uint32_t max_segments, JixTables T,
                                                    uint32_t* seg_ids, uint8_t* accept,
                                                    uint8_t* reject, uint8_t* duplicate,
                                                    prio3_job_index_info* info) {
  __shared__ uint32_t s_part[4][4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool overflow = info->overflow != 0;  // written by k_jix_rank, constant in this launch
  // the wave's counts (wave-uniform) and its lowest duplicate index: its indices ascend with the
  // trips, so that is the first one it meets
  uint32_t c_dup = 0, c_closed = 0, c_err = 0, first_dup = 0xffffffffu;
  // grid-stride over tiles of 256 reports (n <= 2^30: no index wraps)
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < n;
    uint32_t seg = 0xffffffffu;
    bool time_error = false, closed = false;
    if (valid) {
      if (!precision) {
        seg = 0;
      } else {
        unsigned long long start;
        time_error = !jix_start(times[i], precision, &start);
        if (!time_error && !overflow) {
          uint32_t h = jix_hash_start(start) & T.smask;
          for (uint32_t p = 0; p <= T.smask; p++) {
            const unsigned long long cur = T.keys[h];
            if (cur == start) {
              const uint32_t r = T.rank[h];
              seg = r & ~JIX_CLOSED_BIT;
              closed = (r & JIX_CLOSED_BIT) != 0;
              break;
            }
            if (cur == JIX_NO_KEY) break;
            h = (h + 1) & T.smask;
          }
          if (seg >= max_segments) {  // not reached without overflow; keeps later calls in bounds
            seg = 0xffffffffu;
            closed = false;
          }
        }
      }
      seg_ids[i] = seg;
      accept[i] = seg != 0xffffffffu && !closed;
      if (reject) reject[i] = closed ? PRIO3_REJECT_BATCH_COLLECTED : 0;
    }
    bool dup = false;
    if (valid) {
      const uint4 id = jix_id(ids, i);
      uint32_t h = jix_hash_id(id) & T.imask;
      for (uint32_t p = 0; p <= T.imask; p++) {
        const uint32_t j = T.slots[h];
        if (j == i || j == JIX_NO_INDEX) break;
        if (jix_same(jix_id(ids, j < n ? j : i), id)) {
          dup = true;  // the slot holds the ID's lowest index, and it is not this report
          break;
        }
        h = (h + 1) & T.imask;
      }
      if (duplicate) duplicate[i] = dup;
    }
    const unsigned long long m_dup = __ballot(dup), m_closed = __ballot(closed),
                             m_err = __ballot(time_error);
    if (m_dup && first_dup == 0xffffffffu)
      first_dup = i - lane + (uint32_t)(__ffsll((long long)m_dup) - 1);
    c_dup += (uint32_t)__popcll(m_dup);
    c_closed += (uint32_t)__popcll(m_closed);
    c_err += (uint32_t)__popcll(m_err);
  }
  // One atomic per block and counter: with one per wave, the 16 Ki waves of a 1 Mi job whose
  // every wave holds a closed report serialised on n_closed (the kernel took 200 us, not 60).
  if (lane == 0) {
    s_part[wv][0] = c_dup;
    s_part[wv][1] = first_dup;
    s_part[wv][2] = c_closed;
    s_part[wv][3] = c_err;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t d = 0, f = 0xffffffffu, c = 0, t = 0;
    for (uint32_t w = 0; w < 4; w++) {
      d += s_part[w][0];
      f = s_part[w][1] < f ? s_part[w][1] : f;
      c += s_part[w][2];
      t += s_part[w][3];
    }
    if (d) {
      atomicAdd(&info->n_duplicates, d);
      atomicMin(&info->first_duplicate, f);
    }
    if (c) atomicAdd(&info->n_closed, c);
    if (t) atomicAdd(&info->n_time_errors, t);
  }
}

// ---- the job index of a group of host-buffer jobs (prio3_helper_aggregate_job) ----
// One workgroup per job, everything in LDS, first on the group's stream: only the launch order
// orders it against the open, the prepare and the accumulate that read what it writes.  The same
// steps as the four kernels above at job size (n <= JIX_GROUP_MAX_N reports, max_segments <=
// JIX_GROUP_MAX_SEG):
//   IDs      the job's staged IDs are copied into the run (ids_dev) and every report inserts its
//            index into s_slot, 2 next_pow2(n) slots keyed by the 16 ID bytes, atomicMin keeping
//            the lowest index of an ID -- so duplicate[i] is "some j < i has these bytes";
//   starts   every report inserts its start into s_tab (a compare-and-swap on 64-bit keys, 4 x
//            JIX_GROUP_MAX_SEG slots: at most half full below the overflow limit), the distinct
//            ones are gathered into s_key, sorted (bitonic) and the closed flag of each is decided
//            once against the job's k intervals;
//   reports  the rank of each report's start by binary search: R->gseg = seg0 + rank (or
//            0xFFFFFFFF), R->gaccept = index accept & staged host accept, and into the staging the
//            job-local segment ids, reject, duplicate, segment starts and the info struct.
// Every probe loop is bounded by its table; the outputs do not depend on the order of arrival.
constexpr uint32_t JIXG_T = 256;
constexpr uint32_t JIXG_SLOTS = 2 * JIX_GROUP_MAX_N;   // 32 KiB of report indices
constexpr uint32_t JIXG_TAB = 4 * JIX_GROUP_MAX_SEG;   // start table (2 KiB)
constexpr uint32_t JIXG_KEYS = 2 * JIX_GROUP_MAX_SEG;  // sorted starts, padded to a power of two

// LEADER: the sibling for groups of prio3_leader_finish_job jobs (k_jix_lgroup) -- the columns are
// the group's report offsets (no pad columns: pad0 = c0, end = c0 + n), and each report also gets
// its job-local segment id in A.lseg (what k_acc_multi reads beside A.gaccept) and its reject byte
// in A.drej (what the check reads for the outcome), both in device memory.
template <bool LEADER>
__device__ __forceinline__ void jix_group_body(const JixGroupArgs& A) {
  __shared__ uint32_t s_slot[JIXG_SLOTS];
  __shared__ unsigned long long s_tab[JIXG_TAB];
  __shared__ unsigned long long s_key[JIXG_KEYS];
  __shared__ uint8_t s_closed[JIX_GROUP_MAX_SEG];
  __shared__ uint32_t s_found, s_count, s_dup, s_first, s_nclosed, s_err;
  const JixJobDesc D = A.desc[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  // the host checked the limits; a descriptor outside them writes its columns as excluded
  const bool sane = D.n <= JIX_GROUP_MAX_N && D.max_segments >= 1 &&
                    D.max_segments <= JIX_GROUP_MAX_SEG && D.k <= JIX_MAX_CLOSED;
  const uint32_t n = sane ? D.n : 0u, S = sane ? D.max_segments : 0u;
  const unsigned long long precision = D.precision;
  const uint8_t* ids = A.ids_dev + 16 * (size_t)D.c0;  // the job's IDs once they are copied
  const unsigned long long* times = A.times + D.c0;
  uint32_t icap = 4;
  while (icap < 2 * n) icap <<= 1;  // <= JIXG_SLOTS
  const uint32_t imask = icap - 1, tmask = JIXG_TAB - 1;
  // pad columns before and after the job's reports (and all of an insane job's): excluded
  for (uint32_t c = D.pad0 + tid; c < D.end; c += JIXG_T)
    if (c < D.c0 || c >= D.c0 + n) {
      A.gseg[c] = 0xffffffffu;
      A.gaccept[c] = 0;
    }
  for (uint32_t h = tid; h < icap; h += JIXG_T) s_slot[h] = JIX_NO_INDEX;
  for (uint32_t h = tid; h < JIXG_TAB; h += JIXG_T) s_tab[h] = JIX_NO_KEY;
  if (tid == 0) {
    s_found = 0;
    s_count = 0;
    s_dup = 0;
    s_first = 0xffffffffu;
    s_nclosed = 0;
    s_err = 0;
  }
  for (uint32_t i = tid; i < n; i += JIXG_T)
    *(uint4*)(A.ids_dev + 16 * (size_t)(D.c0 + i)) =
        *(const uint4*)(A.ids + 16 * (size_t)(D.c0 + i));
  __threadfence_block();
  __syncthreads();
  for (uint32_t i = tid; i < n; i += JIXG_T) {
    unsigned long long start;
    if (precision && jix_start(times[i], precision, &start)) {
      uint32_t h = jix_hash_start(start) & tmask;
      for (uint32_t p = 0; p <= tmask; p++) {
        if (__hip_atomic_load(&s_found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > S)
          break;  // more than max_segments starts are known: the job ends in overflow
        unsigned long long cur = atomicCAS(s_tab + h, JIX_NO_KEY, start);
        if (cur == JIX_NO_KEY) {
          atomicAdd(&s_found, 1u);
          break;
        }
        if (cur == start) break;
        h = (h + 1) & tmask;
      }
    }
    const uint4 id = jix_id(ids, i);
    uint32_t h = jix_hash_id(id) & imask;
    for (uint32_t p = 0; p <= imask; p++) {
      const uint32_t j = atomicCAS(s_slot + h, JIX_NO_INDEX, i);
      if (j == JIX_NO_INDEX) break;
      if (jix_same(jix_id(ids, j < n ? j : i), id)) {  // j < n: a slot only holds report indices
        if (i < j) atomicMin(s_slot + h, i);
        break;
      }
      h = (h + 1) & imask;
    }
  }
  __syncthreads();
  const uint32_t found = precision ? s_found : (n ? 1u : 0u);
  const bool overflow = found > S;  // block-uniform
  if (precision && !overflow) {
    // found <= max_segments keys are in the table: gathered, padded to a power of two, sorted
    for (uint32_t h = tid; h < JIXG_TAB; h += JIXG_T) {
      const unsigned long long key = s_tab[h];
      if (key != JIX_NO_KEY) {
        const uint32_t at = atomicAdd(&s_count, 1u);
        if (at < JIXG_KEYS) s_key[at] = key;
      }
    }
    uint32_t P = 1;
    while (P < found) P <<= 1;  // <= JIX_GROUP_MAX_SEG
    for (uint32_t s = found + tid; s < P; s += JIXG_T) s_key[s] = JIX_NO_KEY;
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
      for (uint32_t step = size >> 1; step > 0; step >>= 1) {
        for (uint32_t t = tid; t < P / 2; t += JIXG_T) {
          const uint32_t lo = 2 * t - (t & (step - 1)), hi = lo + step;  // lo has bit `step` clear
          const bool up = (lo & size) == 0;
          const unsigned long long a = s_key[lo], b = s_key[hi];
          if ((a > b) == up) {
            s_key[lo] = b;
            s_key[hi] = a;
          }
        }
        __syncthreads();
      }
    }
    for (uint32_t s = tid; s < S; s += JIXG_T) {
      bool closed = false;
      if (s < found) {
        const unsigned long long start = s_key[s];
        for (uint32_t j = 0; j < D.k; j++) {
          const unsigned long long a = A.closed[2 * (size_t)(D.closed0 + j)],
                                   d = A.closed[2 * (size_t)(D.closed0 + j) + 1];
          closed |= start >= a && start - a < d;  // [a, a + d), no wrap-around
        }
      }
      s_closed[s] = closed;
      A.starts_out[D.seg0 + s] = s < found ? s_key[s] : 0;
    }
  } else if (precision) {  // overflow: which starts reached the table is not defined
    for (uint32_t s = tid; s < S; s += JIXG_T) A.starts_out[D.seg0 + s] = 0;
  }
  __syncthreads();
  for (uint32_t base = 0; base < n; base += JIXG_T) {  // whole waves: the ballots below
    const uint32_t i = base + tid;
    const bool valid = i < n;
    uint32_t seg = 0xffffffffu;
    bool time_error = false, closed = false, dup = false;
    if (valid) {
      if (!precision) {
        seg = 0;
      } else {
        unsigned long long start;
        time_error = !jix_start(times[i], precision, &start);
        if (!time_error && !overflow) {
          uint32_t lo = 0, hi = found;  // the first s with s_key[s] >= start
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_key[mid] < start) lo = mid + 1;
            else hi = mid;
          }
          if (lo < found && lo < S && s_key[lo] == start) {
            seg = lo;
            closed = s_closed[lo] != 0;
          }
        }
      }
      const uint4 id = jix_id(ids, i);
      uint32_t h = jix_hash_id(id) & imask;
      for (uint32_t p = 0; p <= imask; p++) {
        const uint32_t j = s_slot[h];
        if (j == i || j == JIX_NO_INDEX) break;
        if (jix_same(jix_id(ids, j < n ? j : i), id)) {
          dup = true;  // the slot holds the ID's lowest index, and it is not this report
          break;
        }
        h = (h + 1) & imask;
      }
      const uint32_t c = D.c0 + i;
      const bool acc = seg != 0xffffffffu && !closed;
      A.gseg[c] = seg != 0xffffffffu ? D.seg0 + seg : 0xffffffffu;
      A.gaccept[c] = acc && A.accept[c] != 0;
      A.seg_out[c] = seg;
      A.rej_out[c] = closed ? PRIO3_REJECT_BATCH_COLLECTED : 0;
      A.dup_out[c] = dup;
      if (LEADER) {
        A.lseg[c] = seg;
        A.drej[c] = closed ? PRIO3_REJECT_BATCH_COLLECTED : 0;
      }
    }
    const unsigned long long m_dup = __ballot(dup), m_closed = __ballot(closed),
                             m_err = __ballot(time_error);
    if ((tid & 63u) == 0) {
      if (m_dup) {
        atomicAdd(&s_dup, (uint32_t)__popcll(m_dup));
        atomicMin(&s_first, i + (uint32_t)(__ffsll((long long)m_dup) - 1));
      }
      if (m_closed) atomicAdd(&s_nclosed, (uint32_t)__popcll(m_closed));
      if (m_err) atomicAdd(&s_err, (uint32_t)__popcll(m_err));
    }
  }
  __syncthreads();
  if (tid == 0) {
    prio3_job_index_info info;
    info.n_segments = overflow ? S + 1 : found;
    info.overflow = overflow ? 1u : 0u;
    info.n_duplicates = s_dup;
    info.first_duplicate = s_first;
    info.n_closed = s_nclosed;
    info.n_time_errors = s_err;
    A.info_out[blockIdx.x] = info;
  }
}

__global__ __launch_bounds__(JIXG_T) void k_jix_group(JixGroupArgs A) { jix_group_body<false>(A); }
__global__ __launch_bounds__(JIXG_T) void k_jix_lgroup(JixGroupArgs A) { jix_group_body<true>(A); }

uint32_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return (uint32_t)p;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int prio3_device_job_index(prio3_engine* e, uint32_t n, const uint8_t* d_report_ids,
                           const uint64_t* d_times, uint64_t time_precision,
                           const uint64_t* closed_intervals, uint32_t k, uint32_t max_segments,
                           uint32_t* d_segment_ids, uint64_t* d_segment_starts,
                           uint8_t* d_accept_mask, uint8_t* d_reject, uint8_t* d_duplicate,
                           prio3_job_index_info* d_info, void* stream) {
  TraceSpan span_("aggregation job index");
  if (!e || !d_info || n > (1u << 30) || max_segments == 0 || max_segments > JIX_MAX_SEG ||
      k > JIX_MAX_CLOSED || (k && !closed_intervals))
    return PRIO3_EINVAL;
  if (n && (!d_report_ids || !d_segment_ids || !d_accept_mask || (time_precision && !d_times)))
    return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  const uint32_t fixed = time_precision == 0;
  // 2 x next_pow2(max_segments + 1) keys: the table stays at most half full up to the overflow
  // limit; next_pow2(2 n) report indices (at least one 16-byte row for the initialising stores)
  const uint32_t scap = 2 * next_pow2((uint64_t)max_segments + 1);
  const uint32_t icap = std::max<uint32_t>(4, next_pow2(2 * (uint64_t)n));
  const size_t o_ctl = 0, o_keys = o_ctl + up256(sizeof(JixCtl)),
               o_rank = o_keys + up256(8 * (size_t)scap),
               o_closed = o_rank + up256(4 * (size_t)scap),
               o_slots = o_closed + up256(16 * (size_t)JIX_MAX_CLOSED),
               total = o_slots + up256(4 * (size_t)icap);
  int rc = PRIO3_OK;
  Slab* sl = ws_acquire(e->device, total, st, &rc);
  if (!sl) return rc;
  uint8_t* b = sl->base;
  JixTables T;
  T.ctl = (JixCtl*)(b + o_ctl);
  T.keys = (unsigned long long*)(b + o_keys);
  T.rank = (uint32_t*)(b + o_rank);
  T.closed = (const unsigned long long*)(b + o_closed);
  T.slots = (uint32_t*)(b + o_slots);
  T.smask = scap - 1;
  T.imask = icap - 1;
  const unsigned long long* times = (const unsigned long long*)d_times;
  rc = [&]() -> int {
    const size_t key_quads = (size_t)scap / 2, slot_quads = (size_t)icap / 4;
    const unsigned init_blocks =
        (unsigned)std::min<size_t>(2048, (std::max(key_quads, slot_quads) + 255) / 256);
    TIMED(e, st, "k_jix_init", (k_jix_init<<<init_blocks, 256, 0, st>>>(T, key_quads, slot_quads)));
    // the host's intervals travel as kernel arguments, so they are read before this call returns
    for (uint32_t first = 0; !fixed && first < k; first += JIX_PUT) {
      JixClosedChunk c;
      const uint32_t count = std::min(JIX_PUT, k - first);
      for (uint32_t j = 0; j < count; j++) {
        c.v[j][0] = closed_intervals[2 * (size_t)(first + j)];
        c.v[j][1] = closed_intervals[2 * (size_t)(first + j) + 1];
      }
      for (uint32_t j = count; j < JIX_PUT; j++) c.v[j][0] = c.v[j][1] = 0;
      TIMED(e, st, "k_jix_closed_put",
            (k_jix_closed_put<<<1, JIX_PUT, 0, st>>>((unsigned long long*)(b + o_closed), first,
                                                     count, c)));
    }
    const unsigned blocks = (n + 255) / 256;
    if (n)
      TIMED(e, st, "k_jix_insert",
            (k_jix_insert<<<blocks, 256, 0, st>>>(n, d_report_ids, times, time_precision,
                                                  max_segments, T)));
    TIMED(e, st, "k_jix_rank",
          (k_jix_rank<<<1, JIX_RANK_T, 0, st>>>(n, fixed, max_segments, fixed ? 0 : k, T,
                                                (unsigned long long*)d_segment_starts, d_info)));
    if (n)
      TIMED(e, st, "k_jix_assign",
            (k_jix_assign<<<std::min(blocks, JIX_ASSIGN_BLOCKS), 256, 0, st>>>(
                n, d_report_ids, times, time_precision, max_segments, T, d_segment_ids,
                d_accept_mask, d_reject, d_duplicate, d_info)));
    return PRIO3_OK;
  }();
  ws_release(sl, st);
  return rc;
}

int launch_jix_group(prio3_engine* e, uint32_t n_jobs, const JixGroupArgs& a, hipStream_t st,
                     bool leader) {
  static_assert(JIX_GROUP_MAX_N == PRIO3_JOB_GROUP_MAX_REPORTS &&
                    JIX_GROUP_MAX_SEG == PRIO3_JOB_GROUP_MAX_SEGMENTS,
                "the header's limits are the kernel's");
  if (!n_jobs) return PRIO3_OK;
  if (leader) {
    if (!a.lseg || !a.drej) return PRIO3_EINVAL;
    TIMED(e, st, "k_jix_lgroup", (k_jix_lgroup<<<n_jobs, JIXG_T, 0, st>>>(a)));
    return PRIO3_OK;
  }
  TIMED(e, st, "k_jix_group", (k_jix_group<<<n_jobs, JIXG_T, 0, st>>>(a)));
  return PRIO3_OK;
}

int prio3_job_index(prio3_engine* e, uint32_t n, const uint8_t* report_ids, const uint64_t* times,
                    uint64_t time_precision, const uint64_t* closed_intervals, uint32_t k,
                    uint32_t max_segments, uint32_t* segment_ids, uint64_t* segment_starts,
                    uint8_t* accept_mask, uint8_t* reject, uint8_t* duplicate,
                    prio3_job_index_info* info) {
  if (!e || !info || n > (1u << 30) || max_segments == 0 || max_segments > JIX_MAX_SEG ||
      k > JIX_MAX_CLOSED || (k && !closed_intervals))
    return PRIO3_EINVAL;
  if (n && (!report_ids || !segment_ids || !accept_mask || (time_precision && !times)))
    return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(e->device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  const size_t N = n ? n : 1, S = max_segments;
  const size_t o_ids = 0, o_t = o_ids + up256(16 * N), o_seg = o_t + up256(8 * N),
               o_starts = o_seg + up256(4 * N), o_acc = o_starts + up256(8 * S),
               o_rej = o_acc + up256(N), o_dup = o_rej + up256(N), o_info = o_dup + up256(N),
               total = o_info + up256(sizeof(prio3_job_index_info));
  int rc = PRIO3_OK;
  Slab* sl = ws_acquire(e->device, total, st, &rc);
  if (!sl) return rc;
  uint8_t* b = sl->base;
  auto h2d = [&](size_t off, const void* src, size_t bytes) {
    return !src || !bytes ||
           hipMemcpyAsync(b + off, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
  };
  auto d2h = [&](void* dst, size_t off, size_t bytes) {
    return !dst || !bytes ||
           hipMemcpyAsync(dst, b + off, bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
  };
  if (!h2d(o_ids, report_ids, 16 * (size_t)n) || !h2d(o_t, times, 8 * (size_t)n))
    rc = PRIO3_EDEVICE;
  if (rc == PRIO3_OK)
    rc = prio3_device_job_index(
        e, n, b + o_ids, times ? (const uint64_t*)(b + o_t) : nullptr, time_precision,
        closed_intervals, k, max_segments, (uint32_t*)(b + o_seg),
        segment_starts ? (uint64_t*)(b + o_starts) : nullptr, b + o_acc,
        reject ? b + o_rej : nullptr, duplicate ? b + o_dup : nullptr,
        (prio3_job_index_info*)(b + o_info), st);
  if (rc == PRIO3_OK &&
      (!d2h(segment_ids, o_seg, 4 * (size_t)n) ||
       !d2h(time_precision ? segment_starts : nullptr, o_starts, 8 * S) ||
       !d2h(accept_mask, o_acc, n) || !d2h(reject, o_rej, n) || !d2h(duplicate, o_dup, n) ||
       !d2h(info, o_info, sizeof(prio3_job_index_info)) ||
       hipStreamSynchronize(st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (e->timing) collect_times(e);
  ws_release(sl, st);
  return rc;
}

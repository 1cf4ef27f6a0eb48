// prio3_accumulate.hip -- MI355X (gfx950) aggregation of prepared reports into per-batch aggregate
// shares [aggregation_job_writer.rs:591-695]; the launch functions are declared in prio3_host.h.
//   run_accumulate     k_acc_seg + k_acc_fin / k_acc_fin_blk: masked, segmented mod-p reduction
//   acc_multi_enqueue  k_acc_multi: the same for many small jobs of different runs in one launch
//   fused_finish       k_agg_parts, k_agg_final / _s: from the wave partials the prepare kernels
//                      left (the fused accumulate's second half)
//   launch_combine, launch_batch_metadata, launch_combine_metadata   k_combine, k_meta*
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "prio3_host.h"
#include "sha256_device.h"

// Zero-fills up to 4 ranges in one launch (zero_ranges, prio3_host.h): the first zeroing of a
// fused run's accumulators where the run has no redo launch to do it (the leader's runs)
__global__ __launch_bounds__(256) void k_zero(ZeroRanges z) {
  zero_ranges(z, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// ------------------------------------------------------------------------------------
// Accumulate: masked segmented mod-p reduction of output shares
// ------------------------------------------------------------------------------------
// Per-report inclusion: a report counts in its segment if its status is FINISHED, the host mask
// is non-zero and its segment id is < n_segments.  A segment id past n_segments excludes the
// report from every aggregate and count, on every path (fused: k_agg_parts; metadata: k_meta).

// Segmented partial sums in one pass over the output shares.  grid: x = output element, y =
// report chunk, z = group of SG segments; each thread keeps SG running sums (one per segment of
// its group) and the block reduces them through LDS into partial[chunk][segment][element]
// (counts into pcount[chunk][segment] from the element-0 blocks).
// Inclusion is decided inline (status, segment id, accept mask; no separate code pass), so the
// accumulate is one launch plus k_acc_fin.
template <class F, int SG>
__global__ __launch_bounds__(256) void k_acc_seg(uint32_t n, size_t ld, uint32_t chunk,
                                                 uint32_t out_len, uint32_t nseg, const void* src,
                                                 const uint8_t* status, const uint32_t* seg,
                                                 const uint8_t* accept, void* partial,
                                                 uint64_t* pcount) {
  typedef typename F::T T;
  __shared__ T red[256];
  __shared__ uint32_t cred[256];
  const uint32_t e = blockIdx.x, c = blockIdx.y, s0 = blockIdx.z * SG;
  const uint32_t lo = c * chunk, hi = min(n, lo + chunk);
  T acc[SG];
  uint32_t cnt[SG];
#pragma unroll
  for (int q = 0; q < SG; q++) {
    acc[q] = F::zero();
    cnt[q] = 0;
  }
  for (uint32_t r = lo + threadIdx.x; r < hi; r += 256) {
    const uint32_t sr = seg ? seg[r] : 0u;
    const bool ok = status[r] == PRIO3_STATUS_FINISHED && sr < nseg && (!accept || accept[r]);
    const uint32_t k = (ok ? sr : 0xffffffffu) - s0;  // ~0 (excluded) wraps past SG
    if (k < (uint32_t)SG) {
      const T x = F::load(src, (size_t)e * ld + r);
#pragma unroll
      for (int q = 0; q < SG; q++)
        if ((uint32_t)q == k) {
          acc[q] = F::add(acc[q], x);
          cnt[q]++;
        }
    }
  }
#pragma unroll
  for (int q = 0; q < SG; q++) {
    if (s0 + q >= nseg) break;  // uniform
    red[threadIdx.x] = acc[q];
    cred[threadIdx.x] = cnt[q];
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
      if (threadIdx.x < st) {
        red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + st]);
        cred[threadIdx.x] += cred[threadIdx.x + st];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      F::store(partial, ((size_t)c * nseg + s0 + q) * out_len + e, red[0]);
      if (e == 0) pcount[(size_t)c * nseg + s0 + q] = cred[0];
    }
    __syncthreads();
  }
}

// grid (ceil(out_len / 256), nseg): per segment and element, the sum over the chunk partials
template <class F>
__global__ void k_acc_fin(uint32_t nchunks, uint32_t out_len, uint32_t nseg, const void* partial,
                          const uint64_t* pcount, uint8_t* agg, uint64_t* count) {
  typedef typename F::T T;
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (e < out_len) {
    T acc = F::zero();
    for (uint32_t c = 0; c < nchunks; c++)
      acc = F::add(acc, F::load(partial, ((size_t)c * nseg + s) * out_len + e));
    F::store(agg, (size_t)s * out_len + e, acc);
  }
  if (e == 0) {
    uint64_t t = 0;
    for (uint32_t c = 0; c < nchunks; c++) t += pcount[(size_t)c * nseg + s];
    count[s] = t;
  }
}


// k_acc_fin for the short outputs (Count, Sum: 2048-report chunks, so hundreds of partials per
// element): grid (out_len, nseg), the block's threads stride over the chunks and reduce in LDS
template <class F>
__global__ __launch_bounds__(256) void k_acc_fin_blk(uint32_t nchunks, uint32_t out_len,
                                                     uint32_t nseg, const void* partial,
                                                     const uint64_t* pcount, uint8_t* agg,
                                                     uint64_t* count) {
  typedef typename F::T T;
  __shared__ T red[256];
  __shared__ uint64_t cred[256];
  const uint32_t e = blockIdx.x, s = blockIdx.y;
  T acc = F::zero();
  uint64_t t = 0;
  for (uint32_t c = threadIdx.x; c < nchunks; c += 256) {
    acc = F::add(acc, F::load(partial, ((size_t)c * nseg + s) * out_len + e));
    if (e == 0) t += pcount[(size_t)c * nseg + s];
  }
  red[threadIdx.x] = acc;
  cred[threadIdx.x] = t;
  __syncthreads();
  for (uint32_t st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + st]);
      cred[threadIdx.x] += cred[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    F::store(agg, (size_t)s * out_len + e, red[0]);
    if (e == 0) count[s] = cred[0];
  }
}

// Accumulate of many small batches in one launch (the accumulate executor: concurrent
// prio3_accumulate calls of Janus's aggregation jobs).  grid: x = output element, y = job; the
// block sums its element over the job's reports (inclusion as k_acc_seg) into up to 8 segments at
// a time and writes the job's aggregate share element and, from element 0, its counts.
template <class F>
__global__ __launch_bounds__(256) void k_acc_multi(const AccDesc* descs, uint8_t* base) {
  typedef typename F::T T;
  __shared__ T red[256];
  __shared__ uint32_t cred[256];
  const AccDesc d = descs[blockIdx.y];
  const uint32_t e = blockIdx.x;
  if (e >= d.out_len) return;  // uniform per block
  const uint32_t* seg = (d.flags & 1) ? (const uint32_t*)(base + d.seg_off) : nullptr;
  const uint8_t* acc = (d.flags & 2) ? base + d.acc_off : nullptr;
  for (uint32_t s0 = 0; s0 < d.nseg; s0 += 8) {
    T a[8];
    uint32_t c[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      a[q] = F::zero();
      c[q] = 0;
    }
    for (uint32_t r = threadIdx.x; r < d.n; r += 256) {
      const uint32_t s = seg ? seg[r] : 0u;
      const bool inc = d.status[r] == PRIO3_STATUS_FINISHED && s < d.nseg && (!acc || acc[r]);
      const uint32_t k = s - s0;
      if (inc && k < 8u) {
        const T x = F::load(d.src, (size_t)e * d.ld + r);
#pragma unroll
        for (int q = 0; q < 8; q++)
          if ((uint32_t)q == k) {
            a[q] = F::add(a[q], x);
            c[q]++;
          }
      }
    }
    const uint32_t ns = min(8u, d.nseg - s0);
    for (uint32_t q = 0; q < ns; q++) {
      T v = F::zero();
      uint32_t cv = 0;
#pragma unroll
      for (int q2 = 0; q2 < 8; q2++)
        if ((uint32_t)q2 == q) {
          v = a[q2];
          cv = c[q2];
        }
      red[threadIdx.x] = v;
      cred[threadIdx.x] = cv;
      __syncthreads();
      for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
          red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + st]);
          cred[threadIdx.x] += cred[threadIdx.x + st];
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        F::store(base + d.agg_off, (size_t)(s0 + q) * d.out_len + e, red[0]);
        if (e == 0) ((uint64_t*)(base + d.cnt_off))[s0 + q] = cred[0];
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------
// Fused accumulate, second half: combine the per-wave half-limb partials per segment,
// then fix up exclusions / non-fused reports and reduce mod p.
// ------------------------------------------------------------------------------------
// k_agg_parts: one grid, two roles chosen by block index range.  The first fix_blocks blocks
// take the fix role (agg_fix_role: status scan, counts, fix-up list), the others the waves role
// (agg_waves_role: the wave partials).  The roles read disjoint inputs and write disjoint
// outputs, so neither waits for the other, and the status scan runs under the partials read
// where it was a launch of its own behind it; the fix blocks come first because each runs longer.
// Waves role, blocks (bx < ceil(M*8/1024), chunk of WCH waves): thread = 4 consecutive slots (element,
// half), read as one 16-byte load per wave (4x the bytes in flight of a slot per thread: the
// 1-slot version moved the 134 MB of a 1 Mi batch's wave partials at 1.8 TB/s).  A chunk whose
// fused waves all carry one segment writes 64-bit chunk partials (cseg[chunk] = its segment); a
// chunk mixing segments adds each run with a 64-bit atomic into agg64 directly (cseg = ~0, as
// for a chunk with no fused wave).
__device__ __forceinline__ void agg_waves_role(uint32_t bx, uint32_t c, uint32_t nwaves,
                                               uint32_t M, const uint32_t* wpart,
                                               const uint32_t* wseg, unsigned long long* cpart,
                                               uint32_t* cseg, unsigned long long* agg64) {
  static_assert(WCH <= 64, "one chunk's wave segments are read by one wave");
  const uint32_t slot = 4 * (bx * blockDim.x + threadIdx.x);
  const uint32_t w0 = c * WCH, w1 = min(nwaves, w0 + WCH), lane = threadIdx.x & 63u;
  // the chunk's wave segments in one load per lane (not a dependent scalar load per wave):
  // bit i of `fused` = wave w0 + i was fused; s0 = the first fused wave's segment
  const uint32_t my = w0 + lane < w1 ? wseg[w0 + lane] : 0xffffffffu;
  const uint64_t fused = __ballot(my != 0xffffffffu);
  const uint32_t s0 = fused ? (uint32_t)__shfl((int)my, __ffsll((long long)fused) - 1) : 0xffffffffu;
  const bool mixed = __any(my != 0xffffffffu && my != s0);
  if (slot == 0) cseg[c] = mixed ? 0xffffffffu : s0;
  if (s0 == 0xffffffffu) return;  // wave-uniform: no fused wave in the chunk
  // Lanes past the last slot (M * 8 is a multiple of 4, not of 256) stay alive through the mixed
  // path's readlane of `my` below: their loads are clamped to slot 0 and their atomics masked.
  const bool act = slot < M * 8;
  const uint32_t ls = act ? slot : 0u;
  const size_t row = (size_t)M * 8;
  if (!mixed) {
    if (!act) return;
    // all WCH loads independent and unconditional (clamped to the last wave, masked by bit)
    unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (uint32_t i = 0; i < WCH; i++) {
      const uint32_t w = min(w0 + i, w1 - 1);
      const uint4 v = *(const uint4*)(wpart + (size_t)w * row + slot);
      const uint32_t m = 0u - (uint32_t)((fused >> i) & 1u);
      a0 += v.x & m, a1 += v.y & m, a2 += v.z & m, a3 += v.w & m;
    }
    unsigned long long* o = cpart + (size_t)c * row + slot;
    o[0] = a0, o[1] = a1, o[2] = a2, o[3] = a3;
    return;
  }
  // segment runs inside the chunk (e.g. the executor's jobs of a few waves each): the loads in
  // batches of 8 waves, unconditional (clamped, masked), the run boundaries read from `my` by
  // shuffle (wave-uniform), one 64-bit atomic per run and slot
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  uint32_t cur = 0xffffffffu;
  auto flush = [&]() {
    if (cur == 0xffffffffu || !act) return;
    unsigned long long* o = agg64 + (size_t)cur * row + slot;
    if (a0) atomicAdd(o, a0);
    if (a1) atomicAdd(o + 1, a1);
    if (a2) atomicAdd(o + 2, a2);
    if (a3) atomicAdd(o + 3, a3);
  };
#pragma unroll 1
  for (uint32_t b = 0; b < WCH; b += 8) {
    uint4 v[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
      v[j] = *(const uint4*)(wpart + (size_t)min(w0 + b + j, w1 - 1) * row + ls);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
      // every lane of the wave is still active here (no early return above), so reading lane
      // b + j of `my` is well defined; ~0 = absent or unfused
      const uint32_t sg = (uint32_t)__builtin_amdgcn_readlane((int)my, (int)(b + j));
      if (sg == 0xffffffffu) continue;
      if (sg != cur) {
        flush();
        cur = sg;
        a0 = a1 = a2 = a3 = 0;
      }
      a0 += v[j].x, a1 += v[j].y, a2 += v[j].z, a3 += v[j].w;
    }
  }
  flush();
}

// Counts the reports the aggregate must contain (status FINISHED and accepted by the host
// mask) per segment and lists every report whose fused inclusion differs (entry = r, or
// r | 0x80000000 when it must be subtracted).  A block covers FIX_R consecutive reports and
// keeps its counts in a small LDS table keyed by segment, flushed with one atomic per entry.
// per: reports per block (1024 for large runs: a block's 4 trips end early enough to run under
// the waves role's partials read, where the 16 trips of a 4096-report block outlasted it; 512
// for the executor's 20-60k-report groups, whose larger blocks left most of the chip idle)
constexpr uint32_t FIX_T = 64;
static uint32_t fix_per(uint32_t n) { return n >= (1u << 18) ? 1024u : 512u; }
// oor_masked: the fused kernel masked lanes with an out-of-range segment id out of its wave
// partials (xofd_body); they are then not part of a fused wave's sum.  0: the wave partials
// include them (the fused leader unpack), so they are subtracted like any excluded report.
// fix: this finish's counter (Run::fix, one of the two); ents: the list; counts: Run::fcnt
struct AggFixArgs {
  uint32_t n;
  const uint8_t* status;
  const uint32_t* seg;
  const uint8_t* accept;
  uint32_t *fix, *ents;
  uint32_t fix_cap, nseg;
  unsigned long long* counts;
  uint32_t oor_masked, per, wshift;
};
__device__ __forceinline__ void agg_fix_role(uint32_t blk, const AggFixArgs& a,
                                             const uint32_t* wseg) {
  const uint32_t n = a.n, nseg = a.nseg, wshift = a.wshift, oor_masked = a.oor_masked;
  const uint32_t fix_cap = a.fix_cap, per = a.per;
  const uint8_t *status = a.status, *accept = a.accept;
  const uint32_t* seg = a.seg;
  uint32_t *fix = a.fix, *ents = a.ents;
  unsigned long long* counts = a.counts;
  __shared__ uint32_t tseg[FIX_T];
  __shared__ unsigned int tcnt[FIX_T];
  if (threadIdx.x < FIX_T) {
    tseg[threadIdx.x] = 0xffffffffu;
    tcnt[threadIdx.x] = 0;
  }
  __syncthreads();
  const uint32_t lo = blk * per, hi = min(n, lo + per);
  for (uint32_t base = lo; base < hi; base += 256) {
    const uint32_t r = base + threadIdx.x;
    const bool valid = r < hi;
    const uint32_t sg = valid ? (seg ? seg[r] : 0u) : 0xffffffffu;
    // out-of-range segment ids are excluded everywhere (as k_mask and k_meta do)
    const bool inc = valid && sg < nseg && status[r] == PRIO3_STATUS_FINISHED &&
                     (!accept || accept[r]);
    const bool fused = valid && wseg[r >> wshift] != 0xffffffffu && (!oor_masked || sg < nseg);
    const uint32_t s0 = (uint32_t)__shfl((int)sg, 0);
    const bool uni = __all(!valid || sg == s0);
    const unsigned long long b = __ballot(inc);
    auto add = [&](uint32_t s, unsigned int k) {
      const uint32_t h = s % FIX_T;
      const uint32_t old = atomicCAS(&tseg[h], 0xffffffffu, s);
      if (old == 0xffffffffu || old == s) atomicAdd(&tcnt[h], k);
      else atomicAdd(&counts[s], (unsigned long long)k);  // table collision
    };
    if (uni) {
      if ((threadIdx.x & 63u) == 0 && b) add(s0, (unsigned int)__popcll(b));
    } else if (inc) {
      add(sg, 1u);
    }
    if (valid && fused != inc) {
      const uint32_t i = atomicAdd(fix, 1u);
      if (i < fix_cap) ents[i] = r | (inc ? 0u : 0x80000000u);
    }
  }
  __syncthreads();
  if (threadIdx.x < FIX_T && tseg[threadIdx.x] != 0xffffffffu && tcnt[threadIdx.x])
    atomicAdd(&counts[tseg[threadIdx.x]], (unsigned long long)tcnt[threadIdx.x]);
}

// grid: fix_blocks + gx * nchunks blocks (see above)
__global__ __launch_bounds__(256) void k_agg_parts(uint32_t fix_blocks, uint32_t gx, AggFixArgs fa,
                                                   uint32_t nwaves, uint32_t M,
                                                   const uint32_t* wpart, const uint32_t* wseg,
                                                   unsigned long long* cpart, uint32_t* cseg,
                                                   unsigned long long* agg64) {
  if (blockIdx.x < fix_blocks) {  // block-uniform
    agg_fix_role(blockIdx.x, fa, wseg);
    return;
  }
  const uint32_t b = blockIdx.x - fix_blocks;
  agg_waves_role(b % gx, b / gx, nwaves, M, wpart, wseg, cpart, cseg, agg64);
}

DEV f128 fold_halves_impl(const unsigned long long (&Hs)[8]);
DEV f128 fold_halves(const unsigned long long (&Hs)[8]) { return fold_halves_impl(Hs); }

// One block per (segment, element): thread (half h = tid & 7, lane cl = tid >> 3) sums the chunk
// partials of its segment for chunks cl, cl+32, ...; then the fix-up list is applied by all
// 256 threads (lazily reduced signed sums), reduced through LDS, and thread 0 folds the
// half-limb totals X = sum_h H_h 2^(16h) (H_h < 2^48) mod p.
// The final kernels leave the run's accumulators clean for its next finish (no zeroing launch):
// each block zeroes the agg64 words it has read, the element-0 block of a segment moves the
// segment's count from the count row to counts[s] and zeroes it, and the first block zeroes the
// other generation's fix-up counter (fa.next), which no block of this finish reads.
struct AggFinalArgs {
  const uint32_t* nfix;  // this finish's fix-up counter
  const uint32_t* ents;  // the list
  uint32_t* next;        // the next finish's counter
  unsigned long long* fcnt;
  unsigned long long* counts;
};
__global__ __launch_bounds__(256) void k_agg_final(uint32_t M, size_t ld,
                                                   unsigned long long* agg64,
                                                   uint32_t nchunks,
                                                   const unsigned long long* cpart,
                                                   const uint32_t* cseg, AggFinalArgs fa,
                                                   const uint32_t* seg, const void* meas,
                                                   uint8_t* agg) {
  const uint32_t idx = blockIdx.x, s = idx / M, e = idx % M;
  const uint32_t tid = threadIdx.x, h = tid & 7u, cl = tid >> 3;
  __shared__ unsigned long long red[256];
  __shared__ f128 fadd[256], fsub[256];
  unsigned long long acc = 0;
  for (uint32_t c = cl; c < nchunks; c += 32)
    if (cseg[c] == s) acc += cpart[((size_t)c * M + e) * 8 + h];
  red[tid] = acc;
  // fix-up entries, strided over the block
  f128 ad = zero128(), sb = zero128();
  const uint32_t nfix = *fa.nfix;
  for (uint32_t i = tid; i < nfix; i += 256) {
    const uint32_t ent = fa.ents[i], r = ent & 0x7fffffffu;
    if ((seg ? seg[r] : 0u) != s) continue;
    const f128 x = Fp128::load(meas, (size_t)e * ld + r);
    if (ent & 0x80000000u) sb = add128(sb, x);
    else ad = add128(ad, x);
  }
  fadd[tid] = ad;
  fsub[tid] = sb;
  __syncthreads();
  for (uint32_t st = 128; st >= 8; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  // (an empty list, block-uniform: fadd[0] and fsub[0] are zero as they stand)
  for (uint32_t st = nfix ? 128 : 0; st >= 1; st >>= 1) {
    if (tid < st) {
      fadd[tid] = add128(fadd[tid], fadd[tid + st]);
      fsub[tid] = add128(fsub[tid], fsub[tid + st]);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  unsigned long long Hs[8];
  for (int hh = 0; hh < 8; hh++) {
    Hs[hh] = red[hh] + agg64[(size_t)idx * 8 + hh];
    agg64[(size_t)idx * 8 + hh] = 0;
  }
  if (e == 0) {
    fa.counts[s] = fa.fcnt[s];
    fa.fcnt[s] = 0;
  }
  if (idx == 0) *fa.next = 0;
  Fp128::store(agg, idx, sub128(add128(fold_halves(Hs), fadd[0]), fsub[0]));
}

// Runs with few chunks and many segments (the executor's groups: one segment per job, 2-8 waves
// each): one block per (segment, 32 elements), thread (element tid / 8, half h = tid % 8), so a
// block does not reduce 256 threads through LDS for one element; the fix-up list (empty when
// every wave fused) is split over the 8 halves and summed by shuffles.
__global__ __launch_bounds__(256) void k_agg_final_s(uint32_t M, size_t ld,
                                                     unsigned long long* agg64,
                                                     uint32_t nchunks,
                                                     const unsigned long long* cpart,
                                                     const uint32_t* cseg, AggFinalArgs fa,
                                                     const uint32_t* seg, const void* meas,
                                                     uint8_t* agg) {
  const uint32_t s = blockIdx.y, tid = threadIdx.x, h = tid & 7u, lane = tid & 63u;
  const uint32_t e = blockIdx.x * 32u + (tid >> 3);
  const bool live = e < M;
  const uint32_t ec = live ? e : 0u;
  unsigned long long H = 0;
  if (live) {  // (a dead thread's H is not used)
    H = agg64[((size_t)s * M + e) * 8 + h];
    agg64[((size_t)s * M + e) * 8 + h] = 0;
  }
  if (blockIdx.x == 0 && tid == 0) {
    fa.counts[s] = fa.fcnt[s];
    fa.fcnt[s] = 0;
    if (s == 0) *fa.next = 0;
  }
  for (uint32_t c = 0; c < nchunks; c++)
    if (cseg[c] == s) H += cpart[((size_t)c * M + ec) * 8 + h];
  f128 ad = zero128(), sb = zero128();
  const uint32_t nfix = *fa.nfix;
  for (uint32_t i = h; i < nfix; i += 8) {
    const uint32_t ent = fa.ents[i], r = ent & 0x7fffffffu;
    if ((seg ? seg[r] : 0u) != s) continue;
    const f128 x = Fp128::load(meas, (size_t)ec * ld + r);
    if (ent & 0x80000000u) sb = add128(sb, x);
    else ad = add128(ad, x);
  }
  if (nfix) {  // block-uniform
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
      f128 xa, xs;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        xa.w[k] = (uint32_t)__shfl_xor((int)ad.w[k], m);
        xs.w[k] = (uint32_t)__shfl_xor((int)sb.w[k], m);
      }
      ad = add128(ad, xa);
      sb = add128(sb, xs);
    }
  }
  unsigned long long Hs[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int src = (int)((lane & ~7u) + (uint32_t)k);
    Hs[k] = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(H >> 32), src) << 32) |
            (uint32_t)__shfl((int)(uint32_t)H, src);
  }
  if (h != 0 || !live) return;
  Fp128::store(agg, (size_t)s * M + e, sub128(add128(fold_halves(Hs), ad), sb));
}

// X = sum_h H_h 2^(16h) (H_h < 2^48) mod p
DEV f128 fold_halves_impl(const unsigned long long (&Hs)[8]) {
  uint32_t w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int hh = 0; hh < 8; hh++) {
    const unsigned long long H = Hs[hh];
    const int sh = 16 * hh, wi = sh >> 5, bi = sh & 31;
    const unsigned long long lo = bi ? (H << 16) & 0xffffffffull : H & 0xffffffffull;
    const unsigned long long mid = bi ? (H >> 16) & 0xffffffffull : H >> 32;
    const unsigned long long hi = bi ? H >> 48 : 0ull;
    unsigned long long c = (unsigned long long)w[wi] + lo;
    w[wi] = (uint32_t)c;
    c = (unsigned long long)w[wi + 1] + mid + (c >> 32);
    w[wi + 1] = (uint32_t)c;
    c = (unsigned long long)w[wi + 2] + hi + (c >> 32);
    w[wi + 2] = (uint32_t)c;
    for (int k = wi + 3; k < 9 && (c >> 32); k++) {
      c = (unsigned long long)w[k] + (c >> 32);
      w[k] = (uint32_t)c;
    }
  }
  return red288(w, w[8]);
}

// sum of k partial aggregates (multi-GPU combine)
template <class F>
__global__ void k_combine(uint32_t k, uint32_t len, uint32_t n_segments, const uint8_t* in,
                          const uint64_t* cin, uint8_t* out, uint64_t* cout) {
  typedef typename F::T T;
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < len) {
    T acc = F::zero();
    for (uint32_t i = 0; i < k; i++) acc = F::add(acc, F::load(in, (size_t)i * len + e));
    F::store(out, e, acc);
  }
  if (e < n_segments) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < k; i++) s += cin[(size_t)i * n_segments + e];
    cout[e] = s;
  }
}

// ------------------------------------------------------------------------------------
// Batch metadata of the per-segment BatchAggregation: besides the
// aggregate share and the count, every finished report XORs SHA-256(report_id) into the
// segment's ReportIdChecksum (core/src/report_id.rs:18-42, called from
// aggregation_job_writer.rs:650-656) and every report aggregation of the segment widens its
// client-timestamp interval (Interval::from_time + merge, core/src/time.rs:294-317; merged for
// failed reports too, aggregation_job_writer.rs:643-647).
// One report per lane: one SHA-256 compression of the padded 16-byte ID, then a block-level
// XOR / min / max reduction when a tile's 1024 reports share a segment (the common case:
// contiguous batches) and per-report atomics on the segment otherwise.
// ------------------------------------------------------------------------------------
// SHA-256 of the 16 bytes id[0..3] (little-endian words as loaded); the digest is returned as
// 8 little-endian words of its byte string (so a byte-wise XOR is a word-wise XOR).
DEV void sha256_id16(const uint32_t id[4], uint32_t out[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = __builtin_bswap32(id[i]);
  w[4] = 0x80000000u;
#pragma unroll
  for (int i = 5; i < 15; i++) w[i] = 0;
  w[15] = 128;  // message length in bits
  uint32_t st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = sha256d::IV[i];
  sha256d::compress(st, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(st[i]);
}

// checksums[s][8 words] = 0, intervals[s] = (UINT64_MAX, 0) as a (min start, max end) pair
__global__ void k_meta_init(uint32_t n_segments, uint32_t* ck, unsigned long long* iv) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_segments) return;
  if (ck)
    for (int i = 0; i < 8; i++) ck[8 * s + i] = 0;
  if (iv) {
    iv[2 * s] = ~0ull;
    iv[2 * s + 1] = 0;
  }
}

// Grid-stride over tiles of 1024 reports (16 waves): a tile whose reports share one segment is
// reduced in the block and folded into the block's running (segment, XOR, min, max) registers,
// which go out with one atomic per word when the segment changes and at the end -- so a 1 Mi
// batch of one segment issues ~5 k atomics on the segment's 10 words instead of ~41 k from
// 256-report blocks, whose serialisation on those addresses had set the kernel's time (112 us).
constexpr uint32_t META_T = 1024, META_W = META_T / 64, META_BLOCKS = 512;
__global__ __launch_bounds__(1024) void k_meta_seg(uint32_t n, const uint8_t* ids,
                                                 const uint64_t* times,
                                                 const uint8_t* status, const uint8_t* mask,
                                                 const uint32_t* seg, uint32_t n_segments,
                                                 uint32_t* ck, unsigned long long* iv) {
  __shared__ uint32_t s_seg0;
  __shared__ uint32_t s_ck[META_W][8];
  __shared__ unsigned long long s_lo[META_W], s_hi[META_W];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  // the block's running partial (block-uniform `cur`; word tid on threads 0..7, the interval on
  // thread 8)
  uint32_t cur = 0xffffffffu, acc_x = 0;
  unsigned long long acc_lo = ~0ull, acc_hi = 0;
  auto flush = [&]() {
    if (cur != 0xffffffffu) {
      if (ck && tid < 8 && acc_x) atomicXor(ck + 8 * cur + tid, acc_x);
      if (iv && tid == 8 && acc_hi) {
        atomicMin(iv + 2 * cur, acc_lo);
        atomicMax(iv + 2 * cur + 1, acc_hi);
      }
    }
    acc_x = 0;
    acc_lo = ~0ull;
    acc_hi = 0;
  };
  for (uint32_t base = blockIdx.x * META_T; base < n; base += gridDim.x * META_T) {
    const uint32_t r = base + tid;
    const bool valid = r < n;
    const uint32_t sg = valid ? (seg ? seg[r] : 0u) : 0xffffffffu;
    const bool in_range = valid && sg < n_segments;
    const bool inc = in_range && status[r] == PRIO3_STATUS_FINISHED && (!mask || mask[r]);
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ck && inc) {
      uint32_t id[4];
      load16(ids + 16 * (size_t)r, id);
      sha256_id16(id, h);
    }
    unsigned long long lo = ~0ull, hi = 0;
    if (times && in_range) {
      lo = times[r];
      hi = lo + 1;  // Interval::from_time: [t, t + 1)
    }
    if (tid == 0) s_seg0 = sg;  // thread 0 of a tile is always a valid report
    __syncthreads();
    const bool uniform = __syncthreads_and(!valid || sg == s_seg0) && s_seg0 < n_segments;
    if (uniform) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] ^= (uint32_t)__shfl_xor((int)h[i], off);
        const unsigned long long l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) s_ck[wv][i] = h[i];
        s_lo[wv] = lo;
        s_hi[wv] = hi;
      }
      __syncthreads();
      if (s_seg0 != cur) {  // block-uniform
        flush();
        cur = s_seg0;
      }
      if (tid < 8) {
        uint32_t x = 0;
        for (uint32_t q = 0; q < META_W; q++) x ^= s_ck[q][tid];
        acc_x ^= x;
      }
      if (tid == 8) {
        for (uint32_t q = 0; q < META_W; q++) {
          acc_lo = s_lo[q] < acc_lo ? s_lo[q] : acc_lo;
          acc_hi = s_hi[q] > acc_hi ? s_hi[q] : acc_hi;
        }
      }
    } else {
      if (ck && inc)
#pragma unroll
        for (int i = 0; i < 8; i++) atomicXor(ck + 8 * sg + i, h[i]);
      if (iv && times && in_range) {
        atomicMin(iv + 2 * sg, lo);
        atomicMax(iv + 2 * sg + 1, hi);
      }
    }
    __syncthreads();  // s_seg0 / s_ck of this tile are read before the next tile writes them
  }
  flush();
}

// k_meta: the whole job in one launch, for up to META_FAST_SEGS segments (a batch, or a job's
// few batch buckets).  A block keeps (XOR, min, max) per segment in LDS over its tiles -- a
// uniform tile folded in by threads 0..8, a tile that mixes segments by LDS atomics -- and writes
// them unconditionally to its row of `rows`, so nothing needs initialising and no global atomic
// runs on the segment's words.  The block that draws the last ticket (one atomic increment
// behind the drained row stores; no block waits for another) reduces the rows, writes the checksums and the finished
// (start, duration) pairs -- (0, 0) for a segment with no report -- and puts the ticket back
// to zero for the next call on its stream.
constexpr uint32_t META_FAST_SEGS = 8;
struct MetaRow {
  uint32_t ck[8];
  unsigned long long lo, hi;
};
constexpr uint32_t META_COLS = 10;  // a row's values per segment: 8 checksum words, lo, hi
__global__ __launch_bounds__(1024) void k_meta(uint32_t n, const uint8_t* ids,
                                             const uint64_t* times, const uint8_t* status,
                                             const uint8_t* mask, const uint32_t* seg,
                                             uint32_t n_segments, uint32_t* ck,
                                             unsigned long long* iv, MetaRow* rows,
                                             uint32_t* ticket) {
  __shared__ uint32_t s_seg0;
  __shared__ uint32_t s_ck[META_W][8];
  __shared__ unsigned long long s_lo[META_W], s_hi[META_W];
  __shared__ uint32_t t_ck[META_FAST_SEGS][8];
  __shared__ unsigned long long t_lo[META_FAST_SEGS], t_hi[META_FAST_SEGS];
  __shared__ unsigned long long s_red[META_T];  // [group][column], the last block's fold
  __shared__ unsigned long long s_fin[8][META_FAST_SEGS * META_COLS];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  if (tid < META_FAST_SEGS * 8) t_ck[tid >> 3][tid & 7u] = 0;
  if (tid < META_FAST_SEGS) {
    t_lo[tid] = ~0ull;
    t_hi[tid] = 0;
  }
  __syncthreads();
  for (uint32_t base = blockIdx.x * META_T; base < n; base += gridDim.x * META_T) {
    const uint32_t r = base + tid;
    const bool valid = r < n;
    const uint32_t sg = valid ? (seg ? seg[r] : 0u) : 0xffffffffu;
    const bool in_range = valid && sg < n_segments;
    const bool inc = in_range && status[r] == PRIO3_STATUS_FINISHED && (!mask || mask[r]);
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ck && inc) {
      uint32_t id[4];
      load16(ids + 16 * (size_t)r, id);
      sha256_id16(id, h);
    }
    unsigned long long lo = ~0ull, hi = 0;
    if (times && in_range) {
      lo = times[r];
      hi = lo + 1;  // Interval::from_time: [t, t + 1)
    }
    if (tid == 0) s_seg0 = sg;  // thread 0 of a tile is always a valid report
    __syncthreads();
    const bool uniform = __syncthreads_and(!valid || sg == s_seg0) && s_seg0 < n_segments;
    if (uniform) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] ^= (uint32_t)__shfl_xor((int)h[i], off);
        const unsigned long long l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) s_ck[wv][i] = h[i];
        s_lo[wv] = lo;
        s_hi[wv] = hi;
      }
      __syncthreads();
      if (tid < 8) {
        uint32_t x = 0;
        for (uint32_t q = 0; q < META_W; q++) x ^= s_ck[q][tid];
        t_ck[s_seg0][tid] ^= x;
      }
      if (tid == 8) {
        unsigned long long a = t_lo[s_seg0], b = t_hi[s_seg0];
        for (uint32_t q = 0; q < META_W; q++) {
          a = s_lo[q] < a ? s_lo[q] : a;
          b = s_hi[q] > b ? s_hi[q] : b;
        }
        t_lo[s_seg0] = a;
        t_hi[s_seg0] = b;
      }
    } else {
      if (ck && inc)
#pragma unroll
        for (int i = 0; i < 8; i++) atomicXor(&t_ck[sg][i], h[i]);
      if (times && in_range) {
        atomicMin(&t_lo[sg], lo);
        atomicMax(&t_hi[sg], hi);
      }
    }
    __syncthreads();  // s_seg0 / s_ck / the table of this tile are done before the next tile
  }
  // the block's row, every word of it
  const uint32_t ncols = n_segments * META_COLS;
  MetaRow* my = rows + (size_t)blockIdx.x * n_segments;
  // (write-through stores, drained by every wave ahead of the barrier: the block needs no
  // release fence, which would write back all of its die's L2)
  if (tid < n_segments * 8)
    __hip_atomic_store(&my[tid >> 3].ck[tid & 7u], t_ck[tid >> 3][tid & 7u], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  if (tid >= 64 && tid < 64 + n_segments) {
    __hip_atomic_store(&my[tid - 64].lo, t_lo[tid - 64], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&my[tid - 64].hi, t_hi[tid - 64], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const uint32_t t =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_seg0 = last ? 1u : 0u;
  }
  __syncthreads();
  if (!s_seg0) return;  // block-uniform
  // the last block: thread (column c = tid % ncols, group g = tid / ncols) folds rows g, g + G,
  // ... -- every thread with a few independent loads, not a few threads with many in a row (the
  // rows come from the other dies' L2 at ~1 us a load) -- then the G partials through LDS in
  // two steps
  const uint32_t G = META_T / ncols, c = tid % ncols, g = tid / ncols;
  auto fold = [](uint32_t k, unsigned long long v, unsigned long long x) {
    return k < 8 ? v ^ x : k == 8 ? (x < v ? x : v) : (x > v ? x : v);
  };
  if (g < G) {
    const uint32_t s = c / META_COLS, k = c % META_COLS;
    unsigned long long v = k == 8 ? ~0ull : 0ull;
    for (uint32_t b = g; b < gridDim.x; b += G) {
      const MetaRow* row = rows + (size_t)b * n_segments + s;
      v = fold(k, v, k < 8 ? row->ck[k] : k == 8 ? row->lo : row->hi);
    }
    s_red[g * ncols + c] = v;
  }
  __syncthreads();
  if (tid < 8 * ncols) {  // part q = tid / ncols of 8: groups q, q + 8, ...
    const uint32_t k = c % META_COLS;
    unsigned long long v = k == 8 ? ~0ull : 0ull;
    for (uint32_t q = g; q < G; q += 8) v = fold(k, v, s_red[q * ncols + c]);
    s_fin[g][c] = v;
  }
  __syncthreads();
  if (tid < ncols) {
    const uint32_t k = c % META_COLS;
    unsigned long long v = s_fin[0][c];
    for (uint32_t q = 1; q < 8; q++) v = fold(k, v, s_fin[q][c]);
    s_fin[0][c] = v;  // (only this thread reads or writes column c of part 0 here)
  }
  __syncthreads();
  if (tid < n_segments * 8 && ck)
    ck[tid] = (uint32_t)s_fin[0][(tid >> 3) * META_COLS + (tid & 7u)];
  if (tid >= 64 && tid < 64 + n_segments && iv) {
    const uint32_t s = tid - 64;
    const unsigned long long lo = s_fin[0][s * META_COLS + 8], hi = s_fin[0][s * META_COLS + 9];
    iv[2 * s] = hi ? lo : 0;
    iv[2 * s + 1] = hi ? hi - lo : 0;
  }
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// multi-GPU combine of k per-rank metadata: checksums XOR, intervals Interval::merge
// (an empty (.., 0) interval is the identity, core/src/time.rs:294-307)
__global__ void k_combine_meta(uint32_t k, uint32_t n_segments, const uint32_t* ck_in,
                               const unsigned long long* iv_in, uint32_t* ck_out,
                               unsigned long long* iv_out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_segments * 8) return;
  const uint32_t s = t >> 3, w = t & 7u;
  if (ck_in && ck_out) {
    uint32_t x = 0;
    for (uint32_t i = 0; i < k; i++) x ^= ck_in[((size_t)i * n_segments + s) * 8 + w];
    ck_out[(size_t)s * 8 + w] = x;
  }
  if (iv_in && iv_out && w == 0) {
    unsigned long long lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < k; i++) {
      const unsigned long long a = iv_in[((size_t)i * n_segments + s) * 2];
      const unsigned long long d = iv_in[((size_t)i * n_segments + s) * 2 + 1];
      if (d == 0) continue;
      lo = a < lo ? a : lo;
      hi = a + d > hi ? a + d : hi;
    }
    iv_out[2 * s] = hi ? lo : 0;
    iv_out[2 * s + 1] = hi ? hi - lo : 0;
  }
}

// (min start, max end) -> (start, duration); a segment with no report -> Interval::EMPTY (0, 0)
__global__ void k_meta_final(uint32_t n_segments, unsigned long long* iv) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_segments) return;
  const unsigned long long lo = iv[2 * s], hi = iv[2 * s + 1];
  iv[2 * s] = hi ? lo : 0;
  iv[2 * s + 1] = hi ? hi - lo : 0;
}

// ====================================================================================
// Host side: the launches
// ====================================================================================

// fn(F{}) with the field of element size es
template <class Fn>
static int by_field(size_t es, Fn fn) {
  return es == 16 ? fn(Fp128{}) : fn(Fp64{});
}

int run_accumulate(prio3_engine* e, Run* R, uint32_t c0, uint32_t n, const uint8_t* d_status,
                   const uint32_t* d_seg, const uint8_t* d_accept, uint32_t nseg, uint8_t* d_agg,
                   uint64_t* d_counts, hipStream_t st) {
  const DevParams& d = R->dp;
  const size_t es = d.es, agg_len = (size_t)d.out_len * es;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(d_agg, 0, agg_len * nseg, st));
    HIPCHK(hipMemsetAsync(d_counts, 0, 8 * (size_t)nseg, st));
    return PRIO3_OK;
  }
  // reports per k_acc_seg block: 8192, or 2048 for the short outputs (Count, Sum) whose grid
  // would otherwise be a few blocks wide
  const bool short_out = d.out_len <= 4;
  const uint32_t chunk = short_out ? 2048 : 8192, nchunks = (n + chunk - 1) / chunk;
  const size_t part_b = ((size_t)nchunks * nseg * agg_len + 255) & ~(size_t)255;
  int rc = PRIO3_OK;
  Slab* tmp = ws_acquire(R->device, part_b + 8 * (size_t)nchunks * nseg, st, &rc);
  if (!tmp) return rc;
  void* partial = tmp->base;
  uint64_t* pcount = (uint64_t*)(tmp->base + part_b);
  const uint8_t* src = run_out_shares(R, c0);
  const size_t ld = d.ld_out;  // output shares: one column per report of the run
  const int SG = nseg == 1 ? 1 : nseg <= 4 ? 4 : 8;
  const dim3 grid(d.out_len, nchunks, (nseg + SG - 1) / SG);
  rc = by_field(es, [&](auto f) -> int {
    using F = decltype(f);
    auto seg = [&](auto sg) -> int {
      TIMED(e, st, "k_acc_seg",
            (k_acc_seg<F, decltype(sg)::value><<<grid, 256, 0, st>>>(
                n, ld, chunk, d.out_len, nseg, src, d_status, d_seg, d_accept, partial, pcount)));
      return PRIO3_OK;
    };
    const int rs = SG == 1   ? seg(std::integral_constant<int, 1>{})
                   : SG == 4 ? seg(std::integral_constant<int, 4>{})
                             : seg(std::integral_constant<int, 8>{});
    if (rs) return rs;
    if (short_out)
      TIMED(e, st, "k_acc_fin",
            (k_acc_fin_blk<F><<<dim3(d.out_len, nseg), 256, 0, st>>>(
                nchunks, d.out_len, nseg, partial, pcount, d_agg, d_counts)));
    else
      TIMED(e, st, "k_acc_fin",
            (k_acc_fin<F><<<dim3((d.out_len + 255) / 256, nseg), 256, 0, st>>>(
                nchunks, d.out_len, nseg, partial, pcount, d_agg, d_counts)));
    return PRIO3_OK;
  });
  ws_release(tmp, st);
  R->last = st;
  return rc;
}

ZeroRanges fused_first_zero(const Run* R) {
  ZeroRanges z{};
  const size_t S = R->nseg ? R->nseg : 1;
  z.dst[0] = (uint8_t*)R->agg64;
  z.bytes[0] = S * R->dp.meas_len * 8 * 8;
  z.dst[1] = (uint8_t*)R->fix;
  z.bytes[1] = 2 * sizeof(uint32_t);
  z.dst[2] = (uint8_t*)R->fcnt;
  z.bytes[2] = 8 * S;
  return z;
}

// k_agg_parts (chunk partials beside the counts and the reports whose fused inclusion differs
// from their verdict), k_agg_final.  seg: the inclusion segment ids; fix_seg: the segment each
// fix-up entry applies to (nullptr: 0 -- the leader's partials are all summed for segment 0, so
// with one segment every fix-up, an out-of-range id included, is a correction of segment 0).
int fused_finish(prio3_engine* e, Run* R, const uint8_t* d_status, const uint32_t* seg,
                 const uint32_t* fix_seg, const uint8_t* d_accept_mask, uint32_t S,
                 uint8_t* d_agg_shares, uint64_t* d_counts, hipStream_t st) {
  const uint32_t n = R->n, M = R->dp.meas_len, ws = R->wshift;
  const uint32_t nwaves = (n + (1u << ws) - 1) >> ws;
  // The accumulators are clean after the run's redo launch and after every finish (the final
  // kernels zero what they consume); only a run without a redo launch, or one whose last finish
  // failed half way, needs the zeroing launch.
  if (!R->fclean) {
    const ZeroRanges z = fused_first_zero(R);
    TIMED(e, st, "k_zero", (k_zero<<<std::min<uint32_t>(256, (uint32_t)((z.bytes[0] / 16 + 255) / 256) + 1), 256, 0, st>>>(z)));
    R->fgen = 0;
  }
  R->fclean = false;
  const uint32_t g = R->fgen & 1u;
  const uint32_t nchunks = (nwaves + WCH - 1) / WCH;
  const uint32_t gx = (M * 8 / 4 + 255) / 256;  // 4 slots per thread (the waves role)
  const uint32_t fix_blocks = (n + fix_per(n) - 1) / fix_per(n);
  AggFixArgs fx{n, d_status, seg, d_accept_mask, R->fix + g, R->fix + 2, (uint32_t)R->fix_cap, S,
                R->fcnt, fix_seg ? 1u : 0u, fix_per(n), ws};
  TIMED(e, st, "k_agg_parts",
        (k_agg_parts<<<fix_blocks + gx * nchunks, 256, 0, st>>>(
            fix_blocks, gx, fx, nwaves, M, R->wpart, R->wseg, R->cpart, R->cseg, R->agg64)));
  const AggFinalArgs fa{R->fix + g, R->fix + 2, R->fix + (g ^ 1u), R->fcnt,
                        (unsigned long long*)d_counts};
  if (nchunks <= 64 && S > 1)
    TIMED(e, st, "k_agg_final",
          (k_agg_final_s<<<dim3((M + 31) / 32, S), 256, 0, st>>>(
              M, R->dp.ld, R->agg64, nchunks, R->cpart, R->cseg, fa, fix_seg, R->sc.meas,
              d_agg_shares)));
  else
    TIMED(e, st, "k_agg_final",
          (k_agg_final<<<S * M, 256, 0, st>>>(M, R->dp.ld, R->agg64, nchunks, R->cpart, R->cseg,
                                               fa, fix_seg, R->sc.meas, d_agg_shares)));
  R->fgen++;
  R->fclean = true;
  return PRIO3_OK;
}

// On failure the stream is drained and the area released here.
Slab* acc_multi_enqueue(int device, uint32_t es, uint8_t* host, const AccLayout& L,
                        uint32_t n_jobs, size_t out_bytes, hipStream_t st, int* rc, Slab* area) {
  const AccDesc* D = (const AccDesc*)(host + L.desc_off);
  uint32_t reps = 0, max_len = 0;
  for (uint32_t i = 0; i < n_jobs; i++) {
    reps = std::max(reps, (uint32_t)((D[i].acc_off - L.acc_off) + D[i].n));
    max_len = std::max(max_len, D[i].out_len);
  }
  Slab* sl = area ? area : ws_acquire(device, L.bytes, st, rc);
  if (!sl) return nullptr;
  uint8_t* b = sl->base;
  auto h2d = [&](size_t off, size_t bytes) {
    return hipMemcpyAsync(b + off, host + off, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
  };
  // (a caller's area holds the segment ids and accept bytes already: the staging's stay out)
  bool ok = h2d(L.desc_off, sizeof(AccDesc) * n_jobs) &&
            (area || (h2d(L.seg_off, 4 * (size_t)reps) && h2d(L.acc_off, reps)));
  if (ok) {
    by_field(es, [&](auto f) -> int {
      k_acc_multi<decltype(f)><<<dim3(max_len, n_jobs), 256, 0, st>>>(
          (const AccDesc*)(b + L.desc_off), b);
      return 0;
    });
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(host + L.out_off, b + L.out_off, out_bytes, hipMemcpyDeviceToHost, st) ==
             hipSuccess;
  }
  if (ok) return sl;
  (void)hipStreamSynchronize(st);
  ws_release(sl, st);
  *rc = PRIO3_EDEVICE;
  return nullptr;
}

int launch_combine(prio3_engine* e, uint32_t k, uint32_t n_segments, const uint8_t* d_in,
                   const uint64_t* d_counts_in, uint8_t* d_out, uint64_t* d_counts_out,
                   hipStream_t st) {
  const uint32_t len = e->dp.out_len * n_segments;
  const uint32_t blocks = (std::max(len, n_segments) + 255) / 256;
  return by_field(e->dp.es, [&](auto f) -> int {
    TIMED(e, st, "k_combine",
          (k_combine<decltype(f)><<<blocks, 256, 0, st>>>(k, len, n_segments, d_in, d_counts_in,
                                                          d_out, d_counts_out)));
    return PRIO3_OK;
  });
}

// The area of stream_zero_words (prio3_host.h): launch_batch_metadata takes no engine lock, so
// calls on two streams may run at once and must not share a ticket.  The area (256 bytes of
// counters, then META_BLOCKS x META_FAST_SEGS rows: 193 KiB) is allocated at a stream's first
// call and its counters zeroed once on that stream ahead of the launch; the calls after the
// first add neither a memset nor an event.  The areas live as long as the process.
constexpr size_t STREAM_ZERO_MAX = 64;
uint32_t* stream_zero_words(int device, hipStream_t st, std::mutex** smu) {
  struct Ctx {
    int device;
    hipStream_t st;
    uint32_t* mem;
    std::mutex* mu;
  };
  static std::mutex mu;
  static std::vector<Ctx> all;
  std::lock_guard<std::mutex> lk(mu);
  for (const Ctx& c : all)
    if (c.device == device && c.st == st) {
      if (smu) *smu = c.mu;
      return c.mem;
    }
  if (all.size() >= STREAM_ZERO_MAX) return nullptr;
  uint32_t* mem = nullptr;
  const size_t bytes = 256 + sizeof(MetaRow) * META_BLOCKS * META_FAST_SEGS;
  if (hipMalloc((void**)&mem, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (hipMemsetAsync(mem, 0, 256, st) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(mem);
    return nullptr;
  }
  all.push_back(Ctx{device, st, mem, new std::mutex});
  if (smu) *smu = all.back().mu;
  return mem;
}

int launch_batch_metadata(prio3_engine* e, uint32_t n, const uint8_t* d_report_ids,
                          const uint64_t* d_times, const uint8_t* d_status,
                          const uint8_t* d_accept_mask, const uint32_t* d_segment_ids,
                          uint32_t n_segments, uint32_t* ck, unsigned long long* iv,
                          hipStream_t st) {
  if (n_segments <= META_FAST_SEGS)
    if (uint32_t* ctx = stream_zero_words(e->device, st)) {
      const uint32_t blocks = std::max(1u, std::min((n + META_T - 1) / META_T, META_BLOCKS));
      TIMED(e, st, "k_meta",
            (k_meta<<<blocks, META_T, 0, st>>>(n, d_report_ids, d_times, d_status, d_accept_mask,
                                               d_segment_ids, n_segments, ck, iv,
                                               (MetaRow*)(ctx + 64), ctx)));
      return PRIO3_OK;
    }
  // many segments (or no ticket left): init, per-segment atomics, final
  const uint32_t sb = (n_segments + 255) / 256;
  TIMED(e, st, "k_meta_init", (k_meta_init<<<sb, 256, 0, st>>>(n_segments, ck, iv)));
  if (n)
    TIMED(e, st, "k_meta",
          (k_meta_seg<<<std::min((n + META_T - 1) / META_T, META_BLOCKS), META_T, 0, st>>>(
              n, d_report_ids, d_times, d_status, d_accept_mask, d_segment_ids, n_segments, ck,
              d_times ? iv : nullptr)));
  if (iv) TIMED(e, st, "k_meta_final", (k_meta_final<<<sb, 256, 0, st>>>(n_segments, iv)));
  return PRIO3_OK;
}

int launch_combine_metadata(prio3_engine* e, uint32_t k, uint32_t n_segments,
                            const uint32_t* ck_in, const unsigned long long* iv_in,
                            uint32_t* ck_out, unsigned long long* iv_out, hipStream_t st) {
  TIMED(e, st, "k_combine_meta",
        (k_combine_meta<<<(n_segments * 8 + 255) / 256, 256, 0, st>>>(k, n_segments, ck_in, iv_in,
                                                                      ck_out, iv_out)));
  return PRIO3_OK;
}

// prio3_engine.hip -- the host half of the MI355X (gfx950) batched Prio3 engine and its C ABI
// (include/janus_prio3.h): instance sizes and constants (fill_sizes), the per-kernel timing list,
// runs (the device state of one prepare call, carved from a pooled slab), the hooks the
// coalescing executors call (prio3_runtime.h) and every entry point.  The prepare kernels and
// their launch plans are in prio3_prepare.hip, the accumulate / aggregate / metadata kernels and
// launches in prio3_accumulate.hip; prio3_host.h declares what crosses.  The only kernels here
// are the copy kernel k_pull, the two sealed-group kernels (k_hpke_merge, k_hpke_retry_list) and
// the self-tests.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/janus_hpke.h"
#include "../../include/janus_prio3.h"
#include "prio3_host.h"
#include "sha256_host.h"

// the copy kernel of PullRanges (prio3_host.h)
DEV void pull_body(const PullRanges& pr, size_t tid, size_t nth) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const size_t n16 = pr.bytes[k] / 16;
    const uint4* s16 = (const uint4*)pr.src[k];
    uint4* d16 = (uint4*)pr.dst[k];
    for (size_t i = tid; i < n16; i += nth) d16[i] = s16[i];
    const size_t t = 16 * n16 + tid;
    if (t < pr.bytes[k] && tid < 16) pr.dst[k][t] = pr.src[k][t];
  }
}
__global__ __launch_bounds__(256) void k_pull(PullRanges pr) {
  pull_body(pr, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}
bool launch_pull(const PullRanges& pr, unsigned blocks, hipStream_t st) {
  k_pull<<<blocks, 256, 0, st>>>(pr);
  return hipGetLastError() == hipSuccess;
}
// the copy of a group's outputs back into its staging: a grid sized to the bytes
static bool pull_outputs(const PullRanges& o, hipStream_t st) {
  const size_t tot = o.bytes[0] + o.bytes[1] + o.bytes[2] + o.bytes[3];
  return launch_pull(o, (unsigned)std::min<size_t>(256, (tot / 16 + 255) / 256 + 1), st);
}

// ------------------------------------------------------------------------------------
// Field self-test (parity of the hand-scheduled Field128 blocks against Python bigints)
// ------------------------------------------------------------------------------------
// op 0: mul128 (compiler code), 1: mul128_asm, 2: add128, 3: sub128,
// op 4: sum_{i<16} a_(16x+i) b_(16x+i) via mac_add + mac_reduce (compiler code),
// op 5: the same with mac_reduce_asm.   a, b, out: [n][16 B] (ops 4/5: a, b [16 n][16 B]).
__global__ void k_selftest_f128(int op, uint32_t n, const uint4* a, const uint4* b, uint4* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  auto ld = [](const uint4* p, size_t k) {
    const uint4 v = p[k];
    return mk128(v.x, v.y, v.z, v.w);
  };
  f128 z;
  if (op == 0) z = mul128(ld(a, i), ld(b, i));
  else if (op == 1) z = mul128_asm(ld(a, i), ld(b, i));
  else if (op == 2) z = add128(ld(a, i), ld(b, i));
  else if (op == 3) z = sub128(ld(a, i), ld(b, i));
  else {
    mac128 m;
    mac_zero(m);
    for (int k = 0; k < 16; k++) mac_add(m, ld(a, (size_t)i * 16 + k), ld(b, (size_t)i * 16 + k));
    z = op == 4 ? mac_reduce(m) : mac_reduce_asm(m);
  }
  out[i] = make_uint4(z.w[0], z.w[1], z.w[2], z.w[3]);
}

// Field64 primitives and the limit-operand pieces of Field128 (prio3_selftest_field64):
// op 0/1/2: mul64f / add64f / sub64f of a[i], b[i];  3: red128_64(lo = a[i], hi = b[i]);
// op 4: sum_{j<k} a_(k i+j) b_(k i+j) via mac64_add + mac64_reduce;  5: Fp64::lt_p(a[i]);
// op 6: Fp128::lt_p(a[i]) (16-byte a);  7: sum_reduce of k sum_add of a[i] (16-byte a and out);
// op 8: TruncSink with nb = k over two entries, elements a_(2 k i ..) -> out[e * n + i] (16-byte).
__global__ void k_selftest_f64(int op, uint32_t n, uint32_t k, const uint64_t* a, const uint64_t* b,
                               uint64_t* out, DevParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  auto ld = [](const uint64_t* q, size_t j) {
    const uint4 v = ((const uint4*)q)[j];
    return mk128(v.x, v.y, v.z, v.w);
  };
  if (op == 0) out[i] = mul64f(a[i], b[i]);
  else if (op == 1) out[i] = add64f(a[i], b[i]);
  else if (op == 2) out[i] = sub64f(a[i], b[i]);
  else if (op == 3) out[i] = red128_64(a[i], b[i]);
  else if (op == 4) {
    mac64 m;
    mac64_zero(m);
    for (uint32_t j = 0; j < k; j++) mac64_add(m, a[(size_t)i * k + j], b[(size_t)i * k + j]);
    out[i] = mac64_reduce(m);
  } else if (op == 5) out[i] = Fp64::lt_p(a[i]) ? 1 : 0;
  else if (op == 6) out[i] = Fp128::lt_p(ld(a, i)) ? 1 : 0;
  else if (op == 7) {
    sum128 sm;
    sum_zero(sm);
    const f128 x = ld(a, i);
    for (uint32_t j = 0; j < k; j++) sum_add(sm, x);
    Fp128::store(out, i, sum_reduce(sm));
  } else {
    TruncSink ts(p, out, i);
    for (uint32_t j = 0; j < 2 * k; j++) ts.put(ld(a, (size_t)i * 2 * k + j));
  }
}

// The fused accumulate's tile reduction (tile_stage / tile_halfsum) on caller-supplied values:
// one wave stages all FTILE slots from in [FTILE][64][16 B] (slot, lane) and writes the 8 addends
// of the first cnt slots to out [cnt][8]; the slots from cnt on are staged too and must not count.
__global__ __launch_bounds__(64) void k_selftest_tile(uint32_t cnt, const uint4* in,
                                                      uint32_t* out) {
  __shared__ uint4 tile[FTILE * 64];
  const uint32_t lane = threadIdx.x;
#pragma unroll
  for (int s = 0; s < FTILE; s++) {
    const uint4 v = in[s * 64 + (int)lane];
    tile_stage(tile, s, lane, mk128(v.x, v.y, v.z, v.w));
  }
  tile_fence();
  const uint32_t tot = tile_halfsum(tile, lane);
  if ((lane & 7u) < cnt) out[(lane & 7u) * 8u + (lane >> 3)] = tot;
}

// ====================================================================================
// Host side
// ====================================================================================

// A batch handle: one job's column range of a (possibly coalesced, shared) device run.  Every
// handle owns its reference, so concurrent jobs of one engine never see each other's output
// shares or verdicts (the run's slab stays out of the pool until the last handle is freed).
// Handles must be freed before their engine is destroyed.
struct prio3_batch {
  prio3_engine* e;
  Run* run;  // nullptr for an empty batch
  uint32_t c0, n;
};

static uint32_t next_pow2(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// prio flp/gadgets.rs optimal_chunk_length: over calls = 2^k - 1, the chunk length minimising
// the ParallelSum proof length 2 * chunk + 2 * ((1 + calls).next_power_of_two() - 1) + 1
// (first minimum from the largest k, as min_by_key over the reversed range keeps)
static uint32_t optimal_chunk_length(uint32_t m) {
  if (m <= 1) return 1;
  uint32_t max_log2 = 0;
  while ((1u << max_log2) < m) max_log2++;
  max_log2 += 1;
  uint64_t best = UINT64_MAX;
  uint32_t best_chunk = 1;
  for (uint32_t l = max_log2; l >= 1; l--) {
    const uint64_t calls = (1ull << l) - 1, chunk = (m + calls - 1) / calls;
    const uint64_t cost = 2 * chunk + 2 * ((1ull << l) - 1) + 1;  // next_pow2(1 + calls) = 2^l
    if (cost < best) {
      best = cost;
      best_chunk = (uint32_t)chunk;
    }
  }
  return best_chunk;
}

static int fill_sizes(const prio3_params* pp, prio3_sizes_t* s, DevParams* dp) {
  if (!pp) return PRIO3_EINVAL;
  uint32_t proofs = pp->num_proofs ? pp->num_proofs : 1;
  const bool mp = pp->kind == PRIO3_SUMVEC_F64_MP;
  if (mp ? (proofs < 2 || proofs > 8) : proofs != 1) return mp ? PRIO3_EINVAL : PRIO3_EUNSUPPORTED;
  DevParams d;
  memset(&d, 0, sizeof d);
  d.kind = pp->kind;
  d.bits = pp->bits;
  d.length = pp->length;
  d.chunk = pp->chunk_length;
  uint32_t algo;
  switch (pp->kind) {
    case PRIO3_COUNT:
      algo = 0;
      d.es = 8;
      d.meas_len = 1;
      d.out_len = 1;
      d.jr_len = 0;
      d.arity = 2;
      d.calls = 1;
      break;
    case PRIO3_SUM:
      if (pp->bits == 0 || pp->bits > 64) return PRIO3_EINVAL;
      algo = 1;
      d.es = 16;
      d.meas_len = pp->bits;
      d.out_len = 1;
      d.jr_len = 1;
      d.arity = 1;
      d.calls = pp->bits;
      break;
    case PRIO3_SUMVEC:
      if (pp->bits == 0 || pp->bits > 64 || pp->length == 0 || pp->chunk_length == 0)
        return PRIO3_EINVAL;
      algo = 2;
      d.es = 16;
      d.meas_len = pp->bits * pp->length;
      d.out_len = pp->length;
      d.jr_len = 1;
      d.arity = 2 * pp->chunk_length;
      d.calls = (d.meas_len + pp->chunk_length - 1) / pp->chunk_length;
      break;
    case PRIO3_SUMVEC_F64_MP:  // SumVec<Field64, ParallelSum<Mul>> (vdaf.rs:173-195)
      if (pp->bits == 0 || pp->bits > 64 || pp->length == 0 || pp->chunk_length == 0)
        return PRIO3_EINVAL;
      algo = 0xFFFF1003u;  // ALGORITHM_ID_PRIO3_SUM_VEC_FIELD64_MULTIPROOF_HMACSHA256_AES128
      d.es = 8;
      d.meas_len = pp->bits * pp->length;
      d.out_len = pp->length;
      d.jr_len = 1;
      d.arity = 2 * pp->chunk_length;
      d.calls = (d.meas_len + pp->chunk_length - 1) / pp->chunk_length;
      break;
    case PRIO3_FPVEC_BOUNDED_L2:  // Prio3FixedPointBoundedL2VecSum (vdaf.rs:292-335)
      if ((pp->bits != 16 && pp->bits != 32) || pp->length == 0 || pp->length > (1u << 22))
        return PRIO3_EINVAL;
      algo = 0xFFFF0000u;
      d.es = 16;
      d.meas_len = pp->bits * pp->length + 2 * pp->bits - 2;
      d.out_len = pp->length;
      d.jr_len = 2;
      d.qr_len = 2;
      d.chunk = optimal_chunk_length(d.meas_len);
      d.arity = 2 * d.chunk;
      d.calls = (d.meas_len + d.chunk - 1) / d.chunk;
      d.chunk1 = optimal_chunk_length(pp->length);
      d.calls1 = (pp->length + d.chunk1 - 1) / d.chunk1;
      break;
    case PRIO3_HISTOGRAM:
      if (pp->length == 0 || pp->chunk_length == 0) return PRIO3_EINVAL;
      algo = 3;
      d.es = 16;
      d.meas_len = pp->length;
      d.out_len = pp->length;
      d.jr_len = 2;
      d.arity = 2 * pp->chunk_length;
      d.calls = (pp->length + pp->chunk_length - 1) / pp->chunk_length;
      break;
    default:
      return PRIO3_EINVAL;
  }
  d.P = next_pow2(1 + d.calls);
  d.logP = 0;
  while ((1u << d.logP) < d.P) d.logP++;
  if (d.logP > MAX_ROOTS) return PRIO3_EUNSUPPORTED;
  d.glen = 2 * (d.P - 1) + 1;
  d.proof_len = d.arity + d.glen;
  d.verifier_len = d.arity + 2;
  if (!d.qr_len) d.qr_len = 1;
  if (d.kind == PRIO3_FPVEC_BOUNDED_L2) {  // second gadget: seeds1 || coeffs1 follow
    d.P1 = next_pow2(1 + d.calls1);
    while ((1u << d.logP1) < d.P1) d.logP1++;
    if (d.logP1 > MAX_ROOTS) return PRIO3_EUNSUPPORTED;
    d.glen1 = 2 * (d.P1 - 1) + 1;
    d.proof_len += d.chunk1 + d.glen1;
    d.verifier_len = 1 + d.arity + 1 + d.chunk1 + 1;
  }
  const uint32_t S = mp ? 32 : 16;  // seed size
  d.helper_share_len = d.jr_len ? 3 * S : 2 * S;
  d.public_share_len = d.jr_len ? 2 * S : 0;
  d.prep_share_len = d.verifier_len * proofs * d.es + (d.jr_len ? S : 0);
  d.leader_share_len = (d.meas_len + d.proof_len * proofs) * d.es + (d.jr_len ? S : 0);
  for (uint32_t u = 1; u <= 7; u++) {
    uint8_t b[8] = {8, 0, (uint8_t)(algo >> 24), (uint8_t)(algo >> 16), (uint8_t)(algo >> 8),
                    (uint8_t)algo, 0, (uint8_t)u};
    memcpy(d.dst[u], b, 8);
  }
  // roots and constants
  {
    u128 g128 = 0;
    for (const char* c = "145091266659756586618791329697897684742"; *c; c++)
      g128 = g128 * 10 + (u128)(*c - '0');
    uint64_t g64 = 1753635133440165772ULL;
    for (int l = 0; l <= MAX_ROOTS; l++) {
      u128 r = g128;
      for (int i = 0; i < 66 - l; i++) r = hmul(r, r, HP128);
      for (int k = 0; k < 4; k++) d.roots128[l][k] = (uint32_t)(r >> (32 * k));
      u128 r64 = g64;
      for (int i = 0; i < 32 - l; i++) r64 = hmul(r64, r64, HP64);
      d.roots64[l] = (uint64_t)r64;
    }
    u128 ip = hpow(d.P, HP128 - 2, HP128), h = hpow(2, HP128 - 2, HP128);
    for (int k = 0; k < 4; k++) {
      d.invP128[k] = (uint32_t)(ip >> (32 * k));
      d.half128[k] = (uint32_t)(h >> (32 * k));
    }
    d.invP64 = (uint64_t)hpow(d.P, HP64 - 2, HP64);
    if (d.kind == PRIO3_FPVEC_BOUNDED_L2) {
      const u128 ip1 = hpow(d.P1, HP128 - 2, HP128);
      // entries * 2^(2n-2) / num_shares (2): < 2^22 * 2^62 / 2 < p
      const u128 nc = ((u128)d.out_len << (2 * d.bits - 2)) >> 1;
      const u128 tn = (u128)1 << d.bits;
      for (int k = 0; k < 4; k++) {
        d.invP1_128[k] = (uint32_t)(ip1 >> (32 * k));
        d.normc128[k] = (uint32_t)(nc >> (32 * k));
        d.twon128[k] = (uint32_t)(tn >> (32 * k));
      }
    }
    if (d.P <= 32) {
      u128 alpha = 0;
      for (int k = 0; k < 4; k++) alpha |= (u128)d.roots128[d.logP][k] << (32 * k);
      for (uint32_t e2 = 0; e2 < d.P; e2++) {
        u128 ae = hpow(alpha, e2, HP128), s = 0, x = 1;
        for (uint32_t cc = 1; cc <= d.calls; cc++) {
          x = hmul(x, ae, HP128);
          s += x;
          if (s < x || s >= HP128) s -= HP128;
        }
        for (int k = 0; k < 4; k++) d.sigma128[e2][k] = (uint32_t)(s >> (32 * k));
      }
      for (uint32_t i = 0; i < d.P / 2; i++) {
        u128 w = hpow(alpha, i, HP128);
        for (int k = 0; k < 4; k++) d.tw128[i][k] = (uint32_t)(w >> (32 * k));
      }
    } else if (d.P == 64 || d.P == 128) {  // k_query_w's four-step DFT
      u128 alpha = 0;
      for (int k = 0; k < 4; k++) alpha |= (u128)d.roots128[d.logP][k] << (32 * k);
      const u128 aq = hpow(alpha, 8, HP128);  // alpha_(P/8)
      for (uint32_t i = 0; i < d.P / 16; i++) {
        const u128 w = hpow(aq, i, HP128);
        for (int k = 0; k < 4; k++) d.tw128[i][k] = (uint32_t)(w >> (32 * k));
      }
      for (uint32_t i = 0; i < 8; i++) {
        const u128 w = hpow(alpha, i, HP128);
        for (int k = 0; k < 4; k++) d.tw128[8 + i][k] = (uint32_t)(w >> (32 * k));
      }
    }
    if (d.P >= 16 && d.P <= 128) {  // k_query_sum's twiddles
      u128 alpha = 0;
      for (int k = 0; k < 4; k++) alpha |= (u128)d.roots128[d.logP][k] << (32 * k);
      const u128 w16 = hpow(alpha, d.P / 16, HP128), a16 = hpow(alpha, 16, HP128);
      for (uint32_t i = 0; i < 8; i++) {
        const u128 v[3] = {hpow(w16, i, HP128), hpow(alpha, i, HP128), hpow(a16, i, HP128)};
        for (int t = 0; t < 3; t++)
          for (int k = 0; k < 4; k++) d.tws[8 * t + i][k] = (uint32_t)(v[t] >> (32 * k));
      }
    }
    d.half64 = (uint64_t)hpow(2, HP64 - 2, HP64);
  }
  if (s) {
    s->field_bytes = d.es;
    s->meas_len = d.meas_len;
    s->out_len = d.out_len;
    s->proof_len = d.proof_len;
    s->verifier_len = d.verifier_len;
    s->joint_rand_len = d.jr_len;
    s->nonce_len = 16;
    s->public_share_len = d.public_share_len;
    s->helper_share_len = d.helper_share_len;
    s->prep_share_len = d.prep_share_len;
    s->prep_msg_len = d.jr_len ? S : 0;
    s->agg_share_len = d.out_len * d.es;
    s->leader_input_share_len = d.leader_share_len;
  }
  d.proof_len *= proofs;  // scratch holds every proof (prio3_sizes_t reports one)
  if (dp) *dp = d;
  return PRIO3_OK;
}

// ---- per-kernel timing (option "timing"; declared with the TIMED macro in prio3_host.h) ----
// The one list of this thread's timing events, whichever unit's launch recorded them.
std::vector<Pending>& pending() {
  static thread_local std::vector<Pending> v;
  return v;
}
size_t time_slot(prio3_engine* e, const char* name) {
  std::lock_guard<std::mutex> lk(e->tmu);
  for (size_t i = 0; i < e->times.size(); i++)
    if (e->times[i].name == name) return i;
  e->times.push_back(KTime{name, 0, 0});
  return e->times.size() - 1;
}
void count_launch(prio3_engine* e, const char* name) {
  const size_t i = time_slot(e, name);
  std::lock_guard<std::mutex> lk(e->tmu);
  e->times[i].launches += 1;
}
void collect_times(prio3_engine* e, bool wait) {
  auto& v = pending();
  std::vector<Pending> keep;
  for (auto& pd : v) {
    if (pd.e != e || (!wait && hipEventQuery(pd.b) == hipErrorNotReady)) {
      keep.push_back(pd);
      continue;
    }
    float ms = 0;
    (void)hipEventSynchronize(pd.b);
    (void)hipEventElapsedTime(&ms, pd.a, pd.b);
    {
      std::lock_guard<std::mutex> lk(e->tmu);
      e->times[pd.idx].ms += ms;
      e->times[pd.idx].launches += 1;
    }
    (void)hipEventDestroy(pd.a);
    (void)hipEventDestroy(pd.b);
  }
  v.swap(keep);
}

// FPVec per-report scratch bytes of one sub-batch column: every buffer indexed [row][column]
// with the sub-batch leading dimension ld (meas, proofs, jr, qr, part, corrected, flag, L, PV,
// beta); the output shares have one column per report of the batch (ld_out).
static size_t fp_column_bytes(const DevParams& d) {
  const size_t es = d.es;
  return es * ((size_t)d.meas_len + d.proof_len + d.jr_len + d.qr_len + 2 * ((size_t)d.P + d.P1) +
               d.calls) +
         16 + 16 + 1;
}

// FPVec sub-batch width: the per-report scratch (2.6 MB at 10^4 entries) of a whole batch does
// not fit, so the batch runs in equal sub-batches of ld columns.  Auto budget: free HBM plus the
// pool's idle slabs, minus the batch's output shares and a fixed reserve for the runtime
// (private segments, queues, the caller's allocator) -- the r01u hipErrorIllegalAddress came
// with a budget of 85% of free HBM and did not recur with an explicit reserve.
// The kernels are latency-bound per lane, so the widest sub-batch wins.
static uint32_t fp_sub_ld(const prio3_engine* e, const DevParams& d, uint32_t ld_out,
                          size_t other_bytes) {
  const size_t per = fp_column_bytes(d);
  int64_t budget = e->fp_sub_bytes;
  if (budget <= 0) {
    size_t fr = 0, tot = 0, idle = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
      (void)hipGetLastError();
      fr = tot = 0;
    }
    (void)ws_pool_bytes(e->device, &idle);
    const int64_t outb = (int64_t)(d.es * d.out_len * (size_t)ld_out + 64 * (size_t)ld_out);
    const int64_t reserve = std::max<int64_t>((int64_t)8 << 30, (int64_t)(0.10 * (double)tot));
    budget = (int64_t)(fr + idle) - outb - reserve - (int64_t)other_bytes;
  }
  uint64_t cols = (uint64_t)std::max<int64_t>(budget, 1) / per;
  cols = std::max<uint64_t>(256, cols & ~255ull);
  return (uint32_t)std::min<uint64_t>(ld_out, cols);
}

// Lays the run's buffers out from `base` (nullptr: sizes only), 256-byte aligned.
static size_t run_carve(Run* R, unsigned flags, uint8_t* base) {
  const DevParams& d = R->dp;
  const size_t es = d.es, ld = d.ld, ldo = d.ld_out, n = R->n ? R->n : 1;
  size_t off = 0;
  auto take = [&](auto** ptr, size_t bytes) {
    *ptr = base ? (std::remove_pointer_t<decltype(ptr)>)(base + off) : nullptr;
    off += (bytes + 255) & ~(size_t)255;
  };
  if (flags & RUN_SCRATCH) {
    const bool fp = d.kind == PRIO3_FPVEC_BOUNDED_L2;
    take(&R->sc.meas, es * d.meas_len * ld);
    take(&R->sc.proofs, es * d.proof_len * ld);
    take(&R->sc.jr, es * (d.jr_len ? d.jr_len : 1) * ld);
    take(&R->sc.qr, es * d.qr_len * ld);
    take(&R->sc.part, 16 * ld);
    take(&R->sc.corrected, 16 * ld);
    take(&R->sc.flag, ld);
    take(&R->sc.Lbuf, es * ((size_t)d.P + d.P1) * ld);
    take(&R->sc.PVbuf, es * ((size_t)d.P + d.P1) * ld);
    take(&R->sc.acc, fp ? 16 : es * d.arity * ld);
    take(&R->sc.out, own_out(d) ? es * d.out_len * ldo : 16);
    take(&R->sc.beta, es * d.calls * ld);
    // k_prep_h's list of flagged reports.  Wider than the plan's redo_list (any Field128 instance
    // with P = 32, whatever the options and the run's size): slab sizes feed the pool budget.
    if (es == 16 && d.P == 32) take(&R->redo_list, 4 * n);
    // FPVec runs in sub-batches of ld columns: the leader's corrected seeds of every report
    // outlive their sub-batch's scratch (prepare_next reads them)
    if (fp) take(&R->corr_all, 16 * n);
  }
  if (flags & RUN_IO) {
    const size_t ml = R->e->sz.prep_msg_len ? R->e->sz.prep_msg_len : 16;
    take(&R->nonces, 16 * n);
    take(&R->pub, (size_t)(d.public_share_len ? d.public_share_len : 16) * n);
    take(&R->helper, (size_t)d.helper_share_len * n);
    take(&R->leader, (size_t)d.prep_share_len * n);
    take(&R->msgs, ml * n);
    take(&R->status, n);
  }
  if (flags & RUN_LINPUT) take(&R->linput, (size_t)d.leader_share_len * n);
  if (flags & RUN_AGG_IO) {
    const size_t S = R->nseg ? R->nseg : 1;
    take(&R->gseg, 4 * n);
    take(&R->gaccept, n);
    take(&R->gagg, (size_t)d.out_len * es * S);
    take(&R->gcnt, 8 * S);
  }
  if (flags & RUN_HPKE) {
    take(&R->hstatus, n);
    take(&R->hpt, (size_t)R->hpke_stride * n);
    take(&R->hretry, 4 * (n + 1));
  }
  if (flags & RUN_JIX) {
    const size_t S = R->nseg ? R->nseg : 1;
    take(&R->gck, 32 * S);
    take(&R->giv, 16 * S);
  }
  if (flags & RUN_FUSED) {
    // sized for 32-report waves (k_prep_hp); the one-lane kernels use the first half
    const size_t waves = (n + 31) / 32, M = d.meas_len, chunks = (waves + WCH - 1) / WCH;
    take(&R->wpart, waves * M * 8 * sizeof(uint32_t));
    take(&R->wseg, waves * sizeof(uint32_t));
    take(&R->cpart, chunks * M * 8 * 8);
    take(&R->cseg, chunks * sizeof(uint32_t));
    take(&R->agg64, (size_t)(R->nseg ? R->nseg : 1) * M * 8 * 8);
    take(&R->fix, (n + 2) * sizeof(uint32_t));
    take(&R->fcnt, 8 * (size_t)(R->nseg ? R->nseg : 1));
  }
  return off;
}

static Run* run_create(prio3_engine* e, uint32_t n, unsigned flags, uint32_t nseg,
                       hipStream_t st, int* rc, uint32_t hpke_stride = 0) {
  Run* R = new Run();
  R->e = e;
  R->hpke_stride = hpke_stride;
  R->device = e->device;
  R->n = n;
  R->nseg = nseg;
  R->dp = e->dp;
  R->dp.n = n;
  R->dp.nseg = nseg ? nseg : 1;
  const uint32_t ld_out = ((n ? n : 1) + 63) & ~63u;
  R->dp.ld_out = ld_out;
  R->dp.ld = ld_out;
  if ((flags & RUN_SCRATCH) && e->dp.kind == PRIO3_FPVEC_BOUNDED_L2) {
    // the rest of the run (I/O copies, the leader's explicit input shares: 2.6 MB per report at
    // 10^4 entries) comes out of the same budget as the scratch sub-batch
    const size_t other = run_carve(R, flags & ~RUN_SCRATCH, nullptr);
    R->dp.ld = fp_sub_ld(e, e->dp, ld_out, other);
  }
  const size_t bytes = run_carve(R, flags, nullptr);
  R->slab = ws_acquire(e->device, bytes, st, rc);
  if (!R->slab) {
    delete R;
    return nullptr;
  }
  run_carve(R, flags, R->slab->base);
  R->keep = e->keep_scratch != 0;
  R->fix_cap = (size_t)n;  // entries behind the two counters
  R->last = st;
  return R;
}

// drops one reference; the last one returns the slab to the pool, ordered after `st` (or the
// stream of the run's latest work)
static void run_release(Run* R, hipStream_t st, bool use_st) {
  if (!R) return;
  if (R->refs.fetch_sub(1) != 1) return;
  ws_release(R->slab, use_st ? st : R->last, R->keep);
  delete R;
}

// columns [c0, c0 + n) of the run's output shares to host, per report (n x out_len x es)
static int run_output_shares(Run* R, uint32_t c0, uint32_t n, uint8_t* out, hipStream_t st) {
  const DevParams& d = R->dp;
  const size_t es = d.es;
  if (n == 0) return PRIO3_OK;
  const uint8_t* src = run_out_shares(R, c0);
  std::vector<uint8_t> soa((size_t)d.out_len * n * es);
  HIPCHK(hipMemcpy2DAsync(soa.data(), n * es, src, (size_t)d.ld_out * es, n * es, d.out_len,
                          hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint32_t r = 0; r < n; r++)
    for (uint32_t i = 0; i < d.out_len; i++)
      memcpy(out + ((size_t)r * d.out_len + i) * es, soa.data() + ((size_t)i * n + r) * es, es);
  return PRIO3_OK;
}

// ---- executor hooks (prio3_runtime.h) ----
int engine_device(const prio3_engine* e) { return e->device; }
int engine_exec_id(const prio3_engine* e) { return e->device * EXEC_LANES + e->lane; }

// Host-buffer jobs of a multi-GPU engine go whole to the member whose executor holds the fewest
// reports (all engines' jobs counted: tasks of one instance share the executors), equally loaded
// members taken round-robin.  No collective: each job's outputs come back from the GPU that ran
// it, and Janus merges the per-job aggregations at collection
// (/root/reference/aggregator/src/aggregator/aggregation_job_writer.rs:510 writes a random `ord`
// shard per job; aggregate_share.rs:55-96 sums the shards).
// upload: an upload job -- only the members on e's own GPU (its openers are bound to it), their
// upload executors' reports counted too; the caller counts the job (placed) once it knows that an
// executor takes it.
static void placed(prio3_engine* m, uint32_t n) {
  m->placed_jobs.fetch_add(1, std::memory_order_relaxed);
  m->placed_reports.fetch_add(n, std::memory_order_relaxed);
}
static prio3_engine* place(prio3_engine* e, uint32_t n, bool upload = false) {
  prio3_engine* best = e;
  const size_t k = e->members.size();
  if (k > 1) {
    const uint32_t s0 = e->rr.fetch_add(1, std::memory_order_relaxed);
    uint64_t bl = UINT64_MAX;
    for (size_t i = 0; i < k; i++) {
      prio3_engine* m = e->members[(s0 + i) % k];
      if (upload && m->device != e->device) continue;
      const int id = engine_exec_id(m);
      const uint64_t l = exec_load(id) + (upload ? exec_upload_load(id) : 0);
      if (l < bl) {
        bl = l;
        best = m;
      }
    }
  }
  if (!upload) placed(best, n);
  return best;
}

void engine_vk(const prio3_engine* e, uint8_t out[16]) { memcpy(out, e->dp.vk, 16); }

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// aggregating jobs start at a wave boundary where the XOF fuses the accumulate (their waves then
// hold one job's reports and fuse; the pad columns carry an out-of-range segment id)
uint32_t engine_job_align(const prio3_engine* e) { return prepare_fuses(e) ? 64u : 1u; }

uint64_t engine_group_key(const prio3_engine* e) {
  uint64_t h = 1469598103934665603ull;
  h = fnv(h, &e->params, sizeof e->params);
  h = fnv(h, &e->device, sizeof e->device);
  // every option that changes what a launch computes or records (an A/B set on one
  // engine must not silently run with the lead engine's options)
  const int opts[] = {e->force_slow, e->chunks, e->fuse_acc,           e->leader_fast,
                      e->leader_fuse_acc, e->fp_round, e->experimental_fpvec, e->force_generic,
                      e->timing, e->pair_max};
  h = fnv(h, opts, sizeof opts);
  h = fnv(h, &e->fp_sub_bytes, sizeof e->fp_sub_bytes);
  // XofHmacSha256Aes128 keys enter the kernels as HMAC midstates: one engine per launch; an
  // engine with coalescing off gets a key of its own for every call
  if (e->dp.kind == PRIO3_SUMVEC_F64_MP || !e->coalesce) {
    static std::atomic<uint64_t> solo{0};
    const uint64_t u[2] = {(uint64_t)(uintptr_t)e, e->coalesce ? 0 : ++solo};
    h = fnv(h, u, sizeof u);
  }
  return h;
}

uint64_t exec_job_key(const ExecJob* j) {
  uint64_t h = engine_group_key(j->e);
  if (j->opener) {  // sealed-input jobs: one keypair and ciphertext shape per launch
    const uint64_t u[4] = {0x5345414C4544ull, hpke_opener_key(j->opener), j->ct_stride,
                           (uint64_t)j->require_taskprov};
    h = fnv(h, u, sizeof u);
    if (j->fallback) {  // and one fallback keypair (jobs without one launch apart: no retry pass)
      const uint64_t f[2] = {0x46414C4C4241434Bull, hpke_opener_key(j->fallback)};
      h = fnv(h, f, sizeof f);
    }
  }
  if (j->jix) {  // jobs whose index the launch makes share no group with jobs that bring theirs
    const uint64_t u = 0x4A4F42494E444558ull;
    h = fnv(h, &u, sizeof u);
  }
  return h;
}

void engine_io_layout(const prio3_engine* e, uint32_t cap, IoLayout* L, const ExecJob* job) {
  const DevParams& d = e->dp;
  const bool sealed = job && job->opener;
  L->len[0] = 16;
  L->len[1] = d.public_share_len;
  L->len[2] = sealed ? 0 : d.helper_share_len;  // sealed: opened into the run on the device
  L->len[3] = d.prep_share_len;
  size_t off = 0;
  for (int f = 0; f < 4; f++) {
    L->off[f] = off;
    off += (L->len[f] * cap + 15) & ~(size_t)15;
  }
  L->slot_off = off;
  off += (2 * (size_t)cap + 15) & ~(size_t)15;
  L->tab_off = off;
  off += 16 * (size_t)exec_max_keys();
  L->msg_len = e->sz.prep_msg_len;
  L->msg_off = off;
  off += L->msg_len * cap;
  L->status_off = off;
  off += cap;
  // aggregating jobs (prio3_helper_prepare_aggregate_batch): group segment ids, accept bytes,
  // and up to max_seg aggregate shares (at most 16 MiB of them) + counts
  off = (off + 15) & ~(size_t)15;
  L->seg_off = off;
  off += (4 * (size_t)cap + 15) & ~(size_t)15;
  L->accept_off = off;
  off += (cap + 15) & ~(size_t)15;
  L->agg_len = (size_t)d.out_len * d.es;
  L->max_seg = (uint32_t)std::max<size_t>(1, std::min<size_t>(EXEC_MAX_SEGS,
                                                                ((size_t)16 << 20) / L->agg_len));
  L->agg_off = off;
  off += (L->agg_len * L->max_seg + 15) & ~(size_t)15;
  L->cnt_off = off;
  off += 8 * (size_t)L->max_seg;
  L->nenc = L->ct_stride = 0;
  if (sealed) {  // the ciphertexts and their AAD fields (report IDs and public shares above)
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    L->nenc = (uint32_t)hpke_opener_nenc(job->opener);
    L->ct_stride = job->ct_stride;
    off = up(off);
    L->enc_off = off;
    off += up((size_t)L->nenc * cap);
    L->ct_off = off;
    off += up((size_t)L->ct_stride * cap);
    L->ctlen_off = off;
    off += up(4 * (size_t)cap);
    L->time_off = off;
    off += up(8 * (size_t)cap);
    L->tslot_off = off;
    off += up(2 * (size_t)cap);
    L->ttab_off = off;
    off += 32 * (size_t)HPKE_MAX_TASKS;
    L->dtab_off = off;
    off += 8 * (size_t)HPKE_MAX_TASKS;
  }
  L->jix = job && job->jix;
  if (L->jix) {  // prio3_helper_aggregate_job: descriptors, closed intervals, index + metadata rows
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t S = L->max_seg;
    off = up(off);
    L->jdesc_off = off;
    off += up(sizeof(JixJobDesc) * S);
    L->jclosed_off = off;
    off += 16 * (size_t)JIX_GROUP_CLOSED;
    L->jseg_off = off;
    off += up(4 * (size_t)cap);
    L->jrej_off = off;
    off += up(cap);
    L->jdup_off = off;
    off += up(cap);
    L->jstart_off = off;
    off += 8 * S;
    L->jinfo_off = off;
    off += up(sizeof(prio3_job_index_info) * S);
    L->ck_off = off;
    off += 32 * S;
    L->iv_off = off;
    off += 16 * S;
  }
  L->bytes = off;
}

// the group's "prepared" event (engine_group_prepared), recorded on its stream now
static void record_prep(GroupRun* gr, hipStream_t st) {
  if (hipEventCreateWithFlags(&gr->prep, hipEventDisableTiming) != hipSuccess ||
      hipEventRecord(gr->prep, st) != hipSuccess) {
    (void)hipGetLastError();
    if (gr->prep) (void)hipEventDestroy(gr->prep);
    gr->prep = nullptr;
  }
}

// The start of a helper or leader group launch: the group's stream (own_queue: from
// ws_exec_stream_get, else the plain pool) and its run, both left in *gr.
static int group_begin(prio3_engine* lead, const DeviceGuard& dg, int jobs, bool own_queue,
                       uint32_t n, unsigned flags, uint32_t nseg, uint32_t hpke_stride,
                       GroupRun* gr) {
  *gr = GroupRun();
  gr->lead = lead;
  gr->jobs = jobs;
  HIPCHK(dg.rc);
  hipStream_t st = own_queue ? ws_exec_stream_get(lead->device) : ws_stream_get(lead->device);
  if (!st) return PRIO3_EDEVICE;
  int rc = PRIO3_OK;
  Run* R = run_create(lead, n, flags, nseg, st, &rc, hpke_stride);
  if (!R) {
    ws_exec_stream_put(lead->device, st);
    return rc;
  }
  gr->st = st;
  gr->R = R;
  return PRIO3_OK;
}
// ... and its failure path: the stream drained, run and stream given back, *gr cleared
static int group_fail(GroupRun* gr, int code) {
  (void)hipStreamSynchronize(gr->st);
  run_release(gr->R, gr->st, true);
  if (gr->prep) (void)hipEventDestroy(gr->prep);
  ws_exec_stream_put(gr->lead->device, gr->st);
  *gr = GroupRun();
  return code;
}

// Sealed-input groups: a report the open rejected (HPKE status 4 or 8) gets status 0x80 | that
// PrepareError, whatever its prepare computed on the zeroed share -- so the accumulate, which
// counts status 0 only, leaves it out, and the caller sees the error Janus records first.
// Then the report deadline (aggregator.rs:2004-2015, after the open and decode, before the VDAF's
// status counts): a report the open accepted whose time is after its job's deadline -- the
// deadline table's entry of its task slot -- gets 0x80 | ReportTooEarly, so it is left out of the
// accumulate the same way.  times == nullptr: no job of the group carries a deadline.
__global__ __launch_bounds__(256) void k_hpke_merge(uint32_t n, const uint8_t* hs, uint8_t* status,
                                                    const uint64_t* times, const uint16_t* tslot,
                                                    const uint64_t* dtab) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if (hs[i])
    status[i] = (uint8_t)(0x80u | hs[i]);
  else if (times && times[i] > dtab[tslot[i]])
    status[i] = (uint8_t)PRIO3_STATUS_REPORT_TOO_EARLY;
}

// The retry list of a group with a fallback keypair: the reports whose first open ended in
// HpkeDecryptError (4) and whose ciphertext length is one an open can accept -- the pad columns
// (length 0) and over- or undersized rows stay 4 under any key, so they cost no second ladder.
// list[0] is the count (zeroed on the stream before this launch), list[1 ..] the report indices,
// one atomic per wave; the order is arbitrary, every listed report rewrites its own row only.
__global__ __launch_bounds__(256) void k_hpke_retry_list(uint32_t n, const uint8_t* hs,
                                                         const uint32_t* ct_len,
                                                         uint32_t ct_stride, uint32_t* list) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool q = false;
  if (i < n && hs[i] == 4) {
    const uint32_t cl = ct_len[i];
    q = cl >= 16 && cl <= ct_stride;
  }
  const uint64_t m = __ballot(q);
  if (!m) return;  // wave-uniform
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(list, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, 0);
  if (q) list[1 + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

// Group launch (host pull, the r03 form).  The kernels read each report's nonce, public share,
// helper share and verify-key slot straight from the pinned staging (mapped), and each lane of the
// fused XOF + query launch copies its own leader prep share, segment id and accept byte into the
// run during its XOF (xofd_body PULL), so the transfer runs under that group's own Keccak work at
// the rate the lanes pull (~35 GB/s, profiles/r04).  One pinned-staging H2D copy per field ahead
// of the prepare, without the overlap (the r02 form), left transfer and prepare in series
// (profiles/r03/r03e_jobs128_*.json: 21.5 M reports/s); SDMA copies of each group issued under the
// previous group's compute (r04 option group_dma) measured 19.5-30.8 against 32-40 M/s for the
// pull and were removed in r05.
int engine_group_issue(prio3_engine* lead, const GroupView& g, GroupRun* gr, bool own_queue) {
  DeviceGuard dg_(lead->device);
  const bool mp = lead->dp.kind == PRIO3_SUMVEC_F64_MP;
  // aggregating jobs: the group's reports are accumulated per job segment in this launch (the
  // wave partials of the XOF where the instance fuses; waves that straddle two jobs and the
  // excluded reports go through the fix-up list)
  const bool agg = g.nseg > 0;
  const bool fuse = agg && prepare_fuses(lead);
  IoLayout L;
  if (g.L)
    L = *g.L;
  else
    engine_io_layout(lead, g.cap, &L);
  const bool sealed = L.ct_stride > 0 && g.opener;
  // prio3_helper_aggregate_job groups: the launch makes the jobs' index and metadata itself
  const bool jix = g.njix > 0 && agg && sealed && L.jix;
  if (g.njix && !jix) return PRIO3_EINVAL;
  int rc = group_begin(lead, dg_, g.jobs, own_queue, g.n,
                       RUN_SCRATCH | RUN_IO | (agg ? (unsigned)RUN_AGG_IO : 0u) |
                           (fuse ? (unsigned)RUN_FUSED : 0u) | (sealed ? (unsigned)RUN_HPKE : 0u) |
                           (jix ? (unsigned)RUN_JIX : 0u),
                       agg ? g.nseg : 0, sealed ? L.ct_stride : 0, gr);
  if (rc) return rc;
  Run* R = gr->R;
  hipStream_t st = gr->st;
  auto fail = [&](int code) { return group_fail(gr, code); };
  const uint8_t* hd = g.stg_dev;
  InPtrs in{hd + L.off[0], L.len[1] ? hd + L.off[1] : nullptr, hd + L.off[2], R->leader};
  if (jix) {
    // first on the stream: each job's workgroup turns its staged IDs, times, closed intervals and
    // host accept bytes into the group segment ids and accept bytes in the run (every column, the
    // pad columns included), where the prepare, the accumulate and the metadata below read them,
    // and into the job's index outputs in the staging
    uint8_t* sd = g.stg_dev;
    JixGroupArgs a{};
    a.desc = (const JixJobDesc*)(hd + L.jdesc_off);
    a.closed = (const unsigned long long*)(hd + L.jclosed_off);
    a.ids = hd + L.off[0];
    a.times = (const unsigned long long*)(hd + L.time_off);
    a.accept = hd + L.accept_off;
    a.ids_dev = R->nonces;
    a.gseg = R->gseg;
    a.gaccept = R->gaccept;
    a.seg_out = (uint32_t*)(sd + L.jseg_off);
    a.rej_out = sd + L.jrej_off;
    a.dup_out = sd + L.jdup_off;
    a.starts_out = (unsigned long long*)(sd + L.jstart_off);
    a.info_out = (prio3_job_index_info*)(sd + L.jinfo_off);
    if (launch_jix_group(lead, g.njix, a, st) != PRIO3_OK) return fail(PRIO3_EDEVICE);
  }
  if (sealed) {
    // the helper's loop body from its first line (aggregator.rs:1847-1990): each report's input
    // share opened, decoded and checked into the run's helper-share buffer, which the prepare
    // below reads from HBM -- the plaintexts never cross PCIe
    HpkeGroupArgs a{};
    a.n = g.n;
    a.ct_stride = L.ct_stride;
    a.share_len = lead->dp.helper_share_len;
    a.pub_len = (uint32_t)L.len[1];
    a.require_taskprov = g.require_taskprov;
    a.enc = hd + L.enc_off;
    a.ct = hd + L.ct_off;
    a.ct_len = (const uint32_t*)(hd + L.ctlen_off);
    a.ids = hd + L.off[0];
    a.times = (const uint64_t*)(hd + L.time_off);
    a.pubs = L.len[1] ? hd + L.off[1] : nullptr;
    a.task_slot = (const uint16_t*)(hd + L.tslot_off);
    a.task_tab = (const uint32_t*)(hd + L.ttab_off);
    a.pt = R->hpt;
    a.shares = R->helper;
    a.status = R->hstatus;
    if (hpke_open_group_launch(g.opener, a, st) != PRIO3_OK) return fail(PRIO3_EDEVICE);
    if (g.fallback) {
      // the reports the first keypair could not decrypt, opened again under the fallback keypair
      // (hpke::Error::Hpke(_) => try_hpke_open(global), aggregator.rs:1864-1878): the list is made
      // and consumed on the stream, the host never sees it; the second launch covers n lanes and
      // its blocks past the list leave at once.  It rewrites the listed rows' share, plaintext
      // and open status, which then pass through the same merge as a first open's.
      if (hipMemsetAsync(R->hretry, 0, 4, st) != hipSuccess) return fail(PRIO3_EDEVICE);
      k_hpke_retry_list<<<(g.n + 255) / 256, 256, 0, st>>>(g.n, R->hstatus, a.ct_len, L.ct_stride,
                                                          R->hretry);
      if (hipGetLastError() != hipSuccess) return fail(PRIO3_EDEVICE);
      a.idx = R->hretry + 1;
      a.n_idx = R->hretry;
      if (hpke_open_group_launch(g.fallback, a, st) != PRIO3_OK) return fail(PRIO3_EDEVICE);
    }
    in.helper = R->helper;
    // the executor may issue the next group as soon as this one's open is done: a group's open
    // (one X25519 ladder per lane, ~1 wave per SIMD on half the SIMDs at 31k reports) then runs
    // beside this group's prepare instead of after it
    record_prep(gr, st);
  }
  if (!mp) {  // the slots and the key table are read from the staging by the XOF
    in.vk_slot = (const uint16_t*)(hd + L.slot_off);
    in.vk_tab = (const uint4*)(hd + L.tab_off);
  }
  // the fused XOF's segment check (an indexed group's ids are made on the device, in the run)
  if (agg) R->seg = jix ? R->gseg : (const uint32_t*)(hd + L.seg_off);
  // the leader prep shares (and the segment ids / accept bytes of the fix-up pass)
  PullRanges pr{};
  pr.src[0] = hd + L.off[3];
  pr.dst[0] = R->leader;
  pr.bytes[0] = L.len[3] * g.n;
  if (agg && !jix) {  // (k_jix_group wrote an indexed group's straight into the run)
    pr.src[1] = hd + L.seg_off;
    pr.dst[1] = (uint8_t*)R->gseg;
    pr.bytes[1] = 4 * (size_t)g.n;
    pr.src[2] = hd + L.accept_off;
    pr.dst[2] = R->gaccept;
    pr.bytes[2] = g.n;
  }
  OutPtrs out{R->msgs, R->status};
  rc = prepare_run(lead, R, in, out, st, fuse, false, &pr);
  if (agg) R->seg = R->gseg;
  if (rc) return fail(rc);
  if (sealed) {  // the open's rejections take precedence (aggregator.rs:1850-1990 before :2020)
    k_hpke_merge<<<(g.n + 255) / 256, 256, 0, st>>>(
        g.n, R->hstatus, R->status, g.deadlines ? (const uint64_t*)(hd + L.time_off) : nullptr,
        (const uint16_t*)(hd + L.tslot_off), (const uint64_t*)(hd + L.dtab_off));
    if (hipGetLastError() != hipSuccess) return fail(PRIO3_EDEVICE);
  }
  // the executor may issue its next group once this group's prepare kernels are done
  if (!gr->prep) record_prep(gr, st);
  if (agg) {
    rc = fuse ? fused_finish(lead, R, R->status, R->gseg, R->gseg, R->gaccept, g.nseg, R->gagg,
                             (uint64_t*)R->gcnt, st)
              : run_accumulate(lead, R, 0, g.n, R->status, R->gseg, R->gaccept, g.nseg, R->gagg,
                               (uint64_t*)R->gcnt, st);
    if (rc) return fail(rc);
  }
  if (jix) {
    // the rest of the BatchAggregation update over the group's columns and segments, from the
    // merged statuses; the rows go back by a copy launch of their own
    rc = launch_batch_metadata(lead, g.n, R->nonces, (const uint64_t*)(hd + L.time_off), R->status,
                               R->gaccept, R->gseg, g.nseg, R->gck, R->giv, st);
    if (rc) return fail(rc);
    PullRanges m{};
    m.src[0] = (const uint8_t*)R->gck;
    m.dst[0] = g.stg_dev + L.ck_off;
    m.bytes[0] = 32 * (size_t)g.nseg;
    m.src[1] = (const uint8_t*)R->giv;
    m.dst[1] = g.stg_dev + L.iv_off;
    m.bytes[1] = 16 * (size_t)g.nseg;
    if (!pull_outputs(m, st)) return fail(PRIO3_EDEVICE);
  }
  {  // the outputs go back by one copy launch writing the mapped staging
    uint8_t* sd = g.stg_dev;
    PullRanges o{};
    o.src[0] = R->status;
    o.dst[0] = sd + L.status_off;
    o.bytes[0] = g.n;
    if (L.msg_len) {
      o.src[1] = R->msgs;
      o.dst[1] = sd + L.msg_off;
      o.bytes[1] = L.msg_len * g.n;
    }
    if (agg) {
      o.src[2] = R->gagg;
      o.dst[2] = sd + L.agg_off;
      o.bytes[2] = L.agg_len * g.nseg;
      o.src[3] = (const uint8_t*)R->gcnt;
      o.dst[3] = sd + L.cnt_off;
      o.bytes[3] = 8 * (size_t)g.nseg;
    }
    if (!pull_outputs(o, st)) return fail(PRIO3_EDEVICE);
  }
  return PRIO3_OK;
}

// the launcher polls these instead of sleeping in hipStreamSynchronize: the group's jobs are woken
// as soon as their outputs land (the blocking wait added ~0.1 ms per group)
bool engine_group_prepared(const GroupRun& gr) {
  return gr.prep && hipEventQuery(gr.prep) == hipSuccess;
}
bool engine_group_done(const GroupRun& gr) { return hipStreamQuery(gr.st) != hipErrorNotReady; }

int engine_group_finish(GroupRun* gr, Run** run_out) {
  *run_out = nullptr;
  hipError_t q = hipStreamQuery(gr->st);
  if (q == hipErrorNotReady) q = hipStreamSynchronize(gr->st);
  if (gr->prep) (void)hipEventDestroy(gr->prep);
  gr->prep = nullptr;
  const int dev = gr->lead->device;
  if (q != hipSuccess) {
    (void)hipGetLastError();
    run_release(gr->R, gr->st, true);
    ws_exec_stream_put(dev, gr->st);
    return PRIO3_EDEVICE;
  }
  if (gr->lead->timing) collect_times(gr->lead, false);
  gr->R->refs.store(gr->jobs);
  *run_out = gr->R;
  ws_exec_stream_put(dev, gr->st);
  return PRIO3_OK;
}


// ---- accumulate-executor hooks (prio3_runtime.h) ----
// One job's part of an accumulate area (`area`: the host staging laid out by L), for both job
// kinds that end in k_acc_multi -- AccJob and an aggregating LNextJob: the bytes of its aggregate
// shares + counts, its descriptor `slot` with its segment ids and accept bytes, and the copy of
// its outputs back to the caller.
static size_t acc_out_bytes(const Run* R, uint32_t nseg) {
  const size_t agg = (size_t)R->dp.out_len * R->dp.es * nseg;
  return ((agg + 7) & ~(size_t)7) + 8 * (size_t)nseg;
}
// an indexed prepare_next job: its segment ids and accept bytes are made on the device
static bool acc_indexed(const AccJob*) { return false; }
static bool acc_indexed(const LNextJob* j) { return j->jix; }
template <class Job>
static void acc_stage(const Job* j, uint32_t slot, uint8_t* area, const AccLayout& L) {
  const Run* R = j->run;
  AccDesc& D = ((AccDesc*)(area + L.desc_off))[slot];
  D.src = run_out_shares(R, j->c0);
  D.status = R->status + j->c0;  // the device verdicts
  D.ld = R->dp.ld_out;
  D.n = j->n;
  D.nseg = j->nseg;
  D.out_len = R->dp.out_len;
  D.flags = (j->seg ? 1u : 0u) | (j->accept ? 2u : 0u);
  D.seg_off = L.seg_off + 4 * (size_t)j->rep_off;
  D.acc_off = L.acc_off + j->rep_off;
  D.agg_off = L.out_off + j->out_off;
  D.cnt_off = D.agg_off + acc_out_bytes(R, j->nseg) - 8 * (size_t)j->nseg;
  if (acc_indexed(j)) {  // the group's index kernel writes both ranges in the device area
    D.flags = 3u;
    return;
  }
  if (j->seg) memcpy(area + D.seg_off, j->seg, 4 * (size_t)j->n);
  if (j->accept) memcpy(area + D.acc_off, j->accept, j->n);
}
template <class Job>
static void acc_unstage(const Job* j, uint32_t slot, const uint8_t* area, const AccLayout& L) {
  const DevParams& d = j->run->dp;
  const AccDesc& D = ((const AccDesc*)(area + L.desc_off))[slot];
  memcpy(j->agg_out, area + D.agg_off, (size_t)d.out_len * d.es * j->nseg);
  memcpy(j->counts_out, area + D.cnt_off, 8 * (size_t)j->nseg);
}

uint32_t engine_acc_key(const AccJob* j) { return j->run->dp.es; }
size_t engine_acc_out_bytes(const AccJob* j) { return acc_out_bytes(j->run, j->nseg); }
void engine_acc_stage(AccJob* j, uint8_t* stg, const AccLayout& L) {
  acc_stage(j, j->slot, stg, L);
}
void engine_acc_unstage(AccJob* j, const uint8_t* stg, const AccLayout& L) {
  acc_unstage(j, j->slot, stg, L);
}

int engine_acc_group(int device, int es, uint8_t* stg, const AccLayout& L, uint32_t n_jobs,
                     size_t out_bytes) {
  DeviceGuard dg_(device);
  HIPCHK(dg_.rc);
  PooledStream ps(device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  int rc = PRIO3_OK;
  Slab* sl = acc_multi_enqueue(device, (uint32_t)es, stg, L, n_jobs, out_bytes, st, &rc);
  if (!sl) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) rc = PRIO3_EDEVICE;
  ws_release(sl, st);
  return rc;
}

// ---- leader-executor hooks (prio3_runtime.h) ----
// The leader groups take the TurboSHAKE instances; FPVec (sub-batched runs) and the multiproof
// instance (HMAC midstates per engine) keep one run per call.
static bool leader_coalescable(const prio3_engine* e) {
  return e->coalesce && e->dp.kind != PRIO3_FPVEC_BOUNDED_L2 && e->dp.kind != PRIO3_SUMVEC_F64_MP;
}

void engine_leader_layout(const prio3_engine* e, uint32_t cap, LeaderLayout* L) {
  const DevParams& d = e->dp;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L->len[0] = 16;
  L->len[1] = d.public_share_len;
  L->len[2] = d.leader_share_len;
  size_t off = 0;
  for (int f = 0; f < 3; f++) {
    L->off[f] = off;
    off += up(L->len[f] * cap);
  }
  L->slot_off = off;
  off += up(2 * (size_t)cap);
  L->tab_off = off;
  off += up(16 * (size_t)exec_max_keys());
  L->ps_len = d.prep_share_len;
  L->ps_off = off;
  off += up(L->ps_len * cap);
  L->status_off = off;
  off += up(cap);
  L->bytes = off;
  L->cap = cap;
  // The executor's leader groups stage the input shares as plain rows, one DMA copies them into
  // the run, and the next group is issued as soon as that copy is done, so its copy runs under this
  // group's kernels.  Interleaved on one box (r06ai): 9.24 / 8.57 / 8.76 M reports/s against
  // 6.97 / 7.31 / 7.58 for the transposed staging read in-kernel (r06), whose
  // host-side transpose (~870 us of CPU per 500-report job) ran the process into the box's 16-CPU
  // quota.  JANUS_LEADER_SOA=1 (A/B): the transposed form.
  static const bool soa = [] {
    const char* v = getenv("JANUS_LEADER_SOA");
    return v && atoi(v) != 0;
  }();
  L->lin_soa = plan_leader(e).soa_staging && soa;
}

// A leader group: the explicit input shares (5.6 KB per Histogram(256) report) go to the run by
// one DMA, the kernels read the nonces, public shares and verify-key slots from the mapped
// staging, the prepare shares go back by the copy engine and one copy launch writes the statuses
// into the staging.
int engine_leader_issue(prio3_engine* lead, const LeaderLayout& L, uint8_t* stg, uint8_t* stg_dev,
                        uint32_t n, int jobs, GroupRun* gr, bool own_queue) {
  DeviceGuard dg_(lead->device);
  int rc = group_begin(lead, dg_, jobs, own_queue, n, RUN_SCRATCH | RUN_IO | RUN_LINPUT, 0, 0, gr);
  if (rc) return rc;
  Run* R = gr->R;
  hipStream_t st = gr->st;
  // The kernels read AoS rows from HBM.  The executor may issue its next group once this group's
  // shares are in HBM, so the next group's copy runs under this group's kernels (as a sealed
  // group's next goes after its open); r05 issued it only after this group's kernels, so copy and
  // kernels ran in series.  With lin_soa (A/B) k_leader_prep reads the transposed staging itself
  // instead, each wave load one 1 KiB PCIe read, and the other leader kernels read AoS rows from
  // the run.
  if (!L.lin_soa) {
    if (hipMemcpyAsync(R->linput, stg_dev + L.off[2], L.len[2] * n, hipMemcpyDefault, st) !=
        hipSuccess)
      return group_fail(gr, PRIO3_EDEVICE);
    record_prep(gr, st);
  }
  rc = leader_init_run(lead, R, stg_dev + L.off[0], L.len[1] ? stg_dev + L.off[1] : nullptr,
                       L.lin_soa ? stg_dev + L.off[2] : R->linput, R->leader, R->status, st,
                       (const uint16_t*)(stg_dev + L.slot_off), (const uint4*)(stg_dev + L.tab_off),
                       L.lin_soa ? L.cap : 0u);
  if (rc) return group_fail(gr, rc);
  if (!gr->prep) record_prep(gr, st);
  // the prepare shares (560 B per Histogram(256) report, 17 MB per 31k group) go back by the
  // copy engine: written by k_pull into the mapped staging they took 0.88 ms per group (~20 GB/s,
  // r06c kernel trace); the statuses by the copy kernel
  if (hipMemcpyAsync(stg + L.ps_off, R->leader, L.ps_len * n, hipMemcpyDeviceToHost, st) !=
      hipSuccess)
    return group_fail(gr, PRIO3_EDEVICE);
  PullRanges o{};
  o.src[0] = R->status;
  o.dst[0] = stg_dev + L.status_off;
  o.bytes[0] = n;
  if (!pull_outputs(o, st)) return group_fail(gr, PRIO3_EDEVICE);
  return PRIO3_OK;
}

uint32_t engine_lnext_key(const LNextJob* j) { return j->run->dp.es | (j->jix ? 0x100u : 0u); }

void engine_lnext_stage(LNextJob* j, uint8_t* stg, const LNextLayout& L) {
  const Run* R = j->run;
  const DevParams& d = R->dp;
  const size_t es = d.es;
  LNextDesc& D = ((LNextDesc*)(stg + L.desc_off))[j->slot];
  D.corrected = R->sc.corrected + j->c0;
  D.meas = (const uint8_t*)R->sc.meas + es * j->c0;
  D.out = own_out(d) ? (uint8_t*)R->sc.out + es * j->c0 : nullptr;
  D.dstatus = R->status + j->c0;
  D.ld = d.ld;
  D.n = j->n;
  D.rep_off = j->rep_off;
  D.kind = d.kind;
  D.bits = d.bits;
  D.out_len = d.out_len;
  D.jr = d.jr_len ? 1u : 0u;
  if (D.jr && j->msgs) memcpy(stg + L.msg_off + 16 * (size_t)j->rep_off, j->msgs, 16 * (size_t)j->n);
  memcpy(stg + L.status_off + j->rep_off, j->status, j->n);
  // its accumulate descriptor (offsets from the accumulate area's base; the verdicts it reads
  // are those of the check in the same launch)
  if (j->nseg) acc_stage(j, j->acc_slot, stg + L.acc_base, L.acc);
  if (!j->jix) return;
  // the index request: IDs, times, the helper's prepare_error and the host's accept bytes by
  // report; the job's descriptor and closed intervals, read here, before the call returns
  const size_t r0 = j->rep_off, n = j->n;
  memcpy(stg + L.id_off + 16 * r0, j->ids, 16 * n);
  memcpy(stg + L.time_off + 8 * r0, j->times, 8 * n);
  if (j->perr)
    memcpy(stg + L.perr_off + r0, j->perr, n);
  else
    memset(stg + L.perr_off + r0, 0xff, n);
  if (j->accept)
    memcpy(stg + L.hacc_off + r0, j->accept, n);
  else
    memset(stg + L.hacc_off + r0, 1, n);
  JixJobDesc jd;
  jd.c0 = j->rep_off;
  jd.n = j->n;
  jd.pad0 = j->rep_off;
  jd.end = j->rep_off + j->n;
  jd.seg0 = j->seg0;
  jd.max_segments = j->nseg;
  jd.closed0 = j->closed0;
  jd.k = j->precision ? j->nclosed : 0;
  jd.precision = j->precision;
  memcpy(stg + L.jdesc_off + sizeof(JixJobDesc) * j->jslot, &jd, sizeof jd);
  if (j->nclosed)
    memcpy(stg + L.jclosed_off + 16 * (size_t)j->closed0, j->closed, 16 * (size_t)j->nclosed);
}

size_t engine_lnext_out_bytes(const LNextJob* j) {
  return j->nseg ? acc_out_bytes(j->run, j->nseg) : 0;
}

void engine_lnext_unstage(LNextJob* j, const uint8_t* stg, const LNextLayout& L) {
  memcpy(j->status, stg + L.status_off + j->rep_off, j->n);
  if (j->nseg) acc_unstage(j, j->acc_slot, stg + L.acc_base, L.acc);
  if (!j->jix) return;
  const size_t r0 = j->rep_off, n = j->n, s0 = j->seg0, S = j->nseg;
  memcpy(j->jseg_out, stg + L.jseg_off + 4 * r0, 4 * n);
  if (j->jrej_out) memcpy(j->jrej_out, stg + L.jrej_off + r0, n);
  if (j->jdup_out) memcpy(j->jdup_out, stg + L.jdup_off + r0, n);
  if (j->outcome_out) memcpy(j->outcome_out, stg + L.outcome_off + r0, n);
  // a fixed-size task has no starts: the caller's array is left as it is (prio3_job_index)
  if (j->jstarts_out && j->precision) memcpy(j->jstarts_out, stg + L.jstart_off + 8 * s0, 8 * S);
  memcpy(j->jinfo_out, stg + L.jinfo_off + sizeof(prio3_job_index_info) * j->jslot,
         sizeof(prio3_job_index_info));
  if (j->ck_out) memcpy(j->ck_out, stg + L.ck_off + 32 * s0, 32 * S);
  if (j->iv_out) memcpy(j->iv_out, stg + L.iv_off + 16 * s0, 16 * S);
}

void engine_lnext_collect(prio3_engine* lead) {
  if (lead && lead->timing) collect_times(lead, false);
}

// The launches of an indexed group (prio3_leader_finish_job), in stream order -- the only
// ordering: k_jix_lgroup (group segment ids, accept and reject bytes into device memory, the
// index outputs into the staging), the check with the prepare_error overlay, k_acc_multi over the
// index's ids and accept bytes, the metadata launch over the group's contiguous reports.
static int lnext_issue_indexed(int device, uint32_t es, uint8_t* stg, uint8_t* stg_dev,
                               const LNextLayout& L, uint32_t n_jobs, uint32_t max_n,
                               uint32_t n_acc, size_t out_bytes, hipStream_t st,
                               const LNextJixGroup& jg, Slab** slab_out, Slab** slab2_out) {
  prio3_engine* e = jg.e;
  if (!L.jix || n_acc != n_jobs || jg.njix != n_jobs || !jg.reps || !jg.nseg ||
      jg.reps > LNEXT_MAX_REPS || jg.nseg > EXEC_MAX_SEGS)
    return PRIO3_EINVAL;
  LNextJixDev V;
  lnext_jix_dev_layout(&V);
  int rc = PRIO3_OK;
  Slab* area = ws_acquire(device, L.acc.bytes, st, &rc);
  if (!area) return rc;
  Slab* dev = ws_acquire(device, V.bytes, st, &rc);
  if (!dev) {
    ws_release(area, st);
    return rc;
  }
  uint8_t *ab = area->base, *db = dev->base;
  const uint8_t* hd = stg_dev;
  rc = [&]() -> int {
    JixGroupArgs a{};
    a.desc = (const JixJobDesc*)(hd + L.jdesc_off);
    a.closed = (const unsigned long long*)(hd + L.jclosed_off);
    a.ids = hd + L.id_off;
    a.times = (const unsigned long long*)(hd + L.time_off);
    a.accept = hd + L.hacc_off;
    a.ids_dev = db + V.ids_off;
    a.gseg = (uint32_t*)(db + V.gseg_off);
    a.gaccept = ab + L.acc.acc_off;
    a.seg_out = (uint32_t*)(stg_dev + L.jseg_off);
    a.rej_out = stg_dev + L.jrej_off;
    a.dup_out = stg_dev + L.jdup_off;
    a.starts_out = (unsigned long long*)(stg_dev + L.jstart_off);
    a.info_out = (prio3_job_index_info*)(stg_dev + L.jinfo_off);
    a.lseg = (uint32_t*)(ab + L.acc.seg_off);
    a.drej = db + V.rej_off;
    int r = launch_jix_group(e, n_jobs, a, st, true);
    if (r) return r;
    LNextJixPtrs jp;
    jp.perr = hd + L.perr_off;
    jp.drej = db + V.rej_off;
    jp.mstatus = db + V.mstatus_off;
    jp.outcome = stg_dev + L.outcome_off;
    TIMED(e, st, "k_leader_next_multi",
          (r = launch_leader_next_multi(es, (const LNextDesc*)(hd + L.desc_off), hd + L.msg_off,
                                        stg_dev + L.status_off, n_jobs, max_n, st, &jp)));
    return r;
  }();
  if (rc == PRIO3_OK) {
    // (on failure acc_multi_enqueue has drained the stream and released the area)
    Slab* got = nullptr;
    const int r2 = [&]() -> int {
      int r = PRIO3_OK;
      TIMED(e, st, "k_acc_multi",
            (got = acc_multi_enqueue(device, es, stg + L.acc_base, L.acc, n_acc, out_bytes, st, &r,
                                     area)));
      return r;
    }();
    if (!got) {
      ws_release(dev, st);
      return r2 ? r2 : PRIO3_EDEVICE;
    }
  } else {
    (void)hipStreamSynchronize(st);
    ws_release(area, st);
    ws_release(dev, st);
    return rc;
  }
  // the rest of the BatchAggregation update over the group's reports and segments, from the merged
  // statuses in device memory; the rows go back into the staging
  rc = launch_batch_metadata(e, jg.reps, db + V.ids_off, (const uint64_t*)(hd + L.time_off),
                             db + V.mstatus_off, ab + L.acc.acc_off,
                             (const uint32_t*)(db + V.gseg_off), jg.nseg,
                             (uint32_t*)(db + V.ck_off), (unsigned long long*)(db + V.iv_off), st);
  if (rc == PRIO3_OK &&
      (hipMemcpyAsync(stg + L.ck_off, db + V.ck_off, 32 * (size_t)jg.nseg, hipMemcpyDeviceToHost,
                      st) != hipSuccess ||
       hipMemcpyAsync(stg + L.iv_off, db + V.iv_off, 16 * (size_t)jg.nseg, hipMemcpyDeviceToHost,
                      st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (rc != PRIO3_OK) {
    (void)hipStreamSynchronize(st);
    ws_release(area, st);
    ws_release(dev, st);
    return rc;
  }
  *slab_out = area;
  *slab2_out = dev;
  return PRIO3_OK;
}

int engine_lnext_issue(int device, uint32_t es, uint8_t* stg, uint8_t* stg_dev,
                       const LNextLayout& L, uint32_t n_jobs, uint32_t max_n, uint32_t n_acc,
                       size_t out_bytes, hipStream_t* st_out, Slab** slab_out, bool own_queue,
                       const LNextJixGroup* jg, Slab** slab2_out) {
  *st_out = nullptr;
  *slab_out = nullptr;
  if (slab2_out) *slab2_out = nullptr;
  DeviceGuard dg_(device);
  HIPCHK(dg_.rc);
  hipStream_t st = own_queue ? ws_exec_stream_get(device) : ws_stream_get(device);
  if (!st) return PRIO3_EDEVICE;
  if (jg && jg->e) {
    const int rc = !slab2_out ? PRIO3_EINVAL
                              : lnext_issue_indexed(device, es, stg, stg_dev, L, n_jobs, max_n,
                                                    n_acc, out_bytes, st, *jg, slab_out, slab2_out);
    if (rc != PRIO3_OK) {
      (void)hipStreamSynchronize(st);
      (void)hipGetLastError();
      ws_exec_stream_put(device, st);
      return rc;
    }
    *st_out = st;
    return PRIO3_OK;
  }
  int rc = launch_leader_next_multi(es, (const LNextDesc*)(stg_dev + L.desc_off),
                                    stg_dev + L.msg_off, stg_dev + L.status_off, n_jobs, max_n, st);
  Slab* sl = nullptr;
  // the aggregating jobs' accumulate (leader_continued's output shares merged by the writer,
  // aggregation_job_writer.rs:591-695) on the same stream, over the staging's accumulate area
  if (rc == PRIO3_OK && n_acc)
    sl = acc_multi_enqueue(device, es, stg + L.acc_base, L.acc, n_acc, out_bytes, st, &rc);
  if (rc != PRIO3_OK) {
    (void)hipStreamSynchronize(st);
    ws_exec_stream_put(device, st);
    return rc;
  }
  *st_out = st;
  *slab_out = sl;
  return PRIO3_OK;
}

// sigma_e = sum_(c = 1 .. calls) alpha^(c e) mod p for e < P: the weights of sum_c g(alpha^c)
// over the coefficients of a polynomial g (alpha a P-th root of unity; p = HP128 or HP64)
static std::vector<u128> sigma_table(u128 alpha, uint32_t P, uint32_t calls, u128 p) {
  std::vector<u128> sig(P);
  for (uint32_t e = 0; e < P; e++) {
    const u128 ae = hpow(alpha, e, p);
    u128 s = 0, x = 1;
    for (uint32_t c = 1; c <= calls; c++) {
      x = hmul(x, ae, p);
      s += x;
      if (s < x || s >= p) s -= p;  // s < x: the sum wrapped past 2^128 (HP128)
    }
    sig[e] = s;
  }
  return sig;
}

extern "C" {

// A blocking host-to-device copy on a pooled non-blocking stream: a synchronous hipMemcpy runs on
// the legacy null stream, which waits for every blocking stream of the device -- the executor's
// CU-masked group streams are such streams -- so an engine created while another
// task's groups run would wait for them.
static int upload_blocking(int device, void* dst, const void* src, size_t bytes) {
  hipStream_t st = ws_stream_get(device);
  if (!st) return PRIO3_EDEVICE;
  const bool ok = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess;
  ws_stream_put(device, st);
  if (!ok) (void)hipGetLastError();
  return ok ? PRIO3_OK : PRIO3_EDEVICE;
}

int prio3_sizes(const prio3_params* params, prio3_sizes_t* out) {
  return fill_sizes(params, out, nullptr);
}

int prio3_engine_create_ex(const prio3_params* params, const uint8_t* verify_key,
                           size_t verify_key_len, int device, prio3_engine** out) {
  if (!params || !verify_key || !out) return PRIO3_EINVAL;
  const bool mp = params->kind == PRIO3_SUMVEC_F64_MP;
  if (verify_key_len != (mp ? 32u : 16u)) return PRIO3_EINVAL;
  prio3_engine* e = new prio3_engine();
  int rc = fill_sizes(params, &e->sz, &e->dp);
  if (rc) {
    delete e;
    return rc;
  }
  e->params = *params;
  if (!mp) memcpy(e->dp.vk, verify_key, 16);
  e->device = device;
  if (hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, device) !=
          hipSuccess ||
      e->n_cu <= 0)
    e->n_cu = 256;
  hipStream_t probe = nullptr;  // a GPU must be present: the product path has no CPU fallback
  DeviceGuard dg_(device);
  if (dg_.rc != hipSuccess ||
      hipStreamCreateWithFlags(&probe, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    delete e;
    return PRIO3_EDEVICE;
  }
  ws_stream_put(device, probe);  // the first member of the GPU's stream pool
  ws_warm(device);               // the rest of it, before any job runs
  const bool fpv = e->dp.kind == PRIO3_FPVEC_BOUNDED_L2;
  if (((e->dp.kind == PRIO3_HISTOGRAM || e->dp.kind == PRIO3_SUMVEC) &&
       (e->dp.P == 32 || e->dp.P == 64 || e->dp.P == 128)) ||
      (fpv && e->dp.logP <= 10 && e->dp.logP1 <= 10)) {
    // k_query_w / k_query_fpw: sigma_e = sum_(c=1..calls) alpha_P^(ce), e < P -- the weights of
    // sum_c p(alpha^c) over the polynomial's coefficients (FPVec: gadget 0's table, then gadget
    // 1's)
    const DevParams& d = e->dp;
    std::vector<uint4> sig;
    auto table = [&](uint32_t logP, uint32_t calls) {
      u128 alpha = 0;
      for (int k = 0; k < 4; k++) alpha |= (u128)d.roots128[logP][k] << (32 * k);
      for (const u128 s : sigma_table(alpha, 1u << logP, calls, HP128))
        sig.push_back(make_uint4((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)(s >> 64),
                                 (uint32_t)(s >> 96)));
    };
    table(d.logP, d.calls);
    if (fpv) table(d.logP1, d.calls1);
    if (hipMalloc((void**)&e->d_sigma128, sizeof(uint4) * sig.size()) != hipSuccess ||
        upload_blocking(device, e->d_sigma128, sig.data(), sizeof(uint4) * sig.size()) !=
            PRIO3_OK) {
      delete e;
      return PRIO3_EDEVICE;
    }
    e->dp.sigma_dev = e->d_sigma128;
  }
  if (mp) {  // prio3_mp64.hip constants
    const DevParams& d = e->dp;
    Mp64Params& m = e->mp;
    m.meas_len = d.meas_len;
    m.out_len = d.out_len;
    m.bits = params->bits;
    m.chunk = params->chunk_length;
    m.calls = d.calls;
    m.P = d.P;
    m.logP = d.logP;
    m.glen = d.glen;
    m.np = params->num_proofs;
    m.proof_len = d.proof_len / m.np;
    m.arity = d.arity;
    m.vlen = d.verifier_len;
    memcpy(m.dst, d.dst, sizeof m.dst);
    hmac_midstates_host(verify_key, 32, m.vk_ist, m.vk_ost);
    static const uint8_t zero32[32] = {0};
    hmac_midstates_host(zero32, 32, m.z_ist, m.z_ost);
    const u128 alpha = d.roots64[d.logP];
    m.alpha = (uint64_t)alpha;
    m.alpha_inv = (uint64_t)hpow(alpha, d.P - 1, HP64);
    m.invP = d.invP64;
    m.half = d.half64;
    std::vector<uint64_t> sig;
    for (const u128 s : sigma_table(alpha, d.P, d.calls, HP64)) sig.push_back((uint64_t)s);
    if (hipMalloc((void**)&e->d_sigma64, 8 * (size_t)d.P) != hipSuccess ||
        upload_blocking(device, e->d_sigma64, sig.data(), 8 * (size_t)d.P) != PRIO3_OK) {
      delete e;
      return PRIO3_EDEVICE;
    }
    m.sigma = e->d_sigma64;
  }
  *out = e;
  return PRIO3_OK;
}

int prio3_engine_create(const prio3_params* params, const uint8_t verify_key[16], int device,
                        prio3_engine** out) {
  return prio3_engine_create_ex(params, verify_key, 16, device, out);
}

int prio3_engine_create_devices(const prio3_params* params, const uint8_t* verify_key,
                                size_t verify_key_len, const int* devices, uint32_t n_devices,
                                prio3_engine** out) {
  if (!out || !devices || n_devices == 0 || n_devices > (uint32_t)EXEC_LANES * 64)
    return PRIO3_EINVAL;
  *out = nullptr;
  std::vector<prio3_engine*> ms;
  for (uint32_t i = 0; i < n_devices; i++) {
    // the lane of a GPU named again: its own executor (a one-GPU rehearsal of the placement)
    int lane = 0;
    for (uint32_t j = 0; j < i; j++) lane += devices[j] == devices[i];
    prio3_engine* m = nullptr;
    const int rc = lane < EXEC_LANES
                       ? prio3_engine_create_ex(params, verify_key, verify_key_len, devices[i], &m)
                       : PRIO3_EINVAL;
    if (rc != PRIO3_OK) {
      for (auto x : ms) prio3_engine_destroy(x);
      return rc;
    }
    m->lane = lane;
    ms.push_back(m);
  }
  prio3_engine* e = ms[0];
  if (ms.size() > 1) {
    e->members = ms;
    for (size_t i = 1; i < ms.size(); i++) ms[i]->owner = e;
  }
  *out = e;
  return PRIO3_OK;
}

int prio3_engine_create_mask(const prio3_params* params, const uint8_t* verify_key,
                             size_t verify_key_len, int device_mask, prio3_engine** out) {
  std::vector<int> devs;
  for (int d = 0; d < 31; d++)
    if (device_mask & (1 << d)) devs.push_back(d);
  if (device_mask <= 0 || devs.empty()) return PRIO3_EINVAL;
  return prio3_engine_create_devices(params, verify_key, verify_key_len, devs.data(),
                                     (uint32_t)devs.size(), out);
}

// the engines of e: its members, or e itself where it is a one-GPU engine
static size_t member_count(const prio3_engine* e) {
  return e->members.empty() ? 1 : e->members.size();
}
static prio3_engine* member_at(const prio3_engine* e, size_t i) {
  return e->members.empty() ? const_cast<prio3_engine*>(e) : e->members[i];
}
// the executor of `kind` that serves m: the accumulate and prepare_next executors are one per GPU
// (lane 0)
static int member_exec_id(const prio3_engine* m, int kind) {
  const bool per_gpu = kind == EXEC_ACC || kind == EXEC_LNEXT;
  return per_gpu ? m->device * EXEC_LANES : engine_exec_id(m);
}

int prio3_engine_members(const prio3_engine* e, prio3_member_info* out, uint32_t cap) {
  if (!e) return PRIO3_EINVAL;
  const uint32_t k = (uint32_t)member_count(e);
  for (uint32_t i = 0; i < k && i < cap && out; i++) {
    const prio3_engine* m = member_at(e, i);
    prio3_member_info& x = out[i];
    x.device = m->device;
    x.lane = (uint32_t)m->lane;
    x.jobs = m->placed_jobs.load();
    x.reports = m->placed_reports.load();
    ExecStats st;
    if (exec_stats(EXEC_PREP, engine_exec_id(m), &st) != PRIO3_OK) st = ExecStats();
    x.exec_jobs = st.jobs;
    x.exec_groups = st.groups;
  }
  return (int)k;
}

int prio3_executor_stats_get(const prio3_engine* e, uint32_t member, int kind,
                             prio3_executor_stats* out) {
  if (!e || !out || kind < 0 || kind >= EXEC_KINDS) return PRIO3_EINVAL;
  if (member >= member_count(e)) return PRIO3_EINVAL;
  ExecStats st;
  const int rc = exec_stats(kind, member_exec_id(member_at(e, member), kind), &st);
  if (rc != PRIO3_OK) return rc;
  out->jobs = st.jobs;
  out->reports = st.reports;
  out->groups = st.groups;
  out->active_jobs = st.active_jobs;
  out->active_reports = st.active_reports;
  return PRIO3_OK;
}

int prio3_executor_control(prio3_engine* e, int which, const char* key, int64_t value) {
  if (!e || !key || which < -1 || which >= EXEC_KINDS) return PRIO3_EINVAL;
  for (size_t i = 0; i < member_count(e); i++)
    for (int kind : {(int)EXEC_PREP, (int)EXEC_ACC, (int)EXEC_LEADER, (int)EXEC_LNEXT,
                     (int)EXEC_UPLOAD}) {
      if (which >= 0 && kind != which) continue;
      const int rc = exec_control(kind, member_exec_id(member_at(e, i), kind), key, value);
      if (rc != PRIO3_OK) return rc;
    }
  return PRIO3_OK;
}

void prio3_engine_destroy(prio3_engine* e) {
  if (!e) return;
  for (size_t i = 1; i < e->members.size(); i++) prio3_engine_destroy(e->members[i]);
  e->members.clear();
  DeviceGuard dg_(e->device);
  (void)hipDeviceSynchronize();
  {
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->cur) run_release(e->cur, nullptr, true);
    e->cur = nullptr;
  }
  collect_times(e);
  if (e->d_sigma64) (void)hipFree(e->d_sigma64);
  if (e->d_sigma128) (void)hipFree(e->d_sigma128);
  for (auto s2 : e->side) (void)hipStreamDestroy(s2);
  for (auto j : e->side_ev) (void)hipEventDestroy(j);
  if (e->fork_ev) (void)hipEventDestroy(e->fork_ev);
  delete e;
}

int prio3_engine_set_option(prio3_engine* e, const char* key, int64_t value) {
  if (!e || !key) return PRIO3_EINVAL;
  for (size_t i = 1; i < e->members.size(); i++) {  // a multi-GPU engine: every member alike
    const int rc = prio3_engine_set_option(e->members[i], key, value);
    if (rc != PRIO3_OK) return rc;
  }
  struct {
    const char* name;
    int* field;
  } ints[] = {{"force_slow_path", &e->force_slow}, {"chunks", &e->chunks},
              {"leader_fast", &e->leader_fast},    {"fuse_acc", &e->fuse_acc},
              {"fp_round", &e->fp_round},          {"timing", &e->timing},
              {"coalesce", &e->coalesce},          {"experimental_fpvec", &e->experimental_fpvec},
              {"leader_fuse_acc", &e->leader_fuse_acc},
              {"force_generic_query", &e->force_generic}, {"pair_max", &e->pair_max},
              {"keep_scratch", &e->keep_scratch},  {"upload_aead", &e->upload_aead}};
  for (auto& o : ints)
    if (!strcmp(key, o.name)) {
      *o.field = (int)value;
      return PRIO3_OK;
    }
#ifdef JANUS_TEST_REJECT
  // test-rejection build only: the samplers also reject candidates whose top `value` bits are ones
  if (!strcmp(key, "test_reject_bits")) {
    if (value < 0 || value > 24) return PRIO3_EINVAL;
    e->dp.test_reject = (uint32_t)value;
    return PRIO3_OK;
  }
#endif
  if (!strcmp(key, "fp_sub_bytes")) {  // FPVec scratch budget per sub-batch (0 = auto)
    if (value < 0) return PRIO3_EINVAL;
    e->fp_sub_bytes = value;
    return PRIO3_OK;
  }
  return PRIO3_EINVAL;
}

// PRIO3_FPVEC_BOUNDED_L2 prepares only after the explicit opt-in (option experimental_fpvec):
// its circuit is an unpinned reconstruction
static bool fpvec_refused(const prio3_engine* e) {
  return e->dp.kind == PRIO3_FPVEC_BOUNDED_L2 && !e->experimental_fpvec;
}

// ---- device-resident entry points ----
// A device-resident prepare replaces the engine's current run: the previous one is released
// (stream-ordered, so its slab can be reused by this very call) and this one stays until the
// next device-resident prepare -- "output shares remain until the next prio3_device_prepare".
static Run* device_run(prio3_engine* e, uint32_t n, unsigned flags, uint32_t nseg,
                       hipStream_t st, int* rc) {
  if (e->cur) run_release(e->cur, st, true);
  e->cur = run_create(e, n, flags, nseg, st, rc);
  return e->cur;
}

int prio3_device_prepare(prio3_engine* e, uint32_t n, const uint8_t* d_nonces,
                         const uint8_t* d_public_shares, const uint8_t* d_helper_shares,
                         const uint8_t* d_leader_prep_shares, uint8_t* d_prep_msgs,
                         uint8_t* d_status, void* stream) {
  TraceSpan span_("VDAF preparation");
  if (!e) return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  if (n == 0) return PRIO3_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  int rc = PRIO3_OK;
  Run* R = device_run(e, n, RUN_SCRATCH, 0, st, &rc);
  if (!R) return rc;
  InPtrs in{d_nonces, d_public_shares, d_helper_shares, d_leader_prep_shares};
  return prepare_run(e, R, in, OutPtrs{d_prep_msgs, d_status}, st, false, true);
}

int prio3_device_prepare_aggregate(prio3_engine* e, uint32_t n, const uint8_t* d_nonces,
                                   const uint8_t* d_public_shares, const uint8_t* d_helper_shares,
                                   const uint8_t* d_leader_prep_shares,
                                   const uint32_t* d_segment_ids, uint32_t n_segments,
                                   uint8_t* d_prep_msgs, uint8_t* d_status, void* stream) {
  TraceSpan span_("VDAF preparation + batch aggregation");
  if (!e || n_segments == 0) return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  const bool fuse = n > 0 && prepare_fuses(e);
  int rc = PRIO3_OK;
  Run* R = device_run(e, n, RUN_SCRATCH | (fuse ? (unsigned)RUN_FUSED : 0u), n_segments, st, &rc);
  if (!R) return rc;
  R->seg = d_segment_ids;
  R->aggregate = true;
  if (n == 0) return PRIO3_OK;
  InPtrs in{d_nonces, d_public_shares, d_helper_shares, d_leader_prep_shares};
  rc = prepare_run(e, R, in, OutPtrs{d_prep_msgs, d_status}, st, fuse, true);
  if (rc == PRIO3_OK) R->fused = fuse;
  return rc;
}

int prio3_device_aggregate_finish(prio3_engine* e, const uint8_t* d_status,
                                  const uint8_t* d_accept_mask, uint8_t* d_agg_shares,
                                  uint64_t* d_counts, void* stream) {
  TraceSpan span_("batch aggregation");
  if (!e) return PRIO3_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  Run* R = e->cur;
  if (!R || !R->aggregate) return PRIO3_EINVAL;  // finish follows prio3_device_prepare_aggregate
  R->last = st;
  if (!R->fused)  // not fusable (or an empty batch): the one-pass segmented reduction
    return run_accumulate(e, R, 0, R->n, d_status, R->seg, d_accept_mask, R->nseg, d_agg_shares,
                          d_counts, st);
  return fused_finish(e, R, d_status, R->seg, R->seg, d_accept_mask, R->nseg, d_agg_shares,
                      d_counts, st);
}

int prio3_device_accumulate(prio3_engine* e, uint32_t n, const uint8_t* d_status,
                            const uint32_t* d_segment_ids, const uint8_t* d_accept_mask,
                            uint32_t n_segments, uint8_t* d_agg_shares, uint64_t* d_counts,
                            void* stream) {
  TraceSpan span_("batch aggregation");
  if (!e || n_segments == 0) return PRIO3_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;  // NULL = the null stream (HIP convention)
  const size_t agg_len = (size_t)e->dp.out_len * e->dp.es;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(d_agg_shares, 0, agg_len * n_segments, st));
    HIPCHK(hipMemsetAsync(d_counts, 0, 8 * (size_t)n_segments, st));
    return PRIO3_OK;
  }
  Run* R = e->cur;
  if (!R || n > R->n) return PRIO3_EINVAL;
  if (R->lfused && n == R->n && n_segments == 1) {
    R->last = st;
    return fused_finish(e, R, d_status, d_segment_ids, nullptr, d_accept_mask, 1, d_agg_shares,
                        d_counts, st);
  }
  return run_accumulate(e, R, 0, n, d_status, d_segment_ids, d_accept_mask, n_segments,
                        d_agg_shares, d_counts, st);
}

int prio3_device_combine(prio3_engine* e, uint32_t k, uint32_t n_segments, const uint8_t* d_in,
                         const uint64_t* d_counts_in, uint8_t* d_out, uint64_t* d_counts_out,
                         void* stream) {
  TraceSpan span_("aggregate share combine");
  if (!e || k == 0 || n_segments == 0) return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  // NULL = the null stream (HIP convention)
  return launch_combine(e, k, n_segments, d_in, d_counts_in, d_out, d_counts_out,
                        (hipStream_t)stream);
}

int prio3_device_batch_metadata(prio3_engine* e, uint32_t n, const uint8_t* d_report_ids,
                                const uint64_t* d_times, const uint8_t* d_status,
                                const uint8_t* d_accept_mask, const uint32_t* d_segment_ids,
                                uint32_t n_segments, uint8_t* d_checksums, uint64_t* d_intervals,
                                void* stream) {
  TraceSpan span_("batch aggregation metadata");
  if (!e || n_segments == 0 || (n && (!d_status || (d_checksums && !d_report_ids))))
    return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  // NULL = the null stream (HIP convention)
  return launch_batch_metadata(e, n, d_report_ids, d_times, d_status, d_accept_mask,
                               d_segment_ids, n_segments, (uint32_t*)d_checksums,
                               (unsigned long long*)d_intervals, (hipStream_t)stream);
}

int prio3_device_combine_metadata(prio3_engine* e, uint32_t k, uint32_t n_segments,
                                  const uint8_t* d_checksums_in, const uint64_t* d_intervals_in,
                                  uint8_t* d_checksums_out, uint64_t* d_intervals_out,
                                  void* stream) {
  if (!e || k == 0 || n_segments == 0) return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  // NULL = the null stream (HIP convention)
  return launch_combine_metadata(e, k, n_segments, (const uint32_t*)d_checksums_in,
                                 (const unsigned long long*)d_intervals_in,
                                 (uint32_t*)d_checksums_out,
                                 (unsigned long long*)d_intervals_out, (hipStream_t)stream);
}

int prio3_batch_metadata(prio3_engine* e, uint32_t n, const uint8_t* report_ids,
                         const uint64_t* times, const uint8_t* status, const uint8_t* accept_mask,
                         const uint32_t* segment_ids, uint32_t n_segments, uint8_t* checksums_out,
                         uint64_t* intervals_out) {
  if (!e || n_segments == 0 || (n && (!status || !report_ids))) return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(e->device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  const size_t N = n ? n : 1, S = n_segments;
  const size_t al = 256;
  auto up = [&](size_t b) { return (b + al - 1) / al * al; };
  const size_t o_ids = 0, o_st = o_ids + up(16 * N), o_t = o_st + up(N), o_mask = o_t + up(8 * N),
               o_seg = o_mask + up(N), o_ck = o_seg + up(4 * N), o_iv = o_ck + up(32 * S),
               total = o_iv + up(16 * S);
  int rc = PRIO3_OK;
  Slab* sl = ws_acquire(e->device, total, st, &rc);
  if (!sl) return rc;
  uint8_t* b = sl->base;
  auto h2d = [&](size_t off, const void* src, size_t bytes) {
    return !src || !bytes ||
           hipMemcpyAsync(b + off, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
  };
  if (!h2d(o_ids, report_ids, 16 * (size_t)n) || !h2d(o_st, status, n) ||
      !h2d(o_t, times, 8 * (size_t)n) || !h2d(o_mask, accept_mask, n) ||
      !h2d(o_seg, segment_ids, 4 * (size_t)n))
    rc = PRIO3_EDEVICE;
  if (rc == PRIO3_OK)
    rc = prio3_device_batch_metadata(
        e, n, b + o_ids, times ? (const uint64_t*)(b + o_t) : nullptr, b + o_st,
        accept_mask ? b + o_mask : nullptr, segment_ids ? (const uint32_t*)(b + o_seg) : nullptr,
        n_segments, checksums_out ? b + o_ck : nullptr,
        intervals_out ? (uint64_t*)(b + o_iv) : nullptr, st);
  if (rc == PRIO3_OK &&
      ((checksums_out && hipMemcpyAsync(checksums_out, b + o_ck, 32 * S, hipMemcpyDeviceToHost,
                                        st) != hipSuccess) ||
       (intervals_out && hipMemcpyAsync(intervals_out, b + o_iv, 16 * S, hipMemcpyDeviceToHost,
                                        st) != hipSuccess) ||
       hipStreamSynchronize(st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (e->timing) collect_times(e);
  ws_release(sl, st);
  return rc;
}

int prio3_device_output_shares(prio3_engine* e, uint32_t n, uint8_t* out) {
  if (!e || !out) return PRIO3_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  Run* R = e->cur;
  if (!R || n > R->n) return PRIO3_EINVAL;
  HIPCHK(hipDeviceSynchronize());  // the run's work may sit on any caller stream
  PooledStream ps(e->device);
  if (!ps.s) return PRIO3_EDEVICE;
  return run_output_shares(R, 0, n, out, ps.s);
}

// ---- tickets (the *_submit entry points) ----
// A job between its submit and its wait.  xt == nullptr: a synchronous path -- the blocking twin
// ran inside submit and the ticket was born done.  Every entry point below has one body for both
// forms: `tk` is nullptr for the blocking call, which then goes through the executor's blocking
// submit exactly as before.
struct prio3_ticket {
  enum Kind { SYNC, HELPER, LEADER_INIT, LEADER_NEXT, UPLOAD };
  Kind kind = SYNC;
  ExecTicket* xt = nullptr;
  prio3_engine* e = nullptr;  // LEADER_INIT: the member the job was placed on, its report count
  uint32_t n = 0;             // and where the batch handle goes
  prio3_batch** batch_out = nullptr;
};

// the end of a synchronous path: the blocking form returns rc; the submit form hands out a done
// ticket and writes the fd -- a failed call leaves nothing outstanding and the fd alone
static int ticket_sync(int rc, int notify_fd, prio3_ticket** tk) {
  if (!tk || rc != PRIO3_OK) return rc;
  *tk = new prio3_ticket();
  const uint64_t one = 1;
  if (notify_fd >= 0) (void)!write(notify_fd, &one, sizeof one);
  return PRIO3_OK;
}

static int ticket_queued(int rc, prio3_ticket::Kind kind, ExecTicket* xt, prio3_ticket** tk,
                         prio3_engine* e = nullptr, uint32_t n = 0,
                         prio3_batch** batch_out = nullptr) {
  if (rc != PRIO3_OK) return rc;
  prio3_ticket* t = new prio3_ticket();
  t->kind = kind;
  t->xt = xt;
  t->e = e;
  t->n = n;
  t->batch_out = batch_out;
  *tk = t;
  return PRIO3_OK;
}

// a helper job of the prepare executor, blocking (tk == nullptr) or ticketed
static int helper_exec(ExecJob* job, int notify_fd, prio3_ticket** tk) {
  if (tk) {
    ExecTicket* xt = nullptr;
    return ticket_queued(exec_submit_begin(job, notify_fd, &xt), prio3_ticket::HELPER, xt, tk);
  }
  const int rc = exec_submit(job);
  if (rc) return rc;
  run_release(job->run, nullptr, false);  // no batch handle: the output shares are not kept
  return PRIO3_OK;
}

static int leader_next_exec(LNextJob* job, int notify_fd, prio3_ticket** tk) {
  if (!tk) return exec_leader_next(job);
  ExecTicket* xt = nullptr;
  return ticket_queued(exec_leader_next_begin(job, notify_fd, &xt), prio3_ticket::LEADER_NEXT, xt,
                       tk);
}

int prio3_ticket_poll(const prio3_ticket* t) {
  if (!t) return 1;
  return !t->xt || exec_ticket_done(t->xt) ? 1 : 0;
}

int prio3_ticket_wait(prio3_ticket* t) {
  if (!t) return PRIO3_EINVAL;
  int rc = PRIO3_OK;
  switch (t->kind) {
    case prio3_ticket::SYNC: break;
    case prio3_ticket::HELPER: {
      TraceSpan span_("handle_aggregate_init_generic threadpool task");
      ExecJob job;
      rc = exec_ticket_complete(t->xt, &job);
      if (rc == PRIO3_OK) run_release(job.run, nullptr, false);
      break;
    }
    case prio3_ticket::LEADER_INIT: {
      TraceSpan span_("leader VDAF preparation");
      LeaderJob job{};
      rc = exec_ticket_complete(t->xt, &job);
      if (rc != PRIO3_OK) break;
      if (t->batch_out)
        *t->batch_out = new prio3_batch{t->e, job.run, job.c0, t->n};
      else
        run_release(job.run, nullptr, false);
      break;
    }
    case prio3_ticket::LEADER_NEXT: {
      TraceSpan span_("leader VDAF preparation");
      rc = exec_ticket_complete(t->xt, nullptr);
      break;
    }
    case prio3_ticket::UPLOAD: {
      TraceSpan span_("handle_upload_generic");
      rc = exec_ticket_complete(t->xt, nullptr);
      break;
    }
  }
  delete t;
  return rc;
}

// ---- host-buffer entry points (what the Rust FFI calls from inside rayon::spawn) ----
// A helper job of the prepare executor; nseg > 0: it also aggregates in the group's launch.  The
// sealed form (helper_aggregate_init) adds its own fields.
static ExecJob helper_job(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                          const uint8_t* public_shares, const uint8_t* helper_shares,
                          const uint8_t* leader_prep_shares, uint8_t* prep_msgs_out,
                          uint8_t* status_out, const uint32_t* segment_ids = nullptr,
                          const uint8_t* accept_mask = nullptr, uint32_t n_segments = 0,
                          uint8_t* agg_shares_out = nullptr, uint64_t* counts_out = nullptr) {
  ExecJob job;
  job.e = e;
  job.n = n;
  job.nonces = nonces;
  job.pub = e->dp.jr_len ? public_shares : nullptr;
  job.helper = helper_shares;
  job.leader = leader_prep_shares;
  job.msgs_out = prep_msgs_out;
  job.status_out = status_out;
  job.seg = segment_ids;
  job.accept = accept_mask;
  job.nseg = n_segments;
  job.agg_out = agg_shares_out;
  job.counts_out = counts_out;
  return job;
}

// (e: the member the job was placed on)
static int helper_prepare_batch(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                const uint8_t* public_shares, const uint8_t* helper_shares,
                                const uint8_t* leader_prep_shares, uint8_t* prep_msgs_out,
                                uint8_t* status_out, prio3_batch** batch_out, bool placed) {
  if (!e || (n && (!nonces || !helper_shares || !leader_prep_shares || !status_out)))
    return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  const DevParams& d = e->dp;
  if (n && d.jr_len && (!public_shares || !prep_msgs_out)) return PRIO3_EINVAL;
  if (n && !placed) e = place(e, n);
  if (n == 0) {
    if (batch_out) *batch_out = new prio3_batch{e, nullptr, 0, 0};
    return PRIO3_OK;
  }
  ExecJob job = helper_job(e, n, nonces, public_shares, helper_shares, leader_prep_shares,
                           prep_msgs_out, status_out);
  const int rc = exec_submit(&job);
  if (rc) return rc;
  if (batch_out)
    *batch_out = new prio3_batch{e, job.run, job.c0, n};
  else
    run_release(job.run, nullptr, false);
  return PRIO3_OK;
}

int prio3_helper_prepare_batch(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                               const uint8_t* public_shares, const uint8_t* helper_shares,
                               const uint8_t* leader_prep_shares, uint8_t* prep_msgs_out,
                               uint8_t* status_out, prio3_batch** batch_out) {
  TraceSpan span_("handle_aggregate_init_generic threadpool task");
  return helper_prepare_batch(e, n, nonces, public_shares, helper_shares, leader_prep_shares,
                              prep_msgs_out, status_out, batch_out, false);
}

static int helper_prepare_aggregate(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                    const uint8_t* public_shares, const uint8_t* helper_shares,
                                    const uint8_t* leader_prep_shares, const uint32_t* segment_ids,
                                    const uint8_t* accept_mask, uint32_t n_segments,
                                    uint8_t* prep_msgs_out, uint8_t* status_out,
                                    uint8_t* agg_shares_out, uint64_t* counts_out, int notify_fd,
                                    prio3_ticket** tk) {
  TraceSpan span_("handle_aggregate_init_generic threadpool task");
  if (!e || n_segments == 0 || !agg_shares_out || !counts_out ||
      (n && (!nonces || !helper_shares || !leader_prep_shares || !status_out)))
    return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  const DevParams& d = e->dp;
  if (n && d.jr_len && (!public_shares || !prep_msgs_out)) return PRIO3_EINVAL;
  if (n) e = place(e, n);
  const size_t agg_len = (size_t)d.out_len * d.es;
  IoLayout L1;
  engine_io_layout(e, 1, &L1);
  if (n == 0 || !e->coalesce || n_segments > L1.max_seg) {
    // not coalescable (or empty): the two calls, as the caller would make them
    prio3_batch* b = nullptr;
    int rc = helper_prepare_batch(e, n, nonces, public_shares, helper_shares,
                                  leader_prep_shares, prep_msgs_out, status_out, &b, true);
    if (rc == PRIO3_OK) rc = prio3_accumulate(b, segment_ids, accept_mask, n_segments,
                                              agg_shares_out, counts_out);
    prio3_batch_free(b);
    if (rc == PRIO3_OK && n == 0) {
      memset(agg_shares_out, 0, agg_len * n_segments);
      memset(counts_out, 0, 8 * (size_t)n_segments);
    }
    return ticket_sync(rc, notify_fd, tk);
  }
  ExecJob job = helper_job(e, n, nonces, public_shares, helper_shares, leader_prep_shares,
                           prep_msgs_out, status_out, segment_ids, accept_mask, n_segments,
                           agg_shares_out, counts_out);
  return helper_exec(&job, notify_fd, tk);
}

int prio3_helper_prepare_aggregate_batch(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                         const uint8_t* public_shares,
                                         const uint8_t* helper_shares,
                                         const uint8_t* leader_prep_shares,
                                         const uint32_t* segment_ids, const uint8_t* accept_mask,
                                         uint32_t n_segments, uint8_t* prep_msgs_out,
                                         uint8_t* status_out, uint8_t* agg_shares_out,
                                         uint64_t* counts_out) {
  return helper_prepare_aggregate(e, n, nonces, public_shares, helper_shares, leader_prep_shares,
                                  segment_ids, accept_mask, n_segments, prep_msgs_out, status_out,
                                  agg_shares_out, counts_out, -1, nullptr);
}

int prio3_helper_prepare_aggregate_batch_submit(
    prio3_engine* e, uint32_t n, const uint8_t* nonces, const uint8_t* public_shares,
    const uint8_t* helper_shares, const uint8_t* leader_prep_shares, const uint32_t* segment_ids,
    const uint8_t* accept_mask, uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out,
    uint8_t* agg_shares_out, uint64_t* counts_out, int notify_fd, prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return helper_prepare_aggregate(e, n, nonces, public_shares, helper_shares, leader_prep_shares,
                                  segment_ids, accept_mask, n_segments, prep_msgs_out, status_out,
                                  agg_shares_out, counts_out, notify_fd, ticket_out);
}

// The two-call form of helper_aggregate_init for a job with more segments than one group can
// aggregate: the open (and the fallback keypair's retry of the HpkeDecryptError rows) as host
// calls, then the prepare + aggregate of what it opened, then the merged statuses.
static int aggregate_init_two_calls(
    prio3_engine* e, janus_hpke_opener* opener, janus_hpke_opener* fallback_opener,
    uint64_t report_deadline, uint32_t n, const uint8_t task_id[32], int require_taskprov,
    const uint8_t* report_ids, const uint64_t* times, const uint8_t* public_shares,
    const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len, uint32_t ct_stride,
    const uint8_t* leader_prep_shares, const uint32_t* segment_ids, const uint8_t* accept_mask,
    uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out,
    uint64_t* counts_out) {
  const DevParams& d = e->dp;
  std::vector<uint8_t> shares((size_t)d.helper_share_len * n), hs(n), acc(n);
  int rc = janus_hpke_open_input_shares(opener, n, task_id, enc, ct, ct_len, ct_stride,
                                        report_ids, times, d.jr_len ? public_shares : nullptr,
                                        d.public_share_len, d.helper_share_len,
                                        require_taskprov, shares.data(), hs.data());
  if (rc) return rc == JANUS_HPKE_EDEVICE ? PRIO3_EDEVICE : PRIO3_EINVAL;
  if (fallback_opener) {  // the HpkeDecryptError rows again, under the fallback keypair
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; i++)
      if (hs[i] == 4 && ct_len[i] >= 16 && ct_len[i] <= ct_stride) idx.push_back(i);
    const uint32_t m = (uint32_t)idx.size();
    if (m) {
      const size_t nenc = hpke_opener_nenc(opener), pl = d.jr_len ? d.public_share_len : 0;
      std::vector<uint8_t> enc2(nenc * m), ct2((size_t)ct_stride * m), ids2(16 * (size_t)m),
          pub2(pl * m), sh2((size_t)d.helper_share_len * m), hs2(m);
      std::vector<uint32_t> cl2(m);
      std::vector<uint64_t> tm2(m);
      for (uint32_t k = 0; k < m; k++) {
        const size_t i = idx[k];
        memcpy(&enc2[nenc * k], enc + nenc * i, nenc);
        memcpy(&ct2[(size_t)ct_stride * k], ct + (size_t)ct_stride * i, ct_stride);
        memcpy(&ids2[16 * (size_t)k], report_ids + 16 * i, 16);
        if (pl) memcpy(&pub2[pl * k], public_shares + pl * i, pl);
        cl2[k] = ct_len[i];
        tm2[k] = times[i];
      }
      rc = janus_hpke_open_input_shares(fallback_opener, m, task_id, enc2.data(), ct2.data(),
                                        cl2.data(), ct_stride, ids2.data(), tm2.data(),
                                        pl ? pub2.data() : nullptr, d.public_share_len,
                                        d.helper_share_len, require_taskprov, sh2.data(),
                                        hs2.data());
      if (rc) return rc == JANUS_HPKE_EDEVICE ? PRIO3_EDEVICE : PRIO3_EINVAL;
      for (uint32_t k = 0; k < m; k++) {
        const size_t i = idx[k];
        memcpy(&shares[(size_t)d.helper_share_len * i], &sh2[(size_t)d.helper_share_len * k],
               d.helper_share_len);
        hs[i] = hs2[k];
      }
    }
  }
  std::vector<uint8_t> late(n);
  for (uint32_t i = 0; i < n; i++) {
    late[i] = hs[i] == 0 && times[i] > report_deadline;
    acc[i] = (!accept_mask || accept_mask[i]) && hs[i] == 0 && !late[i];
  }
  rc = prio3_helper_prepare_aggregate_batch(e, n, report_ids, public_shares, shares.data(),
                                            leader_prep_shares, segment_ids, acc.data(),
                                            n_segments, prep_msgs_out, status_out,
                                            agg_shares_out, counts_out);
  if (rc) return rc;
  for (uint32_t i = 0; i < n; i++)
    if (hs[i])
      status_out[i] = (uint8_t)(0x80u | hs[i]);
    else if (late[i])
      status_out[i] = (uint8_t)PRIO3_STATUS_REPORT_TOO_EARLY;
  return PRIO3_OK;
}

// The helper's whole per-report loop body over one job, from the sealed input shares
// (VdafOps::handle_aggregate_init_generic, /root/reference/aggregator/src/aggregator.rs:1794-2096:
// HPKE open :1847-1890, PlaintextInputShare decode and extension checks :1893-1983,
// helper_initialized + evaluate :2020-2042, then the writer's merge).  One job of the executor: the
// group's launch opens every report's input share into HBM, prepares the reports from there and
// accumulates them per segment; only statuses, prepare messages, aggregate shares and counts come
// back.  A group too wide for its segments takes the same steps as two host calls.
// With the rest of the status contract of aggregator.rs (the _ex form): the task-then-global
// keypair retry (:1864-1878) as a second open pass inside the group launch, and the report deadline
// (:2004-2015) applied where the open's rejections are merged, ahead of the accumulate.
// max_pub: the longest public share the entry point admits (the plain form keeps its 32).
static int helper_aggregate_init(
    prio3_engine* e, janus_hpke_opener* opener, janus_hpke_opener* fallback_opener,
    uint64_t report_deadline, uint32_t max_pub, uint32_t n, const uint8_t task_id[32],
    int require_taskprov, const uint8_t* report_ids, const uint64_t* times,
    const uint8_t* public_shares, const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len,
    uint32_t ct_stride, const uint8_t* leader_prep_shares, const uint32_t* segment_ids,
    const uint8_t* accept_mask, uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out,
    uint8_t* agg_shares_out, uint64_t* counts_out, int notify_fd = -1,
    prio3_ticket** tk = nullptr) {
  TraceSpan span_("handle_aggregate_init_generic threadpool task");
  if (!e || !opener || !task_id || n_segments == 0 || !agg_shares_out || !counts_out ||
      ct_stride == 0 || ct_stride % 16 != 0 ||
      (n && (!report_ids || !times || !enc || !ct || !ct_len || !leader_prep_shares ||
             !status_out)))
    return PRIO3_EINVAL;
  // one enc[n][Nenc] layout serves both opens
  if (fallback_opener && hpke_opener_kem(fallback_opener) != hpke_opener_kem(opener))
    return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  const DevParams& d = e->dp;
  // the open kernel's AAD takes public shares of 0, 32 or 64 bytes (every instance there is)
  if ((d.public_share_len != 0 && d.public_share_len != 32 && d.public_share_len != 64) ||
      d.public_share_len > max_pub)
    return PRIO3_EUNSUPPORTED;
  if (n && d.jr_len && (!public_shares || !prep_msgs_out)) return PRIO3_EINVAL;
  const size_t agg_len = (size_t)d.out_len * d.es;
  if (n == 0) {
    memset(agg_shares_out, 0, agg_len * n_segments);
    memset(counts_out, 0, 8 * (size_t)n_segments);
    return ticket_sync(PRIO3_OK, notify_fd, tk);
  }
  e = place(e, n);
  IoLayout L1;
  engine_io_layout(e, 1, &L1);
  if (n_segments > L1.max_seg)
    return ticket_sync(
        aggregate_init_two_calls(e, opener, fallback_opener, report_deadline, n, task_id,
                                 require_taskprov, report_ids, times, public_shares, enc, ct,
                                 ct_len, ct_stride, leader_prep_shares, segment_ids, accept_mask,
                                 n_segments, prep_msgs_out, status_out, agg_shares_out,
                                 counts_out),
        notify_fd, tk);
  // sealed input shares: no helper shares, the group opens them on the device
  ExecJob job = helper_job(e, n, report_ids, public_shares, nullptr, leader_prep_shares,
                           prep_msgs_out, status_out, segment_ids, accept_mask, n_segments,
                           agg_shares_out, counts_out);
  job.opener = opener;
  job.task_id = task_id;
  job.times = times;
  job.enc = enc;
  job.ct = ct;
  job.ct_len = ct_len;
  job.ct_stride = ct_stride;
  job.require_taskprov = require_taskprov ? 1 : 0;
  job.fallback = fallback_opener;
  job.deadline = report_deadline;
  return helper_exec(&job, notify_fd, tk);
}

// the plain form: no fallback keypair, no report deadline, public shares of 0 or 32 bytes
int prio3_helper_aggregate_init_batch(
    prio3_engine* e, janus_hpke_opener* opener, uint32_t n, const uint8_t task_id[32],
    int require_taskprov, const uint8_t* report_ids, const uint64_t* times,
    const uint8_t* public_shares, const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len,
    uint32_t ct_stride, const uint8_t* leader_prep_shares, const uint32_t* segment_ids,
    const uint8_t* accept_mask, uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out,
    uint8_t* agg_shares_out, uint64_t* counts_out) {
  return helper_aggregate_init(e, opener, nullptr, UINT64_MAX, 32, n, task_id, require_taskprov,
                               report_ids, times, public_shares, enc, ct, ct_len, ct_stride,
                               leader_prep_shares, segment_ids, accept_mask, n_segments,
                               prep_msgs_out, status_out, agg_shares_out, counts_out);
}

int prio3_helper_aggregate_init_batch_ex(
    prio3_engine* e, janus_hpke_opener* opener, janus_hpke_opener* fallback_opener,
    uint64_t report_deadline, uint32_t n, const uint8_t task_id[32], int require_taskprov,
    const uint8_t* report_ids, const uint64_t* times, const uint8_t* public_shares,
    const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len, uint32_t ct_stride,
    const uint8_t* leader_prep_shares, const uint32_t* segment_ids, const uint8_t* accept_mask,
    uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out,
    uint64_t* counts_out) {
  return helper_aggregate_init(e, opener, fallback_opener, report_deadline, 64, n, task_id,
                               require_taskprov, report_ids, times, public_shares, enc, ct,
                               ct_len, ct_stride, leader_prep_shares, segment_ids, accept_mask,
                               n_segments, prep_msgs_out, status_out, agg_shares_out, counts_out);
}

int prio3_helper_aggregate_init_batch_ex_submit(
    prio3_engine* e, janus_hpke_opener* opener, janus_hpke_opener* fallback_opener,
    uint64_t report_deadline, uint32_t n, const uint8_t task_id[32], int require_taskprov,
    const uint8_t* report_ids, const uint64_t* times, const uint8_t* public_shares,
    const uint8_t* enc, const uint8_t* ct, const uint32_t* ct_len, uint32_t ct_stride,
    const uint8_t* leader_prep_shares, const uint32_t* segment_ids, const uint8_t* accept_mask,
    uint32_t n_segments, uint8_t* prep_msgs_out, uint8_t* status_out, uint8_t* agg_shares_out,
    uint64_t* counts_out, int notify_fd, prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return helper_aggregate_init(e, opener, fallback_opener, report_deadline, 64, n, task_id,
                               require_taskprov, report_ids, times, public_shares, enc, ct,
                               ct_len, ct_stride, leader_prep_shares, segment_ids, accept_mask,
                               n_segments, prep_msgs_out, status_out, agg_shares_out, counts_out,
                               notify_fd, ticket_out);
}

// The three calls prio3_helper_aggregate_job stands for, as a caller would make them: what a job
// outside the in-group limits (and an empty one) runs, and what every other job's result equals.
static int helper_job_three_calls(prio3_engine* e, const prio3_helper_job_in& in,
                                  const prio3_helper_job_out& out) {
  const uint32_t n = in.n, S = in.max_segments;
  std::vector<uint8_t> acc(n ? n : 1);
  int rc = prio3_job_index(e, n, in.report_ids, in.times, in.time_precision, in.closed_intervals,
                           in.k, S, out.segment_ids, out.segment_starts, acc.data(), out.reject,
                           out.duplicate, out.info);
  if (rc) return rc;
  if (in.accept_mask)
    for (uint32_t i = 0; i < n; i++) acc[i] = acc[i] && in.accept_mask[i];
  rc = prio3_helper_aggregate_init_batch_ex(
      e, in.opener, in.fallback_opener, in.report_deadline, n, in.task_id, in.require_taskprov,
      in.report_ids, in.times, in.public_shares, in.enc, in.ct, in.ct_len, in.ct_stride,
      in.leader_prep_shares, out.segment_ids, acc.data(), S, out.prep_msgs, out.status,
      out.agg_shares, out.counts);
  if (rc) return rc;
  if (!out.checksums && !out.intervals) return PRIO3_OK;
  return prio3_batch_metadata(e, n, in.report_ids, in.times, out.status, acc.data(),
                              out.segment_ids, S, out.checksums, out.intervals);
}

static int helper_aggregate_job(prio3_engine* e, const prio3_helper_job_in* in,
                                const prio3_helper_job_out* out, int notify_fd,
                                prio3_ticket** tk) {
  TraceSpan span_("handle_aggregate_init_generic threadpool task");
  if (!e || !in || !out || !out->info) return PRIO3_EINVAL;
  const uint32_t n = in->n, S = in->max_segments;
  // the argument rules of the three calls, checked before any of them runs
  if (n > (1u << 30) || S == 0 || S > 4096 || in->k > 1024 || (in->k && !in->closed_intervals) ||
      !in->opener || !in->task_id || !out->agg_shares || !out->counts || in->ct_stride == 0 ||
      in->ct_stride % 16 != 0 ||
      (n && (!in->report_ids || !in->times || !in->enc || !in->ct || !in->ct_len ||
             !in->leader_prep_shares || !out->status || !out->segment_ids)))
    return PRIO3_EINVAL;
  if (in->fallback_opener && hpke_opener_kem(in->fallback_opener) != hpke_opener_kem(in->opener))
    return PRIO3_EINVAL;
  if (fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  const DevParams& d = e->dp;
  if (d.public_share_len != 0 && d.public_share_len != 32 && d.public_share_len != 64)
    return PRIO3_EUNSUPPORTED;
  if (n && d.jr_len && (!in->public_shares || !out->prep_msgs)) return PRIO3_EINVAL;
  IoLayout L1;
  engine_io_layout(e, 1, &L1);
  if (n == 0 || n > JIX_GROUP_MAX_N || S > JIX_GROUP_MAX_SEG || S > L1.max_seg)
    return ticket_sync(helper_job_three_calls(e, *in, *out), notify_fd, tk);
  e = place(e, n);
  ExecJob job = helper_job(e, n, in->report_ids, in->public_shares, nullptr,
                           in->leader_prep_shares, out->prep_msgs, out->status, nullptr,
                           in->accept_mask, S, out->agg_shares, out->counts);
  job.opener = in->opener;
  job.task_id = in->task_id;
  job.times = in->times;
  job.enc = in->enc;
  job.ct = in->ct;
  job.ct_len = in->ct_len;
  job.ct_stride = in->ct_stride;
  job.require_taskprov = in->require_taskprov ? 1 : 0;
  job.fallback = in->fallback_opener;
  job.deadline = in->report_deadline;
  job.jix = true;
  job.precision = in->time_precision;
  job.closed = in->closed_intervals;
  job.nclosed = in->k;
  job.jseg_out = out->segment_ids;
  job.jstarts_out = out->segment_starts;
  job.jrej_out = out->reject;
  job.jdup_out = out->duplicate;
  job.jinfo_out = out->info;
  job.ck_out = out->checksums;
  job.iv_out = out->intervals;
  return helper_exec(&job, notify_fd, tk);
}

int prio3_helper_aggregate_job(prio3_engine* e, const prio3_helper_job_in* in,
                               const prio3_helper_job_out* out) {
  return helper_aggregate_job(e, in, out, -1, nullptr);
}

int prio3_helper_aggregate_job_submit(prio3_engine* e, const prio3_helper_job_in* in,
                                      const prio3_helper_job_out* out, int notify_fd,
                                      prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return helper_aggregate_job(e, in, out, notify_fd, ticket_out);
}

int prio3_accumulate(prio3_batch* b, const uint32_t* segment_ids, const uint8_t* accept_mask,
                     uint32_t n_segments, uint8_t* agg_shares_out, uint64_t* counts_out) {
  TraceSpan span_("batch aggregation");
  if (!b || !agg_shares_out || !counts_out || n_segments == 0) return PRIO3_EINVAL;
  prio3_engine* e = b->e;
  const size_t agg_len = (size_t)e->dp.out_len * e->dp.es, S = n_segments;
  if (!b->run || b->n == 0) {
    memset(agg_shares_out, 0, agg_len * S);
    memset(counts_out, 0, 8 * S);
    return PRIO3_OK;
  }
  Run* R = b->run;
  const uint32_t n = b->n;
  if (n <= (1u << 14) && e->coalesce) {  // a job-sized batch: coalesced with concurrent ones
    AccJob job;
    job.device = e->device;
    job.run = R;
    job.c0 = b->c0;
    job.n = n;
    job.seg = segment_ids;
    job.accept = accept_mask;
    job.nseg = n_segments;
    job.agg_out = agg_shares_out;
    job.counts_out = counts_out;
    if (engine_acc_out_bytes(&job) <= ((size_t)16 << 20)) return exec_accumulate(&job);
  }
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(e->device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_seg = 0, o_acc = up(4 * (size_t)n), o_agg = o_acc + up(n),
               o_cnt = o_agg + up(agg_len * S), total = o_cnt + up(8 * S);
  int rc = PRIO3_OK;
  Slab* sl = ws_acquire(e->device, total, st, &rc);
  if (!sl) return rc;
  uint8_t* base = sl->base;
  if ((segment_ids && hipMemcpyAsync(base + o_seg, segment_ids, 4 * (size_t)n,
                                     hipMemcpyHostToDevice, st) != hipSuccess) ||
      (accept_mask &&
       hipMemcpyAsync(base + o_acc, accept_mask, n, hipMemcpyHostToDevice, st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (rc == PRIO3_OK)
    rc = run_accumulate(e, R, b->c0, n, R->status + b->c0,
                        segment_ids ? (const uint32_t*)(base + o_seg) : nullptr,
                        accept_mask ? base + o_acc : nullptr, n_segments, base + o_agg,
                        (uint64_t*)(base + o_cnt), st);
  if (rc == PRIO3_OK &&
      (hipMemcpyAsync(agg_shares_out, base + o_agg, agg_len * S, hipMemcpyDeviceToHost, st) !=
           hipSuccess ||
       hipMemcpyAsync(counts_out, base + o_cnt, 8 * S, hipMemcpyDeviceToHost, st) !=
           hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (e->timing) collect_times(e);
  ws_release(sl, st);
  return rc;
}

int prio3_debug_output_shares(prio3_batch* b, uint8_t* out) {
  if (!b || !out) return PRIO3_EINVAL;
  if (!b->run) return PRIO3_OK;
  DeviceGuard dg_(b->e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(b->e->device);
  if (!ps.s) return PRIO3_EDEVICE;
  return run_output_shares(b->run, b->c0, b->n, out, ps.s);
}

void prio3_batch_free(prio3_batch* b) {
  if (!b) return;
  if (b->run) run_release(b->run, nullptr, false);
  delete b;
}

int prio3_engine_timing(prio3_engine* e, char* names, size_t cap_names, double* ms,
                        uint64_t* launches, int cap) {
  if (!e) return PRIO3_EINVAL;
  // a multi-GPU engine: its members' times, summed per kernel name
  std::vector<KTime> sum;
  for (size_t i = 0; i < member_count(e); i++) {
    prio3_engine* m = member_at(e, i);
    DeviceGuard dg_(m->device);
    collect_times(m);
    std::lock_guard<std::mutex> lk(m->tmu);
    for (auto& t : m->times) {
      size_t j = 0;
      while (j < sum.size() && sum[j].name != t.name) j++;
      if (j == sum.size()) sum.push_back(KTime{t.name, 0, 0});
      sum[j].ms += t.ms;
      sum[j].launches += t.launches;
    }
  }
  std::string all;
  int k = 0;
  for (auto& t : sum) {
    if (k < cap) {
      if (ms) ms[k] = t.ms;
      if (launches) launches[k] = t.launches;
    }
    if (!all.empty()) all += ",";
    all += t.name;
    k++;
  }
  if (names && cap_names) {
    strncpy(names, all.c_str(), cap_names - 1);
    names[cap_names - 1] = 0;
  }
  return k;
}

void prio3_engine_timing_reset(prio3_engine* e) {
  if (!e) return;
  for (size_t i = 1; i < e->members.size(); i++) prio3_engine_timing_reset(e->members[i]);
  collect_times(e);
  std::lock_guard<std::mutex> lk(e->tmu);
  for (auto& t : e->times) {
    t.ms = 0;
    t.launches = 0;
  }
}

// ---- leader side ----
// The leader's prepare_next over columns [c0, c0 + n) of a run, on st: d_msgs / d_status are
// those columns' prepare messages and statuses (FPVec and multiproof runs are whole: c0 = 0).
static int leader_next_launch(prio3_engine* e, Run* R, uint32_t c0, uint32_t n,
                              const uint8_t* d_msgs, uint8_t* d_status, hipStream_t st) {
  DevParams dp = R->dp;
  dp.n = n;
  R->last = st;
  Scratch sc = R->sc;
  if (R->corr_all) sc.corrected = R->corr_all;  // FPVec: seeds of every sub-batch
  if (c0) {
    sc.corrected += c0;
    sc.meas = (uint8_t*)sc.meas + (size_t)dp.es * c0;
    sc.out = (uint8_t*)sc.out + (size_t)dp.es * c0;
  }
  int rc = PRIO3_OK;
  if (dp.kind == PRIO3_SUMVEC_F64_MP)
    TIMED(e, st, "k_leader_next", rc = launch_mp64_leader_next(n, d_msgs, sc, d_status, st));
  else
    TIMED(e, st, "k_leader_next", rc = launch_leader_next(dp, d_msgs, sc, d_status, st));
  return rc;
}

int prio3_device_leader_prepare_init(prio3_engine* e, uint32_t n, const uint8_t* d_nonces,
                                     const uint8_t* d_public_shares,
                                     const uint8_t* d_leader_input_shares, uint8_t* d_prep_shares,
                                     uint8_t* d_status, void* stream) {
  TraceSpan span_("leader VDAF preparation");
  if (e && fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  if (!e) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  if (!d_nonces || !d_leader_input_shares || !d_prep_shares || !d_status ||
      (e->dp.jr_len && !d_public_shares))
    return PRIO3_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = (hipStream_t)stream;
  int rc = PRIO3_OK;
  const bool lfuse = plan_leader(e).fuse_acc;
  Run* R = device_run(e, n, RUN_SCRATCH | (lfuse ? (unsigned)RUN_FUSED : 0u), lfuse ? 1u : 0u, st,
                      &rc);
  if (!R) return rc;
  R->lfused = lfuse;
  return leader_init_run(e, R, d_nonces, d_public_shares, d_leader_input_shares, d_prep_shares,
                         d_status, st);
}

int prio3_device_leader_prepare_next(prio3_engine* e, uint32_t n, const uint8_t* d_prep_msgs,
                                     uint8_t* d_status, void* stream) {
  TraceSpan span_("leader VDAF preparation");
  if (e && fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  if (!e) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  if (!d_status || (e->dp.jr_len && !d_prep_msgs)) return PRIO3_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  Run* R = e->cur;
  if (!R || n > R->n) return PRIO3_EINVAL;
  return leader_next_launch(e, R, 0, n, d_prep_msgs, d_status, (hipStream_t)stream);
}

static int leader_prepare_init_sync(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                    const uint8_t* public_shares,
                                    const uint8_t* leader_input_shares, uint8_t* prep_shares_out,
                                    uint8_t* status_out, prio3_batch** batch_out);

static int leader_prepare_init(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                               const uint8_t* public_shares, const uint8_t* leader_input_shares,
                               uint8_t* prep_shares_out, uint8_t* status_out,
                               prio3_batch** batch_out, int notify_fd, prio3_ticket** tk) {
  TraceSpan span_("leader VDAF preparation");
  if (e && fpvec_refused(e)) return PRIO3_EUNSUPPORTED;
  if (!e || (n && (!nonces || !leader_input_shares || !prep_shares_out || !status_out)))
    return PRIO3_EINVAL;
  const DevParams& d = e->dp;
  if (n && d.jr_len && !public_shares) return PRIO3_EINVAL;
  if (n == 0) {
    if (batch_out) *batch_out = new prio3_batch{e, nullptr, 0, 0};
    return ticket_sync(PRIO3_OK, notify_fd, tk);
  }
  e = place(e, n);
  if (leader_coalescable(e)) {  // concurrent jobs (of any task of the instance): one launch
    LeaderJob job{};
    job.e = e;
    job.n = n;
    job.nonces = nonces;
    job.pub = d.jr_len ? public_shares : nullptr;
    job.linput = leader_input_shares;
    job.prep_out = prep_shares_out;
    job.status_out = status_out;
    if (tk) {  // the wait makes the batch handle
      ExecTicket* xt = nullptr;
      return ticket_queued(exec_leader_begin(&job, notify_fd, &xt), prio3_ticket::LEADER_INIT, xt,
                           tk, e, n, batch_out);
    }
    const int rc = exec_leader(&job);
    if (rc) return rc;
    if (batch_out)
      *batch_out = new prio3_batch{e, job.run, job.c0, n};
    else
      run_release(job.run, nullptr, false);
    return PRIO3_OK;
  }
  return ticket_sync(leader_prepare_init_sync(e, n, nonces, public_shares, leader_input_shares,
                                              prep_shares_out, status_out, batch_out),
                     notify_fd, tk);
}

// an engine whose leader jobs do not coalesce (FPVec, the multiproof instance, coalesce off): one
// run per call (e: the member the job was placed on)
static int leader_prepare_init_sync(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                    const uint8_t* public_shares,
                                    const uint8_t* leader_input_shares, uint8_t* prep_shares_out,
                                    uint8_t* status_out, prio3_batch** batch_out) {
  const DevParams& d = e->dp;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(e->device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  int rc = PRIO3_OK;
  Run* R = run_create(e, n, RUN_SCRATCH | RUN_IO | RUN_LINPUT, 0, st, &rc);
  if (!R) return rc;
  if (hipMemcpyAsync(R->nonces, nonces, 16 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
      (d.jr_len && hipMemcpyAsync(R->pub, public_shares, (size_t)d.public_share_len * n,
                                  hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(R->linput, leader_input_shares, (size_t)d.leader_share_len * n,
                     hipMemcpyHostToDevice, st) != hipSuccess)
    rc = PRIO3_EDEVICE;
  if (rc == PRIO3_OK)
    rc = leader_init_run(e, R, R->nonces, d.jr_len ? R->pub : nullptr, R->linput, R->leader,
                         R->status, st);
  if (rc == PRIO3_OK &&
      (hipMemcpyAsync(status_out, R->status, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(prep_shares_out, R->leader, (size_t)d.prep_share_len * n,
                      hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (e->timing) collect_times(e);
  if (rc != PRIO3_OK) {
    run_release(R, st, true);
    return rc;
  }
  if (batch_out)
    *batch_out = new prio3_batch{e, R, 0, n};
  else
    run_release(R, st, true);
  return PRIO3_OK;
}

int prio3_leader_prepare_init_batch(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                    const uint8_t* public_shares,
                                    const uint8_t* leader_input_shares, uint8_t* prep_shares_out,
                                    uint8_t* status_out, prio3_batch** batch_out) {
  return leader_prepare_init(e, n, nonces, public_shares, leader_input_shares, prep_shares_out,
                             status_out, batch_out, -1, nullptr);
}

int prio3_leader_prepare_init_batch_submit(prio3_engine* e, uint32_t n, const uint8_t* nonces,
                                           const uint8_t* public_shares,
                                           const uint8_t* leader_input_shares,
                                           uint8_t* prep_shares_out, uint8_t* status_out,
                                           prio3_batch** batch_out, int notify_fd,
                                           prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return leader_prepare_init(e, n, nonces, public_shares, leader_input_shares, prep_shares_out,
                             status_out, batch_out, notify_fd, ticket_out);
}

int prio3_leader_prepare_next_batch(prio3_batch* b, const uint8_t* prep_msgs,
                                    uint8_t* status_inout) {
  TraceSpan span_("leader VDAF preparation");
  if (!b || !status_inout) return PRIO3_EINVAL;
  prio3_engine* e = b->e;
  const uint32_t n = b->n;
  const DevParams& d = e->dp;
  if (n == 0 || !b->run) return PRIO3_OK;
  if (d.jr_len && !prep_msgs) return PRIO3_EINVAL;
  Run* R = b->run;
  if (!R->msgs || !R->linput) return PRIO3_EINVAL;  // a leader batch
  const uint32_t c0 = b->c0;
  if (leader_coalescable(e) && n <= LNEXT_MAX_REPS) {
    // concurrent jobs' prepare_next (of any runs of this GPU) in one launch
    LNextJob job;
    job.device = e->device;
    job.run = R;
    job.c0 = c0;
    job.n = n;
    job.msgs = d.jr_len ? prep_msgs : nullptr;
    job.status = status_inout;
    return exec_leader_next(&job);
  }
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  PooledStream ps(e->device);
  hipStream_t st = ps.s;
  if (!st) return PRIO3_EDEVICE;
  if (d.jr_len)
    HIPCHK(hipMemcpyAsync(R->msgs + 16 * (size_t)c0, prep_msgs, (size_t)e->sz.prep_msg_len * n,
                          hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(R->status + c0, status_inout, n, hipMemcpyHostToDevice, st));
  const int rc2 = leader_next_launch(e, R, c0, n, R->msgs + 16 * (size_t)c0, R->status + c0, st);
  if (rc2) return rc2;
  HIPCHK(hipMemcpyAsync(status_inout, R->status + c0, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (e->timing) collect_times(e);
  return PRIO3_OK;
}

// leader_continued on the helper's messages and the writer's merge of the job's output shares
// (/root/reference/aggregator/src/aggregator/aggregation_job_driver.rs:677-691, then
// aggregation_job_writer.rs:591-695) in one launch of the prepare_next executor: the check of
// each report, then the per-segment sum of the reports it kept, for many jobs at once.
int prio3_leader_prepare_next_aggregate_batch(prio3_batch* b, const uint8_t* prep_msgs,
                                              uint8_t* status_inout, const uint32_t* segment_ids,
                                              const uint8_t* accept_mask, uint32_t n_segments,
                                              uint8_t* agg_shares_out, uint64_t* counts_out) {
  TraceSpan span_("leader VDAF preparation");
  if (!b || !status_inout || n_segments == 0 || !agg_shares_out || !counts_out)
    return PRIO3_EINVAL;
  prio3_engine* e = b->e;
  const uint32_t n = b->n;
  const DevParams& d = e->dp;
  Run* R = b->run;
  const bool one = R && n && leader_coalescable(e) && n <= LNEXT_MAX_REPS && R->msgs &&
                   R->linput;
  LNextJob job;
  job.device = e->device;
  job.run = R;
  job.nseg = n_segments;
  if (one && engine_lnext_out_bytes(&job) <= LNEXT_MAX_OUT) {
    if (d.jr_len && !prep_msgs) return PRIO3_EINVAL;
    job.c0 = b->c0;
    job.n = n;
    job.msgs = d.jr_len ? prep_msgs : nullptr;
    job.status = status_inout;
    job.seg = segment_ids;
    job.accept = accept_mask;
    job.agg_out = agg_shares_out;
    job.counts_out = counts_out;
    return exec_leader_next(&job);
  }
  int rc = prio3_leader_prepare_next_batch(b, prep_msgs, status_inout);
  if (rc == PRIO3_OK)
    rc = prio3_accumulate(b, segment_ids, accept_mask, n_segments, agg_shares_out, counts_out);
  return rc;
}

// The composition prio3_leader_finish_job stands for, as a caller would make it: what a job
// outside the in-group path runs, and what every other job's result equals.
static int leader_job_composition(prio3_batch* b, const prio3_leader_job_in& in,
                                  const prio3_leader_job_out& out) {
  prio3_engine* e = b->e;
  const uint32_t n = b->n, S = in.max_segments;
  std::vector<uint8_t> acc(n ? n : 1);
  for (uint32_t i = 0; i < n; i++) {  // the helper's prepare_error laid over the init status
    const uint8_t ls = in.leader_status[i], pe = in.prepare_error ? in.prepare_error[i] : 0xFF;
    out.status[i] = ls ? ls : pe != 0xFF ? (uint8_t)PRIO3_STATUS_PEER_MISMATCH : 0;
  }
  std::vector<uint8_t> rej(n ? n : 1);
  int rc = prio3_job_index(e, n, in.report_ids, in.times, in.time_precision, in.closed_intervals,
                           in.k, S, out.segment_ids, out.segment_starts, acc.data(), rej.data(),
                           out.duplicate, out.info);
  if (rc) return rc;
  if (in.accept_mask)
    for (uint32_t i = 0; i < n; i++) acc[i] = acc[i] && in.accept_mask[i];
  uint8_t none = 0;  // an empty job may come without a status array
  rc = prio3_leader_prepare_next_aggregate_batch(b, in.prep_msgs, n ? out.status : &none,
                                                 out.segment_ids, acc.data(), S, out.agg_shares,
                                                 out.counts);
  if (rc) return rc;
  if (out.checksums || out.intervals) {
    rc = prio3_batch_metadata(e, n, in.report_ids, in.times, out.status, acc.data(),
                              out.segment_ids, S, out.checksums, out.intervals);
    if (rc) return rc;
  }
  if (out.reject && n) memcpy(out.reject, rej.data(), n);
  if (out.outcome)
    for (uint32_t i = 0; i < n; i++) {
      uint8_t o = in.prepare_error ? in.prepare_error[i] : 0xFF;
      if (o == 0xFF && out.status[i] != PRIO3_STATUS_FINISHED) o = 5;  // VdafPrepError
      if (in.leader_status[i] != PRIO3_STATUS_FINISHED) o = 5;
      if (o == 0xFF && rej[i]) o = 0;  // BatchCollected, unless the report had failed already
      out.outcome[i] = o;
    }
  return PRIO3_OK;
}

// process_response_from_helper's per-report work and the writer's bookkeeping for one leader job
// (aggregation_job_driver.rs:629-770, aggregation_job_writer.rs:540-695) in one trip through the
// prepare_next executor: index, overlay + check, accumulate, metadata.
static int leader_finish_job(prio3_batch* b, const prio3_leader_job_in* in,
                             const prio3_leader_job_out* out, int notify_fd, prio3_ticket** tk) {
  TraceSpan span_("leader VDAF preparation");
  if (!b || !in || !out || !out->info) return PRIO3_EINVAL;
  prio3_engine* e = b->e;
  const uint32_t n = b->n, S = in->max_segments;
  const DevParams& d = e->dp;
  // the argument rules of the three calls, checked before any of them runs
  if (n > (1u << 30) || S == 0 || S > 4096 || in->k > 1024 || (in->k && !in->closed_intervals) ||
      !out->agg_shares || !out->counts ||
      (n && (!in->report_ids || !in->times || !in->leader_status || !out->status ||
             !out->segment_ids)))
    return PRIO3_EINVAL;
  Run* R = b->run;
  if (n && R && d.jr_len && !in->prep_msgs) return PRIO3_EINVAL;
  LNextJob job;
  job.device = e->device;
  job.run = R;
  job.nseg = S;
  const bool group = R && n && n <= JIX_GROUP_MAX_N && S <= JIX_GROUP_MAX_SEG &&
                     leader_coalescable(e) && R->msgs && R->linput &&
                     engine_lnext_out_bytes(&job) <= LNEXT_MAX_OUT;
  if (!group) return ticket_sync(leader_job_composition(b, *in, *out), notify_fd, tk);
  memcpy(out->status, in->leader_status, n);  // in/out: the overlay is the kernel's
  job.c0 = b->c0;
  job.n = n;
  job.msgs = d.jr_len ? in->prep_msgs : nullptr;
  job.status = out->status;
  job.accept = in->accept_mask;
  job.agg_out = out->agg_shares;
  job.counts_out = out->counts;
  job.jix = true;
  job.e = e;
  job.ids = in->report_ids;
  job.times = in->times;
  job.perr = in->prepare_error;
  job.precision = in->time_precision;
  job.closed = in->closed_intervals;
  job.nclosed = in->k;
  job.jseg_out = out->segment_ids;
  job.jstarts_out = out->segment_starts;
  job.jrej_out = out->reject;
  job.jdup_out = out->duplicate;
  job.jinfo_out = out->info;
  job.outcome_out = out->outcome;
  job.ck_out = out->checksums;
  job.iv_out = out->intervals;
  return leader_next_exec(&job, notify_fd, tk);
}

int prio3_leader_finish_job(prio3_batch* b, const prio3_leader_job_in* in,
                            const prio3_leader_job_out* out) {
  return leader_finish_job(b, in, out, -1, nullptr);
}

int prio3_leader_finish_job_submit(prio3_batch* b, const prio3_leader_job_in* in,
                                   const prio3_leader_job_out* out, int notify_fd,
                                   prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return leader_finish_job(b, in, out, notify_fd, ticket_out);
}

// ---- the leader's upload as an executor job ----
static int upload_batch_of(prio3_engine* e, const prio3_upload_job_in* in,
                           const prio3_upload_job_out* out) {
  return prio3_leader_upload_batch(
      e, in->task_opener, in->task_config_id, in->global_opener, in->global_config_id, in->n,
      in->task_id, in->now, in->report_deadline, in->task_expiration, in->report_expiry_age,
      in->reports, in->report_stride, in->report_len, out->report_ids, out->times,
      out->public_shares, out->leader_input_shares, out->extensions, out->ext_len, in->ext_stride,
      out->helper_config_ids, out->helper_enc, in->helper_enc_len, out->helper_ct,
      out->helper_ct_len, in->helper_ct_stride, out->leader_config_ids, out->status);
}

static int leader_upload_job(prio3_engine* e, const prio3_upload_job_in* in,
                             const prio3_upload_job_out* out, int notify_fd, prio3_ticket** tk) {
  TraceSpan span_("handle_upload_generic");
  if (!e || !in || !out) return PRIO3_EINVAL;
  // the argument checks of prio3_leader_upload_batch, in its order
  if (e->dp.kind == PRIO3_FPVEC_BOUNDED_L2) return PRIO3_EUNSUPPORTED;
  if ((!in->task_opener && !in->global_opener) || in->report_stride % 4 != 0 ||
      in->ext_stride % 4 != 0 || in->report_stride >= (1u << 31) || in->helper_enc_len > 0xFFFF)
    return PRIO3_EINVAL;
  for (auto* o : {in->task_opener, in->global_opener})
    if (o && hpke_opener_device(o) != e->device) return PRIO3_EINVAL;
  const uint32_t n = in->n;
  if (n == 0) return ticket_sync(PRIO3_OK, notify_fd, tk);
  if (!in->reports || !in->report_len || !out->report_ids || !out->times ||
      !out->leader_input_shares || !out->ext_len || !out->helper_config_ids ||
      !out->helper_ct_len || !out->leader_config_ids || !out->status ||
      (e->sz.public_share_len && !out->public_shares) || (in->ext_stride && !out->extensions) ||
      (in->helper_enc_len && !out->helper_enc) || (in->helper_ct_stride && !out->helper_ct))
    return PRIO3_EINVAL;
  e = place(e, n, true);
  UploadJob job;
  job.e = e;
  job.op[0] = in->task_opener;
  job.op[1] = in->global_opener;
  job.cfg[0] = in->task_config_id;
  job.cfg[1] = in->global_config_id;
  for (int p = 0; p < 2; p++) job.wide[p] = job.op[p] && upload_job_wide(e, job.op[p]);
  job.n = n;
  memcpy(job.task_id, in->task_id, 32);
  job.now = in->now;
  job.deadline = in->report_deadline;
  job.task_exp = in->task_expiration;
  job.expiry_age = in->report_expiry_age;
  job.reports = in->reports;
  job.report_len = in->report_len;
  job.stride = in->report_stride;
  job.ext_stride = in->ext_stride;
  job.henc_len = in->helper_enc_len;
  job.hct_stride = in->helper_ct_stride;
  job.ids = out->report_ids;
  job.times = out->times;
  job.pub = out->public_shares;
  job.shares = out->leader_input_shares;
  job.ext = out->extensions;
  job.ext_len = out->ext_len;
  job.hcfg = out->helper_config_ids;
  job.henc = out->helper_enc;
  job.hct = out->helper_ct;
  job.hct_len = out->helper_ct_len;
  job.lcfg = out->leader_config_ids;
  job.status = out->status;
  // what one group cannot hold, and an engine that does not coalesce: the batch form, here
  if (!e->coalesce || n > PRIO3_UPLOAD_JOB_MAX_REPORTS ||
      upload_report_bytes(&job) * n > UPLOAD_STAGING_BYTES)
    return ticket_sync(upload_batch_of(e, in, out), notify_fd, tk);
  placed(e, n);
  if (tk) {
    ExecTicket* xt = nullptr;
    return ticket_queued(exec_upload_begin(&job, notify_fd, &xt), prio3_ticket::UPLOAD, xt, tk);
  }
  return exec_upload(&job);
}

int prio3_leader_upload_job(prio3_engine* e, const prio3_upload_job_in* in,
                            const prio3_upload_job_out* out) {
  return leader_upload_job(e, in, out, -1, nullptr);
}

int prio3_leader_upload_job_submit(prio3_engine* e, const prio3_upload_job_in* in,
                                   const prio3_upload_job_out* out, int notify_fd,
                                   prio3_ticket** ticket_out) {
  if (!ticket_out) return PRIO3_EINVAL;
  *ticket_out = nullptr;
  return leader_upload_job(e, in, out, notify_fd, ticket_out);
}

int prio3_trace_enabled(void) { return trace_enabled() ? 1 : 0; }

int prio3_selftest_field(int op, uint32_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  if (op < 0 || op > 5) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  const size_t m = (op >= 4 ? 16 : 1) * (size_t)n * 16;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = PRIO3_OK;
  if (hipMalloc(&da, m) != hipSuccess || hipMalloc(&db, m) != hipSuccess ||
      hipMalloc(&dout, (size_t)n * 16) != hipSuccess ||
      hipMemcpy(da, a, m, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(db, b, m, hipMemcpyHostToDevice) != hipSuccess) {
    rc = PRIO3_EDEVICE;
  } else {
    k_selftest_f128<<<(n + 255) / 256, 256>>>(op, n, (const uint4*)da, (const uint4*)db, (uint4*)dout);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(out, dout, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess)
      rc = PRIO3_EDEVICE;
  }
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

int prio3_selftest_field64(int op, uint32_t n, uint32_t k, const uint8_t* a, const uint8_t* b,
                           uint8_t* out) {
  if (op < 0 || op > 8 || !a || !out) return PRIO3_EINVAL;
  if ((op == 4 || op == 7) && k == 0) return PRIO3_EINVAL;
  if (op == 8 && (k == 0 || k > 32)) return PRIO3_EINVAL;
  if (op <= 4 && !b) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  const size_t per = op == 4 ? k : op == 8 ? 2 * (size_t)k : 1, es = op >= 6 ? 16 : 8;
  const size_t ma = per * n * es, mb = op <= 4 ? ma : 0;
  const size_t mo = (size_t)n * (op == 7 ? 16 : op == 8 ? 32 : 8);
  DevParams p{};
  p.ld_out = n;
  p.bits = k;
  p.out_len = 2;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  int rc = PRIO3_OK;
  if (hipMalloc(&da, ma) != hipSuccess || (mb && hipMalloc(&db, mb) != hipSuccess) ||
      hipMalloc(&dout, mo) != hipSuccess ||
      hipMemcpy(da, a, ma, hipMemcpyHostToDevice) != hipSuccess ||
      (mb && hipMemcpy(db, b, mb, hipMemcpyHostToDevice) != hipSuccess)) {
    rc = PRIO3_EDEVICE;
  } else {
    k_selftest_f64<<<(n + 255) / 256, 256>>>(op, n, k, (const uint64_t*)da, (const uint64_t*)db,
                                             (uint64_t*)dout, p);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(out, dout, mo, hipMemcpyDeviceToHost) != hipSuccess)
      rc = PRIO3_EDEVICE;
  }
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

int prio3_selftest_tile(uint32_t n_elems, const uint8_t* values, uint32_t* out) {
  if (n_elems == 0 || n_elems > (uint32_t)FTILE || !values || !out) return PRIO3_EINVAL;
  const size_t m = (size_t)FTILE * 64 * 16, mo = (size_t)n_elems * 8 * sizeof(uint32_t);
  void *din = nullptr, *dout = nullptr;
  int rc = PRIO3_OK;
  if (hipMalloc(&din, m) != hipSuccess || hipMalloc(&dout, mo) != hipSuccess ||
      hipMemcpy(din, values, m, hipMemcpyHostToDevice) != hipSuccess) {
    rc = PRIO3_EDEVICE;
  } else {
    k_selftest_tile<<<1, 64>>>(n_elems, (const uint4*)din, (uint32_t*)dout);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(out, dout, mo, hipMemcpyDeviceToHost) != hipSuccess)
      rc = PRIO3_EDEVICE;
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

}  // extern "C"

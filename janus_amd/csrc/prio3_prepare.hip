// prio3_prepare.hip -- MI355X (gfx950) batched Prio3 prepare: the helper's kernels, the same
// kernels in their leader role, and the host code that plans their launches over a run.
// One work-item = one report; SoA scratch [element][report], so every wave-wide load/store is
// 64 x 16 B contiguous.  [prio Prio3::prepare_init, FlpGeneric::query/decide,
// prepare_shares_to_prepare_message, prepare_next; VDAF-08 7.2.2]
//   XOF      k_xof, k_xofd (two Keccak states: one squeezes the measurement share while the
//            other absorbs it into the joint-rand part), k_xof_a + k_jrpart; a rejection-sampling
//            hit flags the report for k_xof_slow / k_slow_redo* (the byte-level sponge)
//   query    k_query, k_query_ps, k_query_h: wire polynomials at t, decide, prepare message
//   fused    k_prep_h, k_prep_sum, k_prep_gen: XOF and query of the same reports in one launch
//   leader   k_leader_unpack, k_leader_prep, k_leader_slowfix: prepare_init from the explicit share
// launch_prepare and leader_init_run choose among these and the families with files of their own
// (launch_* in prio3_common.h).  Entry points: prio3_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "prio3_host.h"
#include "prio3_query_sum.h"

// threads per block of the kernels with the fused accumulate (k_prep_h, k_xofd): each of their
// waves owns 8 KiB of the block's LDS (xofd_body), 32 KiB per block and 96 KiB per CU
#ifndef XOFD_BLOCK
#define XOFD_BLOCK 256
#endif
#ifndef XOFD_OCC
#define XOFD_OCC 3
#endif
template <class F>
__device__ __forceinline__ void xof_body(const DevParams& p, const InPtrs& in, const Scratch& sc,
                                         const uint32_t r) {
  // r: this lane's report
  if (r >= p.n) return;
  constexpr uint32_t ES = F::ES;
  uint32_t flag = p.force_slow;
  uint32_t nonce[4], km[4], kp[4], kb[4] = {0, 0, 0, 0};
  load16(in.nonces + 16 * (size_t)r, nonce);
  const uint8_t* hs = in.helper + (size_t)r * p.helper_share_len;
  load16(hs, km);
  load16(hs + 16, kp);
  const bool JR = p.jr_len > 0;
  if (JR) load16(hs + 32, kb);

  // 1. query randomness: XOF(vk, dst(5), [PROOFS] || nonce), qr_len elements (<= 10)
  {
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[5]);
    {
      uint32_t vk[4];
      load_vk(p, in, r, vk);
      msg_bytes16(m, 9, vk);
    }
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
    msg_absorb_final(s, m, 42);
    uint32_t q0 = 0, q1 = 0;
    squeeze_block<F>(p, s, 0, p.qr_len, q0, q1, sc.qr, r, flag);
  }

  // 2. measurement share XOF(k_meas, dst(1), [1]) fused with the joint-rand part
  //    XOF(k_blind, dst(7), [1] || nonce || enc(meas)).
  KState ms;
  kzero(ms);
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[1]);
    msg_bytes16(m, 9, km);
    msg_byte(m, 25, 1);
    msg_absorb_final(ms, m, 26);
  }
  const uint32_t M = p.meas_len;
  const uint32_t mbytes = M * ES;
  const uint32_t K = (mbytes + 167) / 168;
  const uint32_t L = 42 + mbytes;
  const uint32_t B = L / 168, rem = L % 168;
  KState js;
  uint32_t pre[11], tail[11];
  uint32_t part[4] = {0, 0, 0, 0};
  if (JR) {
    kzero(js);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[7]);
    msg_bytes16(m, 9, kb);
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
#pragma unroll
    for (int j = 0; j < 11; j++) pre[j] = m.w[j];
  }
#pragma unroll
  for (int j = 0; j < 11; j++) tail[j] = 0;
  uint32_t pend0 = 0, pend1 = 0;
  const uint32_t nb = JR ? B + 1 : K;
  for (uint32_t b = 0; b < nb; b++) {
    const bool hasW = b < K;
    if (hasW) squeeze_block<F>(p, ms, b, M, pend0, pend1, sc.meas, r, flag);
    if (JR && b < B) {  // full block: each message word goes straight into the state
      const uint32_t w0 = hasW ? kword(ms, 0) : 0u;
#pragma unroll
      for (int j = 0; j < 10; j++)
        kxor_word(js, j, b == 0 ? pre[j] : __builtin_amdgcn_alignbit(tail[j + 1], tail[j], 16));
      kxor_word(js, 10, b == 0 ? ((pre[10] & 0xffffu) | (w0 << 16))
                               : __builtin_amdgcn_alignbit(w0, tail[10], 16));
#pragma unroll
      for (int j = 11; j < 42; j++)
        kxor_word(js, j, hasW ? __builtin_amdgcn_alignbit(kword(ms, j - 10), kword(ms, j - 11), 16)
                              : 0u);
      keccak_p12(js);
    } else if (JR) {
      uint32_t x[42];
#pragma unroll
      for (int j = 0; j < 10; j++)
        x[j] = b == 0 ? pre[j] : __builtin_amdgcn_alignbit(tail[j + 1], tail[j], 16);
      uint32_t w0 = hasW ? kword(ms, 0) : 0u;
      x[10] = b == 0 ? ((pre[10] & 0xffffu) | (w0 << 16))
                     : __builtin_amdgcn_alignbit(w0, tail[10], 16);
#pragma unroll
      for (int j = 11; j < 42; j++)
        x[j] = hasW ? __builtin_amdgcn_alignbit(kword(ms, j - 10), kword(ms, j - 11), 16) : 0u;
      {
#pragma unroll
        for (int j = 0; j < 42; j++) {
          const uint32_t lo = 4 * j;
          uint32_t mask = (lo + 4 <= rem) ? 0xffffffffu
                                          : (lo >= rem ? 0u : ((1u << (8 * (rem - lo))) - 1u));
          x[j] &= mask;
          if ((uint32_t)j == (rem >> 2)) x[j] ^= 1u << (8 * (rem & 3));
        }
        x[41] ^= 0x80000000u;
#pragma unroll
        for (int j = 0; j < 42; j++) kxor_word(js, j, x[j]);
        keccak_p12(js);
        part[0] = kword(js, 0);
        part[1] = kword(js, 1);
        part[2] = kword(js, 2);
        part[3] = kword(js, 3);
      }
    }
    if (hasW) {
#pragma unroll
      for (int t = 0; t < 11; t++) tail[t] = kword(ms, 31 + t);
    }
    if (b + 1 < K) keccak_p12(ms);
  }

  // 3. proofs share XOF(k_proofs, dst(2), [PROOFS, 1])
  {
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[2]);
    msg_bytes16(m, 9, kp);
    msg_byte(m, 25, 1);
    msg_byte(m, 26, 1);
    msg_absorb_final(s, m, 27);
    const uint32_t PL = p.proof_len;
    const uint32_t Kp = (PL * ES + 167) / 168;
    uint32_t q0 = 0, q1 = 0;
    for (uint32_t b = 0; b < Kp; b++) {
      squeeze_block<F>(p, s, b, PL, q0, q1, sc.proofs, r, flag);
      if (b + 1 < Kp) keccak_p12(s);
    }
  }

  // 4. corrected joint-rand seed and joint randomness
  if (JR) {
    uint32_t pub0[4];
    load16(in.pub + (size_t)r * p.public_share_len, pub0);
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[6]);
    msg_bytes16(m, 25, pub0);
    msg_bytes16(m, 41, part);
    msg_absorb_final(s, m, 57);
    uint32_t cor[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
    KState t;
    kzero(t);
    Msg m2;
    msg_zero(m2);
    msg_dst(m2, p.dst[3]);
    msg_bytes16(m2, 9, cor);
    msg_byte(m2, 25, 1);
    msg_absorb_final(t, m2, 26);
    uint32_t q0 = 0, q1 = 0;
    squeeze_block<F>(p, t, 0, p.jr_len, q0, q1, sc.jr, r, flag);
    sc.part[r] = make_uint4(part[0], part[1], part[2], part[3]);
    sc.corrected[r] = make_uint4(cor[0], cor[1], cor[2], cor[3]);
  }
  sc.flag[r] = (uint8_t)flag;
}
template <class F>
__global__ __launch_bounds__(256, XOFD_OCC) void k_xof(DevParams p, InPtrs in, Scratch sc) {
  xof_body<F>(p, in, sc, blockIdx.x * blockDim.x + threadIdx.x);
}


// ------------------------------------------------------------------------------------
// k_xofd: k_xof_a + k_jrpart in one pass with two live Keccak states -- each squeezed
// measurement-share block is absorbed into the joint-rand-part sponge while still in
// registers (no 4 KiB re-read), the two permutation streams give each wave 2x the ILP.
// Field128 joint-randomness instances with at least three joint-rand blocks; peeled first and
// last blocks keep the steady-state loop free of the prefix / padding code.
// ------------------------------------------------------------------------------------
// FUSE: the optimistic per-segment aggregate of the fused path (see k_jrpart<true>) is taken
// here, from the squeezed elements while they are in registers; a wave in which any report got
// flagged for the slow path is un-fused at the end (its partials are ignored, its reports go
// through the fix-up list with their corrected shares).
// TR: the measurement share is also truncated into sc.out on the fly (DevParams::trunc_xof).
// PULL (executor groups): the lane's leader prep share is copied from the mapped host staging
// (in.leader_src) into in.leader in 16-byte pieces spread over the share loop -- each load issued
// before the iteration's two permutations and stored after them, so the PCIe latency hides under
// the Keccak work and the transfer runs at the XOF's pace -- plus its segment id and accept byte.
// LIST (k_prep_h): flagged lanes append their report to the run's redo list (Scratch::redo_cnt,
// redo_list) -- under a wave-uniform test of the ballot, one atomic per wave on the counter -- so
// the run's redo launch strides over the list instead of scanning every flag byte.
template <bool FUSE, bool TR = false, bool PULL = false, bool LIST = false>
__device__ __forceinline__ void xofd_body(const DevParams& p, const InPtrs& in, const Scratch& sc,
                                          const uint32_t r) {  // r & 63 == this lane
  typedef Fp128 F;
  const uint32_t lane = threadIdx.x & 63u;
  bool fuse = false, oor = false, haspad = false;
  uint32_t s0 = 0;
  if constexpr (FUSE) {
    const bool valid = r < p.n;
    const uint32_t sg = valid ? (sc.seg ? sc.seg[r] : 0u) : 0xffffffffu;
    // A segment id >= n_segments puts the report in no aggregate.  Such lanes (the executor's
    // pad columns between jobs, excluded reports) are masked out of the wave partials, so they
    // do not keep the wave's other 63 reports from fusing; k_agg_parts knows them (oor_masked).
    const uint64_t inr = __ballot(valid && sg < p.nseg);
    s0 = inr ? (uint32_t)__shfl((int)sg, __ffsll((long long)inr) - 1) : 0xffffffffu;
    oor = valid && sg >= p.nseg;
    fuse = inr != 0 && __all(valid && (sg == s0 || sg >= p.nseg));
    haspad = __any(oor);
    if (lane == 0 && (r - lane) < p.n && !fuse) sc.wseg[r >> 6] = 0xffffffffu;
  }
  if (r >= p.n) return;
  uint32_t flag = p.force_slow;
  uint32_t nonce[4], km[4], kb[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  const uint8_t* hs = in.helper + (size_t)r * p.helper_share_len;
  load16(hs, km);
  load16(hs + 32, kb);
  {  // query randomness
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[5]);
    {
      uint32_t vk[4];
      load_vk(p, in, r, vk);
      msg_bytes16(m, 9, vk);
    }
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
    msg_absorb_final(s, m, 42);
    if (p.qr_len == 1) {  // wave-uniform
      uint32_t w[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
      put_elem<F>(p, sc.qr, 0, r, w, flag);
    } else {  // FPVec: one query point per gadget
      uint32_t q0 = 0, q1 = 0;
      squeeze_block<F>(p, s, 0, p.qr_len, q0, q1, sc.qr, r, flag);
    }
  }
  const uint32_t M = p.meas_len, K = (M * 16 + 167) / 168;
  const uint32_t L = 42 + M * 16, B = L / 168, rem = L % 168;  // B >= 2 (checked on the host)
  KState ms, js;
  kzero(ms);
  kzero(js);
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[1]);
    msg_bytes16(m, 9, km);
    msg_byte(m, 25, 1);
    msg_absorb_final(ms, m, 26);
  }
  uint32_t pend0 = 0, pend1 = 0;
  TruncSink ts(p, sc.out, r);
  const int Mi = (int)M;
  // The fused accumulate: the wave totals of the share elements go to sc.wpart a tile at a time
  // through the wave's 8 KiB of LDS (tile_stage / tile_halfsum, prio3_device.h).  Two share
  // blocks hold 21 elements, e0 .. e0+20 with e0 = 21 (b >> 1): 10 whole ones and the first half
  // of e0+10 in the even block, the rest in the odd one.  They are cut into the tiles
  // A = e0..e0+7, B = e0+8..e0+15 and C = e0+16..e0+20, staged and flushed at two places per
  // block, fuse_top before and fuse_mid after the joint-rand permutation, so that every flush
  // reads what was stored a permutation earlier and all 8 slots are free again when it has run:
  //   even top: flush C of the blocks before, stage A     even mid: flush A, stage e0+8, e0+9
  //   odd top:  stage e0+10 .. e0+15                      odd mid:  flush B, stage C
  // and fuse_tail after the last block's fuse_mid flushes what that has staged.  Elements >= M
  // are neither staged nor stored.
  uint4* tile = nullptr;
  if constexpr (FUSE) {
    __shared__ uint4 fuse_tiles[XOFD_BLOCK / 64][FTILE * 64];
    tile = fuse_tiles[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  }
  // the wave's rows of sc.wpart: a scalar base (r >> 6 is the same on all 64 lanes), except in
  // the pulling variant, which has no two SGPRs left for it through the share loop (it spilled
  // them and grew its frame to 80 B) and forms the address per lane instead
  uint32_t* const wrow =
      FUSE && !PULL ? sc.wpart + (size_t)__builtin_amdgcn_readfirstlane(r >> 6) * M * 8u
                    : nullptr;
  const uint32_t wlane = (lane & 7u) * 8u + (lane >> 3);
  auto mword = [&](int w) __attribute__((always_inline)) {  // the element at words w .. w+3 of ms
    return mk128(kword(ms, w), kword(ms, w + 1), kword(ms, w + 2), kword(ms, w + 3));
  };
  auto stage = [&](int e, int slot, f128 x) __attribute__((always_inline)) {
    if (e >= Mi) return;               // wave-uniform
    if (haspad && oor) x = zero128();  // wave-uniform test; the masked lanes add nothing
    tile_stage(tile, slot, lane, x);
  };
  // slots 0 .. n-1 hold elements eb .. eb+n-1; lane l stores element eb + (l & 7), addend l >> 3
  auto flush = [&](int eb, int n) __attribute__((always_inline)) {
    const int cnt = min(n, Mi - eb);
    if (cnt <= 0) return;  // wave-uniform
    tile_fence();
    const uint32_t tot = tile_halfsum(tile, lane);
    if ((int)(lane & 7u) < cnt) {
      if constexpr (PULL) sc.wpart[((size_t)(r >> 6) * M + (uint32_t)eb) * 8u + wlane] = tot;
      else (wrow + (size_t)eb * 8u)[wlane] = tot;
    }
    tile_fence();
  };
  // share block b is in ms; q0, q1: the half element carried from block b-1
  auto fuse_top = [&](uint32_t b, uint32_t q0, uint32_t q1) __attribute__((always_inline)) {
    const int e0 = 21 * (int)(b >> 1);
    if ((b & 1) == 0) {
      if (b) flush(e0 - 5, 5);
#pragma unroll
      for (int t = 0; t < 8; t++) stage(e0 + t, t, mword(4 * t));
    } else {
      stage(e0 + 10, 2, mk128(q0, q1, kword(ms, 0), kword(ms, 1)));
#pragma unroll
      for (int t = 0; t < 5; t++) stage(e0 + 11 + t, 3 + t, mword(2 + 4 * t));
    }
  };
  auto fuse_mid = [&](uint32_t b) __attribute__((always_inline)) {
    const int e0 = 21 * (int)(b >> 1);
    if ((b & 1) == 0) {
      flush(e0, 8);
      stage(e0 + 8, 0, mword(32));
      stage(e0 + 9, 1, mword(36));
    } else {
      flush(e0 + 8, 8);
#pragma unroll
      for (int t = 0; t < 5; t++) stage(e0 + 16 + t, t, mword(22 + 4 * t));
    }
  };
  auto fuse_tail = [&](uint32_t b) __attribute__((always_inline)) {  // b: the last share block
    const int e0 = 21 * (int)(b >> 1);
    if ((b & 1) == 0) flush(e0 + 8, 2);
    else flush(e0 + 16, 5);
  };
  // Joint-rand block b holds the last 42 bytes of share block b-1 (words 0..10, a 16-bit funnel
  // shift) and the first 126 bytes of share block b (words 10..41).  The first part is XORed into
  // js as soon as js has been permuted for block b-1 and before ms moves on, so no share words
  // are carried across a permutation (the 11-word tail buffer spilled at 168 VGPRs).
  auto wmask = [&](int j) __attribute__((always_inline)) {  // bytes of word j below rem
    const uint32_t lo = 4u * (uint32_t)j;
    return (lo + 4 <= rem) ? 0xffffffffu : (lo >= rem ? 0u : ((1u << (8 * (rem - lo))) - 1u));
  };
  auto carry_tail = [&](bool last) __attribute__((always_inline)) {  // last: block B is next
#pragma unroll
    for (int j = 0; j < 10; j++) {
      uint32_t x = __builtin_amdgcn_alignbit(kword(ms, 32 + j), kword(ms, 31 + j), 16);
      if (last) x &= wmask(j);
      kxor_word(js, j, x);
    }
    uint32_t x = kword(ms, 41) >> 16;
    if (last) x &= wmask(10);
    kxor_word(js, 10, x);
  };
  // block 0: prefix (42 bytes) + the first 126 bytes of the share
  {
    if (FUSE && fuse) fuse_top(0, 0, 0);
    squeeze_meas<TR>(p, ms, 0, M, pend0, pend1, sc.meas, r, flag, ts);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[7]);
    msg_bytes16(m, 9, kb);
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
#pragma unroll
    for (int j = 0; j < 10; j++) kxor_word(js, j, m.w[j]);
    kxor_word(js, 10, (m.w[10] & 0xffffu) | (kword(ms, 0) << 16));
#pragma unroll
    for (int j = 11; j < 42; j++)
      kxor_word(js, j, __builtin_amdgcn_alignbit(kword(ms, j - 10), kword(ms, j - 11), 16));
    keccak_p12(js);
    if (FUSE && fuse) fuse_mid(0);
    carry_tail(B == 1);
    keccak_p12(ms);
  }
  if constexpr (PULL) {
    if (in.seg_dst) in.seg_dst[r] = in.seg_src[r];
    if (in.accept_dst) in.accept_dst[r] = in.accept_src[r];
  }
  // PULL: the wave's 64 leader shares are one contiguous run of 64 Q 16-byte pieces; iteration b
  // copies rows [Q (b-1) / (B-1), Q b / (B-1)) (1 or 2) of 64 pieces, lane l taking piece
  // 64 row + l, so every load instruction reads 1 KiB of consecutive host bytes (one 16-byte
  // piece per report per lane made the PCIe reads scattered: 18.5 GB/s, profiles/r03/r03o)
  const uint32_t Q = PULL ? p.prep_share_len / 16 : 0u;
  const size_t wbase = PULL ? (size_t)(r - lane) * (p.prep_share_len / 16) + lane : 0;
  const uint4* lsrc = PULL ? (const uint4*)in.leader_src + wbase : nullptr;
  uint4* ldst = PULL ? (uint4*)in.leader + wbase : nullptr;
  // full joint-rand blocks 1 .. B-1 (B <= K, so share block b exists for every b < B)
#pragma unroll 1
  for (uint32_t b = 1; b < B; b++) {
    uint4 pc0, pc1;
    uint32_t q0 = 0, q1 = 0;
    if constexpr (PULL) {
      q0 = Q * (b - 1) / (B - 1);
      q1 = Q * b / (B - 1);
      if (q0 < q1) pc0 = lsrc[64 * (size_t)q0];
      if (q0 + 1 < q1) pc1 = lsrc[64 * (size_t)(q0 + 1)];
    }
    if (FUSE && fuse) fuse_top(b, pend0, pend1);
    squeeze_meas<TR>(p, ms, b, M, pend0, pend1, sc.meas, r, flag, ts);
    kxor_word(js, 10, kword(ms, 0) << 16);
#pragma unroll
    for (int j = 11; j < 42; j++)
      kxor_word(js, j, __builtin_amdgcn_alignbit(kword(ms, j - 10), kword(ms, j - 11), 16));
    keccak_p12(js);
    if (FUSE && fuse) fuse_mid(b);
    carry_tail(b + 1 == B);
    if (b + 1 < K) keccak_p12(ms);
    if constexpr (PULL) {
      if (q0 < q1) ldst[64 * (size_t)q0] = pc0;
      if (q0 + 1 < q1) ldst[64 * (size_t)(q0 + 1)] = pc1;
    }
  }
  // final joint-rand block B: remaining share bytes, padding
  uint32_t part[4];
  {
    const bool hasW = B < K;
    if (FUSE && fuse && hasW) fuse_top(B, pend0, pend1);
    if (hasW) squeeze_meas<TR>(p, ms, B, M, pend0, pend1, sc.meas, r, flag, ts);
#pragma unroll
    for (int j = 0; j < 42; j++) {
      uint32_t x = 0;
      if (j == 10) x = hasW ? kword(ms, 0) << 16 : 0u;
      else if (j > 10)
        x = hasW ? __builtin_amdgcn_alignbit(kword(ms, j - 10), kword(ms, j - 11), 16) : 0u;
      x &= wmask(j);
      if ((uint32_t)j == (rem >> 2)) x ^= 1u << (8 * (rem & 3));
      if (j == 41) x ^= 0x80000000u;
      kxor_word(js, j, x);
    }
    keccak_p12(js);
    if (FUSE && fuse) {  // the last share block is B, or B-1 (its fuse_mid has run in the loop)
      if (hasW) fuse_mid(B);
      fuse_tail(hasW ? B : B - 1);
    }
    part[0] = kword(js, 0);
    part[1] = kword(js, 1);
    part[2] = kword(js, 2);
    part[3] = kword(js, 3);
  }
  {  // proofs share
    uint32_t kp[4];  // loaded here: it was live across the share loop
    load16(hs + 16, kp);
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[2]);
    msg_bytes16(m, 9, kp);
    msg_byte(m, 25, 1);
    msg_byte(m, 26, 1);
    msg_absorb_final(s, m, 27);
    const uint32_t PL = p.proof_len, Kp = (PL * 16 + 167) / 168;
    uint32_t q0 = 0, q1 = 0;
    for (uint32_t b = 0; b < Kp; b++) {
      squeeze_block<F>(p, s, b, PL, q0, q1, sc.proofs, r, flag);
      if (b + 1 < Kp) keccak_p12(s);
    }
  }
  {  // corrected seed, joint randomness
    uint32_t pub0[4];
    load16(in.pub + (size_t)r * p.public_share_len, pub0);
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[6]);
    msg_bytes16(m, 25, pub0);
    msg_bytes16(m, 41, part);
    msg_absorb_final(s, m, 57);
    uint32_t cor[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
    KState t;
    kzero(t);
    Msg m2;
    msg_zero(m2);
    msg_dst(m2, p.dst[3]);
    msg_bytes16(m2, 9, cor);
    msg_byte(m2, 25, 1);
    msg_absorb_final(t, m2, 26);
    uint32_t q0 = 0, q1 = 0;
    squeeze_block<F>(p, t, 0, p.jr_len, q0, q1, sc.jr, r, flag);
    sc.part[r] = make_uint4(part[0], part[1], part[2], part[3]);
    sc.corrected[r] = make_uint4(cor[0], cor[1], cor[2], cor[3]);
  }
  sc.flag[r] = (uint8_t)flag;
  if constexpr (LIST) {
    const uint64_t fm = __ballot(flag != 0);
    if (fm && sc.redo_cnt) {  // wave-uniform
      const uint32_t first = (uint32_t)__ffsll((long long)fm) - 1u;
      uint32_t base = 0;
      if (lane == first) base = atomicAdd(sc.redo_cnt, (uint32_t)__popcll(fm));
      base = (uint32_t)__shfl((int)base, (int)first);
      if (flag)
        sc.redo_list[base + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull))] = sc.redo_c0 + r;
    }
  }
  if constexpr (FUSE) {
    if (fuse) {  // all 64 lanes are live here
      const bool anyflag = __any(flag != 0);
      if (lane == 0) sc.wseg[r >> 6] = anyflag ? 0xffffffffu : s0;
    }
  }
}
template <bool FUSE, bool TR = false>
__global__ __launch_bounds__(XOFD_BLOCK, XOFD_OCC) void k_xofd(DevParams p, InPtrs in, Scratch sc) {
  xofd_body<FUSE, TR>(p, in, sc, blockIdx.x * blockDim.x + threadIdx.x);
}


// ------------------------------------------------------------------------------------
// Split XOF path (one Keccak state live per kernel, for occupancy):
//   k_xof_a   query randomness, measurement share and proofs share squeezed to scratch
//   k_jrpart  joint-rand part absorbed from the measurement share in scratch, corrected
//             seed, joint randomness.  The 42-byte prefix leaves every message word a 16-bit
//             funnel shift of two share words whose element/word offsets are compile-time
//             constants relative to 21*(b/2) (b = block index), so each 168-byte block is 11-12
//             coalesced 16-byte loads + 42 v_alignbit.
// ------------------------------------------------------------------------------------
template <class F>
#ifndef XOF_OCC
#define XOF_OCC 4
#endif
#ifndef JR_OCC
#define JR_OCC 4
#endif
__global__ __launch_bounds__(256, XOF_OCC) void k_xof_a(DevParams p, InPtrs in, Scratch sc) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  constexpr uint32_t ES = F::ES;
  uint32_t flag = p.force_slow;
  uint32_t nonce[4], km[4], kp[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  const uint8_t* hs = in.helper + (size_t)r * p.helper_share_len;
  load16(hs, km);
  load16(hs + 16, kp);
  {
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[5]);
    {
      uint32_t vk[4];
      load_vk(p, in, r, vk);
      msg_bytes16(m, 9, vk);
    }
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
    msg_absorb_final(s, m, 42);
    uint32_t w[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
    put_elem<F>(p, sc.qr, 0, r, w, flag);
  }
  {
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[1]);
    msg_bytes16(m, 9, km);
    msg_byte(m, 25, 1);
    msg_absorb_final(s, m, 26);
    const uint32_t M = p.meas_len, K = (M * ES + 167) / 168;
    uint32_t q0 = 0, q1 = 0;
    for (uint32_t b = 0; b < K; b++) {
      squeeze_block<F>(p, s, b, M, q0, q1, sc.meas, r, flag);
      if (b + 1 < K) keccak_p12(s);
    }
  }
  {
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[2]);
    msg_bytes16(m, 9, kp);
    msg_byte(m, 25, 1);
    msg_byte(m, 26, 1);
    msg_absorb_final(s, m, 27);
    const uint32_t PL = p.proof_len, Kp = (PL * ES + 167) / 168;
    uint32_t q0 = 0, q1 = 0;
    for (uint32_t b = 0; b < Kp; b++) {
      squeeze_block<F>(p, s, b, PL, q0, q1, sc.proofs, r, flag);
      if (b + 1 < Kp) keccak_p12(s);
    }
  }
  sc.flag[r] = (uint8_t)flag;
}

// Field128 only (every joint-randomness Prio3 instance uses Field128).
// FUSE: the measurement share streams through here anyway, so the (optimistic) per-segment
// aggregate is accumulated on the way: every element of the share is summed over the wave's 64
// reports by wave_halfsum2 and the wave's half-limb partials go to sc.wpart.  Only waves whose
// 64 reports are all present and in one segment are fused (sc.wseg records which); the rest,
// and every report the verdict or the host mask excludes, are fixed up in aggregate_finish.
// LEADER: agg_id 0 -- the blind is the last 16 bytes of the explicit leader input share
// (in.helper then points at the leader input shares), the binder byte is 0, and the corrected
// seed is derive_seed(own part || public part 1) (leader part first).
template <bool FUSE, bool LEADER = false>
__global__ __launch_bounds__(256, JR_OCC) void k_jrpart(DevParams p, InPtrs in, Scratch sc) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  bool fuse = false;
  if constexpr (FUSE) {
    const bool valid = r < p.n;
    const uint32_t sg = valid ? (sc.seg ? sc.seg[r] : 0u) : 0xffffffffu;
    const uint32_t s0 = (uint32_t)__shfl((int)sg, 0);
    // a report flagged for the rejection-sampling slow path gets its share rewritten later:
    // its wave is left to the fix-up pass
    const bool flagged = valid && sc.flag[r];
    fuse = __all(valid && sg == s0 && sg < p.nseg && !flagged);
    if (lane == 0 && (r - lane) < p.n) sc.wseg[r >> 6] = fuse ? s0 : 0xffffffffu;
  }
  if (r >= p.n) return;
  const size_t ld = p.ld;
  const int M = (int)p.meas_len;
  uint32_t nonce[4], kb[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  if constexpr (LEADER)
    load16(in.helper + (size_t)r * p.leader_share_len + (size_t)(p.meas_len + p.proof_len) * 16, kb);
  else
    load16(in.helper + (size_t)r * p.helper_share_len + 32, kb);
  uint32_t pre[11];
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[7]);
    msg_bytes16(m, 9, kb);
    msg_byte(m, 25, LEADER ? 0 : 1);
    msg_bytes16(m, 26, nonce);
#pragma unroll
    for (int j = 0; j < 11; j++) pre[j] = m.w[j];
  }
  const uint4* meas = (const uint4*)sc.meas;
  auto ldel = [&](int e) -> uint4 {
    const bool ok = e >= 0 && e < M;
    uint4 v = meas[(size_t)(ok ? e : 0) * ld + r];
    return ok ? v : make_uint4(0, 0, 0, 0);
  };
  auto wsel = [](const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; };
  // wave totals of elements e0, e0+1 (zero outside [0, M)); lanes 0..15 store slot lane
  auto fused_pair = [&](int e0, const uint4& a, const uint4& b) {
    if (e0 + 1 < 0 || e0 >= M) return;  // wave-uniform
    const uint32_t tot = wave_halfsum2(mk128(a.x, a.y, a.z, a.w), mk128(b.x, b.y, b.z, b.w), lane);
    const int e = e0 + (int)(lane >> 5);  // slot lane >> 2 on each lane of a quad
    if ((lane & 3u) == 0 && e >= 0 && e < M)
      sc.wpart[((size_t)(r >> 6) * (uint32_t)M + (uint32_t)e) * 8u + ((lane >> 2) & 7u)] = tot;
  };
  const uint32_t L = 42 + (uint32_t)M * 16;
  const uint32_t B = L / 168, rem = L % 168;
  KState s;
  kzero(s);
  for (uint32_t b = 0; b <= B; b++) {
    uint32_t x[42];
    const int q21 = 21 * (int)(b >> 1);
    if ((b & 1) == 0) {
      // u = 84q + j - 11: element 21q + floor((j-11)/4), word (j-11) mod 4; window 21q-3..21q+7
      uint4 E[11];
#pragma unroll
      for (int t = 0; t < 11; t++) E[t] = ldel(q21 - 3 + t);
      if (FUSE && fuse) {  // this window accounts for elements q21-2 .. q21+7 (E[1..10])
#pragma unroll
        for (int t = 1; t < 11; t += 2) fused_pair(q21 - 3 + t, E[t], E[t + 1]);
      }
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const int u0 = j - 11 + 12, u1 = j - 10 + 12;  // +12 keeps the offsets non-negative
        const uint32_t w0 = wsel(E[u0 >> 2], u0 & 3), w1 = wsel(E[u1 >> 2], u1 & 3);
        x[j] = __builtin_amdgcn_alignbit(w1, w0, 16);
      }
      if (b == 0) {
#pragma unroll
        for (int j = 0; j < 10; j++) x[j] = pre[j];
        x[10] = (pre[10] & 0xffffu) | (wsel(E[3], 0) << 16);
      }
    } else {
      // u = 84q + 31 + j: element 21q + 7 + floor((j+3)/4), word (j+3) mod 4; window 21q+7..21q+18
      uint4 E[12];
#pragma unroll
      for (int t = 0; t < 12; t++) E[t] = ldel(q21 + 7 + t);
      if (FUSE && fuse) {  // elements q21+8 .. q21+18 (E[1..11])
#pragma unroll
        for (int t = 1; t < 12; t += 2)
          fused_pair(q21 + 7 + t, E[t], t + 1 < 12 ? E[t + 1] : make_uint4(0, 0, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const int u0 = j + 3, u1 = j + 4;
        const uint32_t w0 = wsel(E[u0 >> 2], u0 & 3), w1 = wsel(E[u1 >> 2], u1 & 3);
        x[j] = __builtin_amdgcn_alignbit(w1, w0, 16);
      }
    }
    if (b == B) {
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const uint32_t lo = 4 * j;
        uint32_t mask = (lo + 4 <= rem) ? 0xffffffffu
                                        : (lo >= rem ? 0u : ((1u << (8 * (rem - lo))) - 1u));
        x[j] &= mask;
        if ((uint32_t)j == (rem >> 2)) x[j] ^= 1u << (8 * (rem & 3));
      }
      x[41] ^= 0x80000000u;
    }
#pragma unroll
    for (int j = 0; j < 42; j++) kxor_word(s, j, x[j]);
    keccak_p12(s);
  }
  uint32_t part[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
  uint32_t flag = sc.flag[r];
  uint32_t pub0[4];
  load16(in.pub + (size_t)r * p.public_share_len + (LEADER ? 16 : 0), pub0);
  KState c;
  kzero(c);
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[6]);
    msg_bytes16(m, 25, LEADER ? part : pub0);
    msg_bytes16(m, 41, LEADER ? pub0 : part);
    msg_absorb_final(c, m, 57);
  }
  uint32_t cor[4] = {kword(c, 0), kword(c, 1), kword(c, 2), kword(c, 3)};
  {
    KState t;
    kzero(t);
    Msg m2;
    msg_zero(m2);
    msg_dst(m2, p.dst[3]);
    msg_bytes16(m2, 9, cor);
    msg_byte(m2, 25, 1);
    msg_absorb_final(t, m2, 26);
    uint32_t q0 = 0, q1 = 0;
    squeeze_block<Fp128>(p, t, 0, p.jr_len, q0, q1, sc.jr, r, flag);
  }
  sc.part[r] = make_uint4(part[0], part[1], part[2], part[3]);
  sc.corrected[r] = make_uint4(cor[0], cor[1], cor[2], cor[3]);
  sc.flag[r] = (uint8_t)flag;
}


// ------------------------------------------------------------------------------------
// k_leader_unpack: the leader's explicit input share (AoS, leader_input_share_len bytes per
// report) into the SoA measurement / proofs scratch with the canonical-encoding check, plus the
// query randomness (1 permutation) -- the leader analogue of k_xof_a.
// ------------------------------------------------------------------------------------
// wpart / wseg (non-null: the device leader's fused accumulate, leader_fuse_acc): while a chunk
// sits in LDS, thread (element tid / 8, half-limb tid % 8) also sums that 16-bit half-limb over
// the block's 64 reports -- the wave partials k_agg_parts reads (the layout of wave_halfsum2's)
// -- and the block's wave is marked fused for segment 0 when all 64 reports are present and
// canonical.
__global__ __launch_bounds__(256) void k_leader_unpack(DevParams p, InPtrs in, Scratch sc,
                                                       uint8_t* status, uint32_t* wpart,
                                                       uint32_t* wseg) {
  // block = 64 reports; the explicit shares are transposed through LDS in chunks of 32
  // elements (rows read 512 B contiguous per report, columns written 1 KiB contiguous per
  // element) -- per-lane row streaming of the 5.6 KiB rows ran at a fraction of HBM speed.
  typedef Fp128 F;
  constexpr int RB = 64, CE = 32;
  __shared__ uint4 tile[RB][CE + 1];
  __shared__ uint32_t bad[RB];
  const uint32_t tid = threadIdx.x, r0 = blockIdx.x * RB;
  const size_t ld = p.ld;
  const uint32_t M = p.meas_len, PL = p.proof_len, E = M + PL;
  const uint32_t nrep = min((uint32_t)RB, p.n - r0);
  if (tid < RB) bad[tid] = 0;
  for (uint32_t c0 = 0; c0 < E; c0 += CE) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RB * CE / 256; i++) {
      const uint32_t idx = tid + 256 * i, rr = idx / CE, e = c0 + idx % CE;
      if (rr < nrep && e < E) {
        const uint4 v =
            ((const uint4*)(in.helper + (size_t)(r0 + rr) * p.leader_share_len))[e];
        if (!F::lt_p(mk128(v.x, v.y, v.z, v.w))) atomicOr(&bad[rr], 1u);
        tile[rr][idx % CE] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RB * CE / 256; i++) {
      const uint32_t idx = tid + 256 * i, rr = idx % RB, el = idx / RB, e = c0 + el;
      if (rr < nrep && e < E) {
        if (e < M)
          ((uint4*)sc.meas)[(size_t)e * ld + r0 + rr] = tile[rr][el];
        else
          ((uint4*)sc.proofs)[(size_t)(e - M) * ld + r0 + rr] = tile[rr][el];
      }
    }
    if (wpart && nrep == RB && c0 < M) {  // uniform
      const uint32_t el = tid >> 3, h = tid & 7u, e = c0 + el;
      if (e < M) {
        uint32_t sum = 0;
#pragma unroll 8
        for (uint32_t rr = 0; rr < RB; rr++) {
          const uint32_t* w = (const uint32_t*)&tile[rr][el];
          sum += (w[h >> 1] >> ((h & 1u) * 16u)) & 0xffffu;
        }
        wpart[((size_t)blockIdx.x * M + e) * 8u + h] = sum;
      }
    }
  }
  __syncthreads();
  if (tid >= nrep) return;
  const uint32_t r = r0 + tid;
  uint32_t flag = p.force_slow;
  uint32_t nonce[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  KState s;
  kzero(s);
  Msg m;
  msg_zero(m);
  msg_dst(m, p.dst[5]);
  {
    uint32_t vk[4];
    load_vk(p, in, r, vk);  // coalesced groups of several tasks: the report's own key
    msg_bytes16(m, 9, vk);
  }
  msg_byte(m, 25, 1);
  msg_bytes16(m, 26, nonce);
  msg_absorb_final(s, m, 42);
  uint32_t w[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
  put_elem<F>(p, sc.qr, 0, r, w, flag);
  if (p.qr_len > 1) {  // FPVec: one query point per gadget, from the same squeeze block
    uint32_t w1[4] = {kword(s, 4), kword(s, 5), kword(s, 6), kword(s, 7)};
    put_elem<F>(p, sc.qr, 1, r, w1, flag);
  }
  sc.flag[r] = (uint8_t)flag;
  status[r] = bad[tid] ? PRIO3_STATUS_INPUT_SHARE_DECODE : PRIO3_STATUS_FINISHED;
  if (wseg) {
    const bool fuse = nrep == RB && __all(!bad[tid]);  // nrep == RB: all 64 lanes are here
    if (tid == 0) wseg[blockIdx.x] = fuse ? 0u : 0xffffffffu;
  }
}

// ------------------------------------------------------------------------------------
// leader_jr_body (the first half of k_leader_prep): k_leader_unpack + k_jrpart<false, true> on
// one lane, once a kernel of its own (k_leader_jr, the figures below).  Each lane absorbs its
// own report's measurement share into the joint-rand sponge straight from the AoS input (the
// 11-12 16-byte loads of a sponge block run back to back over the same 176-192 bytes of the
// row), checks the encodings and writes the SoA measurement / proofs scratch the query reads;
// the share is read from HBM once instead of twice.  Then the joint-rand part, corrected seed,
// joint randomness (k_jrpart) and the query randomness (k_leader_unpack).  wpart / wseg as
// k_leader_unpack's (the device leader's fused accumulate): the wave totals of each element by
// wave_halfsum2, the wave marked fused when all 64 reports are present and canonical.
// Interleaved on one box (profiles/r05/leader_jr/): 173.4-173.9 against 165.4-166.5 M reports/s
// for the two kernels (k_leader_jr 3.76 ms against 2.32 + 1.70 ms per 1 Mi).  Staging each
// sponge block's 64 x 11-12 elements through LDS with coalesced row segments instead (one wave
// per block, 12 KiB, 3 waves per SIMD) took 4.12 ms.
// ------------------------------------------------------------------------------------
DEV void leader_jr_body(const DevParams& p, const InPtrs& in, const Scratch& sc,
                        uint8_t* status, uint32_t* wpart, uint32_t* wseg, const uint32_t r) {
  typedef Fp128 F;
  const uint32_t lane = threadIdx.x & 63u;
  const bool acc = wpart != nullptr && __all(r < p.n);  // wave-uniform
  if (r >= p.n) return;
  const size_t ld = p.ld;
  const int M = (int)p.meas_len;
  const uint32_t PL = p.proof_len;
  const uint4* row = (const uint4*)(in.helper + (size_t)r * p.leader_share_len);
  // the executor's SoA staging (InPtrs::lin_ld): element e of report r at cell e * lin_ld + r
  const uint4* soa = (const uint4*)in.helper + r;
  const size_t sld = in.lin_ld;
  auto rel = [&](int e) -> uint4 { return sld ? soa[(size_t)e * sld] : row[e]; };
  uint32_t bad = 0;
  uint32_t nonce[4], kb[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  {
    const uint4 k = rel(M + (int)PL);
    kb[0] = k.x;
    kb[1] = k.y;
    kb[2] = k.z;
    kb[3] = k.w;
  }
  uint32_t pre[11];
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[7]);
    msg_bytes16(m, 9, kb);
    msg_byte(m, 25, 0);
    msg_bytes16(m, 26, nonce);
#pragma unroll
    for (int j = 0; j < 11; j++) pre[j] = m.w[j];
  }
  uint4* meas = (uint4*)sc.meas;
  auto ldel = [&](int e) -> uint4 {
    const bool ok = e >= 0 && e < M;
    const uint4 v = rel(ok ? e : 0);
    return ok ? v : make_uint4(0, 0, 0, 0);
  };
  // element e (owned by this window): canonical check and the SoA copy
  auto own = [&](int e, const uint4& v) {
    if (e < 0 || e >= M) return;
    if (!F::lt_p(mk128(v.x, v.y, v.z, v.w))) bad = 1;
    meas[(size_t)e * ld + r] = v;
  };
  auto wsel = [](const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; };
  // wave totals of elements e0, e0 + 1 (the second only if below lim)
  auto acc_pair = [&](int e0, const uint4& a, const uint4& b, int lim) {
    if (e0 + 1 < 0 || e0 >= M) return;  // wave-uniform
    const uint32_t tot = wave_halfsum2(mk128(a.x, a.y, a.z, a.w), mk128(b.x, b.y, b.z, b.w), lane);
    const int e = e0 + (int)(lane >> 5);
    if ((lane & 3u) == 0 && e >= 0 && e < M && e < lim)
      wpart[((size_t)(r >> 6) * (uint32_t)M + (uint32_t)e) * 8u + ((lane >> 2) & 7u)] = tot;
  };
  const uint32_t L = 42 + (uint32_t)M * 16;
  const uint32_t B = L / 168, rem = L % 168;
  KState s;
  kzero(s);
  for (uint32_t b = 0; b <= B; b++) {
    uint32_t x[42];
    const int q21 = 21 * (int)(b >> 1);
    if ((b & 1) == 0) {
      // window q21-3 .. q21+7; this block owns q21-2 .. q21+7 (E[1..10])
      uint4 E[11];
#pragma unroll
      for (int t = 0; t < 11; t++) E[t] = ldel(q21 - 3 + t);
#pragma unroll
      for (int t = 1; t < 11; t++) own(q21 - 3 + t, E[t]);
      if (acc) {
#pragma unroll
        for (int t = 1; t < 11; t += 2) acc_pair(q21 - 3 + t, E[t], E[t + 1], q21 + 8);
      }
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const int u0 = j - 11 + 12, u1 = j - 10 + 12;
        const uint32_t w0 = wsel(E[u0 >> 2], u0 & 3), w1 = wsel(E[u1 >> 2], u1 & 3);
        x[j] = __builtin_amdgcn_alignbit(w1, w0, 16);
      }
      if (b == 0) {
#pragma unroll
        for (int j = 0; j < 10; j++) x[j] = pre[j];
        x[10] = (pre[10] & 0xffffu) | (wsel(E[3], 0) << 16);
      }
    } else {
      // window q21+7 .. q21+18; this block owns q21+8 .. q21+18 (E[1..11])
      uint4 E[12];
#pragma unroll
      for (int t = 0; t < 12; t++) E[t] = ldel(q21 + 7 + t);
#pragma unroll
      for (int t = 1; t < 12; t++) own(q21 + 7 + t, E[t]);
      if (acc) {
#pragma unroll
        for (int t = 1; t < 12; t += 2)
          acc_pair(q21 + 7 + t, E[t], t + 1 < 12 ? E[t + 1] : make_uint4(0, 0, 0, 0), q21 + 19);
      }
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const int u0 = j + 3, u1 = j + 4;
        const uint32_t w0 = wsel(E[u0 >> 2], u0 & 3), w1 = wsel(E[u1 >> 2], u1 & 3);
        x[j] = __builtin_amdgcn_alignbit(w1, w0, 16);
      }
    }
    if (b == B) {
#pragma unroll
      for (int j = 0; j < 42; j++) {
        const uint32_t lo = 4 * j;
        uint32_t mask = (lo + 4 <= rem) ? 0xffffffffu
                                        : (lo >= rem ? 0u : ((1u << (8 * (rem - lo))) - 1u));
        x[j] &= mask;
        if ((uint32_t)j == (rem >> 2)) x[j] ^= 1u << (8 * (rem & 3));
      }
      x[41] ^= 0x80000000u;
    }
#pragma unroll
    for (int j = 0; j < 42; j++) kxor_word(s, j, x[j]);
    keccak_p12(s);
  }
  {  // the proofs share: canonical check and SoA copy
    uint4* proofs = (uint4*)sc.proofs;
    for (uint32_t e = 0; e < PL; e++) {
      const uint4 v = rel(M + (int)e);
      if (!F::lt_p(mk128(v.x, v.y, v.z, v.w))) bad = 1;
      proofs[(size_t)e * ld + r] = v;
    }
  }
  uint32_t flag = p.force_slow;
  {  // query randomness (k_leader_unpack)
    KState q;
    kzero(q);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[5]);
    {
      uint32_t vk[4];
      load_vk(p, in, r, vk);
      msg_bytes16(m, 9, vk);
    }
    msg_byte(m, 25, 1);
    msg_bytes16(m, 26, nonce);
    msg_absorb_final(q, m, 42);
    uint32_t w[4] = {kword(q, 0), kword(q, 1), kword(q, 2), kword(q, 3)};
    put_elem<F>(p, sc.qr, 0, r, w, flag);
  }
  uint32_t part[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
  uint32_t pub0[4];
  load16(in.pub + (size_t)r * p.public_share_len + 16, pub0);
  KState c;
  kzero(c);
  {
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[6]);
    msg_bytes16(m, 25, part);
    msg_bytes16(m, 41, pub0);
    msg_absorb_final(c, m, 57);
  }
  uint32_t cor[4] = {kword(c, 0), kword(c, 1), kword(c, 2), kword(c, 3)};
  {
    KState t;
    kzero(t);
    Msg m2;
    msg_zero(m2);
    msg_dst(m2, p.dst[3]);
    msg_bytes16(m2, 9, cor);
    msg_byte(m2, 25, 1);
    msg_absorb_final(t, m2, 26);
    uint32_t q0 = 0, q1 = 0;
    squeeze_block<Fp128>(p, t, 0, p.jr_len, q0, q1, sc.jr, r, flag);
  }
  sc.part[r] = make_uint4(part[0], part[1], part[2], part[3]);
  sc.corrected[r] = make_uint4(cor[0], cor[1], cor[2], cor[3]);
  sc.flag[r] = (uint8_t)flag;
  status[r] = bad ? PRIO3_STATUS_INPUT_SHARE_DECODE : PRIO3_STATUS_FINISHED;
  if (wseg) {
    const bool fuse = acc && __all(!bad);
    if (lane == 0) wseg[r >> 6] = fuse ? 0u : 0xffffffffu;
  }
}

// Leader slow path: reports whose query or joint-rand expansion hit a rejection-sampling
// event (flagged by k_leader_unpack / k_jrpart) get both redone by the byte-level sponge.
__global__ __launch_bounds__(64) void k_leader_slowfix(DevParams p, InPtrs in, Scratch sc) {
  typedef Fp128 F;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n || !sc.flag[r]) return;
  uint32_t nonce[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  uint8_t b[17];
  b[0] = 1;
  for (int i = 0; i < 16; i++) b[1 + i] = (uint8_t)(nonce[i >> 2] >> (8 * (i & 3)));
  uint32_t vk[4];
  load_vk(p, in, r, vk);
  bx_expand<F>(p, p.dst[5], vk, b, 17, p.qr_len, sc.qr, p.ld, r);
  const uint4 c = sc.corrected[r];
  const uint32_t cor[4] = {c.x, c.y, c.z, c.w};
  bx_expand<F>(p, p.dst[3], cor, b, 1, p.jr_len, sc.jr, p.ld, r);
}

// ------------------------------------------------------------------------------------
// k_xof_slow: general byte-level sponge with rejection sampling (flagged reports only)
// ------------------------------------------------------------------------------------
// (byte-level sponge helpers BX / bx_* live in prio3_common.h)
// The sponges run one at a time (one Keccak state live): the joint-rand-part sponge absorbs the
// measurement share from the scratch rows this lane has just written, instead of beside the
template <class F, int SITE = 0>
__device__ __noinline__ void xof_slow_one(const DevParams& p, const InPtrs& in, const Scratch& sc,
                                          uint32_t r) {
  uint32_t nonce[4];
  load16(in.nonces + 16 * (size_t)r, nonce);
  const uint8_t* hs = in.helper + (size_t)r * p.helper_share_len;
  const bool JR = p.jr_len > 0;
  uint32_t w[4];
  {  // query rand
    BX x;
    BX_SET_REJ(x, p);
    uint32_t vk[4];
    load_vk(p, in, r, vk);
    bx_init(x, p.dst[5], vk);
    bx_absorb(x, 1);
    bx_absorb_w(x, nonce, 16);
    bx_finalize(x);
    for (uint32_t i = 0; i < p.qr_len; i++) {
      bx_next_elem<F>(x, w);
      F::store(sc.qr, (size_t)i * p.ld + r, F::from_words(w));
    }
  }
  {  // measurement share
    BX x;
    BX_SET_REJ(x, p);
    uint32_t km[4];
    load16(hs, km);
    bx_init(x, p.dst[1], km);
    bx_absorb(x, 1);
    bx_finalize(x);
    if constexpr (F::ES == 16) {
      TruncSink ts(p, sc.out, r);
      for (uint32_t i = 0; i < p.meas_len; i++) {
        bx_next_elem<F>(x, w);
        F::store(sc.meas, (size_t)i * p.ld + r, F::from_words(w));
        if (p.trunc_xof) ts.put(mk128(w[0], w[1], w[2], w[3]));
      }
    } else {
      for (uint32_t i = 0; i < p.meas_len; i++) {
        bx_next_elem<F>(x, w);
        F::store(sc.meas, (size_t)i * p.ld + r, F::from_words(w));
      }
    }
  }
  uint32_t part[4] = {0, 0, 0, 0};
  if (JR) {  // joint-rand part over the encoded share, read back from this lane's rows
    BX y;
    uint32_t kb[4];
    load16(hs + 32, kb);
    bx_init(y, p.dst[7], kb);
    bx_absorb(y, 1);
    bx_absorb_w(y, nonce, 16);
    for (uint32_t i = 0; i < p.meas_len; i++) {
      const typename F::T v = F::load(sc.meas, (size_t)i * p.ld + r);
      if constexpr (F::ES == 16) {
        w[0] = v.w[0], w[1] = v.w[1], w[2] = v.w[2], w[3] = v.w[3];
      } else {
        w[0] = (uint32_t)v, w[1] = (uint32_t)(v >> 32);
      }
      bx_absorb_w(y, w, F::ES);
    }
    bx_finalize(y);
    for (int k = 0; k < 4; k++) {
      uint32_t v = 0;
      for (int b = 0; b < 4; b++) v |= (uint32_t)bx_squeeze(y) << (8 * b);
      part[k] = v;
    }
  }
  {  // proofs
    BX x;
    BX_SET_REJ(x, p);
    uint32_t kp[4];
    load16(hs + 16, kp);
    bx_init(x, p.dst[2], kp);
    bx_absorb(x, 1);
    bx_absorb(x, 1);
    bx_finalize(x);
    for (uint32_t i = 0; i < p.proof_len; i++) {
      bx_next_elem<F>(x, w);
      F::store(sc.proofs, (size_t)i * p.ld + r, F::from_words(w));
    }
  }
  if (JR) {
    uint32_t cor[4];
    {
      BX x;
      uint32_t pub0[4], zero[4] = {0, 0, 0, 0};
      load16(in.pub + (size_t)r * p.public_share_len, pub0);
      bx_init(x, p.dst[6], zero);
      bx_absorb_w(x, pub0, 16);
      bx_absorb_w(x, part, 16);
      bx_finalize(x);
      for (int k = 0; k < 4; k++) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) v |= (uint32_t)bx_squeeze(x) << (8 * b);
        cor[k] = v;
      }
    }
    BX y;
    BX_SET_REJ(y, p);
    bx_init(y, p.dst[3], cor);
    bx_absorb(y, 1);
    bx_finalize(y);
    for (uint32_t i = 0; i < p.jr_len; i++) {
      bx_next_elem<F>(y, w);
      F::store(sc.jr, (size_t)i * p.ld + r, F::from_words(w));
    }
    sc.part[r] = make_uint4(part[0], part[1], part[2], part[3]);
    sc.corrected[r] = make_uint4(cor[0], cor[1], cor[2], cor[3]);
  }
  sc.flag[r] = p.slow_defer ? 2u : 0u;
}

// The slow path's launch: each lane scans the flags of 16 reports with one 16-byte load and
// re-runs the byte-level XOF only for flagged ones (a rejection has probability ~2^-59 per
// Field128 element, so in practice every lane exits after its one load; the old one-lane-per-
// report grid of 64-thread blocks cost a mean 15 us per launch).
template <class F, int RPL = 16>
__global__ __launch_bounds__(64) void k_xof_slow(DevParams p, InPtrs in, Scratch sc) {
  const uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) * RPL;
  if (r0 >= p.n) return;
  const uint8_t* fl = sc.flag + r0;
  uint32_t any = 0;
  if (RPL == 16 && r0 + 16 <= p.n && ((uintptr_t)fl & 15) == 0) {
    const uint4 v = *(const uint4*)fl;
    any = v.x | v.y | v.z | v.w;
  } else {
    for (uint32_t i = 0; i < RPL && r0 + i < p.n; i++) any |= fl[i];
  }
  if (!any) return;
  for (uint32_t i = 0; i < RPL && r0 + i < p.n; i++)
    if (fl[i]) xof_slow_one<F>(p, in, sc, r0 + i);
}

// launch geometry of k_xof_slow: 16 reports per lane, one wave per block (a one-wave block
// needs one SIMD with room for it, not four on one CU, beside the other streams' kernels)
static inline uint32_t slow_blocks(uint32_t n) { return (n + 1023) / 1024; }
// the deferred slow path's redo launches (k_slow_redo*): REDO_RPL reports scanned per lane, so a
// run without flagged reports costs few waves
constexpr uint32_t REDO_RPL = 64;
static inline uint32_t redo_blocks(uint32_t n) {
  return (n + 64 * REDO_RPL - 1) / (64 * REDO_RPL);
}
// any flag among reports [r0, r0 + REDO_RPL) of the run
__device__ __forceinline__ bool redo_any(const DevParams& p, const Scratch& sc, uint32_t r0) {
  const uint8_t* fl = sc.flag + r0;
  uint32_t any = 0;
  if (r0 + REDO_RPL <= p.n && ((uintptr_t)fl & 15) == 0) {
#pragma unroll
    for (uint32_t k = 0; k < REDO_RPL / 16; k++) {
      const uint4 v = ((const uint4*)fl)[k];
      any |= v.x | v.y | v.z | v.w;
    }
  } else {
    for (uint32_t i = 0; i < REDO_RPL && r0 + i < p.n; i++) any |= fl[i];
  }
  return any != 0;
}

// ------------------------------------------------------------------------------------
// k_query: FLP query + decide + prepare message + prepare_next + truncate
// ------------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void query_body(const DevParams& p, const InPtrs& in, const Scratch& sc,
                                           const OutPtrs& out, const uint32_t r) {
  typedef typename F::T T;
  // r: this lane's report; slow_defer / redo (DevParams) as in query_h_body
  if (r >= p.n) return;
  if (p.redo) {
    if (sc.flag[r] != 2) return;
  } else if (p.slow_defer && sc.flag[r]) {
    return;
  }
  const size_t ld = p.ld;
  const uint32_t A = p.arity;
  uint8_t status = PRIO3_STATUS_FINISHED;
  const T t = ldf<F>(sc.qr, 0, ld, r);
  T v, pt;
  if (!flp_query_lane<F>(p, sc.meas, sc.proofs, sc.jr, t, sc.Lbuf, sc.PVbuf, sc.acc, r, v, pt))
    status = PRIO3_STATUS_PREP_INIT;
  // combine with the leader's verifier share and decide
  const uint8_t* lps = in.leader + (size_t)r * p.prep_share_len;
  bool decode_ok = true;
  auto lv = [&](uint32_t e) {
    T x = F::load(lps, e);
    if (!F::lt_p(x)) decode_ok = false;
    return x;
  };
  const T V0 = F::add(lv(0), v);
  T G = F::zero();
  if (p.kind == PRIO3_COUNT) {
    T a = F::add(lv(1), F::load(sc.acc, 0 * ld + r));
    T b = F::add(lv(2), F::load(sc.acc, 1 * ld + r));
    G = F::mul(a, b);
  } else if (p.kind == PRIO3_SUM) {
    T a = F::add(lv(1), F::load(sc.acc, r));
    G = F::sub(F::mul(a, a), a);
  } else {
    for (uint32_t j = 0; j < p.chunk; j++) {
      T a = F::add(lv(1 + 2 * j), F::load(sc.acc, (size_t)(2 * j) * ld + r));
      T b = F::add(lv(2 + 2 * j), F::load(sc.acc, (size_t)(2 * j + 1) * ld + r));
      G = F::add(G, F::mul(a, b));
    }
  }
  const T PT = F::add(lv(A + 1), pt);
  if (status == PRIO3_STATUS_FINISHED) {
    if (!decode_ok)
      status = PRIO3_STATUS_PREP_SHARE_DECODE;
    else if (!F::is_zero(V0) || !F::eq(G, PT))
      status = PRIO3_STATUS_PREP_MSG;
  }
  uint32_t msg[4] = {0, 0, 0, 0};
  if (p.jr_len > 0) {
    uint32_t lpart[4], hpart[4];
    load16(lps + (size_t)p.verifier_len * F::ES, lpart);
    uint4 hp = sc.part[r];
    hpart[0] = hp.x;
    hpart[1] = hp.y;
    hpart[2] = hp.z;
    hpart[3] = hp.w;
    KState s;
    kzero(s);
    Msg m;
    msg_zero(m);
    msg_dst(m, p.dst[6]);
    msg_bytes16(m, 25, lpart);
    msg_bytes16(m, 41, hpart);
    msg_absorb_final(s, m, 57);
    uint4 cor = sc.corrected[r];
    msg[0] = kword(s, 0);
    msg[1] = kword(s, 1);
    msg[2] = kword(s, 2);
    msg[3] = kword(s, 3);
    if (status == PRIO3_STATUS_FINISHED &&
        (msg[0] != cor.x || msg[1] != cor.y || msg[2] != cor.z || msg[3] != cor.w))
      status = PRIO3_STATUS_PREP_NEXT;
    if (status != PRIO3_STATUS_FINISHED) msg[0] = msg[1] = msg[2] = msg[3] = 0;
    ((uint4*)out.prep_msgs)[r] = make_uint4(msg[0], msg[1], msg[2], msg[3]);
  }
  out.status[r] = status;
  // truncate (Count/Histogram: identity, read straight from the meas scratch)
  if (p.kind == PRIO3_SUM) {
    T acc = F::zero(), pw = F::one();
    for (uint32_t i = 0; i < p.meas_len; i++) {
      acc = F::add(acc, F::mul(pw, ldf<F>(sc.meas, i, ld, r)));
      pw = F::add(pw, pw);
    }
    F::store(sc.out, r, acc);
  } else if (p.kind == PRIO3_SUMVEC) {
    for (uint32_t e = 0; e < p.out_len; e++) {
      T acc = F::zero(), pw = F::one();
      for (uint32_t b = 0; b < p.bits; b++) {
        acc = F::add(acc, F::mul(pw, ldf<F>(sc.meas, e * p.bits + b, ld, r)));
        pw = F::add(pw, pw);
      }
      F::store(sc.out, (size_t)e * ld + r, acc);
    }
  }
}
template <class F>
__global__ __launch_bounds__(256) void k_query(DevParams p, InPtrs in, Scratch sc, OutPtrs out) {
  query_body<F>(p, in, sc, out, blockIdx.x * blockDim.x + threadIdx.x);
}

// k_prep_gen<F>: the generic XOF and query of one report on one lane in one launch (Prio3Count,
// C1), the slow path deferred to the run's redo launch, as k_prep_h.  (Taking the byte-level
// sponge inline for a flagged report instead -- a noinline call in the kernel -- doubled the
// kernel, 37.6 -> 73.6 us per 100k, r05ai; the 13 us redo launch stays.)
template <class F>
__global__ __launch_bounds__(256) void k_prep_gen(DevParams p, InPtrs in, Scratch sc, OutPtrs out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  xof_body<F>(p, in, sc, r);
  query_body<F>(p, in, sc, out, r);
}

// k_slow_redo_gen<F>: k_prep_gen's deferred slow path in one launch (as k_slow_redo): each lane
// scans the flags of REDO_RPL reports and, for a flagged one, re-runs its XOF on the
// byte-level sponge (flag := 2) and then its query (p.redo = 1)
template <class F>
__global__ __launch_bounds__(64) void k_slow_redo_gen(DevParams p, InPtrs in, Scratch sc,
                                                      OutPtrs out) {
  const uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) * REDO_RPL;
  if (r0 >= p.n || !redo_any(p, sc, r0)) return;
  const uint8_t* fl = sc.flag + r0;
  for (uint32_t i = 0; i < REDO_RPL && r0 + i < p.n; i++)
    if (fl[i]) {
      xof_slow_one<F>(p, in, sc, r0 + i);
      query_body<F>(p, in, sc, out, r0 + i);
    }
}

// ------------------------------------------------------------------------------------
// k_query_ps: FLP query + decide for the ParallelSum(Mul, C) circuits (Histogram, SumVec).
//
// Wire 2j of gadget call k carries r^(Ck+j+1) m_(Ck+j), wire 2j+1 carries m_(Ck+j) - 1/2, so
// with beta_k = L_(k+1)(t) r^(Ck):
//   f_2j(t)   = seed_2j L_0 + r^(j+1) sum_k beta_k m_(Ck+j)
//   f_2j+1(t) = seed_2j+1 L_0 + sum_k L_(k+1) m_(Ck+j) - (1/2) sum_k L_(k+1)
// The 2C wire accumulators are swept GS wires-pairs at a time in registers (each measurement
// element is read exactly once from HBM), two Field128 multiplies per element.
// ------------------------------------------------------------------------------------
template <int GS>
__global__ __launch_bounds__(256) void k_query_ps(DevParams p, InPtrs in, Scratch sc,
                                                  OutPtrs out) {
  typedef Fp128 F;
  typedef f128 T;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const size_t ld = p.ld;
  const uint32_t P = p.P, A = p.arity, C = p.chunk, M = p.meas_len, K = p.calls;
  uint8_t status = PRIO3_STATUS_FINISHED;
  const T t = ldf<F>(sc.qr, 0, ld, r);
  {
    T tp = t;
    for (uint32_t l = 0; l < p.logP; l++) tp = F::mul(tp, tp);
    if (F::eq(tp, F::one())) status = PRIO3_STATUS_PREP_INIT;
  }
  // Lagrange basis at t (one size-P DFT of t^e/P) and gadget polynomial at the P-th roots
  {
    T pw = FC<F>::invP(p);
    for (uint32_t e = 0; e < P; e++) {
      F::store(sc.Lbuf, (size_t)bitrev(e, p.logP) * ld + r, pw);
      pw = F::mul(pw, t);
    }
    dft_lane<F>(p, sc.Lbuf, r, P, p.logP);
    for (uint32_t e = 0; e < P; e++) {
      T q = ldf<F>(sc.proofs, A + e, ld, r);
      if (e + P < p.glen) q = F::add(q, ldf<F>(sc.proofs, A + e + P, ld, r));
      F::store(sc.PVbuf, (size_t)bitrev(e, p.logP) * ld + r, q);
    }
    dft_lane<F>(p, sc.PVbuf, r, P, p.logP);
  }
  auto Lc = [&](uint32_t c) { return ldf<F>(sc.Lbuf, (P - c) & (P - 1), ld, r); };
  T pt = F::zero();
  for (uint32_t e = p.glen; e-- > 0;) pt = F::add(F::mul(pt, t), ldf<F>(sc.proofs, A + e, ld, r));
  // beta_k, sum of L_(k+1), sum of p(alpha^(k+1))
  const T r0 = ldf<F>(sc.jr, 0, ld, r);
  T rC = F::one();
  for (uint32_t j = 0; j < C; j++) rC = F::mul(rC, r0);
  T sumL = F::zero(), range = F::zero();
  {
    T rk = F::one();
    for (uint32_t k = 0; k < K; k++) {
      const T L = Lc(k + 1);
      sumL = F::add(sumL, L);
      range = F::add(range, ldf<F>(sc.PVbuf, k + 1, ld, r));
      F::store(sc.beta, (size_t)k * ld + r, F::mul(L, rk));
      rk = F::mul(rk, rC);
    }
  }
  const T L0 = Lc(0);
  const T half = FC<F>::half(p);
  const T halfL = F::mul(half, sumL);
  const uint8_t* lps = in.leader + (size_t)r * p.prep_share_len;
  bool decode_ok = true;
  auto lv = [&](uint32_t e) {
    T x = F::load(lps, e);
    if (!F::lt_p(x)) decode_ok = false;
    return x;
  };
  T S = F::zero(), G = F::zero(), rj = r0;
  const T Z = F::zero();
  for (uint32_t jg = 0; jg < C; jg += GS) {
    T Aa[GS], Bb[GS];
#pragma unroll
    for (int q = 0; q < GS; q++) Aa[q] = Bb[q] = Z;
    // software-pipelined as in k_query_fp: call k+1's loads are in flight during call k's
    // products; invalid slots load element 0 and are zeroed at use
    auto ldm = [&](uint32_t k, int q) {
      const uint32_t i = k * C + jg + (uint32_t)q;
      return ldf<F>(sc.meas, (jg + q < C && i < M) ? i : 0, ld, r);
    };
    T be_n = ldf<F>(sc.beta, 0, ld, r), L_n = Lc(1), mn[GS];
#pragma unroll
    for (int q = 0; q < GS; q++) mn[q] = ldm(0, q);
#pragma unroll 1
    for (uint32_t k = 0; k < K; k++) {
      const T be = be_n, L = L_n;
      T mc[GS];
#pragma unroll
      for (int q = 0; q < GS; q++) mc[q] = mn[q];
      const uint32_t kn = k + 1 < K ? k + 1 : k;
      be_n = ldf<F>(sc.beta, kn, ld, r);
      L_n = Lc(kn + 1);
#pragma unroll
      for (int q = 0; q < GS; q++) mn[q] = ldm(kn, q);
      const uint32_t base = k * C + jg;
#pragma unroll
      for (int q = 0; q < GS; q++) {
        const bool valid = (jg + q < C) && (base + q < M);
        const T m = F::sel(valid, mc[q], Z);
        Aa[q] = F::add(Aa[q], F::mul(be, m));
        Bb[q] = F::add(Bb[q], F::mul(L, m));
        S = F::add(S, m);
      }
    }
#pragma unroll
    for (int q = 0; q < GS; q++) {
      const uint32_t j = jg + q;
      const bool valid = j < C;
      const uint32_t jj = valid ? j : 0;
      const T f0 = F::add(F::mul(ldf<F>(sc.proofs, 2 * jj, ld, r), L0), F::mul(rj, Aa[q]));
      const T f1 = F::sub(F::add(F::mul(ldf<F>(sc.proofs, 2 * jj + 1, ld, r), L0), Bb[q]), halfL);
      const T prod = F::mul(F::add(lv(1 + 2 * jj), f0), F::add(lv(2 + 2 * jj), f1));
      G = F::add(G, F::sel(valid, prod, Z));
      rj = F::sel(valid, F::mul(rj, r0), rj);
    }
  }
  T v;
  if (p.kind == PRIO3_SUMVEC) {
    v = range;
  } else {
    const T r1 = ldf<F>(sc.jr, 1, ld, r);
    v = F::add(F::mul(r1, range), F::mul(F::mul(r1, r1), F::sub(S, half)));
  }
  const T V0 = F::add(lv(0), v);
  const T PT = F::add(lv(A + 1), pt);
  if (status == PRIO3_STATUS_FINISHED) {
    if (!decode_ok)
      status = PRIO3_STATUS_PREP_SHARE_DECODE;
    else if (!F::is_zero(V0) || !F::eq(G, PT))
      status = PRIO3_STATUS_PREP_MSG;
  }
  uint32_t lpart[4], hpart[4];
  load16(lps + (size_t)p.verifier_len * F::ES, lpart);
  {
    uint4 hp = sc.part[r];
    hpart[0] = hp.x;
    hpart[1] = hp.y;
    hpart[2] = hp.z;
    hpart[3] = hp.w;
  }
  KState s;
  kzero(s);
  Msg mm;
  msg_zero(mm);
  msg_dst(mm, p.dst[6]);
  msg_bytes16(mm, 25, lpart);
  msg_bytes16(mm, 41, hpart);
  msg_absorb_final(s, mm, 57);
  uint4 cor = sc.corrected[r];
  uint32_t msg[4] = {kword(s, 0), kword(s, 1), kword(s, 2), kword(s, 3)};
  if (status == PRIO3_STATUS_FINISHED &&
      (msg[0] != cor.x || msg[1] != cor.y || msg[2] != cor.z || msg[3] != cor.w))
    status = PRIO3_STATUS_PREP_NEXT;
  if (status != PRIO3_STATUS_FINISHED) msg[0] = msg[1] = msg[2] = msg[3] = 0;
  ((uint4*)out.prep_msgs)[r] = make_uint4(msg[0], msg[1], msg[2], msg[3]);
  out.status[r] = status;
  if (p.kind == PRIO3_SUMVEC) {
    for (uint32_t e = 0; e < p.out_len; e++) {
      T acc = F::zero(), pw = F::one();
      for (uint32_t b = 0; b < p.bits; b++) {
        acc = F::add(acc, F::mul(pw, ldf<F>(sc.meas, e * p.bits + b, ld, r)));
        pw = F::add(pw, pw);
      }
      F::store(sc.out, (size_t)e * ld + r, acc);
    }
  }
}

// ------------------------------------------------------------------------------------
// k_query_h<GS, PP>: k_query_ps specialised for a compile-time wire-polynomial length
// PP <= 32 (Prio3Histogram(256,16) has PP = 32).  The Lagrange basis comes from an
// in-register PP-point DFT of (t^e / P) -- no scratch round trips -- and the circuit only
// needs sum_c p(alpha^c) = sum_e coef_e * sigma_(e mod P) (sigma precomputed on the host),
// so the gadget polynomial is never evaluated on the roots.  The measurement loads of the
// next gadget call are issued before the current call's arithmetic (register double buffer).
// ------------------------------------------------------------------------------------
// LEADER = 1: the leader's prepare_init (agg_id 0) on the same data flow -- the wire values
// f_j(t), v and p(t) are written as the leader prepare share (out.prep_msgs is the prepare
// share buffer, stride prep_share_len) instead of being decided against a peer's share.
template <int GS, int PP, int LEADER = 0>
__device__ __forceinline__ void query_h_body(const DevParams& p, const InPtrs& in, const Scratch& sc,
                                             const OutPtrs& out, const uint32_t r) {
  typedef Fp128 F;
  typedef f128 T;
  constexpr int LOGP = PP <= 2 ? 1 : PP <= 4 ? 2 : PP <= 8 ? 3 : PP <= 16 ? 4 : 5;
  if (r >= p.n) return;
  // slow_defer: a report the XOF flagged (a rejected sample) is skipped here; after the whole
  // run, k_xof_slow re-runs its XOF (flag := 2) and this kernel runs again with p.redo = 1 for
  // exactly those reports -- no k_xof_slow launch between the XOF and the query of each chunk
  if constexpr (!LEADER) {
    if (p.redo) {
      if (sc.flag[r] != 2) return;
    } else if (p.slow_defer && sc.flag[r]) {
      return;
    }
  } else {
    // the fused leader kernel (k_leader_prep) defers a flagged report; k_leader_slowfix redoes
    // its randomness and this query runs again for exactly those reports (p.redo)
    if (p.redo) {
      if (!sc.flag[r]) return;
    } else if (p.slow_defer && sc.flag[r]) {
      return;
    }
  }
  const size_t ld = p.ld;
  const uint32_t A = p.arity, C = p.chunk, M = p.meas_len, K = p.calls;
  uint8_t status = LEADER ? out.status[r] : PRIO3_STATUS_FINISHED;  // leader: unpack verdict
  uint8_t* lout = LEADER ? out.prep_msgs + (size_t)r * p.prep_share_len : nullptr;
  const T t = ldf<F>(sc.qr, 0, ld, r);
  T sumL = F::zero();
  // u_e = t^e / P.  PP <= 16: one in-register DFT.  PP == 32: decimation in frequency,
  // X[2k] = DFT16(u_e + u_(e+16)), X[2k+1] = DFT16((u_e - u_(e+16)) w32^e), each a geometric
  // sequence, so only 16 values (64 VGPRs) are live at a time.
  auto store_L = [&](int idx, const T& val) {  // X[idx] = L_c with c = (P - idx) mod P
    const uint32_t c = (uint32_t)((PP - idx) & (PP - 1));
    if (c == 0) {
      F::store(sc.Lbuf, r, val);  // row 0: L_0, read back with each sweep's finish operands
    } else if (c <= K) {
      F::store(sc.Lbuf, (size_t)c * ld + r, val);
      sumL = F::add(sumL, val);
    }
  };
  if constexpr (PP <= 16) {
    T x[PP];
    T pw = FC<F>::invP(p);
#pragma unroll
    for (int e = 0; e < PP; e++) {
      x[__builtin_bitreverse32(e) >> (32 - LOGP)] = pw;
      pw = F::mul(pw, t);
    }
    if (F::eq(pw, FC<F>::invP(p))) status = PRIO3_STATUS_PREP_INIT;  // t^P == 1
    dft_reg<PP, LOGP>(p, x, 1);
#pragma unroll
    for (int k = 0; k < PP; k++) store_L(k, x[k]);
  } else {
    static_assert(PP == 32, "PP must be <= 32");
    // Four phases of an 8-point DFT: X[4k + ph] = DFT8(y^ph)[k] with y^ph_n = (G_ph / P)(t w^ph)^n,
    // w = w32 and G_ph = sum_(i<4) (t^8 w4^ph)^i, so only 8 values (32 VGPRs) are live at a time
    // (two 16-point phases held 64 and spilled at 168 VGPRs).
    T t8 = t;
#pragma unroll
    for (int i = 0; i < 3; i++) t8 = F::mul(t8, t8);
    const T t16 = F::mul(t8, t8);
    const T t32 = F::mul(t16, t16);
    if (F::eq(t32, F::one())) status = PRIO3_STATUS_PREP_INIT;
    const T ip = FC<F>::invP(p);
    const T a = F::add(F::one(), t16), b = F::sub(F::one(), t16);
    const T c = F::mul(t8, a), wd = F::mul(F::mul(t8, b), F::from_words(p.tw128[8]));  // w4 = w32^8
#pragma unroll
    for (int ph = 0; ph < 4; ph++) {
      const T g = ph == 0 ? F::add(a, c) : ph == 1 ? F::add(b, wd) : ph == 2 ? F::sub(a, c)
                                                                              : F::sub(b, wd);
      T x[8];
      T pw = F::mul(ip, g);
      const T ratio = ph == 0 ? t : F::mul(t, F::from_words(p.tw128[ph]));
#pragma unroll
      for (int e = 0; e < 8; e++) {
        x[__builtin_bitreverse32(e) >> 29] = pw;
        if (e + 1 < 8) pw = F::mul(pw, ratio);
      }
      dft_reg<8, 3>(p, x, 4);
#pragma unroll
      for (int k = 0; k < 8; k++) store_L(4 * k + ph, x[k]);
    }
  }
  // p(t) and range = sum_c p(alpha^c) = sum_e coef_e sigma_(e mod P); the range sum is a lazily
  // reduced dot product with the (uniform) sigma.
  T pt = F::zero(), range;
  // p(t) = sum_q (t^8)^q S_q, S_q = sum_(i<8) coef_(8q+i) t^i: 63 lazy MACs against t^0..t^7
  // (6 multiplies), one reduction per block of eight and a Horner step in t^8 per block -- 13
  // full multiplies + 8 reductions instead of 63 multiplies (r05)
  {
    constexpr int GLEN = 2 * (PP - 1) + 1, NB = (GLEN + 7) / 8;
    T pw[8];
    pw[0] = F::one();
    pw[1] = t;
#pragma unroll
    for (int i = 2; i < 8; i++) pw[i] = F::mul(pw[i - 1], t);
    const T t8b = F::mul(pw[7], t);
    mac128 R;
    mac_zero(R);
    auto ldc = [&](int e) { return ldf<F>(sc.proofs, A + (e < GLEN ? e : 0), ld, r); };
    T cb[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cb[i] = ldc(8 * (NB - 1) + i);
#pragma unroll 1
    for (int q = NB - 1; q >= 0; q--) {
      T cn[8];
      const int qn = q > 0 ? q - 1 : 0;
#pragma unroll
      for (int i = 0; i < 8; i++) cn[i] = ldc(8 * qn + i);  // the next block's, one block ahead
      mac128 S;
      mac_zero(S);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int e = 8 * q + i;
        if (e < GLEN) {  // uniform
          mac_add(S, cb[i], pw[i]);
          mac_add(R, cb[i], F::from_words(p.sigma128[e & (PP - 1)]));
        }
        cb[i] = cn[i];
      }
      const T sq = mac_reduce_f(S);
      pt = q == NB - 1 ? sq : F::add(F::mul(pt, t8b), sq);
    }
    range = mac_reduce_f(R);
  }
  // p(t), the range sum and (below) L/2 are not needed inside the wire sweeps: they wait in this
  // lane's column of PVbuf (unused on this path) instead of in registers the sweeps are short of
  F::store(sc.PVbuf, (size_t)1 * ld + r, pt);
  F::store(sc.PVbuf, (size_t)2 * ld + r, range);
  const T r0 = ldf<F>(sc.jr, 0, ld, r);
  {
    // r0^C by square-and-multiply over the (uniform) bits of C
    T rC = F::one(), sq = r0;
    for (uint32_t e = C; e; e >>= 1) {
      if (e & 1) rC = F::mul(rC, sq);
      if (e > 1) sq = F::mul(sq, sq);
    }
    // beta_k = L_(k+1) r^(Ck), eight L values loaded at a time
    T rk = F::one();
    for (uint32_t k0 = 0; k0 < K; k0 += 8) {
      T lb[8];
#pragma unroll
      for (int q = 0; q < 8; q++) lb[q] = ldf<F>(sc.Lbuf, k0 + q < K ? k0 + q + 1 : 1, ld, r);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        if (k0 + q < K) {
          F::store(sc.beta, (size_t)(k0 + q) * ld + r, F::mul(lb[q], rk));
          rk = F::mul(rk, rC);
        }
      }
    }
  }
  const T half = FC<F>::half(p);
  F::store(sc.PVbuf, r, F::mul(half, sumL));
  const uint8_t* lps = in.leader + (size_t)r * p.prep_share_len;
  bool decode_ok = true;
  auto lv = [&](uint32_t e) {
    T x = F::load(lps, e);
    if (!F::lt_p(x)) decode_ok = false;
    return x;
  };
  sum128 Ssum;
  sum_zero(Ssum);
  T G = F::zero(), rj = r0;
  uint64_t lane = (uint64_t)sc.meas + (uint64_t)r * F::ES;  // see ldrow below
  asm("" : "+v"(lane));
  for (uint32_t jg = 0; jg < C; jg += GS) {
    mac128 Aa[GS], Bb[GS];
#pragma unroll
    for (int q = 0; q < GS; q++) {
      mac_zero(Aa[q]);
      mac_zero(Bb[q]);
    }
    // The operands of one gadget call: its GS measurement elements, beta_k and L_(k+1), each one
    // dwordx4 load from a clamped (always in-bounds) address.  Padding elements are zeroed at
    // their use with a wave-uniform mask (a select on the loaded value made the compiler split
    // the load into four branch-guarded dword loads).
    //
    // A call's operands are issued WIRE_AHEAD trips before the trip that multiplies by them:
    // the rows come from L2 misses, and one trip's arithmetic (64 v_mad_u64_u32) is what hides
    // the round trip.  Written as "load the next call's into temporaries, copy at the end of the
    // trip", the compiler moved the beta / L loads across the back edge to the top of the trip
    // that consumes them (only the measurement elements stayed a trip ahead).  So the loop is
    // unrolled over WIRE_AHEAD + 1 register sets with no copy between them, and use() opens with
    // a compiler-level barrier that neither the loads above it nor the multiplies below it can
    // cross (tools/isa_load_use.py reads the result off the assembly).  Two trips ahead also
    // fits the registers and measured slower (profiles/r09/SUMMARY.txt).
    constexpr int WIRE_AHEAD = 1;
    struct wire_ops {
      T m[GS];
      T be, L;
    };
    // Row e of scratch array X for this lane is read at lane + ((X - meas) + e * ld * ES): one
    // 64-bit lane address for all six arrays of the sweep, the bracket wave-uniform (SGPRs).
    // Left to itself the compiler keeps a lane address pair per array live through the sweep,
    // which the second register set has no room for.  The lane address is opaque and the
    // offset goes through readfirstlane so that the sum is not split up and hoisted again.
    auto ldrow = [&](const void* base, uint32_t e) {
      const uint64_t off = ((uint64_t)base - (uint64_t)sc.meas) + (uint64_t)e * ld * F::ES;
      const uint64_t offu =
          ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(off >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)off);
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)(lane + offu);  // global
      return mk128(v.x, v.y, v.z, v.w);
    };
    const uint32_t Klast = K ? K - 1 : 0;
    auto issue = [&](uint32_t k, wire_ops& s) {
#pragma unroll
      for (int q = 0; q < GS; q++) {
        const uint32_t i = k * C + jg + q;
        const bool valid = (k < K) && (jg + q < C) && (i < M);
        s.m[q] = ldrow(sc.meas, i & (valid ? 0xffffffffu : 0u));  // a mask, not a branch
      }
      const uint32_t kc = min(k, Klast);
      s.be = ldrow(sc.beta, kc);
      s.L = ldrow(sc.Lbuf, kc + 1);
    };
    auto use = [&](uint32_t k, wire_ops& s) {  // k < K
      // the barrier: the loads issued before it stay above it, and this call's multiplies,
      // which all read m[q], stay below it
#pragma unroll
      for (int q = 0; q < GS; q++)
        asm volatile(""
                     : "+v"(s.m[q].w[0]), "+v"(s.m[q].w[1]), "+v"(s.m[q].w[2]), "+v"(s.m[q].w[3])
                     :
                     : "memory");
#pragma unroll
      for (int q = 0; q < GS; q++) {
        const bool valid = (jg + q < C) && (k * C + jg + q < M);
        const uint32_t msk = valid ? 0xffffffffu : 0u;
        const T mc = mk128(s.m[q].w[0] & msk, s.m[q].w[1] & msk, s.m[q].w[2] & msk,
                           s.m[q].w[3] & msk);
        mac_add(Aa[q], s.be, mc);
        mac_add(Bb[q], s.L, mc);
        sum_add(Ssum, mc);
      }
    };
    constexpr int NS = WIRE_AHEAD + 1;
    wire_ops ws[NS];
    // (opaque, so that the row offsets of these first loads are formed here and not kept in
    // SGPRs across all sweeps, which spilled them)
    uint32_t k = __builtin_amdgcn_readfirstlane(0);
    asm volatile("" : "+s"(k));
#pragma unroll
    for (int u = 0; u < WIRE_AHEAD; u++) issue(k + u, ws[u]);
    // K mod NS leading trips (these copy between the sets), then whole rounds of NS trips
#pragma unroll 1
    for (uint32_t e = K % NS; e; e--, k++) {
      issue(k + WIRE_AHEAD, ws[WIRE_AHEAD]);
      use(k, ws[0]);
#pragma unroll
      for (int u = 0; u < WIRE_AHEAD; u++) ws[u] = ws[u + 1];
    }
#pragma unroll 1
    for (; k < K; k += NS) {
#pragma unroll
      for (int u = 0; u < NS; u++) {
        issue(k + u + WIRE_AHEAD, ws[(u + WIRE_AHEAD) % NS]);
        use(k + u, ws[u]);
      }
    }
    // The sweep's finish operands -- L_0, r, the two proof seeds of each wire and, for the
    // helper, its two leader verifier elements -- go into the registers the loop has just freed,
    // in two batches: what the first reduction needs right after the last trip, the rest behind
    // that reduction, which frees an accumulator and hides their round trip.  One exposed wait
    // per sweep instead of three per wire.  An idle second wire (j >= C) loads the first wire's
    // operands again and does not use them.
    T sd[2 * GS], lw[2 * GS], r0f;
    auto fin_load = [&](int q) {
      const uint32_t jc = jg + q < C ? jg + q : jg;
      if constexpr (!LEADER) {
        lw[2 * q] = F::load(lps, 1 + 2 * jc);
        lw[2 * q + 1] = F::load(lps, 2 + 2 * jc);
      }
    };
    const T L0 = ldrow(sc.Lbuf, 0), halfL = ldrow(sc.PVbuf, 0);
#pragma unroll
    for (int q = 0; q < GS; q++) {
      const uint32_t jc = jg + q < C ? jg + q : jg;
      sd[2 * q + 1] = ldrow(sc.proofs, 2 * jc + 1);
      sd[2 * q] = ldrow(sc.proofs, 2 * jc);
    }
    fin_load(0);
    asm volatile("" ::: "memory");
    // Wire values at t, lazily reduced: f1 = seed_(2j+1) L0 + B_j - L/2 folds the seed term into
    // B's accumulator, f0 = seed_2j L0 + r^(j+1) A_j is one two-product MAC, and the gadget
    // products of the group are summed in one MAC before a single reduction.
    mac128 Gq;
    mac_zero(Gq);
#pragma unroll
    for (int q = 0; q < GS; q++) {
      const uint32_t j = jg + q;
      if (q == 0 || j < C) {  // wave-uniform; the first wire of a sweep always exists
        mac_add(Bb[q], sd[2 * q + 1], L0);
        T f1 = F::sub(mac_reduce_f(Bb[q]), halfL);
        if (q == 0) {
          // second batch, kept behind the first reduction by the barrier on its result
          asm volatile("" : "+v"(f1.w[0])::"memory");
          r0f = ldrow(sc.jr, 0);
#pragma unroll
          for (int q2 = 1; q2 < GS; q2++) fin_load(q2);
          asm volatile("" ::: "memory");
        }
        const T Aq = mac_reduce_f(Aa[q]);
        mac128 F0;
        mac_zero(F0);
        mac_add(F0, sd[2 * q], L0);
        mac_add(F0, rj, Aq);
        const T f0 = mac_reduce_f(F0);
        if constexpr (LEADER) {
          F::store(lout, 1 + 2 * j, f0);
          F::store(lout, 2 + 2 * j, f1);
        } else {
          if (!F::lt_p(lw[2 * q]) || !F::lt_p(lw[2 * q + 1])) decode_ok = false;
          mac_add(Gq, F::add(lw[2 * q], f0), F::add(lw[2 * q + 1], f1));
        }
        rj = F::mul(rj, r0f);
      }
    }
    if constexpr (!LEADER) G = F::add(G, mac_reduce_f(Gq));
  }
  const T S = sum_reduce(Ssum);
  pt = ldf<F>(sc.PVbuf, 1, ld, r);
  range = ldf<F>(sc.PVbuf, 2, ld, r);
  T v;
  if (p.kind == PRIO3_SUMVEC) {
    v = range;
  } else {
    const T r1 = ldf<F>(sc.jr, 1, ld, r);
    v = F::add(F::mul(r1, range), F::mul(F::mul(r1, r1), F::sub(S, half)));
  }
  if constexpr (LEADER) {
    F::store(lout, 0, v);
    F::store(lout, A + 1, pt);
    *(uint4*)(lout + (size_t)p.verifier_len * F::ES) = sc.part[r];
    out.status[r] = status;
  } else {
  const T V0 = F::add(lv(0), v);
  const T PT = F::add(lv(A + 1), pt);
  if (status == PRIO3_STATUS_FINISHED) {
    if (!decode_ok)
      status = PRIO3_STATUS_PREP_SHARE_DECODE;
    else if (!F::is_zero(V0) || !F::eq(G, PT))
      status = PRIO3_STATUS_PREP_MSG;
  }
  uint32_t lpart[4], msg[4];
  load16(lps + (size_t)p.verifier_len * F::ES, lpart);
  if (!prep_msg_check(p, in, sc, r, lpart, msg) && status == PRIO3_STATUS_FINISHED)
    status = PRIO3_STATUS_PREP_NEXT;
  if (status != PRIO3_STATUS_FINISHED) msg[0] = msg[1] = msg[2] = msg[3] = 0;
  ((uint4*)out.prep_msgs)[r] = make_uint4(msg[0], msg[1], msg[2], msg[3]);
  out.status[r] = status;
  }
  if (p.kind == PRIO3_SUMVEC) {
    for (uint32_t e = 0; e < p.out_len; e++) {
      T acc = F::zero(), pw = F::one();
      for (uint32_t b = 0; b < p.bits; b++) {
        acc = F::add(acc, F::mul(pw, ldf<F>(sc.meas, e * p.bits + b, ld, r)));
        pw = F::add(pw, pw);
      }
      F::store(sc.out, (size_t)e * ld + r, acc);
    }
  }
}
template <int GS, int PP, int LEADER = 0>
__global__ __launch_bounds__(256, 3) void k_query_h(DevParams p, InPtrs in, Scratch sc,
                                                  OutPtrs out) {
  query_h_body<GS, PP, LEADER>(p, in, sc, out, blockIdx.x * blockDim.x + threadIdx.x);
}

// k_prep_h<FUSE>: the whole helper prepare of Prio3Histogram with P = 32 in one launch -- the
// dual-state XOF (xofd_body) and then the query (query_h_body; flagged reports deferred to the
// run's redo pass, slow_defer) of the same 64 reports on the same wave.  Both phases fit 3 waves per SIMD, and the waves of a
// SIMD drift apart, so one wave's memory-bound query runs beside other waves' issue-bound Keccak
// without a kernel boundary, a second stream or the k_xof_slow launch between them.  The query
// reads the scratch rows its own lane has just written.
template <bool FUSE, bool PULL = false>
__global__ __launch_bounds__(XOFD_BLOCK, 3) void k_prep_h(DevParams p, InPtrs in, Scratch sc,
                                                   OutPtrs out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  xofd_body<FUSE, false, PULL, true>(p, in, sc, r);
  // two wires per sweep: 3 and 4 spill inside the wire loop
  query_h_body<2, 32>(p, in, sc, out, r);
}

// k_leader_prep<PP>: the leader's prepare_init of Prio3Histogram / SumVec in one launch, as
// k_prep_h is the helper's: leader_jr_body (the explicit share streamed once into the joint-rand
// sponge and the SoA scratch) and then query_h_body<2, PP, 1> on the scratch rows the same lane
// has just written, so one wave's memory-bound share streaming runs beside other waves' query.
// Flagged reports are deferred to k_leader_slowfix + a k_query_h redo launch.
template <int PP>
__global__ __launch_bounds__(256, 3) void k_leader_prep(DevParams p, InPtrs in, Scratch sc,
                                                        OutPtrs out, uint32_t* wpart,
                                                        uint32_t* wseg) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  leader_jr_body(p, in, sc, out.status, wpart, wseg, r);
  query_h_body<2, PP, 1>(p, in, sc, out, r);
}

// k_prep_sum<NPH>: the same for Prio3Sum (P = 16 NPH): the dual-state XOF and k_query_sum's body
// (prio3_query_sum.h) on the same wave, flagged reports deferred to the run's redo launch
template <int NPH>
__global__ __launch_bounds__(256, 3) void k_prep_sum(DevParams p, InPtrs in, Scratch sc,
                                                     OutPtrs out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  xofd_body<false, false>(p, in, sc, r);
  qsum::query_sum_body<NPH, 0>(p, in, sc, out, r);
}

// The deferred slow path of a run whose k_query_h launches skipped the reports the XOF flagged
// (slow_defer): one k_slow_redo launch over the whole run redoes their XOF (marking them 2) and
// then their query (redo = 1), lane by lane.  One launch per run instead of one k_xof_slow
// launch between the XOF and the query of every chunk, where its one-wave blocks waited behind
// the other stream's kernels (~0.2 ms per chunk in the r02 trace).
// k_slow_redo<PP>: both halves in one launch -- each lane scans the flags of REDO_RPL reports
// (16-byte loads) and, for a flagged report, re-runs its XOF (flag := 2) and then its query on
// the same lane.
// z: the accumulators of a fused run's aggregate (fused_first_zero), zeroed here by the launch's
// threads ahead of their scan, so that the run's first fused_finish needs no zeroing launch;
// empty for the other runs.
template <int PP>
__global__ __launch_bounds__(64) void k_slow_redo(DevParams p, InPtrs in, Scratch sc, OutPtrs out,
                                                  ZeroRanges z) {
  zero_ranges(z, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
  if (sc.redo_cnt) {
    // k_prep_h's list: REDO_LIST_BLOCKS blocks whatever the run's size, the lanes stride over
    // the entries (any number of them; slow for many, which only force_slow makes).  Each block,
    // done with the counter, draws a ticket; the last one puts counter and ticket back to zero
    // for the stream's next prepare.  No block waits for another.
    const uint32_t cnt = __hip_atomic_load(sc.redo_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
      const uint32_t r = sc.redo_list[i];
      xof_slow_one<Fp128>(p, in, sc, r);
      query_h_body<2, PP>(p, in, sc, out, r);
    }
    if (threadIdx.x == 0) {  // (one wave per block: its read of the counter is behind it)
      const uint32_t t = __hip_atomic_fetch_add(sc.redo_cnt + 1, 1u, __ATOMIC_ACQ_REL,
                                                __HIP_MEMORY_SCOPE_AGENT);
      if (t == gridDim.x - 1) {
        __hip_atomic_store(sc.redo_cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sc.redo_cnt + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    return;
  }
  const uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) * REDO_RPL;
  if (r0 >= p.n || !redo_any(p, sc, r0)) return;
  const uint8_t* fl = sc.flag + r0;
  for (uint32_t i = 0; i < REDO_RPL && r0 + i < p.n; i++)
    if (fl[i]) {
      xof_slow_one<Fp128>(p, in, sc, r0 + i);
      query_h_body<2, PP>(p, in, sc, out, r0 + i);
    }
}

template <int NPH>
__global__ __launch_bounds__(64) void k_slow_redo_sum(DevParams p, InPtrs in, Scratch sc,
                                                      OutPtrs out) {
  const uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) * REDO_RPL;
  if (r0 >= p.n || !redo_any(p, sc, r0)) return;
  const uint8_t* fl = sc.flag + r0;
  for (uint32_t i = 0; i < REDO_RPL && r0 + i < p.n; i++)
    if (fl[i]) {
      xof_slow_one<Fp128>(p, in, sc, r0 + i);
      qsum::query_sum_body<NPH, 0>(p, in, sc, out, r0 + i);
    }
}

// ====================================================================================
// Host side: which kernels a run takes, and their launches
// ====================================================================================

// FPVec sub-batch sizes for n reports in scratch of cap columns: nsub equal sub-batches (columns
// rounded to 256), except that under the eight-lane query (k_query_fpw, two waves per SIMD, eight
// reports per wave) the first nsub - 1 are rounded down to whole query rounds -- n_cu x 4 SIMDs x
// 2 waves x 8 reports (16,384 on MI355X) -- when the last still fits the scratch (option
// fp_round).  The query's waves all take the same time, so a sub-batch of 3.05 rounds takes 4:
// 2 x 50,000 run 8 rounds, 49,152 + 50,848 run 7, while the XOF of either size keeps at most two
// waves per SIMD.
static void fp_sub_sizes(const prio3_engine* e, uint32_t n, uint32_t cap, bool wide,
                         uint32_t& nsub, uint32_t& sub) {
  nsub = (n + cap - 1) / cap;
  sub = std::min(cap, (((n + nsub - 1) / nsub) + 255) & ~255u);
  if (wide && e->fp_round && nsub > 1) {
    const uint32_t Q = (uint32_t)e->n_cu * 4u * 2u * 8u;
    const uint32_t s2 = sub / Q * Q;
    if (s2 > 0 && n - (nsub - 1) * s2 <= cap) sub = s2;
  }
}

template <class F>
static void launch_xof_slow(const prio3_engine* e, const DevParams& p, const InPtrs& in,
                            const Scratch& sc, hipStream_t st) {
  (void)e;
  k_xof_slow<F><<<slow_blocks(p.n), 64, 0, st>>>(p, in, sc);
}

// The one dispatch from a run-time value to a template argument of the prepare kernels:
// f(std::integral_constant<int, V>{}) for the first V of the list that equals v, else for the last.
// <32, 16, 8>: PP of k_query_h, k_slow_redo and k_leader_prep; <16, 32, 64, 128>: the P of
// k_prep_sum and k_slow_redo_sum, whose NPH is P / 16; <1, 0>: a bool.
template <int V, int... Vs, class F>
static void with_value(uint32_t v, F&& f) {
  if constexpr (sizeof...(Vs) == 0)
    f(std::integral_constant<int, V>{});
  else if (v == V)
    f(std::integral_constant<int, V>{});
  else
    with_value<Vs...>(v, f);
}

// The one statement of which kernels a helper prepare takes; pure.
PrepPlan plan_prepare(const prio3_engine* e, const DevParams& dp, uint32_t n, bool fuse,
                      bool pulling) {
  PrepPlan p{};
  const bool ps = dp.kind == PRIO3_HISTOGRAM || dp.kind == PRIO3_SUMVEC;
  const bool two = share_spans_two_blocks(dp.meas_len);
  // The fused accumulate applies where the output share is the measurement share (Histogram;
  // truncate is the identity) and the joint-rand kernel streams that share.
  p.fusable = e->fuse_acc && dp.kind == PRIO3_HISTOGRAM && dp.jr_len && two;
  if (dp.kind == PRIO3_SUMVEC_F64_MP) {
    p.chain = PrepChain::MP64;
  } else if (dp.kind == PRIO3_FPVEC_BOUNDED_L2) {
    // the lane-pair XOF (k_xof_pair, the entries decoded as the share is squeezed), else the
    // dual-state k_xofd; both decode the entries (the output share) on the fly
    p.chain = PrepChain::FPVEC;
    p.dual = p.trunc_xof = two;
    p.xof = two ? XofKernel::PAIR : XofKernel::XOF;
    p.query = !e->force_generic && fpvec_query_wide_takes(dp) ? QueryKernel::FPW : QueryKernel::FP;
  } else if (dp.es != 16) {  // Field64 (Prio3Count): XOF + query in one launch
    p.chain = PrepChain::GEN64;
    p.slow_defer = true;
    p.redo = RedoFamily::GEN64;
  } else {
    p.dual = dp.jr_len && two;
    // XOF + query in one launch: Prio3Sum (k_prep_sum) and Histogram / SumVec with P = 32
    // (k_prep_h); the slow path of both is deferred to the run's redo launch
    if (!e->force_generic && p.dual && dp.kind == PRIO3_SUM && !fuse && query_sum_takes(dp)) {
      p.chain = PrepChain::FUSED_SUM;
      p.redo = RedoFamily::SUM;
    } else if (!e->force_generic && p.dual && ps && dp.P == 32) {
      p.chain = PrepChain::FUSED_H;
      p.redo = RedoFamily::QH;
    } else {
      // two kernels: the XOF (dual-state k_xofd when the share spans >= 2 joint-rand blocks, else
      // k_xof_a + k_jrpart), then the query
      p.chain = PrepChain::XOF_QUERY;
      p.xof = p.dual ? XofKernel::XOFD : XofKernel::XOF_A_JRPART;
      // P = 64 / 128 on eight lanes per report (k_query_w)
      const bool wide = ps && !e->force_generic && dp.P != 32 && query_wide_takes(dp);
      // SumVec under k_query_w: the truncation rides on the XOF's squeeze (the query then reads
      // the share once)
      p.trunc_xof = dp.kind == PRIO3_SUMVEC && wide && p.dual && !fuse;
      // k_query_h defers flagged reports to the run's redo pass; the other queries read the
      // shares the k_xof_slow launch rewrote
      const bool qh = ps && !e->force_generic && !wide && (dp.P == 32 || dp.P == 16 || dp.P == 8);
      if (qh) p.redo = RedoFamily::QH;
      const bool qsum = !ps && !e->force_generic && query_sum_takes(dp);
      p.query = wide   ? QueryKernel::WIDE
                : qh   ? QueryKernel::H
                : ps   ? QueryKernel::PS
                : qsum ? QueryKernel::SUM
                       : QueryKernel::GENERIC;
    }
    p.slow_defer = p.redo != RedoFamily::NONE;
  }
  const bool fused_h = p.chain == PrepChain::FUSED_H;
  // k_prep_h can pull the leader prep shares inside its XOF (the query reads them only after the
  // same lane's XOF): 16-byte pieces over the B - 1 iterations of the share loop, whole waves only
  // (the executor pads its groups to 64 columns for these instances).
  p.pull_in_xof = pulling && fused_h && dp.prep_share_len % 16 == 0 &&
                  dp.prep_share_len / 16 <= 2 * (jr_share_blocks(dp.meas_len) - 1) && n % 64 == 0;
  // small Histogram runs (the executor's groups) on lane pairs: twice the waves, half the work each
  if (fused_h && e->pair_max > 0 && n != 0 && n <= (uint32_t)e->pair_max) {
    DevParams d = dp;
    d.n = n;
    p.pair = prep_pair_takes(d, p.pull_in_xof);
  }
  p.redo_list = fused_h && !p.pair;
  // Option "chunks" > 1 (auto: one chunk per 128Ki reports on the two-kernel chain, measured best
  // on MI355X at 1Mi reports: 8 chunks +4-5% over 1; 16: slower); one launch for the fused kernels
  // (A/B on MI355X, 1 Mi reports: 169.9 M/s at 1 chunk vs 163.2 M/s at 8) and for the one-kernel
  // multiproof prepare (1 M reports: 93.1-93.3 M/s at 1 chunk vs 89.0-91.5 at 8, r04e2)
  const bool one_launch = fused_h || p.chain == PrepChain::FUSED_SUM || p.chain == PrepChain::MP64;
  const uint32_t K = e->chunks > 0 ? (uint32_t)e->chunks
                     : one_launch  ? 1u
                                   : std::max(1u, (n + (1u << 16)) >> 17);
  p.chunk_cols = ((n + K - 1) / K + 255) & ~255u;
  p.chunks = p.pair || p.pull_in_xof || K == 1 || n <= p.chunk_cols ||
                     p.chain == PrepChain::FPVEC
                 ? 1u
                 : (n + p.chunk_cols - 1) / p.chunk_cols;
  return p;
}

// side streams + their join events and the fork event, created once per engine
static int ensure_side_streams(prio3_engine* e) {
  while (e->side.size() < 2) {
    hipStream_t s2;
    hipEvent_t j;
    HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&j, hipEventDisableTiming));
    e->side.push_back(s2);
    e->side_ev.push_back(j);
  }
  if (!e->fork_ev) HIPCHK(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
  return PRIO3_OK;
}

constexpr uint32_t REDO_LIST_BLOCKS = 32;
// The plan's chain over columns [c0, c0 + n) of the run.  Where the plan defers the slow path
// (slow_defer), the caller ends the run with launch_slow_redo.
// plan.pull_in_xof: the leader prep shares are still in the mapped host staging (in.leader_src)
// and the fused k_prep_h<.., PULL> copies them lane by lane during its XOF.
static int launch_prepare(prio3_engine* e, const PrepPlan& plan, const DevParams& base,
                          uint32_t c0, uint32_t n, InPtrs in, OutPtrs out, Scratch sc,
                          hipStream_t st, bool fuse) {
  DevParams dp = base;
  dp.n = n;
  dp.force_slow = (uint32_t)e->force_slow;
  dp.trunc_xof = plan.trunc_xof;
  dp.slow_defer = plan.slow_defer;
  dp.redo = 0;
  const size_t es = dp.es;
  in.nonces += 16 * (size_t)c0;
  if (in.pub) in.pub += (size_t)dp.public_share_len * c0;
  in.helper += (size_t)dp.helper_share_len * c0;
  in.leader += (size_t)dp.prep_share_len * c0;
  if (in.vk_slot) in.vk_slot += c0;
  out.prep_msgs += (size_t)(dp.kind == PRIO3_SUMVEC_F64_MP ? 32 : 16) * c0;
  out.status += c0;
  void** soa[] = {&sc.meas, &sc.proofs, &sc.jr, &sc.qr, &sc.Lbuf, &sc.PVbuf, &sc.acc, &sc.out,
                  &sc.beta};
  for (auto q : soa)
    if (*q) *q = (uint8_t*)*q + es * c0;
  sc.part += c0;
  sc.corrected += c0;
  sc.flag += c0;
  if (sc.seg) sc.seg += c0;
  if (sc.wseg) sc.wseg += c0 / 64;
  if (sc.wpart) sc.wpart += (size_t)(c0 / 64) * dp.meas_len * 8;
  sc.redo_c0 = c0;
  const uint32_t blocks = (n + 255) / 256;
  const uint32_t xblocks = (n + XOFD_BLOCK - 1) / XOFD_BLOCK;  // k_prep_h, k_xofd
  if (plan.chain == PrepChain::MP64) {
    int rc = PRIO3_OK;
    TIMED(e, st, "k_mp64_prepare", (rc = launch_mp64(e, n, dp.ld, in, out, sc, st)));
    return rc;
  }
  if (plan.chain == PrepChain::FPVEC) {
    // Sub-batches of dp.ld reports through the per-report scratch (the whole batch's meas
    // shares would not fit: 2.56 MB per report at 10^4 entries); output shares keep one
    // column per report of the batch (ld_out), so accumulate runs once over all of them.
    // Equal sub-batches, cut at whole query rounds (fp_sub_sizes): per-lane latency, not lane
    // count, sets a launch's duration.
    uint32_t nsub, sub;
    const bool qwide = plan.query == QueryKernel::FPW;
    fp_sub_sizes(e, n, dp.ld, qwide, nsub, sub);
    for (uint32_t si = 0; si < nsub; si++) {
      const uint32_t s0 = si * sub;
      DevParams q = dp;
      q.n = si + 1 < nsub ? sub : n - s0;
      InPtrs qi = in;
      qi.nonces += 16 * (size_t)s0;
      qi.pub += (size_t)dp.public_share_len * s0;
      qi.helper += (size_t)dp.helper_share_len * s0;
      qi.leader += (size_t)dp.prep_share_len * s0;
      if (qi.vk_slot) qi.vk_slot += s0;
      OutPtrs qo = out;
      qo.prep_msgs += 16 * (size_t)s0;
      qo.status += s0;
      Scratch qs = sc;
      qs.out = (uint8_t*)sc.out + es * s0;
      const uint32_t qb = (q.n + 255) / 256;
      bool paired = false;
      if (plan.xof == XofKernel::PAIR)
        TIMED(e, st, "k_xof_pair", (paired = launch_xof_pair(q, qi, qs, st)));
      if (!paired && plan.dual)
        TIMED(e, st, "k_xofd",
              (k_xofd<false, true><<<(q.n + XOFD_BLOCK - 1) / XOFD_BLOCK, XOFD_BLOCK, 0, st>>>(
                  q, qi, qs)));
      else if (!paired)  // one-block share: no valid FPVec instance (kept as found, untested)
        TIMED(e, st, "k_xof", (k_xof<Fp128><<<qb, 256, 0, st>>>(q, qi, qs)));
      TIMED(e, st, "k_xof_slow", launch_xof_slow<Fp128>(e, q, qi, qs, st));
      if (qwide)
        TIMED(e, st, "k_query_fpw", launch_fpvec_query(q, qi, qs, qo, st, true, false));
      else
        TIMED(e, st, "k_query_fp", launch_fpvec_query(q, qi, qs, qo, st, false, false));
    }
    return PRIO3_OK;
  }
  if (plan.chain == PrepChain::GEN64) {
    TIMED(e, st, "k_prep_gen", (k_prep_gen<Fp64><<<blocks, 256, 0, st>>>(dp, in, sc, out)));
  } else if (plan.chain == PrepChain::FUSED_SUM) {
    TIMED(e, st, "k_prep_sum", (with_value<16, 32, 64, 128>(dp.P, [&](auto p) {
            k_prep_sum<decltype(p)::value / 16><<<blocks, 256, 0, st>>>(dp, in, sc, out);
          })));
  } else if (plan.chain == PrepChain::FUSED_H) {
    bool paired = false;
    if (plan.pair) {
      // no list on lane pairs, nor for k_prep_h should launch_prep_pair decline (it listed before
      // the plan; unreachable: the plan asked prep_pair_takes the same question): the redo scans
      sc.redo_cnt = nullptr;
      TIMED(e, st, "k_prep_hp",
            (paired = launch_prep_pair(dp, in, sc, out, st, fuse, plan.pull_in_xof)));
    }
    if (!paired)
      TIMED(e, st, "k_prep_h", (with_value<1, 0>(fuse, [&](auto f) {
              with_value<1, 0>(plan.pull_in_xof, [&](auto pl) {
                k_prep_h<decltype(f)::value != 0, decltype(pl)::value != 0>
                    <<<xblocks, XOFD_BLOCK, 0, st>>>(dp, in, sc, out);
              });
            })));
  } else {
    if (plan.xof == XofKernel::XOFD) {
      if (fuse)
        TIMED(e, st, "k_xofd", (k_xofd<true><<<xblocks, XOFD_BLOCK, 0, st>>>(dp, in, sc)));
      else if (plan.trunc_xof)
        TIMED(e, st, "k_xofd", (k_xofd<false, true><<<xblocks, XOFD_BLOCK, 0, st>>>(dp, in, sc)));
      else
        TIMED(e, st, "k_xofd", (k_xofd<false><<<xblocks, XOFD_BLOCK, 0, st>>>(dp, in, sc)));
    } else {
      TIMED(e, st, "k_xof_a", (k_xof_a<Fp128><<<blocks, 256, 0, st>>>(dp, in, sc)));
      TIMED(e, st, "k_jrpart", (k_jrpart<false><<<blocks, 256, 0, st>>>(dp, in, sc)));
    }
    if (!plan.slow_defer) TIMED(e, st, "k_xof_slow", launch_xof_slow<Fp128>(e, dp, in, sc, st));
    // the queries with a launch_* of their own return false for an instance they do not take:
    // k_query_ps then stands in for k_query_w, k_query for k_query_sum
    bool done = false;
    if (plan.query == QueryKernel::WIDE)
      TIMED(e, st, "k_query_w", (done = launch_query_wide(dp, in, sc, out, st)));
    else if (plan.query == QueryKernel::SUM)
      TIMED(e, st, "k_query_sum", (done = launch_query_sum(dp, in, sc, out, st)));
    if (done) {
    } else if (plan.query == QueryKernel::H)
      TIMED(e, st, "k_query_h", (with_value<32, 16, 8>(dp.P, [&](auto pp) {
              k_query_h<2, decltype(pp)::value><<<blocks, 256, 0, st>>>(dp, in, sc, out);
            })));
    else if (plan.query == QueryKernel::WIDE || plan.query == QueryKernel::PS)
      TIMED(e, st, "k_query_ps", (k_query_ps<4><<<blocks, 256, 0, st>>>(dp, in, sc, out)));
    else
      TIMED(e, st, "k_query", (k_query<Fp128><<<blocks, 256, 0, st>>>(dp, in, sc, out)));
  }
  return PRIO3_OK;
}

// The run's one redo launch (plan.redo).  R (nullable): the run, whose fused-aggregate
// accumulators the k_slow_redo<PP> launch zeroes.
static int launch_slow_redo(prio3_engine* e, const PrepPlan& plan, const DevParams& base,
                            uint32_t n, InPtrs in, OutPtrs out, Scratch sc, hipStream_t st,
                            Run* R) {
  const bool list = plan.redo_list && sc.redo_cnt;
  if (!list) sc.redo_cnt = nullptr;  // (the pair kernel and k_query_h list nothing)
  const bool clean = R && R->agg64 && plan.redo == RedoFamily::QH;
  const ZeroRanges z = clean ? fused_first_zero(R) : ZeroRanges{};
  DevParams dp = base;
  dp.n = n;
  dp.force_slow = (uint32_t)e->force_slow;
  dp.trunc_xof = 0;
  dp.slow_defer = 1;
  dp.redo = 1;
  const uint32_t g = list ? REDO_LIST_BLOCKS : redo_blocks(n);
  if (plan.redo == RedoFamily::GEN64)  // k_prep_gen<Fp64>: XOF redo, then the generic query
    TIMED(e, st, "k_slow_redo", (k_slow_redo_gen<Fp64><<<g, 64, 0, st>>>(dp, in, sc, out)));
  else if (plan.redo == RedoFamily::SUM)
    TIMED(e, st, "k_slow_redo", (with_value<16, 32, 64, 128>(dp.P, [&](auto p) {
            k_slow_redo_sum<decltype(p)::value / 16><<<g, 64, 0, st>>>(dp, in, sc, out);
          })));
  else
    TIMED(e, st, "k_slow_redo", (with_value<32, 16, 8>(dp.P, [&](auto pp) {
            k_slow_redo<decltype(pp)::value><<<g, 64, 0, st>>>(dp, in, sc, out, z);
          })));
  if (clean) {
    R->fclean = true;
    R->fgen = 0;
  }
  return PRIO3_OK;
}

// The kernel chain over the whole run.  Option "chunks" > 1 (auto: one chunk per 128Ki reports,
// measured best on MI355X at 1Mi reports: 8 chunks +4-5% over 1; 16: slower): the batch is cut
// into column ranges whose chains alternate over the engine's two side streams (joined to `st`
// before and after), so one chunk's memory-bound query overlaps the next chunk's VALU-bound
// Keccak.  Side streams are per engine: callers that may overlap (the executor's concurrent
// groups) pass allow_chunks = false.
// pull (nullable; executor groups): copies the leader prep shares (and the fix-up inputs) from
// the mapped host staging into the run -- inside the fused XOF + query launch where the chain is
// k_prep_h (plan.pull_in_xof), else by one copy launch ahead of the chain.
int prepare_run(prio3_engine* e, Run* R, InPtrs in, OutPtrs out, hipStream_t st, bool fuse,
                bool allow_chunks, const PullRanges* pull) {
  const uint32_t n = R->n;
  const PrepPlan plan = plan_prepare(e, R->dp, n, fuse, pull != nullptr);
  if (plan.pull_in_xof) {
    in.leader_src = pull->src[0];
    in.seg_src = (const uint32_t*)pull->src[1];
    in.seg_dst = (uint32_t*)pull->dst[1];
    in.accept_src = pull->src[2];
    in.accept_dst = pull->dst[2];
  } else if (pull) {
    if (!launch_pull(*pull, 256, st)) return PRIO3_EDEVICE;
  }
  Scratch sc = R->sc;
  sc.seg = R->seg;
  sc.wpart = R->wpart;
  sc.wseg = R->wseg;
  // k_prep_h chains list their flagged reports for the redo launch (in the stream's zero words)
  // and hold the stream's mutex until the redo launch is enqueued
  std::unique_lock<std::mutex> zlock;
  if (R->redo_list && plan.chain == PrepChain::FUSED_H) {
    std::mutex* zmu = nullptr;
    if (uint32_t* zw = stream_zero_words(R->device, st, &zmu)) {
      zlock = std::unique_lock<std::mutex>(*zmu);
      sc.redo_cnt = zw + 1;
      sc.redo_list = R->redo_list;
    }
  }
  R->last = st;
  R->wshift = plan.pair ? 5u : 6u;
  if (!allow_chunks || plan.chunks == 1) {
    const int rc = launch_prepare(e, plan, R->dp, 0, n, in, out, sc, st, fuse);
    if (rc == PRIO3_OK && plan.redo != RedoFamily::NONE)
      return launch_slow_redo(e, plan, R->dp, n, in, out, sc, st, R);
    return rc;
  }
  int rc = ensure_side_streams(e);
  if (rc) return rc;
  HIPCHK(hipEventRecord(e->fork_ev, st));
  for (auto s2 : e->side) HIPCHK(hipStreamWaitEvent(s2, e->fork_ev, 0));
  const uint32_t csz = plan.chunk_cols;
  uint32_t c = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += csz, c++) {
    rc = launch_prepare(e, plan, R->dp, c0, std::min(csz, n - c0), in, out, sc, e->side[c % 2],
                        fuse);
    if (rc) return rc;
  }
  for (size_t i = 0; i < e->side.size(); i++) {
    HIPCHK(hipEventRecord(e->side_ev[i], e->side[i]));
    HIPCHK(hipStreamWaitEvent(st, e->side_ev[i], 0));
  }
  if (plan.redo != RedoFamily::NONE) return launch_slow_redo(e, plan, R->dp, n, in, out, sc, st, R);
  return PRIO3_OK;
}

// FPVec leader (agg_id 0): sub-batches of the run's ld columns, each through the helper's
// kernels in their leader role -- k_leader_unpack (explicit share -> SoA, canonical check, both
// query points), k_jrpart<false, true> (the leader's joint-rand part over its 2.56 MB share,
// corrected seed, joint randomness), k_leader_slowfix, k_query_fpw<GS, LEADER> (verifier share,
// the decoded entries as output shares) -- and the corrected seeds saved for prepare_next.
static int leader_init_fpvec(prio3_engine* e, Run* R, const uint8_t* d_nonces,
                             const uint8_t* d_pub, const uint8_t* d_lin, uint8_t* d_prep_shares,
                             uint8_t* d_status, hipStream_t st) {
  DevParams dp = R->dp;
  dp.force_slow = (uint32_t)e->force_slow;
  dp.trunc_xof = 0;
  if (!fpvec_query_wide_takes(dp) || !R->corr_all) return PRIO3_EUNSUPPORTED;
  const uint32_t n = R->n, cap = dp.ld;
  uint32_t nsub, sub;
  fp_sub_sizes(e, n, cap, true, nsub, sub);
  const size_t es = dp.es;
  for (uint32_t si = 0; si < nsub; si++) {
    const uint32_t s0 = si * sub;
    DevParams q = dp;
    q.n = si + 1 < nsub ? sub : n - s0;
    InPtrs qi{d_nonces + 16 * (size_t)s0,
              d_pub ? d_pub + (size_t)dp.public_share_len * s0 : nullptr,
              d_lin + (size_t)dp.leader_share_len * s0, nullptr};
    OutPtrs qo{d_prep_shares + (size_t)dp.prep_share_len * s0, d_status + s0};
    Scratch qs = R->sc;
    qs.out = (uint8_t*)R->sc.out + es * s0;
    const uint32_t blocks = (q.n + 255) / 256, blocks64 = (q.n + 63) / 64;
    TIMED(e, st, "k_leader_unpack",
          (k_leader_unpack<<<(q.n + 63) / 64, 256, 0, st>>>(q, qi, qs, qo.status, nullptr, nullptr)));
    TIMED(e, st, "k_jrpart", (k_jrpart<false, true><<<blocks, 256, 0, st>>>(q, qi, qs)));
    TIMED(e, st, "k_leader_slowfix", (k_leader_slowfix<<<blocks64, 64, 0, st>>>(q, qi, qs)));
    TIMED(e, st, "k_query_fpw", launch_fpvec_query(q, qi, qs, qo, st, true, true));
    HIPCHK(hipMemcpyAsync(R->corr_all + s0, qs.corrected, 16 * (size_t)q.n,
                          hipMemcpyDeviceToDevice, st));
  }
  return PRIO3_OK;
}

// The one statement of which kernels the leader's prepare_init takes.
LeaderPlan plan_leader(const prio3_engine* e) {
  const DevParams& d = e->dp;
  LeaderPlan p{};
  // the helper kernels in their leader role: one k_leader_prep launch
  const bool prep = e->leader_fast && (d.kind == PRIO3_HISTOGRAM || d.kind == PRIO3_SUMVEC) &&
                    d.jr_len && (d.P == 32 || d.P == 16 || d.P == 8);
  const bool sum = d.kind == PRIO3_SUM && e->leader_fast && query_sum_takes(d);
  p.chain = d.kind == PRIO3_FPVEC_BOUNDED_L2 ? LeaderChain::FPVEC
            : d.kind == PRIO3_SUMVEC_F64_MP  ? LeaderChain::MP64
            : prep                           ? LeaderChain::K_LEADER_PREP
            : sum                            ? LeaderChain::SUM
                                             : LeaderChain::GENERIC;
  // k_leader_prep is the only leader kernel that reads the input shares from SoA staging
  // (InPtrs::lin_ld); the staging takes that form only for a share without trailing bytes
  p.soa_staging = prep && d.leader_share_len == 16 * (d.meas_len + d.proof_len + 1);
  // Device leader init with the accumulate fused into k_leader_prep (option leader_fuse_acc):
  // Histogram, whose output share is the measurement share that leader_jr_body streams through
  p.fuse_acc = e->leader_fuse_acc && prep && d.kind == PRIO3_HISTOGRAM && d.es == 16;
  return p;
}

// vk_slot / vk_tab (nullable): per-report verify keys of a coalesced group of several tasks
int leader_init_run(prio3_engine* e, Run* R, const uint8_t* d_nonces,
                    const uint8_t* d_public_shares, const uint8_t* d_leader_input_shares,
                    uint8_t* d_prep_shares, uint8_t* d_status, hipStream_t st,
                    const uint16_t* vk_slot, const uint4* vk_tab, uint32_t lin_ld) {
  const LeaderPlan plan = plan_leader(e);
  DevParams dp = R->dp;
  dp.force_slow = (uint32_t)e->force_slow;
  const uint32_t n = R->n;
  R->last = st;
  InPtrs in{d_nonces, d_public_shares, d_leader_input_shares, nullptr};
  OutPtrs out{d_prep_shares, d_status};
  int rc = PRIO3_OK;
  switch (plan.chain) {
    case LeaderChain::FPVEC:
      return leader_init_fpvec(e, R, d_nonces, d_public_shares, d_leader_input_shares,
                               d_prep_shares, d_status, st);
    case LeaderChain::MP64:
      TIMED(e, st, "k_mp64_prepare", (rc = launch_mp64_leader(e, n, dp.ld, in, out, R->sc, st)));
      return rc;
    case LeaderChain::GENERIC:
      TIMED(e, st, "k_leader_init",
            rc = launch_leader_init(dp, d_nonces, d_public_shares, d_leader_input_shares, R->sc,
                                    d_prep_shares, d_status, st, vk_slot, vk_tab));
      return rc;
    default: break;
  }
  in.vk_slot = vk_slot;
  in.vk_tab = vk_tab;
  const uint32_t blocks = (n + 255) / 256, blocks64 = (n + 63) / 64;
  if (plan.chain == LeaderChain::K_LEADER_PREP) {
    in.lin_ld = lin_ld;
    // R->lfused: the wave partials of the share for segment 0, fixed up at accumulate
    uint32_t* wp = R->lfused ? R->wpart : nullptr;
    uint32_t* wsg = R->lfused ? R->wseg : nullptr;
    // one launch; flagged reports redone after k_leader_slowfix
    DevParams d1 = dp;
    d1.slow_defer = 1;
    TIMED(e, st, "k_leader_prep", (with_value<32, 16, 8>(dp.P, [&](auto pp) {
            k_leader_prep<decltype(pp)::value><<<blocks, 256, 0, st>>>(d1, in, R->sc, out, wp, wsg);
          })));
    dp.redo = 1;
    TIMED(e, st, "k_leader_slowfix", (k_leader_slowfix<<<blocks64, 64, 0, st>>>(dp, in, R->sc)));
    TIMED(e, st, "k_query_h", (with_value<32, 16, 8>(dp.P, [&](auto pp) {
            k_query_h<2, decltype(pp)::value, 1><<<blocks, 256, 0, st>>>(dp, in, R->sc, out);
          })));
    return PRIO3_OK;
  }
  // Prio3Sum: the same unpack / joint-rand kernels, then k_query_sum in its leader role
  // (leader_jr_body's per-lane row streaming loses here: the short share leaves little Keccak
  // to hide the 1.6 KB rows' uncoalesced reads -- 2.63 against 1.30 + 0.46 ms per 1.25 M)
  TIMED(e, st, "k_leader_unpack",
        (k_leader_unpack<<<blocks64, 256, 0, st>>>(dp, in, R->sc, d_status, nullptr, nullptr)));
  TIMED(e, st, "k_jrpart", (k_jrpart<false, true><<<blocks, 256, 0, st>>>(dp, in, R->sc)));
  TIMED(e, st, "k_leader_slowfix", (k_leader_slowfix<<<blocks64, 64, 0, st>>>(dp, in, R->sc)));
  bool ok = false;
  TIMED(e, st, "k_query_sum", (ok = launch_query_sum(dp, in, R->sc, out, st, true)));
  return ok ? PRIO3_OK : PRIO3_EDEVICE;
}

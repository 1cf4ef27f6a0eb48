// hpke_device.h -- the device code the HPKE open (hpke.hip) and seal (hpke_seal.hip) kernels
// share: GF(2^255 - 19) and the X25519 ladders, GHASH, ChaCha20 and Poly1305, the suite
// parameters of one opener / sealer (HpkeParams) and the RFC 9180 key schedule.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "prio3_device.h"
#include "sha256_device.h"
#include "sha512_device.h"
#include "ghash_device.h"

// -------------------------------------------------------------------------------------
// GF(2^255 - 19), values in [0, 2^256) (loosely reduced), 8 little-endian 32-bit limbs
// -------------------------------------------------------------------------------------
struct fe {
  uint32_t v[8];
};

DEV fe fe_set(uint32_t x) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = i ? 0u : x;
  return r;
}

#ifndef FE_ASM
#define FE_ASM 1  // 1: the generated single-asm-statement field routines (fe25519_asm.h)
#endif
#if FE_ASM
#include "fe25519_asm.h"
#else
// r = lo + 38 * c (c small), folded twice so the result is < 2^256
DEV void fe_fold(uint32_t r[8], uint32_t c) {
  uint32_t cy;
  r[0] = addc(r[0], c * 38u, 0, &cy);
#pragma unroll
  for (int i = 1; i < 8; i++) r[i] = addc(r[i], 0, cy, &cy);
  r[0] = addc(r[0], cy * 38u, 0, &cy);  // second carry leaves r < 76: no further carry
}

DEV fe fe_add(const fe& a, const fe& b) {
  fe r;
  uint32_t cy;
  r.v[0] = addc(a.v[0], b.v[0], 0, &cy);
#pragma unroll
  for (int i = 1; i < 8; i++) r.v[i] = addc(a.v[i], b.v[i], cy, &cy);
  fe_fold(r.v, cy);
  return r;
}

// a - b: a wrap adds 2^256 = 38 (mod p), compensated by subtracting 38 (twice at most)
DEV fe fe_sub(const fe& a, const fe& b) {
  fe r;
  uint32_t bw;
  r.v[0] = subb(a.v[0], b.v[0], 0, &bw);
#pragma unroll
  for (int i = 1; i < 8; i++) r.v[i] = subb(a.v[i], b.v[i], bw, &bw);
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    r.v[0] = subb(r.v[0], bw * 38u, 0, &bw);
#pragma unroll
    for (int i = 1; i < 8; i++) r.v[i] = subb(r.v[i], 0, bw, &bw);
  }
  return r;
}

// X = sum_k c[k] 2^(32k) + sum_k h[k] 2^(32(k+2)) -> 16 words, then reduce (2^256 = 38)
DEV fe fe_reduce512(const uint32_t w[16]) {
  fe r;
  uint32_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)w[8 + i] * 38u + w[i] + cy;
    r.v[i] = (uint32_t)t;
    cy = (uint32_t)(t >> 32);
  }
  fe_fold(r.v, cy);
  return r;
}

DEV void fe_normalize(const uint64_t c[15], const uint32_t h[14], uint32_t w[16]) {
  uint32_t cy;
#pragma unroll
  for (int k = 0; k < 15; k += 2) {  // even columns: a plain concatenation
    w[k] = (uint32_t)c[k];
    w[k + 1] = (uint32_t)(c[k] >> 32);
  }
  // + odd columns: c[k] (k odd) at words k, k+1
  w[1] = addc(w[1], (uint32_t)c[1], 0, &cy);
  w[2] = addc(w[2], (uint32_t)(c[1] >> 32), cy, &cy);
#pragma unroll
  for (int k = 3; k < 14; k += 2) {
    w[k] = addc(w[k], (uint32_t)c[k], cy, &cy);
    w[k + 1] = addc(w[k + 1], (uint32_t)(c[k] >> 32), cy, &cy);
  }
  w[15] = addc(w[15], 0, cy, &cy);
  // + overflow words: h[k] at word k + 2
  w[3] = addc(w[3], h[1], 0, &cy);
#pragma unroll
  for (int k = 2; k < 14; k++) w[k + 2] = addc(w[k + 2], h[k], cy, &cy);
}

DEV fe fe_mul(const fe& a, const fe& b) {
  uint64_t c[15];
  uint32_t h[14];
#pragma unroll
  for (int k = 0; k < 15; k++) c[k] = 0;
#pragma unroll
  for (int k = 0; k < 14; k++) h[k] = 0;
  asm(
            "v_mad_u64_u32 %0, vcc, %28, %36, %0\n\t"
      "v_mad_u64_u32 %1, vcc, %28, %37, %1\n\t"
      "v_addc_co_u32 %15, vcc, 0, %15, vcc\n\t"
      "v_mad_u64_u32 %2, vcc, %28, %38, %2\n\t"
      "v_addc_co_u32 %16, vcc, 0, %16, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %28, %39, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %28, %40, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %28, %41, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %28, %42, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %28, %43, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %1, vcc, %29, %36, %1\n\t"
      "v_addc_co_u32 %15, vcc, 0, %15, vcc\n\t"
      "v_mad_u64_u32 %2, vcc, %29, %37, %2\n\t"
      "v_addc_co_u32 %16, vcc, 0, %16, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %29, %38, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %29, %39, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %29, %40, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %29, %41, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %29, %42, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %29, %43, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %2, vcc, %30, %36, %2\n\t"
      "v_addc_co_u32 %16, vcc, 0, %16, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %30, %37, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %30, %38, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %30, %39, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %30, %40, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %30, %41, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %30, %42, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %30, %43, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %31, %36, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %31, %37, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %31, %38, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %31, %39, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %31, %40, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %31, %41, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %31, %42, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %31, %43, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %32, %36, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %32, %37, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %32, %38, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %32, %39, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %32, %40, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %32, %41, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %32, %42, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %32, %43, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %33, %36, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %33, %37, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %33, %38, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %33, %39, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %33, %40, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %33, %41, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %33, %42, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %12, vcc, %33, %43, %12\n\t"
      "v_addc_co_u32 %26, vcc, 0, %26, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %34, %36, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %34, %37, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %34, %38, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %34, %39, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %34, %40, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %34, %41, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %12, vcc, %34, %42, %12\n\t"
      "v_addc_co_u32 %26, vcc, 0, %26, vcc\n\t"
      "v_mad_u64_u32 %13, vcc, %34, %43, %13\n\t"
      "v_addc_co_u32 %27, vcc, 0, %27, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %35, %36, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %35, %37, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %35, %38, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %35, %39, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %35, %40, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %12, vcc, %35, %41, %12\n\t"
      "v_addc_co_u32 %26, vcc, 0, %26, vcc\n\t"
      "v_mad_u64_u32 %13, vcc, %35, %42, %13\n\t"
      "v_addc_co_u32 %27, vcc, 0, %27, vcc\n\t"
      "v_mad_u64_u32 %14, vcc, %35, %43, %14\n\t"
      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]),
        "+v"(c[7]), "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]),
        "+v"(c[14]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(h[4]), "+v"(h[5]), "+v"(h[6]),
        "+v"(h[7]), "+v"(h[8]), "+v"(h[9]), "+v"(h[10]), "+v"(h[11]), "+v"(h[12]), "+v"(h[13])
      : "v"(a.v[0]), "v"(a.v[1]), "v"(a.v[2]), "v"(a.v[3]), "v"(a.v[4]), "v"(a.v[5]),
        "v"(a.v[6]), "v"(a.v[7]), "v"(b.v[0]), "v"(b.v[1]), "v"(b.v[2]), "v"(b.v[3]),
        "v"(b.v[4]), "v"(b.v[5]), "v"(b.v[6]), "v"(b.v[7])
      : "vcc");
  uint32_t w[16];
  fe_normalize(c, h, w);
  return fe_reduce512(w);
}

DEV fe fe_sqr(const fe& a) {
  uint64_t c[15];
  uint32_t h[14];
#pragma unroll
  for (int k = 0; k < 15; k++) c[k] = 0;
#pragma unroll
  for (int k = 0; k < 14; k++) h[k] = 0;
  asm(
            "v_mad_u64_u32 %1, vcc, %28, %29, %1\n\t"
      "v_addc_co_u32 %15, vcc, 0, %15, vcc\n\t"
      "v_mad_u64_u32 %2, vcc, %28, %30, %2\n\t"
      "v_addc_co_u32 %16, vcc, 0, %16, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %28, %31, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %28, %32, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %28, %33, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %28, %34, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %28, %35, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %29, %30, %3\n\t"
      "v_addc_co_u32 %17, vcc, 0, %17, vcc\n\t"
      "v_mad_u64_u32 %4, vcc, %29, %31, %4\n\t"
      "v_addc_co_u32 %18, vcc, 0, %18, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %29, %32, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %29, %33, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %29, %34, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %29, %35, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %5, vcc, %30, %31, %5\n\t"
      "v_addc_co_u32 %19, vcc, 0, %19, vcc\n\t"
      "v_mad_u64_u32 %6, vcc, %30, %32, %6\n\t"
      "v_addc_co_u32 %20, vcc, 0, %20, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %30, %33, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %30, %34, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %30, %35, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %7, vcc, %31, %32, %7\n\t"
      "v_addc_co_u32 %21, vcc, 0, %21, vcc\n\t"
      "v_mad_u64_u32 %8, vcc, %31, %33, %8\n\t"
      "v_addc_co_u32 %22, vcc, 0, %22, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %31, %34, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %31, %35, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %9, vcc, %32, %33, %9\n\t"
      "v_addc_co_u32 %23, vcc, 0, %23, vcc\n\t"
      "v_mad_u64_u32 %10, vcc, %32, %34, %10\n\t"
      "v_addc_co_u32 %24, vcc, 0, %24, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %32, %35, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %11, vcc, %33, %34, %11\n\t"
      "v_addc_co_u32 %25, vcc, 0, %25, vcc\n\t"
      "v_mad_u64_u32 %12, vcc, %33, %35, %12\n\t"
      "v_addc_co_u32 %26, vcc, 0, %26, vcc\n\t"
      "v_mad_u64_u32 %13, vcc, %34, %35, %13\n\t"
      "v_addc_co_u32 %27, vcc, 0, %27, vcc\n\t"

      : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]),
        "+v"(c[7]), "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]),
        "+v"(c[14]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(h[4]), "+v"(h[5]), "+v"(h[6]),
        "+v"(h[7]), "+v"(h[8]), "+v"(h[9]), "+v"(h[10]), "+v"(h[11]), "+v"(h[12]), "+v"(h[13])
      : "v"(a.v[0]), "v"(a.v[1]), "v"(a.v[2]), "v"(a.v[3]), "v"(a.v[4]), "v"(a.v[5]),
        "v"(a.v[6]), "v"(a.v[7])
      : "vcc");
  uint32_t w[16], d[16];
  fe_normalize(c, h, w);  // off-diagonal sum S
  // 2S (S < 2^511) + D, D = sum a_i^2 2^(64 i) (non-overlapping 64-bit products)
#pragma unroll
  for (int i = 15; i > 0; i--) w[i] = __builtin_amdgcn_alignbit(w[i], w[i - 1], 31);
  w[0] <<= 1;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t q = (uint64_t)a.v[i] * a.v[i];
    d[2 * i] = (uint32_t)q;
    d[2 * i + 1] = (uint32_t)(q >> 32);
  }
  uint32_t cy;
  w[0] = addc(w[0], d[0], 0, &cy);
#pragma unroll
  for (int i = 1; i < 16; i++) w[i] = addc(w[i], d[i], cy, &cy);
  return fe_reduce512(w);
}

DEV fe fe_mul121665(const fe& a) {
  fe r;
  uint32_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a.v[i] * 121665u + cy;
    r.v[i] = (uint32_t)t;
    cy = (uint32_t)(t >> 32);
  }
  fe_fold(r.v, cy);
  return r;
}

#endif

DEV fe fe_sqr_n(fe a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) a = fe_sqr(a);
  return a;
}

// z^(p - 2) (the ref10 addition chain: 254 squarings, 11 multiplications)
DEV fe fe_inv(const fe& z) {
  const fe z2 = fe_sqr(z);
  const fe z9 = fe_mul(fe_sqr_n(z2, 2), z);
  const fe z11 = fe_mul(z9, z2);
  const fe z5_0 = fe_mul(fe_sqr(z11), z9);
  const fe z10_0 = fe_mul(fe_sqr_n(z5_0, 5), z5_0);
  const fe z20_0 = fe_mul(fe_sqr_n(z10_0, 10), z10_0);
  const fe z40_0 = fe_mul(fe_sqr_n(z20_0, 20), z20_0);
  const fe z50_0 = fe_mul(fe_sqr_n(z40_0, 10), z10_0);
  const fe z100_0 = fe_mul(fe_sqr_n(z50_0, 50), z50_0);
  const fe z200_0 = fe_mul(fe_sqr_n(z100_0, 100), z100_0);
  const fe z250_0 = fe_mul(fe_sqr_n(z200_0, 50), z50_0);
  return fe_mul(fe_sqr_n(z250_0, 5), z11);
}

// canonical representative in [0, p): at most two subtractions of p (values < 2^256 = 2p + 38)
DEV fe fe_freeze(fe a) {
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    fe t;
    uint32_t bw;
    t.v[0] = subb(a.v[0], 0xffffffedu, 0, &bw);
#pragma unroll
    for (int i = 1; i < 7; i++) t.v[i] = subb(a.v[i], 0xffffffffu, bw, &bw);
    t.v[7] = subb(a.v[7], 0x7fffffffu, bw, &bw);
#pragma unroll
    for (int i = 0; i < 8; i++) a.v[i] = bw ? a.v[i] : t.v[i];
  }
  return a;
}

DEV void fe_cswap(bool swap, fe& a, fe& b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t x = a.v[i], y = b.v[i];
    a.v[i] = swap ? y : x;
    b.v[i] = swap ? x : y;
  }
}

// X25519(k, u) (RFC 7748 section 5); k = the clamped scalar (LE words, wave-uniform)
DEV fe x25519_ladder(const uint32_t* k, const fe& u) {
  const fe x1 = u;
  fe x2 = fe_set(1), z2 = fe_set(0), x3 = u, z3 = fe_set(1);
  bool swap = false;
#pragma unroll 1
  for (int t = 254; t >= 0; t--) {
    const bool kt = (k[t >> 5] >> (t & 31)) & 1u;
    swap ^= kt;
    fe_cswap(swap, x2, x3);
    fe_cswap(swap, z2, z3);
    swap = kt;
    const fe A = fe_add(x2, z2), B = fe_sub(x2, z2);
    const fe AA = fe_sqr(A), BB = fe_sqr(B);
    const fe E = fe_sub(AA, BB);
    const fe C = fe_add(x3, z3), D = fe_sub(x3, z3);
    const fe DA = fe_mul(D, A), CB = fe_mul(C, B);
    x3 = fe_sqr(fe_add(DA, CB));
    z3 = fe_mul(x1, fe_sqr(fe_sub(DA, CB)));
    x2 = fe_mul(AA, BB);
    z2 = fe_mul(E, fe_add(AA, fe_mul121665(E)));
  }
  fe_cswap(swap, x2, x3);
  fe_cswap(swap, z2, z3);
  return fe_freeze(fe_mul(x2, fe_inv(z2)));
}

// The same ladder on a lane pair (both lanes hold the whole state; `odd` = the pair's second lane):
// per step each lane runs one square and one product of the first stage (lane 0: AA = A^2,
// DA = D A; lane 1: BB = B^2, CB = C B), they swap them by DPP, then three products of the
// second stage (lane 0: x2 = AA BB, z2 = E (AA + a24 E); lane 1: x3 = (DA + CB)^2,
// t = (DA - CB)^2, z3 = x1 t) and swap again -- 1S + 4M per lane instead of 4S + 5M, so a small
// group's open (one wave per SIMD, each lane's ladder a long dependent chain) runs on twice the
// waves with a shorter chain per lane.  Both lanes end with the same result.
DEV uint32_t pair_swap(uint32_t x) {  // the value of the other lane of the pair (quad_perm 1,0,3,2)
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);
}
DEV fe fe_pair_swap(const fe& a) {
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = pair_swap(a.v[i]);
  return r;
}
DEV fe fe_sel(bool c, const fe& a, const fe& b) {  // c ? a : b
  fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
DEV fe x25519_ladder_pair(const uint32_t* k, const fe& u, const bool odd) {
  const fe x1 = u;
  fe x2 = fe_set(1), z2 = fe_set(0), x3 = u, z3 = fe_set(1);
  bool swap = false;
#pragma unroll 1
  for (int t = 254; t >= 0; t--) {
    const bool kt = (k[t >> 5] >> (t & 31)) & 1u;
    swap ^= kt;
    fe_cswap(swap, x2, x3);
    fe_cswap(swap, z2, z3);
    swap = kt;
    // stage 1: lane 0 (A, D), lane 1 (B, C); every choice is a select -- no branch, so the two
    // lanes run one instruction stream
    const fe A = fe_add(x2, z2), B = fe_sub(x2, z2), C = fe_add(x3, z3), D = fe_sub(x3, z3);
    const fe X = fe_sel(odd, B, A), Y = fe_sel(odd, C, D);
    const fe s1 = fe_sqr(X), m1 = fe_mul(Y, X);
    const fe s1o = fe_pair_swap(s1), m1o = fe_pair_swap(m1);
    const fe AA = fe_sel(odd, s1o, s1), BB = fe_sel(odd, s1, s1o);
    const fe DA = fe_sel(odd, m1o, m1), CB = fe_sel(odd, m1, m1o);
    // stage 2
    const fe E = fe_sub(AA, BB);
    const fe sp = fe_add(DA, CB), sm = fe_sub(DA, CB);
    const fe G = fe_add(AA, fe_mul121665(E));
    const fe r1 = fe_mul(fe_sel(odd, sp, AA), fe_sel(odd, sp, BB));  // x3 | x2
    const fe r2 = fe_mul(fe_sel(odd, sm, E), fe_sel(odd, sm, G));    // t  | z2
    const fe r3 = fe_mul(x1, r2);                                    // z3 | -
    const fe r1o = fe_pair_swap(r1), r2o = fe_pair_swap(r2), r3o = fe_pair_swap(r3);
    x2 = fe_sel(odd, r1o, r1);
    z2 = fe_sel(odd, r2o, r2);
    x3 = fe_sel(odd, r1, r1o);
    z3 = fe_sel(odd, r3, r3o);
  }
  fe_cswap(swap, x2, x3);
  fe_cswap(swap, z2, z3);
  return fe_freeze(fe_mul(x2, fe_inv(z2)));
}

// -------------------------------------------------------------------------------------
// ChaCha20 (RFC 8439 2.3) and Poly1305 (2.5) for the ChaCha20Poly1305 AEAD (2.8)
// -------------------------------------------------------------------------------------
DEV uint32_t rotl32(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, 32 - n); }
#define CHACHA_QR(a, b, c, d)                  \
  a += b, d ^= a, d = rotl32(d, 16);           \
  c += d, b ^= c, b = rotl32(b, 12);           \
  a += b, d ^= a, d = rotl32(d, 8);            \
  c += d, b ^= c, b = rotl32(b, 7)

// one 64-byte keystream block as 16 little-endian words
DEV void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3],
                        uint32_t out[16]) {
  uint32_t x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1],
                    key[2],      key[3],      key[4],      key[5],      key[6], key[7],
                    counter,     nonce[0],    nonce[1],    nonce[2]};
#pragma unroll
  for (int i = 0; i < 10; i++) {
    CHACHA_QR(x[0], x[4], x[8], x[12]);
    CHACHA_QR(x[1], x[5], x[9], x[13]);
    CHACHA_QR(x[2], x[6], x[10], x[14]);
    CHACHA_QR(x[3], x[7], x[11], x[15]);
    CHACHA_QR(x[0], x[5], x[10], x[15]);
    CHACHA_QR(x[1], x[6], x[11], x[12]);
    CHACHA_QR(x[2], x[7], x[8], x[13]);
    CHACHA_QR(x[3], x[4], x[9], x[14]);
  }
  const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1],
                          key[2],      key[3],      key[4],      key[5],      key[6], key[7],
                          counter,     nonce[0],    nonce[1],    nonce[2]};
#pragma unroll
  for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}

// Poly1305 over 16-byte blocks with the 2^128 pad bit (the AEAD's zero-padded data): h and r in
// five 26-bit limbs, 32 x 32 -> 64-bit products (v_mad_u64_u32)
struct Poly1305 {
  uint32_t r0, r1, r2, r3, r4, h0, h1, h2, h3, h4, pad[4];
};
DEV void poly_init(Poly1305& P, const uint32_t otk[8]) {  // one-time key: r || s, LE words
  P.r0 = otk[0] & 0x3ffffffu;
  P.r1 = ((otk[0] >> 26) | (otk[1] << 6)) & 0x3ffff03u;
  P.r2 = ((otk[1] >> 20) | (otk[2] << 12)) & 0x3ffc0ffu;
  P.r3 = ((otk[2] >> 14) | (otk[3] << 18)) & 0x3f03fffu;
  P.r4 = (otk[3] >> 8) & 0x00fffffu;
  P.h0 = P.h1 = P.h2 = P.h3 = P.h4 = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) P.pad[i] = otk[4 + i];
}
DEV void poly_block(Poly1305& P, const uint32_t m[4]) {  // m: 16 bytes as LE words
  constexpr uint32_t M26 = 0x3ffffffu;
  P.h0 += m[0] & M26;
  P.h1 += ((m[0] >> 26) | (m[1] << 6)) & M26;
  P.h2 += ((m[1] >> 20) | (m[2] << 12)) & M26;
  P.h3 += ((m[2] >> 14) | (m[3] << 18)) & M26;
  P.h4 += (m[3] >> 8) | (1u << 24);
  const uint32_t s1 = P.r1 * 5, s2 = P.r2 * 5, s3 = P.r3 * 5, s4 = P.r4 * 5;
  typedef uint64_t u64;
  u64 d0 = (u64)P.h0 * P.r0 + (u64)P.h1 * s4 + (u64)P.h2 * s3 + (u64)P.h3 * s2 + (u64)P.h4 * s1;
  u64 d1 = (u64)P.h0 * P.r1 + (u64)P.h1 * P.r0 + (u64)P.h2 * s4 + (u64)P.h3 * s3 + (u64)P.h4 * s2;
  u64 d2 = (u64)P.h0 * P.r2 + (u64)P.h1 * P.r1 + (u64)P.h2 * P.r0 + (u64)P.h3 * s4 + (u64)P.h4 * s3;
  u64 d3 = (u64)P.h0 * P.r3 + (u64)P.h1 * P.r2 + (u64)P.h2 * P.r1 + (u64)P.h3 * P.r0 + (u64)P.h4 * s4;
  u64 d4 = (u64)P.h0 * P.r4 + (u64)P.h1 * P.r3 + (u64)P.h2 * P.r2 + (u64)P.h3 * P.r1 + (u64)P.h4 * P.r0;
  uint32_t c = (uint32_t)(d0 >> 26);
  P.h0 = (uint32_t)d0 & M26;
  d1 += c, c = (uint32_t)(d1 >> 26), P.h1 = (uint32_t)d1 & M26;
  d2 += c, c = (uint32_t)(d2 >> 26), P.h2 = (uint32_t)d2 & M26;
  d3 += c, c = (uint32_t)(d3 >> 26), P.h3 = (uint32_t)d3 & M26;
  d4 += c, c = (uint32_t)(d4 >> 26), P.h4 = (uint32_t)d4 & M26;
  P.h0 += c * 5, c = P.h0 >> 26, P.h0 &= M26;
  P.h1 += c;
}
// tag = (h mod 2^130 - 5) + s mod 2^128, LE words
DEV void poly_finish(Poly1305& P, uint32_t tag[4]) {
  constexpr uint32_t M26 = 0x3ffffffu;
  uint32_t h0 = P.h0, h1 = P.h1, h2 = P.h2, h3 = P.h3, h4 = P.h4, c;
  c = h1 >> 26, h1 &= M26, h2 += c;
  c = h2 >> 26, h2 &= M26, h3 += c;
  c = h3 >> 26, h3 &= M26, h4 += c;
  c = h4 >> 26, h4 &= M26, h0 += c * 5;
  c = h0 >> 26, h0 &= M26, h1 += c;
  uint32_t g0 = h0 + 5;  // h - p = h + 5 - 2^130
  c = g0 >> 26, g0 &= M26;
  uint32_t g1 = h1 + c;
  c = g1 >> 26, g1 &= M26;
  uint32_t g2 = h2 + c;
  c = g2 >> 26, g2 &= M26;
  uint32_t g3 = h3 + c;
  c = g3 >> 26, g3 &= M26;
  const uint32_t g4 = h4 + c - (1u << 26);
  const uint32_t keep_g = (g4 >> 31) - 1u;  // all ones when h >= p
  h0 = (h0 & ~keep_g) | (g0 & keep_g);
  h1 = (h1 & ~keep_g) | (g1 & keep_g);
  h2 = (h2 & ~keep_g) | (g2 & keep_g);
  h3 = (h3 & ~keep_g) | (g3 & keep_g);
  h4 = (h4 & ~keep_g) | (g4 & keep_g);
  const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14),
                 w3 = (h3 >> 18) | (h4 << 8);
  uint64_t f = (uint64_t)w0 + P.pad[0];
  tag[0] = (uint32_t)f;
  f = (uint64_t)w1 + P.pad[1] + (f >> 32);
  tag[1] = (uint32_t)f;
  f = (uint64_t)w2 + P.pad[2] + (f >> 32);
  tag[2] = (uint32_t)f;
  f = (uint64_t)w3 + P.pad[3] + (f >> 32);
  tag[3] = (uint32_t)f;
}

// -------------------------------------------------------------------------------------
// Suite parameters and the key schedule
// -------------------------------------------------------------------------------------
struct HpkeParams {
  uint32_t sk[8];        // clamped X25519 scalar, LE words
  uint32_t pk[8];        // pkRm bytes, LE-packed words
  uint32_t ksc[17];      // key_schedule_context (65 bytes) as BE words, zero padded (KDF 0x0001)
  uint32_t task[8];      // task ID (input-share AAD), BE words
  uint32_t ipad0[8], opad0[8];  // HMAC-SHA256 midstates of the empty key
  uint32_t aead;                // AEAD id (1, 2, 3), wave-uniform
  uint32_t kem;                 // KEM id (0x20 X25519, 0x10 P-256, 0x21 X448, 0x12 P-521)
  uint32_t kdf;                 // key-schedule KDF id (1 HKDF-SHA256, 2 -SHA384, 3 -SHA512)
  uint8_t pk65[68];             // P-256: pkRm, the 65-byte uncompressed point (kem_context)
  int8_t p256_dig[88];          // P-256: signed window digits of the private key (p256_recode)
  uint64_t ksc64[17];           // key_schedule_context (97 / 129 bytes) as BE 64-bit words (KDF 2, 3)
  uint64_t ipad0_64[8], opad0_64[8];  // HMAC-SHA512 midstates of the empty key (X448, P-521 KEMs)
  uint32_t sk448[14];           // X448: clamped scalar, LE words
  uint8_t pkraw[136];           // X448 / P-521: pkRm bytes (56 / 133)
  int8_t p521_dig[136];         // P-521: signed window digits of the private key (recode_w4)
  int8_t p384_dig[96];          // P-384: the same (recode_w4, 96 digits)
  uint64_t ipad0_384[8], opad0_384[8];  // HMAC-SHA384 midstates of the empty key (P-384 KEM)
};

// KEM constants (RFC 9180 7.1): Nenc (= Npk) and Nsecret, i.e. the Nh of the KEM's own KDF
template <int KEM>
struct KemC {
  static constexpr int NENC =
      KEM == 0x20 ? 32 : KEM == 0x10 ? 65 : KEM == 0x21 ? 56 : KEM == 0x11 ? 97 : 133;
  static constexpr int NSS_W =  // shared secret (the KEM KDF's Nh), 32-bit words
      (KEM == 0x20 || KEM == 0x10) ? 8 : KEM == 0x11 ? 12 : 16;
};
constexpr int P521_DIGITS = 131;  // w = 4 digits of a 521-bit key (130 windows + the top digit)
constexpr int P384_DIGITS = 96;   // 95 windows of a 384-bit key + the top digit

DEV void load16(const uint8_t* p, uint32_t* w) {
  const uint4 v = *(const uint4*)p;
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
}

DEV void load_words(const uint8_t* p, uint32_t* w, int n16) {
#pragma unroll
  for (int i = 0; i < n16; i++) load16(p + 16 * i, w + 4 * i);
}

// suite_id = "HPKE" || kem || kdf || aead at byte pos of a SHA-256 / SHA-512 message
template <class M>
DEV void msuite(M& m, int pos, uint32_t kem, uint32_t kdf, uint32_t aead) {
  mstr(m, pos, "HPKE");
  mbyte(m, pos + 4, 0x00);
  mbyte(m, pos + 5, kem);
  mbyte(m, pos + 6, 0x00);
  mbyte(m, pos + 7, kdf);
  mbyte(m, pos + 8, 0x00);
  mbyte(m, pos + 9, aead);
}

// RFC 9180 5.1 KeySchedule(mode_base) with HKDF-SHA256 (KDF 0x0001): shared secret (NSS 32-bit
// BE words) -> AEAD key (BE words) and base_nonce (3 BE words).  key_schedule_context is
// constant per opener (P.ksc, host-computed).
template <int NSS>
__device__ __noinline__ void key_schedule_sha256(const HpkeParams& P, uint32_t kem, const uint32_t* ss,
                             uint32_t keyw[8], uint32_t noncew[3]) {
  const uint32_t AEAD = P.aead, NK = AEAD == 1 ? 16 : 32;
  uint32_t secret[8];
  {  // secret = LabeledExtract(shared_secret, "secret", "")
    Msg32<16> m;
    mz(m);
    mstr(m, 0, "HPKE-v1");
    msuite(m, 7, kem, 1, AEAD);
    mstr(m, 17, "secret");
    HmacKey k;
    hmac_keyw<NSS>(k, ss);
    hmac(k, m, 23, secret);
  }
  // key / base_nonce = LabeledExpand(secret, "key" | "base_nonce", ksc, Nk | 12)
  HmacKey k;
  hmac_key32(k, secret);
  Msg32<32> m;
  mz(m);
  mbyte(m, 0, 0);
  mbyte(m, 1, NK);
  mstr(m, 2, "HPKE-v1");
  msuite(m, 9, kem, 1, AEAD);
  mstr(m, 19, "key");
  mwords_be(m, 22, P.ksc, 17);  // 65 bytes + 3 zero padding bytes
  mbyte(m, 87, 0x01);
  hmac(k, m, 88, keyw);
  Msg32<32> n2;
  mz(n2);
  mbyte(n2, 0, 0);
  mbyte(n2, 1, 12);
  mstr(n2, 2, "HPKE-v1");
  msuite(n2, 9, kem, 1, AEAD);
  mstr(n2, 19, "base_nonce");
  mwords_be(n2, 29, P.ksc, 17);
  mbyte(n2, 94, 0x01);
  uint32_t nw[8];
  hmac(k, n2, 95, nw);
  noncew[0] = nw[0], noncew[1] = nw[1], noncew[2] = nw[2];
}

// The same with HKDF-SHA384 (S384, KDF 0x0002) or HKDF-SHA512 (KDF 0x0003): Nh = 48 / 64, so
// key_schedule_context is 97 / 129 bytes (P.ksc64) and the expand messages take two blocks.
template <int NSS, bool S384>
__device__ __noinline__ void key_schedule_sha512(const HpkeParams& P, uint32_t kem, const uint32_t* ss,
                             uint32_t keyw[8], uint32_t noncew[3]) {
  constexpr int NH = S384 ? 48 : 64, KSC = 1 + 2 * NH;
  constexpr uint32_t KDF = S384 ? 2 : 3;
  const uint32_t AEAD = P.aead, NK = AEAD == 1 ? 16 : 32;
  uint64_t secret[8];
  {  // secret = LabeledExtract(shared_secret, "secret", "")
    uint64_t key[NSS / 2];
#pragma unroll
    for (int i = 0; i < NSS / 2; i++) key[i] = (uint64_t)ss[2 * i] << 32 | ss[2 * i + 1];
    HmacKey64 k;
    hmac64_key(k, key, NSS / 2, S384);
    Msg64<16> m;
    mz(m);
    mstr(m, 0, "HPKE-v1");
    msuite(m, 7, kem, KDF, AEAD);
    mstr(m, 17, "secret");
    hmac64(k, m, 23, secret);
  }
  HmacKey64 k;
  hmac64_key(k, secret, NH / 8, S384);
  uint64_t o[8];
  {  // key = LabeledExpand(secret, "key", ksc, Nk)
    Msg64<32> m;
    mz(m);
    mbyte(m, 0, 0);
    mbyte(m, 1, NK);
    mstr(m, 2, "HPKE-v1");
    msuite(m, 9, kem, KDF, AEAD);
    mstr(m, 19, "key");
    mwords64(m, 22, P.ksc64, 17);  // KSC bytes + zero padding
    mbyte(m, 22 + KSC, 0x01);
    hmac64(k, m, 23 + KSC, o);
#pragma unroll
    for (int i = 0; i < 4; i++) keyw[2 * i] = (uint32_t)(o[i] >> 32), keyw[2 * i + 1] = (uint32_t)o[i];
  }
  {  // base_nonce = LabeledExpand(secret, "base_nonce", ksc, 12)
    Msg64<32> m;
    mz(m);
    mbyte(m, 0, 0);
    mbyte(m, 1, 12);
    mstr(m, 2, "HPKE-v1");
    msuite(m, 9, kem, KDF, AEAD);
    mstr(m, 19, "base_nonce");
    mwords64(m, 29, P.ksc64, 17);
    mbyte(m, 29 + KSC, 0x01);
    hmac64(k, m, 30 + KSC, o);
    noncew[0] = (uint32_t)(o[0] >> 32), noncew[1] = (uint32_t)o[0], noncew[2] = (uint32_t)(o[1] >> 32);
  }
}

// the arguments of k_hpke_seal (hpke_seal.hip); filled by the sealer's entry points (hpke.hip)
struct SealArgs {
  uint32_t n, ct_stride, pt_stride, aad_stride, share_len;
  int taskprov;  // MODE 1: the plaintext carries the one empty taskprov extension
  const uint8_t *sk, *pt, *aad, *ids, *pubs, *shares;
  const uint32_t *pt_len, *aad_len;
  const uint64_t* times;
  uint8_t *enc, *ct, *status;
  uint32_t* ct_len;
  // P-256: the sealer's tables (G's, then pkR's: p256::kTabWords words each) and pkR's validity
  const uint4* tab;
  const uint32_t* pk_ok;
};

// hpke_seal.hip: the seal launch (mode 0 explicit AAD, 1 DAP input share with pub = 0 / 32 / 64
// bytes of public share) and the build of a P-256 sealer's tables (2 * p256 kTabWords words at
// d_tab, pkR's validity at d_pk_ok), both on st
int hpke_seal_launch(const HpkeParams& P, int mode, int pub, const SealArgs& a, hipStream_t st);
int hpke_seal_tables_launch(const uint8_t pk65[65], uint32_t* d_tab, uint32_t* d_pk_ok,
                            hipStream_t st);

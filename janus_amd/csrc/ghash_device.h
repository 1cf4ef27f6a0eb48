// ghash_device.h -- the GHASH multiplication of AES-GCM, shared by the HPKE open and seal kernels
// (hpke_device.h) and the leader upload's wide AEAD (prio3_upload.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef DEV
#define DEV __device__ __forceinline__
#endif

// GHASH step (SP 800-38D Algorithm 1): y = (y ^ x) * H in GF(2^128), big-endian words
DEV void ghash_block(uint32_t y[4], const uint32_t x[4], const uint32_t H[4]) {
  uint32_t X[4] = {y[0] ^ x[0], y[1] ^ x[1], y[2] ^ x[2], y[3] ^ x[3]};
  uint32_t Z[4] = {0, 0, 0, 0}, V[4] = {H[0], H[1], H[2], H[3]};
#pragma unroll
  for (int wi = 0; wi < 4; wi++) {
#pragma unroll 8
    for (int bit = 31; bit >= 0; bit--) {
      const uint32_t m = 0u - ((X[wi] >> bit) & 1u);
      Z[0] ^= V[0] & m;
      Z[1] ^= V[1] & m;
      Z[2] ^= V[2] & m;
      Z[3] ^= V[3] & m;
      const uint32_t lsb = 0u - (V[3] & 1u);
      V[3] = __builtin_amdgcn_alignbit(V[2], V[3], 1);
      V[2] = __builtin_amdgcn_alignbit(V[1], V[2], 1);
      V[1] = __builtin_amdgcn_alignbit(V[0], V[1], 1);
      V[0] = (V[0] >> 1) ^ (0xe1000000u & lsb);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) y[i] = Z[i];
}

// hpke_seal.hip -- batched HPKE seal on MI355X (gfx950): RFC 9180 SetupBaseS and one Seal at
// sequence number 0 per report, the direction Janus's client, the helper's aggregate-share handler
// and the leader's collection job driver take (core/src/hpke.rs:167-189).
//
// One report per lane.  The scalar is the report's ephemeral private key, so unlike k_hpke_open it
// differs in every lane, and both points (the KEM's base point and the recipient's pkR) are fixed
// per sealer: X25519 runs its two ladders one after the other with per-lane swaps; P-256 recodes
// the scalar in the lane and walks two per-sealer tables of odd multiples (p256_device.h).  The key
// schedule, the LDS AES tables, GHASH and Poly1305 are the opener's (hpke_device.h); the AEAD
// encrypts first and authenticates what it produced.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/janus_hpke.h"
#include "prio3_device.h"
#include "sha256_device.h"
#include "aes_device.h"
#include "p256_device.h"
#include "sha512_device.h"
#include "hpke_device.h"

// -------------------------------------------------------------------------------------
// Seal: RFC 9180 SetupBaseS + one Seal at sequence number 0, one report per lane
// -------------------------------------------------------------------------------------
// X25519(k, u) with a per-lane scalar (the sealer's ephemeral keys; k clamped, LE words): the
// scalar is shifted left one bit a step and its top bit read, so no word of it is indexed at run
// time (a runtime-indexed private array would live in scratch); the swaps are per-lane selects.
DEV fe x25519_ladder_lane(const uint32_t* kw, const fe& u) {
  uint32_t k[8];
#pragma unroll
  for (int i = 7; i > 0; i--) k[i] = __builtin_amdgcn_alignbit(kw[i], kw[i - 1], 31);
  k[0] = kw[0] << 1;  // bit 254 on top
  const fe x1 = u;
  fe x2 = fe_set(1), z2 = fe_set(0), x3 = u, z3 = fe_set(1);
  bool swap = false;
#pragma unroll 1
  for (int t = 254; t >= 0; t--) {
    const bool kt = (k[7] >> 31) != 0;
#pragma unroll
    for (int i = 7; i > 0; i--) k[i] = __builtin_amdgcn_alignbit(k[i], k[i - 1], 31);
    k[0] <<= 1;
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

// InputShareAad: task_id (32) || report_id (16) || time (u64 BE) || u32 BE len || public share,
// zero padded to 16 bytes, as big-endian words (messages/src/lib.rs:1825-1872)
template <int PUB>
DEV void input_share_aad_be(const HpkeParams& P, const SealArgs& a, uint32_t r,
                            uint32_t aw[(60 + PUB + 15) / 16 * 4]) {
#pragma unroll
  for (int i = 0; i < (60 + PUB + 15) / 16 * 4; i++) aw[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) aw[i] = P.task[i];
  uint32_t idw[4];
  load16(a.ids + 16 * (size_t)r, idw);
#pragma unroll
  for (int i = 0; i < 4; i++) aw[8 + i] = __builtin_bswap32(idw[i]);
  const uint64_t tm = a.times[r];
  aw[12] = (uint32_t)(tm >> 32);
  aw[13] = (uint32_t)tm;
  aw[14] = PUB;
  if constexpr (PUB > 0) {
    uint32_t pw[PUB / 4];
#pragma unroll
    for (int i = 0; i < PUB / 16; i++) load16(a.pubs + (size_t)PUB * r + 16 * i, pw + 4 * i);
#pragma unroll
    for (int i = 0; i < PUB / 4; i++) aw[15 + i] = __builtin_bswap32(pw[i]);
  }
}

// the P-256 tables of one sealer: work-item 0 G's, work-item 1 pkR's (validated as the opener
// validates enc; *pk_ok = 0 fails every report of the sealer)
struct P256Point {
  uint8_t b[68];
};
__global__ __launch_bounds__(64) void k_p256_seal_tables(P256Point pk, uint32_t* tab,
                                                         uint32_t* pk_ok) {
  const uint32_t t = threadIdx.x;
  if (blockIdx.x != 0 || t >= 2) return;
  p256::fp x = p256::kGx, y = p256::kGy;
  if (t == 1) *pk_ok = p256::decode_point(pk.b, x, y) ? 1u : 0u;
  p256::odd_multiples(x, y, (p256::fp*)(tab + p256::kTabWords * t));
}

// MODE 0: explicit plaintext and AAD rows.  MODE 1: DAP helper input share -- the
// PlaintextInputShare framing (messages/src/lib.rs:1326-1341: u16 extensions length, the one empty
// taskprov extension if asked for, u32 payload length, the helper share) and the InputShareAad
// with PUB bytes of public share are built here.  KEM 0x20 (X25519) or 0x10 (P-256); the
// key-schedule KDF and the AEAD are wave-uniform arguments as in k_hpke_open.
// A report that fails (status != OK) gets all-zero enc and ct rows and ct_len 0.
template <int MODE, int PUB, int KEM>
__global__ __launch_bounds__(256) void k_hpke_seal(HpkeParams P, SealArgs a) {
  static_assert(KEM == 0x20 || KEM == 0x10, "KEM id");
  const uint32_t AEAD = P.aead;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ AesT T;
  aes_tables_init(T);
  __syncthreads();
  if (r >= a.n) return;
  // ---- lengths: a row never reads or writes past its stride ---------------------------------
  const uint32_t hdr = a.taskprov ? 10u : 6u;  // MODE 1: bytes before the helper share
  uint32_t pt_len, aad_len;
  bool len_ok = true;
  if constexpr (MODE == 1) {
    pt_len = hdr + a.share_len;  // + 16 <= ct_stride: checked by the host
    aad_len = 60 + PUB;
  } else {
    pt_len = a.pt_len[r];
    aad_len = a.aad_stride ? a.aad_len[r] : 0u;
    len_ok = pt_len <= a.pt_stride && pt_len <= a.ct_stride - 16 && aad_len <= a.aad_stride;
  }
  // ---- DHKEM Encap (RFC 9180 4.1) with the caller's skE: enc = pk(skE), dh = DH(skE, pkR) -----
  uint32_t skw[8];
  load_words(a.sk + 32 * (size_t)r, skw, 2);
  uint32_t ss[8], keyw[8], noncew[3], prk[8];
  bool ok;
  HmacKey k0;  // the empty-key HMAC midstates (eae_prk extraction)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k0.ist[i] = P.ipad0[i];
    k0.ost[i] = P.opad0[i];
  }
  if constexpr (KEM == 0x20) {
    skw[0] &= 0xfffffff8u;  // decodeScalar25519 (RFC 7748 section 5)
    skw[7] = (skw[7] & 0x7fffffffu) | 0x40000000u;
    // the two ladders (u = 9, u = pkR) one after the other in this lane: the register need of
    // one ladder, and the key schedule and the AEAD run once per report
    fe pub, dh;
#pragma unroll 1
    for (int w = 0; w < 2; w++) {
      fe u = fe_set(9);
      if (w) {
#pragma unroll
        for (int i = 0; i < 8; i++) u.v[i] = P.pk[i];
        u.v[7] &= 0x7fffffffu;  // decodeUCoordinate masks bit 255
      }
      const fe q = x25519_ladder_lane(skw, u);
      if (w)
        dh = q;
      else
        pub = q;
    }
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= dh.v[i];
    ok = nz != 0 && len_ok;  // all-zero shared secret: ValidationError
    {
      uint4* ep = (uint4*)(a.enc + 32 * (size_t)r);
      ep[0] = ok ? make_uint4(pub.v[0], pub.v[1], pub.v[2], pub.v[3]) : make_uint4(0, 0, 0, 0);
      ep[1] = ok ? make_uint4(pub.v[4], pub.v[5], pub.v[6], pub.v[7]) : make_uint4(0, 0, 0, 0);
    }
    {  // eae_prk = LabeledExtract("", "eae_prk", dh)
      Msg32<16> m;
      mz(m);
      mstr(m, 0, "HPKE-v1");
      mstr(m, 7, "KEM");
      mbyte(m, 10, 0x00);
      mbyte(m, 11, 0x20);
      mstr(m, 12, "eae_prk");
      mwords_le(m, 19, dh.v, 8);
      hmac(k0, m, 51, prk);
    }
    {  // shared_secret = LabeledExpand(eae_prk, "shared_secret", enc || pkRm, 32)
      Msg32<32> m;
      mz(m);
      mbyte(m, 0, 0);
      mbyte(m, 1, 32);
      mstr(m, 2, "HPKE-v1");
      mstr(m, 9, "KEM");
      mbyte(m, 12, 0x00);
      mbyte(m, 13, 0x20);
      mstr(m, 14, "shared_secret");
      mwords_le(m, 27, pub.v, 8);
      mwords_le(m, 59, P.pk, 8);
      mbyte(m, 91, 0x01);
      HmacKey k;
      hmac_key32(k, prk);
      hmac(k, m, 92, ss);
    }
  } else {
    // skE is a big-endian scalar; both scalar multiplications run over the sealer's tables
    uint32_t s[8], kp[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = __builtin_bswap32(skw[7 - i]);
    bool negated;
    ok = p256::seal_scalar(s, kp, negated) && *a.pk_ok != 0 && len_ok;
    p256::jac A, B;  // k' G, k' pkR
#pragma unroll 1
    for (int w = 0; w < 2; w++) {
      const p256::jac q = p256::mul_window(kp, a.tab + (p256::kTabWords / 4) * w);
      if (w)
        B = q;
      else
        A = q;
    }
    ok = ok && !p256::is_zero(A.Z) && !p256::is_zero(B.Z);
    // one inversion for the two results; k' = n - skE negated the point: y back
    const p256::fp zi = p256::inv(p256::mul(A.Z, B.Z));
    const p256::fp za = p256::mul(zi, B.Z), zb = p256::mul(zi, A.Z), za2 = p256::sqr(za);
    const p256::fp ex = p256::freeze(p256::mul(A.X, za2));
    p256::fp ey = p256::mul(A.Y, p256::mul(za2, za));
    const p256::fp ney = p256::neg(ey);
#pragma unroll
    for (int i = 0; i < 8; i++) ey.v[i] = negated ? ney.v[i] : ey.v[i];
    ey = p256::freeze(ey);
    const p256::fp dx = p256::freeze(p256::mul(B.X, p256::sqr(zb)));
    uint32_t xbe[8], ybe[8], dh[8];  // big-endian words
#pragma unroll
    for (int i = 0; i < 8; i++) xbe[i] = ex.v[7 - i], ybe[i] = ey.v[7 - i], dh[i] = dx.v[7 - i];
    {  // enc = 0x04 || X || Y (rows of 65 bytes: byte stores)
      uint8_t* ep = a.enc + 65 * (size_t)r;
      ep[0] = ok ? 0x04 : 0;
#pragma unroll
      for (int i = 0; i < 32; i++) {
        ep[1 + i] = ok ? (uint8_t)(xbe[i >> 2] >> (24 - 8 * (i & 3))) : 0;
        ep[33 + i] = ok ? (uint8_t)(ybe[i >> 2] >> (24 - 8 * (i & 3))) : 0;
      }
    }
    {  // eae_prk = LabeledExtract("", "eae_prk", dh)
      Msg32<16> m;
      mz(m);
      mstr(m, 0, "HPKE-v1");
      mstr(m, 7, "KEM");
      mbyte(m, 10, 0x00);
      mbyte(m, 11, 0x10);
      mstr(m, 12, "eae_prk");
      mwords_be(m, 19, dh, 8);
      hmac(k0, m, 51, prk);
    }
    {  // shared_secret = LabeledExpand(eae_prk, "shared_secret", enc || pkRm (130 B), 32)
      Msg32<48> m;
      mz(m);
      mbyte(m, 0, 0);
      mbyte(m, 1, 32);
      mstr(m, 2, "HPKE-v1");
      mstr(m, 9, "KEM");
      mbyte(m, 12, 0x00);
      mbyte(m, 13, 0x10);
      mstr(m, 14, "shared_secret");
      mbyte(m, 27, 0x04);
      mwords_be(m, 28, xbe, 8);
      mwords_be(m, 60, ybe, 8);
#pragma unroll
      for (int i = 0; i < 65; i++) mbyte(m, 92 + i, P.pk65[i]);
      mbyte(m, 157, 0x01);
      HmacKey k;
      hmac_key32(k, prk);
      hmac(k, m, 158, ss);
    }
  }
  // ---- KeySchedule(mode_base) with the suite's KDF -----------------------------------------
  if (P.kdf == 1)
    key_schedule_sha256<8>(P, KEM, ss, keyw, noncew);
  else if (P.kdf == 2)
    key_schedule_sha512<8, true>(P, KEM, ss, keyw, noncew);
  else
    key_schedule_sha512<8, false>(P, KEM, ss, keyw, noncew);
  if (!ok) pt_len = 0, aad_len = 0;  // a failed report reads nothing and writes zeros
  // ---- the plaintext and the AAD, 16 bytes at a time -----------------------------------------
  uint8_t* cp = a.ct + (size_t)a.ct_stride * r;
  const uint8_t* sp = MODE == 1 ? a.shares + (size_t)a.share_len * r : a.pt + (size_t)a.pt_stride * r;
  // MODE 1: the framing's bytes, little-endian packed (they all lie in the first block)
  const uint64_t lenb = (uint64_t)__builtin_bswap32(a.share_len);  // the u32 length's four bytes
  const uint64_t hlo = a.taskprov ? 0x00ff0400ull | lenb << 48 : lenb << 16;
  const uint64_t hhi = a.taskprov ? lenb >> 16 : 0ull;
  auto keep_mask = [](uint32_t lo, uint32_t len) {  // the bytes of a word at lo that lie below len
    return lo + 4 <= len ? 0xffffffffu : lo >= len ? 0u : (1u << (8 * (len - lo))) - 1u;
  };
  auto pt_words = [&](uint32_t off, uint32_t pw[4]) {  // LE-packed, zero past pt_len
    if constexpr (MODE == 1) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t q = off + 4 * i + j;
          uint32_t b = 0;
          if (q < hdr)
            b = (uint32_t)((q < 8 ? hlo >> (8 * q) : hhi >> (8 * (q - 8))) & 0xffu);
          else if (q < pt_len)
            b = sp[q - hdr];
          w |= b << (8 * j);
        }
        pw[i] = w;
      }
    } else {
      load16(sp + off, pw);
#pragma unroll
      for (int i = 0; i < 4; i++) pw[i] &= keep_mask(off + 4 * i, pt_len);
    }
  };
  auto aad_words = [&](uint32_t off, uint32_t xw[4]) {  // MODE 0: LE-packed, zero past aad_len
    load16(a.aad + (size_t)a.aad_stride * r + off, xw);
#pragma unroll
    for (int i = 0; i < 4; i++) xw[i] &= keep_mask(off + 4 * i, aad_len);
  };
  constexpr int AWP = (60 + PUB + 15) / 16 * 4;  // MODE 1: the AAD's words, padded to blocks
  uint32_t tagw[4];                             // the tag, LE-packed bytes
  auto gcm_seal = [&](auto nr_tag) {  // NR = 10 (AES-128-GCM) or 14 (AES-256-GCM)
    constexpr int NR = decltype(nr_tag)::value;
    uint32_t kcol[8], rk[4 * (NR + 1)];
#pragma unroll
    for (int i = 0; i < 8; i++) kcol[i] = __builtin_bswap32(keyw[i]);
    if constexpr (NR == 10)
      aes128_expand(T, kcol, rk);
    else
      aes256_expand(T, kcol, rk);
    uint32_t H[4];
    {
      const uint32_t z[4] = {0, 0, 0, 0};
      uint32_t hc[4];
      aes_encrypt<NR>(T, rk, z, hc);
#pragma unroll
      for (int i = 0; i < 4; i++) H[i] = __builtin_bswap32(hc[i]);
    }
    uint32_t y[4] = {0, 0, 0, 0};
    if constexpr (MODE == 1) {
      uint32_t aw[AWP];
      input_share_aad_be<PUB>(P, a, r, aw);
      if (ok) {
#pragma unroll
        for (int b = 0; b < AWP / 4; b++) ghash_block(y, aw + 4 * b, H);
      }
    } else {
      for (uint32_t off = 0; off < aad_len; off += 16) {
        uint32_t xw[4];
        aad_words(off, xw);
#pragma unroll
        for (int i = 0; i < 4; i++) xw[i] = __builtin_bswap32(xw[i]);
        ghash_block(y, xw, H);
      }
    }
    uint32_t ctr[4];
#pragma unroll
    for (int i = 0; i < 3; i++) ctr[i] = __builtin_bswap32(noncew[i]);
    // encrypt, then authenticate what was produced; the rest of the row is zero-filled
    for (uint32_t off = 0, blk = 2; off < a.ct_stride; off += 16, blk++) {
      uint32_t cw[4] = {0, 0, 0, 0};
      if (off < pt_len) {
        uint32_t pw[4], ks[4], xw[4];
        pt_words(off, pw);
        ctr[3] = __builtin_bswap32(blk);
        aes_encrypt<NR>(T, rk, ctr, ks);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          cw[i] = (pw[i] ^ ks[i]) & keep_mask(off + 4 * i, pt_len);
          xw[i] = __builtin_bswap32(cw[i]);
        }
        ghash_block(y, xw, H);
      }
      *(uint4*)(cp + off) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    }
    const uint32_t lw[4] = {0, aad_len * 8, 0, pt_len * 8};
    ghash_block(y, lw, H);
    ctr[3] = __builtin_bswap32(1u);
    uint32_t ek[4];
    aes_encrypt<NR>(T, rk, ctr, ek);
#pragma unroll
    for (int i = 0; i < 4; i++) tagw[i] = __builtin_bswap32(y[i]) ^ ek[i];
  };
  if (AEAD == 3) {
    // ---- ChaCha20Poly1305 seal (RFC 8439 2.8), sequence number 0 ---------------------------
    uint32_t ckey[8], cnon[3];
#pragma unroll
    for (int i = 0; i < 8; i++) ckey[i] = __builtin_bswap32(keyw[i]);  // key bytes as LE words
#pragma unroll
    for (int i = 0; i < 3; i++) cnon[i] = __builtin_bswap32(noncew[i]);
    Poly1305 mac;
    {
      uint32_t b0[16];
      chacha20_block(ckey, 0, cnon, b0);  // Poly1305 one-time key = first 32 bytes of block 0
      poly_init(mac, b0);
    }
    if constexpr (MODE == 1) {
      uint32_t aw[AWP];
      input_share_aad_be<PUB>(P, a, r, aw);
#pragma unroll
      for (int i = 0; i < AWP; i++) aw[i] = __builtin_bswap32(aw[i]);
      if (ok) {
#pragma unroll
        for (int b = 0; b < AWP / 4; b++) poly_block(mac, aw + 4 * b);
      }
    } else {
      for (uint32_t off = 0; off < aad_len; off += 16) {
        uint32_t xw[4];
        aad_words(off, xw);
        poly_block(mac, xw);
      }
    }
    for (uint32_t off0 = 0, blk = 1; off0 < a.ct_stride; off0 += 64, blk++) {
      uint32_t ks[16];
      if (off0 < pt_len) chacha20_block(ckey, blk, cnon, ks);
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++) {
        const uint32_t off = off0 + 16 * c4;
        if (off >= a.ct_stride) break;
        uint32_t cw[4] = {0, 0, 0, 0};
        if (off < pt_len) {
          uint32_t pw[4];
          pt_words(off, pw);
#pragma unroll
          for (int i = 0; i < 4; i++) cw[i] = (pw[i] ^ ks[4 * c4 + i]) & keep_mask(off + 4 * i, pt_len);
          poly_block(mac, cw);
        }
        *(uint4*)(cp + off) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
      }
    }
    const uint32_t lw[4] = {aad_len, 0, pt_len, 0};  // le64(aad_len) || le64(ct_len)
    poly_block(mac, lw);
    poly_finish(mac, tagw);
  } else if (AEAD == 2) {
    gcm_seal(std::integral_constant<int, 14>{});
  } else {
    gcm_seal(std::integral_constant<int, 10>{});
  }
  if (ok) {  // the tag follows the ciphertext at any byte offset: byte stores over the zero fill
#pragma unroll
    for (int i = 0; i < 16; i++) cp[pt_len + i] = (uint8_t)(tagw[i >> 2] >> (8 * (i & 3)));
  }
  a.ct_len[r] = ok ? pt_len + 16 : 0u;
  a.status[r] = ok ? JANUS_HPKE_OK
                   : len_ok ? JANUS_HPKE_SEAL_KEY_ERROR : JANUS_HPKE_SEAL_LENGTH_ERROR;
}


// -------------------------------------------------------------------------------------
// Launchers (the sealer's entry points are in hpke.hip)
// -------------------------------------------------------------------------------------
int hpke_seal_tables_launch(const uint8_t pk65[65], uint32_t* d_tab, uint32_t* d_pk_ok,
                            hipStream_t st) {
  P256Point pk{};
  for (int i = 0; i < 65; i++) pk.b[i] = pk65[i];
  k_p256_seal_tables<<<1, 64, 0, st>>>(pk, d_tab, d_pk_ok);
  return hipGetLastError() == hipSuccess ? JANUS_HPKE_SUCCESS : JANUS_HPKE_EDEVICE;
}

int hpke_seal_launch(const HpkeParams& P, int mode, int pub, const SealArgs& a, hipStream_t st) {
  const uint32_t blocks = (a.n + 255) / 256;
#define JANUS_HPKE_SEAL_LAUNCH(KE)                          \
  if (mode == 0)                                            \
    k_hpke_seal<0, 0, KE><<<blocks, 256, 0, st>>>(P, a);    \
  else if (pub == 64)                                       \
    k_hpke_seal<1, 64, KE><<<blocks, 256, 0, st>>>(P, a);   \
  else if (pub == 32)                                       \
    k_hpke_seal<1, 32, KE><<<blocks, 256, 0, st>>>(P, a);   \
  else                                                      \
    k_hpke_seal<1, 0, KE><<<blocks, 256, 0, st>>>(P, a);
  if (P.kem == JANUS_HPKE_KEM_P256_HKDF_SHA256) {
    JANUS_HPKE_SEAL_LAUNCH(0x10)
  } else {
    JANUS_HPKE_SEAL_LAUNCH(0x20)
  }
#undef JANUS_HPKE_SEAL_LAUNCH
  return hipGetLastError() == hipSuccess ? JANUS_HPKE_SUCCESS : JANUS_HPKE_EDEVICE;
}

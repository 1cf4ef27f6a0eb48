// prio3_upload.hip -- the leader's upload handler for a batch of one task on MI355X (gfx950):
// VdafOps::handle_upload_generic (aggregator.rs) from the uploaded `Report` bodies to the buffers
// prio3_device_leader_prepare_init and janus_dap_agg_init_req_encode_device read, with a status per
// report (include/janus_prio3.h, "Leader upload").
//
//   k_rep_decode (dap_codec.hip)  Report::get_decoded: field offsets, small fields, helper rows
//   k_up_pre      one lane per report: the checks that need no key, in the reference's order (time
//                 against the deadline, the task expiration and the expiry age, the public share's
//                 length, the leader config ID, enc / payload lengths); the reports to open go on
//                 the task opener's list or the global opener's
//   per opener (the task's, then the global one with the reports whose task open failed):
//     k_up_gather   one wave per listed report: `enc` into the rows k_hpke_open reads; for the
//                   one-lane AEAD also the payload and the InputShareAad into aligned rows
//     one-lane:     k_hpke_open<0> (hpke.hip: Decap, key schedule and AEAD, a lane per report),
//                   k_up_post1 (status, retry list)
//     wide:         k_hpke_open<2> (stage A: Decap and key schedule -> key, base nonce),
//                   k_aead_open_wide (stage B, below)
//   k_up_finish   one wave per report: PlaintextInputShare decode, the leader share's length and
//                 canonical field elements, then the output rows (zero unless the status is 0)
//
// k_aead_open_wide: AES-128/256-GCM open with G = 16 lanes per report (a DPP row), so a 64-lane wave
// opens four reports and a 5.6 KB payload is 23 dependent blocks per lane instead of 361.
//  - Block sequence S = AAD blocks (InputShareAad, built from the task ID and the row's first
//    28 + public_share_len bytes), then the ciphertext blocks, N in all; lane j takes blocks
//    s = j, j + G, ...: the group's 16-byte loads and plaintext stores are contiguous.
//  - The payload sits at 35 + public_share_len + Nenc in the row (never 16-byte aligned, odd for
//    X25519): every block is read as five aligned dwords and shifted into place (v_alignbit);
//    no dword that starts at or past the payload's end is loaded.
//  - CTR blocks are independent (counter = block index + 2).  The AES round keys are expanded per
//    lane into registers (one block's worth of S-box lookups against ~22 blocks of work); the
//    T-tables are the workgroup's, in LDS.
//  - GHASH: tag = sum_s X_s H^(N - s + 1) + LEN H.  Lane j runs y = y H^G + X over its blocks, so
//    its last block carries H^0 and the lane's sum still needs H^(d + 2), d = (N mod G - 1 - j)
//    mod G.  The lanes rotate so that lane d holds the sum that needs H^d (one ds_bpermute), then
//    four butterfly steps z = m ^ partner(m), m = bit k of d ? z H^(2^k) : z with DPP partners
//    (quad_perm, row_half_mirror, row_mirror) both XOR-reduce the group and apply the powers; the
//    squarings that give H^2 .. H^16 are the only other multiplications: T + 9 per lane for
//    T = ceil(N / G) blocks.  A short last block is masked before it is hashed and stored.
//  - A failed tag (or KEM) zeroes the plaintext row, sets DecryptFailure and, when the global
//    keypair has the same config ID, puts the report on the global opener's list.
//
// The group form (prio3_leader_upload_job: the upload executor's coalesced group, prio3_runtime.h)
// runs the same chain once for the jobs of many tasks.  What differs between the jobs -- task ID,
// now, deadline, task expiration, expiry age -- sits in the group's job table, and each report
// carries its length and its job's slot (UploadMeta).  The kernels that read one of those are
// templates over TAB: the one-task instantiations (TAB = false) are the code above, the group's
// take the task-ID words and the times from the report's own job row.
//   k_up_front    k_rep_decode and k_up_pre in one launch, one wave per report: the walk over the
//                 prefixes, the small outputs, then the checks on the values still in registers
//                 (lane 0 stores the verdict); one list atomic per workgroup and list.  It writes
//                 no helper rows: the job form cuts them out of its staged input on the host.  The
//                 list counters arrive as zeros with the group's first DMA (no memset).
//   then per opener k_up_gather<true>, k_hpke_open / k_hpke_keys (group-uniform: the openers are in
//   the group key), k_up_post1 or k_aead_open_wide<NR, true> (the four reports of a wave may belong
//   to four jobs: each 16-lane row reads its own job's task ID), and k_up_finish<true>.
//   One opener: 5 launches (7 in the one-task form, the counter memset included); two: 8 (10).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/janus_dap.h"
#include "../../include/janus_hpke.h"
#include "../../include/janus_prio3.h"
#include "dap_report.h"
#include "prio3_host.h"
#include "aes_device.h"
#include "ghash_device.h"

namespace {

constexpr uint32_t UP_G = 16;  // lanes per report of k_aead_open_wide (one DPP row)
// auto (option upload_aead = 0): the wide AEAD for expected payloads of at least this many bytes
constexpr uint32_t UP_WIDE_MIN_PAYLOAD = 5632;

enum : uint32_t { F_PUB_OFF, F_PUB_LEN, F_LENC_OFF, F_LENC_LEN, F_LPAY_OFF, F_LPAY_LEN };

struct UpArgs {
  uint32_t n, stride, psl, share_len, blind_len, es, ext_stride, pt_stride, aad_stride;
  uint32_t henc_len, hct_stride;
  uint64_t now, deadline, task_exp, expiry_age;
  uint32_t has[2], cfg[2], nenc[2];  // [0] the task's opener, [1] the global one
  uint32_t task[8];                  // task ID, BE words
  const uint8_t* rows;
  // decode outputs (the caller's buffers) and scratch
  uint8_t *ids, *lcfg, *hcfg, *henc, *hct, *bad;
  uint64_t* times;
  uint32_t *fields, *hct_len;
  uint8_t *sel, *status, *pt, *enc, *ct, *aad, *hst;
  uint32_t *ct_len, *aad_len, *keys;
  uint32_t* list[2];
  uint32_t* cnt;  // [2]
  // outputs
  uint8_t *pub, *shares, *ext;
  uint32_t* ext_len;
  // the group form (TAB instantiations): per report its length and job slot, the job table
  const UploadMeta* meta;
  const UploadJobRow* jtab;
};
// word i of the task ID in report r's AAD: the launch's (one task) or its job's (TAB)
template <bool TAB>
DEV uint32_t task_word(const UpArgs& a, uint32_t r, uint32_t i) {
  if constexpr (TAB)
    return a.jtab[a.meta[r].slot].task[i];
  else
    return a.task[i];
}

// bytes [off, off + 16) of a 4-byte aligned row as LE words; no dword that starts at or past `end`
// is loaded (it reads as zero), so nothing past the field's last dword is touched
DEV void ld16u(const uint8_t* row, uint32_t off, uint32_t end, uint32_t w[4]) {
  const uint32_t a = off & ~3u, sh = 8 * (off & 3u);
  uint32_t d[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint32_t pos = a + 4 * k;
    d[k] = pos < end ? *(const uint32_t*)(row + pos) : 0u;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = sh ? __builtin_amdgcn_alignbit(d[k + 1], d[k], sh) : d[k];
}
// mask of the bytes of word i (bytes lo .. lo + 3 of a field) that lie below len
DEV uint32_t keep_mask(uint32_t lo, uint32_t len) {
  return lo + 4 <= len ? 0xffffffffu : lo >= len ? 0u : (1u << (8 * (len - lo))) - 1u;
}

__global__ __launch_bounds__(256) void k_up_pre(UpArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < a.n;
  const uint32_t* f = a.fields + (size_t)JANUS_DAP_REPORT_FIELDS * (live ? r : 0);
  uint32_t st = 0, sel = 0;
  int pass = -1;
  if (!live) {
  } else if (a.bad[r]) {
    st = PRIO3_UPLOAD_MALFORMED;
  } else {
    const uint64_t t = a.times[r];
    const uint32_t cfg = a.lcfg[r];
    const bool mt = a.has[0] && cfg == a.cfg[0], mg = a.has[1] && cfg == a.cfg[1];
    const bool et = mt && f[F_LENC_LEN] == a.nenc[0], eg = mg && f[F_LENC_LEN] == a.nenc[1];
    if (t > a.deadline)
      st = PRIO3_UPLOAD_TOO_EARLY;
    else if (t > a.task_exp)  // UINT64_MAX: no expiration
      st = PRIO3_UPLOAD_TASK_EXPIRED;
    else if (a.expiry_age != ~0ull && t + a.expiry_age < t)
      st = PRIO3_UPLOAD_HOST;  // Time::add overflows: the reference's internal error
    else if (a.expiry_age != ~0ull && a.now > t + a.expiry_age)
      st = PRIO3_UPLOAD_EXPIRED;
    else if (f[F_PUB_LEN] != a.psl)
      st = PRIO3_UPLOAD_DECODE_FAILURE;
    else if (!mt && !mg)
      st = PRIO3_UPLOAD_OUTDATED_HPKE_CONFIG;
    else if (f[F_LPAY_LEN] < 16 || (!et && !eg))
      st = PRIO3_UPLOAD_DECRYPT_FAILURE;
    else {
      pass = et ? 0 : 1;
      sel = et && eg ? 2u : 0u;  // the task open's failure goes on to the global keypair
    }
  }
  if (live) {
    a.status[r] = (uint8_t)st;
    a.sel[r] = (uint8_t)sel;
  }
  // one atomic per wave and list: with one per report, 256 Ki same-address atomics took 3.0 ms of a
  // 17 ms call
#pragma unroll
  for (int p = 0; p < 2; p++) {
    const uint64_t mask = __ballot(pass == p);
    if (!mask) continue;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(a.cnt + p, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, leader);
    if (pass == p) a.list[p][base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = r;
  }
}

// The group form's front: k_rep_decode and k_up_pre over the reports of a coalesced group, one
// wave per report.  Every lane walks the prefixes (wave-uniform addresses, as in k_rep_decode), the
// lanes share the small outputs, and the checks of k_up_pre run on the time and config ID still in
// registers against the report's job row; lane 0 stores the verdict.  The four waves of a workgroup
// share one atomic per list.
__global__ __launch_bounds__(256) void k_up_front(UpArgs a) {
  __shared__ int s_pass[4];
  __shared__ uint32_t s_at[4];
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * 4 + w;
  int pass = -1;
  if (r < a.n) {
    const uint8_t* row = a.rows + (size_t)a.stride * r;
    const UploadMeta m = a.meta[r];
    uint32_t f[JANUS_DAP_REPORT_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, cfg[2] = {0, 0};
    const bool ok = m.len <= a.stride && rep_parse(row, m.len, f, cfg);
    if (!ok) {
#pragma unroll
      for (int i = 0; i < JANUS_DAP_REPORT_FIELDS; i++) f[i] = 0;
      cfg[0] = cfg[1] = 0;
    }
    const bool hok = ok && f[7] == a.henc_len && f[9] <= a.hct_stride;
    uint64_t t = 0;
    if (ok)
      for (int i = 0; i < 8; i++) t = (t << 8) | row[16 + i];
    if (l < 16) a.ids[16 * (size_t)r + l] = ok ? row[l] : (uint8_t)0;
    if (l == 16) a.times[r] = t;
    if (l == 17) {
#pragma unroll
      for (int i = 0; i < JANUS_DAP_REPORT_FIELDS; i++)
        a.fields[(size_t)JANUS_DAP_REPORT_FIELDS * r + i] = f[i];
    }
    if (l == 18) {
      a.lcfg[r] = (uint8_t)cfg[0];
      a.hcfg[r] = (uint8_t)cfg[1];
      a.hct_len[r] = hok ? f[9] : 0u;
    }
    const UploadJobRow* jr = a.jtab + m.slot;
    uint32_t st = 0, sel = 0;
    if (!ok) {
      st = PRIO3_UPLOAD_MALFORMED;
    } else {
      const bool mt = a.has[0] && cfg[0] == a.cfg[0], mg = a.has[1] && cfg[0] == a.cfg[1];
      const bool et = mt && f[F_LENC_LEN] == a.nenc[0], eg = mg && f[F_LENC_LEN] == a.nenc[1];
      const uint64_t age = jr->expiry_age;
      if (t > jr->deadline)
        st = PRIO3_UPLOAD_TOO_EARLY;
      else if (t > jr->task_exp)  // UINT64_MAX: no expiration
        st = PRIO3_UPLOAD_TASK_EXPIRED;
      else if (age != ~0ull && t + age < t)
        st = PRIO3_UPLOAD_HOST;  // Time::add overflows: the reference's internal error
      else if (age != ~0ull && jr->now > t + age)
        st = PRIO3_UPLOAD_EXPIRED;
      else if (f[F_PUB_LEN] != a.psl)
        st = PRIO3_UPLOAD_DECODE_FAILURE;
      else if (!mt && !mg)
        st = PRIO3_UPLOAD_OUTDATED_HPKE_CONFIG;
      else if (f[F_LPAY_LEN] < 16 || (!et && !eg))
        st = PRIO3_UPLOAD_DECRYPT_FAILURE;
      else {
        pass = et ? 0 : 1;
        sel = et && eg ? 2u : 0u;  // the task open's failure goes on to the global keypair
      }
    }
    if (l == 0) {
      a.status[r] = (uint8_t)st;
      a.sel[r] = (uint8_t)sel;
    }
  }
  if (l == 0) s_pass[w] = pass;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c0 = 0, c1 = 0;
    for (int i = 0; i < 4; i++) {
      if (s_pass[i] == 0) s_at[i] = c0++;
      if (s_pass[i] == 1) s_at[i] = c1++;
    }
    const uint32_t b0 = c0 ? atomicAdd(a.cnt, c0) : 0u;
    const uint32_t b1 = c1 ? atomicAdd(a.cnt + 1, c1) : 0u;
    for (int i = 0; i < 4; i++) {
      if (s_pass[i] == 0) s_at[i] += b0;
      if (s_pass[i] == 1) s_at[i] += b1;
    }
  }
  __syncthreads();
  if (l == 0 && pass >= 0) a.list[pass][s_at[w]] = r;
}

// one wave per listed report: enc into [nenc] rows; one-lane AEAD: payload and AAD rows too
template <bool TAB>
__global__ __launch_bounds__(256) void k_up_gather(UpArgs a, int pass, int one_lane) {
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (q >= min(a.cnt[pass], a.n)) return;
  const uint32_t r = a.list[pass][q];
  const uint32_t* f = a.fields + (size_t)JANUS_DAP_REPORT_FIELDS * r;
  const uint8_t* row = a.rows + (size_t)a.stride * r;
  const uint32_t nenc = a.nenc[pass];
  for (uint32_t k = l; k < nenc; k += 64) a.enc[(size_t)nenc * r + k] = row[f[F_LENC_OFF] + k];
  if (!one_lane) return;
  const uint32_t pl = f[F_LPAY_LEN], po = f[F_LPAY_OFF], end = po + pl;
  uint32_t* ct = (uint32_t*)(a.ct + (size_t)a.pt_stride * r);
  for (uint32_t k = l; 4 * k < pl; k += 64) {  // dword k of the payload (pl <= pt_stride)
    const uint32_t off = po + 4 * k, al = off & ~3u, sh = 8 * (off & 3u);
    const uint32_t lo = *(const uint32_t*)(row + al);
    const uint32_t hi = sh && al + 4 < end ? *(const uint32_t*)(row + al + 4) : 0u;
    ct[k] = sh ? __builtin_amdgcn_alignbit(hi, lo, sh) : lo;
  }
  const uint32_t al = 60 + a.psl;
  uint8_t* aad = a.aad + (size_t)a.aad_stride * r;
  for (uint32_t k = l; k < a.aad_stride; k += 64)
    aad[k] = k < 32    ? (uint8_t)(task_word<TAB>(a, r, k >> 2) >> (8 * (3 - (k & 3))))
             : k < al ? row[k - 32]
                      : (uint8_t)0;
  if (l == 0) {
    a.ct_len[r] = pl;
    a.aad_len[r] = al;
  }
}

__global__ __launch_bounds__(256) void k_up_post1(UpArgs a, int pass) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= min(a.cnt[pass], a.n)) return;
  const uint32_t r = a.list[pass][q];
  const bool ok = a.hst[r] == JANUS_HPKE_OK;
  a.status[r] = ok ? 0 : PRIO3_UPLOAD_DECRYPT_FAILURE;
  if (!ok && pass == 0 && (a.sel[r] & 2u)) a.list[1][atomicAdd(a.cnt + 1, 1u)] = r;
}

// x * H in GF(2^128) (GHASH's field)
DEV void gf_mul(uint32_t y[4], const uint32_t H[4]) {
  const uint32_t z[4] = {0, 0, 0, 0};
  ghash_block(y, z, H);
}
template <int CTRL>
DEV uint32_t dpp_row(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, false);
}
// one butterfly step of the group reduce: m = bit ? z * Hk : z, then z = m ^ partner's m
template <int CTRL>
DEV void gf_fold(uint32_t z[4], const uint32_t Hk[4], bool bit) {
  uint32_t p[4] = {z[0], z[1], z[2], z[3]};
  gf_mul(p, Hk);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t m = bit ? p[i] : z[i];
    z[i] = m ^ dpp_row<CTRL>(m);
  }
}

template <int NR, bool TAB>
__global__ __launch_bounds__(256) void k_aead_open_wide(UpArgs a, int pass) {
  const uint32_t lim = min(a.cnt[pass], a.n);
  if (blockIdx.x * (256 / UP_G) >= lim) return;
  __shared__ AesT T;
  aes_tables_init(T);
  __syncthreads();
  const uint32_t q = blockIdx.x * (256 / UP_G) + (threadIdx.x / UP_G), j = threadIdx.x % UP_G;
  if (q >= lim) return;
  const uint32_t r = a.list[pass][q];
  const uint32_t* f = a.fields + (size_t)JANUS_DAP_REPORT_FIELDS * r;
  const uint8_t* row = a.rows + (size_t)a.stride * r;
  const uint32_t po = f[F_LPAY_OFF], pl = f[F_LPAY_LEN];  // pl >= 16 (k_up_pre)
  const uint32_t ptl = pl - 16, nblk = (ptl + 15) / 16;
  const uint32_t hdr = 28 + a.psl, aad_len = 32 + hdr, na = (aad_len + 15) / 16;
  const uint32_t N = na + nblk;
  uint8_t* pp = a.pt + (size_t)a.pt_stride * r;
  const uint32_t* kw = a.keys + 12 * (size_t)r;
  uint32_t rk[4 * (NR + 1)], ctr[4];
  {
    uint32_t kcol[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kcol[i] = __builtin_bswap32(kw[i]);
    if constexpr (NR == 10)
      aes128_expand(T, kcol, rk);
    else
      aes256_expand(T, kcol, rk);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) ctr[i] = __builtin_bswap32(kw[8 + i]);
  const bool kem_ok = kw[11] != 0;
  uint32_t H1[4], H2[4], H4[4], H8[4], H16[4];
  {
    const uint32_t z[4] = {0, 0, 0, 0};
    uint32_t hc[4];
    aes_encrypt<NR>(T, rk, z, hc);
#pragma unroll
    for (int i = 0; i < 4; i++) H1[i] = __builtin_bswap32(hc[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) H2[i] = H1[i];
    gf_mul(H2, H1);
#pragma unroll
    for (int i = 0; i < 4; i++) H4[i] = H2[i];
    gf_mul(H4, H2);
#pragma unroll
    for (int i = 0; i < 4; i++) H8[i] = H4[i];
    gf_mul(H8, H4);
#pragma unroll
    for (int i = 0; i < 4; i++) H16[i] = H8[i];
    gf_mul(H16, H8);
  }
  static_assert(UP_G == 16, "the lane's Horner multiplier is H^16 and the reduce has four steps");
  uint32_t y[4] = {0, 0, 0, 0};
  const uint32_t Tn = (N + UP_G - 1) / UP_G;
#pragma unroll 1
  for (uint32_t t = 0; t < Tn; t++) {
    const uint32_t s = j + UP_G * t;
    uint32_t x[4] = {0, 0, 0, 0};
    if (s < na) {  // an AAD block: task ID (two blocks), then the row's first hdr bytes
      if (s < 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if constexpr (TAB)  // the 16-lane row's own job
            x[i] = task_word<true>(a, r, 4 * s + i);
          else
            x[i] = s ? a.task[4 + i] : a.task[i];
        }
      } else {
        const uint32_t off = 16 * (s - 2);
        uint32_t w[4];
        ld16u(row, off, hdr, w);
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = __builtin_bswap32(w[i] & keep_mask(off + 4 * i, hdr));
      }
    } else if (s < N) {  // ciphertext block i: decrypt, store, hash
      const uint32_t i0 = s - na, off = 16 * i0;
      uint32_t cw[4], ks[4], pw[4];
      ld16u(row, po + off, po + ptl, cw);
      ctr[3] = __builtin_bswap32(i0 + 2);
      aes_encrypt<NR>(T, rk, ctr, ks);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t keep = keep_mask(off + 4 * i, ptl);
        x[i] = __builtin_bswap32(cw[i] & keep);
        pw[i] = (cw[i] ^ ks[i]) & keep;
      }
      *(uint4*)(pp + off) = make_uint4(pw[0], pw[1], pw[2], pw[3]);  // off + 16 <= pt_stride
    }
    // y = y H^16 ^ X for a lane that has a block in this round; the others keep their sum
    uint32_t p[4] = {y[0], y[1], y[2], y[3]};
    if (t) gf_mul(p, H16);
    if (s < N) {
#pragma unroll
      for (int i = 0; i < 4; i++) y[i] = p[i] ^ x[i];
    }
  }
  // lane j's last block is s = N - e + 1 for e = d + 2, d = (N mod G - 1 - j) mod G, and carries H^0
  const uint32_t rem = N % UP_G;
  uint32_t z[4];
  {
    const uint32_t src = (rem + UP_G - 1 - j) % UP_G;  // lane d = j takes the sum that needs H^d
#pragma unroll
    for (int i = 0; i < 4; i++) z[i] = (uint32_t)__shfl((int)y[i], (int)src, (int)UP_G);
  }
  gf_fold<0xB1>(z, H1, (j & 1u) != 0);   // quad_perm [1,0,3,2]
  gf_fold<0x4E>(z, H2, (j & 2u) != 0);   // quad_perm [2,3,0,1]
  gf_fold<0x141>(z, H4, (j & 4u) != 0);  // row_half_mirror (z is uniform within quads)
  gf_fold<0x140>(z, H8, (j & 8u) != 0);  // row_mirror (uniform within halves)
  // every lane of the group holds sum_d y_d H^d: tag = ((z H) ^ LEN) H ^ E_K(J0)
  gf_mul(z, H1);
  const uint32_t lw[4] = {0, aad_len * 8, 0, ptl * 8};
  ghash_block(z, lw, H1);
  ctr[3] = __builtin_bswap32(1u);
  uint32_t ek[4], tg[4];
  aes_encrypt<NR>(T, rk, ctr, ek);
  ld16u(row, po + ptl, po + pl, tg);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) diff |= (__builtin_bswap32(z[i]) ^ ek[i]) ^ tg[i];
  const bool ok = kem_ok && diff == 0;
  if (!ok)  // a failed open leaves no plaintext behind
    for (uint32_t i0 = j; i0 < nblk; i0 += UP_G) *(uint4*)(pp + 16 * i0) = make_uint4(0, 0, 0, 0);
  if (j == 0) {
    a.status[r] = ok ? 0 : PRIO3_UPLOAD_DECRYPT_FAILURE;
    if (!ok && pass == 0 && (a.sel[r] & 2u)) a.list[1][atomicAdd(a.cnt + 1, 1u)] = r;
  }
}

DEV uint32_t pt_be16(const uint8_t* p, uint32_t o) { return (uint32_t)p[o] << 8 | p[o + 1]; }

// one wave per report: the plaintext's decode and checks, then every output row (TAB: but the
// helper's rows, which the group form does not make on the device)
template <bool TAB>
__global__ __launch_bounds__(256) void k_up_finish(UpArgs a) {
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (r >= a.n) return;
  const uint32_t* f = a.fields + (size_t)JANUS_DAP_REPORT_FIELDS * r;
  const uint8_t* row = a.rows + (size_t)a.stride * r;
  uint8_t* pp = a.pt + (size_t)a.pt_stride * r;
  uint32_t st = a.status[r], el = 0, pay = 0;
  const uint32_t ptl = f[F_LPAY_LEN] >= 16 ? f[F_LPAY_LEN] - 16 : 0;
  if (st == 0) {
    // PlaintextInputShare::get_decoded: u16-prefixed extensions { u16 type (Tbd or Taskprov, the
    // codec's ExtensionType), u16-prefixed data }, u32-prefixed payload, nothing after it
    bool good = ptl >= 2;
    el = good ? pt_be16(pp, 0) : 0u;
    good = good && 2 + el <= ptl;
    uint32_t q = 2;
    while (good && q < 2 + el) {
      if (q + 4 > 2 + el) {
        good = false;
        break;
      }
      const uint32_t ty = pt_be16(pp, q), dl = pt_be16(pp, q + 2);
      if (q + 4 + dl > 2 + el || (ty != 0 && ty != 0xFF00u)) good = false;
      q += 4 + dl;
    }
    q = 2 + el;
    good = good && q + 4 <= ptl;
    const uint32_t pl = good ? (pt_be16(pp, q) << 16 | pt_be16(pp, q + 2)) : 0u;
    good = good && pl == ptl - q - 4 && pl == a.share_len;
    pay = q + 4;
    if (good) {  // Prio3 leader share: measurement and proofs shares of canonical elements, blind
      const uint32_t ne = (a.share_len - a.blind_len) / a.es;
      bool bad = false;
      if (a.es == 16) {
        for (uint32_t k = l; k < ne; k += 64) {
          uint32_t w[4];
          ld16u(pp, pay + 16 * k, ptl, w);
          // p = 0xffffffffffffffe4_0000000000000001
          const uint64_t hi = (uint64_t)w[3] << 32 | w[2], lo = (uint64_t)w[1] << 32 | w[0];
          bad = bad || hi > 0xffffffffffffffe4ull || (hi == 0xffffffffffffffe4ull && lo != 0);
        }
      } else {
        for (uint32_t k = l; k < (ne + 1) / 2; k += 64) {  // two Field64 elements per load
          uint32_t w[4];
          ld16u(pp, pay + 16 * k, pay + 8 * ne, w);
          bad = bad || (w[1] == 0xffffffffu && w[0] != 0) || (w[3] == 0xffffffffu && w[2] != 0);
        }
      }
      good = !__any(bad);
    }
    st = !good ? PRIO3_UPLOAD_DECODE_FAILURE : el > a.ext_stride ? PRIO3_UPLOAD_HOST : 0u;
  }
  const bool ok = st == 0;
  if (l == 0) {
    a.status[r] = (uint8_t)st;
    a.ext_len[r] = ok ? el : 0u;
    if (!ok) {
      a.times[r] = 0;
      a.hcfg[r] = 0;
      a.hct_len[r] = 0;
    }
  }
  if (!ok) {
    if (l < 16) a.ids[16 * (size_t)r + l] = 0;
    if constexpr (!TAB) {
      for (uint32_t k = l; k < a.henc_len; k += 64) a.henc[(size_t)a.henc_len * r + k] = 0;
      for (uint32_t k = l; k < a.hct_stride; k += 64) a.hct[(size_t)a.hct_stride * r + k] = 0;
    }
    for (uint32_t k = l; 16 * k < ptl; k += 64) *(uint4*)(pp + 16 * k) = make_uint4(0, 0, 0, 0);
  }
  for (uint32_t k = l; k < a.psl; k += 64) a.pub[(size_t)a.psl * r + k] = ok ? row[28 + k] : (uint8_t)0;
  uint32_t* so = (uint32_t*)(a.shares + (size_t)a.share_len * r);  // share_len % 8 == 0
  for (uint32_t k = l; k < a.share_len / 4; k += 64) {
    uint32_t v = 0;
    if (ok) {
      const uint32_t off = pay + 4 * k, al = off & ~3u, sh = 8 * (off & 3u);
      const uint32_t lo = *(const uint32_t*)(pp + al);
      const uint32_t hi = sh ? *(const uint32_t*)(pp + al + 4) : 0u;  // al + 4 < ptl <= pt_stride
      v = sh ? __builtin_amdgcn_alignbit(hi, lo, sh) : lo;
    }
    so[k] = v;
  }
  for (uint32_t k = l; k < a.ext_stride; k += 64)
    a.ext[(size_t)a.ext_stride * r + k] = ok && k < el ? pp[2 + k] : (uint8_t)0;
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the engine's option upload_aead (one lock per call)
int upload_aead_option(prio3_engine* e) {
  std::lock_guard<std::mutex> lk(e->mu);
  return e->upload_aead;
}
// the AEAD kernel an upload through opener o takes on engine e under option value opt:
// k_aead_open_wide or the one-lane body
bool upload_wide(const prio3_engine* e, const janus_hpke_opener* o, int opt) {
  const uint32_t expect = 6 + e->sz.leader_input_share_len + 16;  // a report without extensions
  return hpke_opener_aead(o) != JANUS_HPKE_AEAD_CHACHA20_POLY1305 &&
         (opt == 2 || (opt == 0 && expect >= UP_WIDE_MIN_PAYLOAD));
}

// One run of the chain: validated arguments, device buffers.
struct UpCall {
  janus_hpke_opener* op[2];  // the task's opener, the global one
  uint8_t cfg[2];
  uint32_t n, stride, ext_stride, henc_len, hct_stride;
  const uint8_t* rows;
  // outputs [n]...
  uint8_t *ids, *pub, *shares, *ext, *hcfg, *lcfg, *status;
  uint64_t* times;
  uint32_t *ext_len, *hct_len;
  // the one-task form: the launch's task and times, the row lengths, the helper's rows
  const uint8_t* task_id;
  uint64_t now, deadline, task_exp, expiry_age;
  const uint32_t* len;
  uint8_t *henc, *hct;
  // the group form (meta != nullptr; at most UPLOAD_MAX_GROUP reports): the staged meta and job
  // table, the list counters the group's DMA zeroed, the field table in the output block, the
  // AEAD choice of the group's key
  const UploadMeta* meta;
  const UploadJobRow* jtab;
  uint32_t *cnt, *fields;
  bool wide[2];
};

// The per-opener launches and k_up_finish over the m reports of a.
template <bool TAB>
int upload_open_finish(prio3_engine* e, UpArgs& a, janus_hpke_opener* const op[2],
                       const bool wide[2], uint32_t m, hipStream_t st) {
  for (int p = 0; p < 2; p++) {
    if (!op[p]) continue;
    TIMED(e, st, "k_up_gather", (k_up_gather<TAB><<<(m + 3) / 4, 256, 0, st>>>(a, p, !wide[p])));
    int hrc = PRIO3_OK;
    if (wide[p]) {
      TIMED(e, st, "k_hpke_keys",
            hrc = hpke_upload_keys_launch(op[p], m, a.enc, a.keys, a.list[p], a.cnt + p, st));
      if (hrc != PRIO3_OK) return hrc;
      const uint32_t blocks = (m + 256 / UP_G - 1) / (256 / UP_G);
      if (hpke_opener_aead(op[p]) == JANUS_HPKE_AEAD_AES_256_GCM)
        TIMED(e, st, "k_aead_open_wide",
              (k_aead_open_wide<14, TAB><<<blocks, 256, 0, st>>>(a, p)));
      else
        TIMED(e, st, "k_aead_open_wide",
              (k_aead_open_wide<10, TAB><<<blocks, 256, 0, st>>>(a, p)));
    } else {
      TIMED(e, st, "k_hpke_open",
            hrc = hpke_upload_open_launch(op[p], m, a.enc, a.ct, a.ct_len, a.pt_stride, a.aad,
                                          a.aad_len, a.aad_stride, a.pt, a.hst, a.list[p],
                                          a.cnt + p, st));
      if (hrc != PRIO3_OK) return hrc;
      TIMED(e, st, "k_up_post1", (k_up_post1<<<(m + 255) / 256, 256, 0, st>>>(a, p)));
    }
  }
  TIMED(e, st, "k_up_finish", (k_up_finish<TAB><<<(m + 3) / 4, 256, 0, st>>>(a)));
  return PRIO3_OK;
}

// The chain of call c on e's device (current) and stream st, in chunks of at most 65536 reports --
// fewer when the pool cannot give a whole chunk's scratch -- for both forms.
int upload_chain(prio3_engine* e, const UpCall& c, hipStream_t st) {
  const bool grp = c.meta != nullptr;
  const uint32_t n = c.n;
  if (grp && n > UPLOAD_MAX_GROUP) return PRIO3_EINVAL;
  const uint32_t psl = e->sz.public_share_len, L = e->sz.leader_input_share_len;
  UpArgs a{};
  a.stride = c.stride;
  a.psl = psl;
  a.share_len = L;
  a.blind_len = e->sz.joint_rand_len ? e->sz.prep_msg_len : 0;
  a.es = e->sz.field_bytes;
  a.ext_stride = c.ext_stride;
  a.pt_stride = (c.stride + 15) & ~15u;
  a.aad_stride = (60 + psl + 15) & ~15u;
  a.henc_len = c.henc_len;
  a.hct_stride = c.hct_stride;
  a.now = c.now;
  a.deadline = c.deadline;
  a.task_exp = c.task_exp;
  a.expiry_age = c.expiry_age;
  uint32_t encmax = 0;
  bool wide[2] = {false, false}, any_one = false;
  const int opt = grp ? 0 : upload_aead_option(e);
  for (int p = 0; p < 2; p++) {
    if (!c.op[p]) continue;
    a.has[p] = 1;
    a.cfg[p] = c.cfg[p];
    a.nenc[p] = (uint32_t)hpke_opener_nenc(c.op[p]);
    encmax = std::max(encmax, a.nenc[p]);
    wide[p] = grp ? c.wide[p] : upload_wide(e, c.op[p], opt);
    any_one = any_one || !wide[p];
  }
  for (int i = 0; c.task_id && i < 8; i++)
    a.task[i] = (uint32_t)c.task_id[4 * i] << 24 | (uint32_t)c.task_id[4 * i + 1] << 16 |
                (uint32_t)c.task_id[4 * i + 2] << 8 | c.task_id[4 * i + 3];
  a.jtab = c.jtab;
  // per-report scratch, each array 256-byte aligned: fields and malformed (the one-task form: the
  // group's fields are in its output block and its front keeps no malformed byte), sel, keys, enc,
  // plaintext, two lists; the one-lane AEAD's payload, AAD, lengths and status rows
  const size_t rows[12] = {grp ? 0u : 4u * JANUS_DAP_REPORT_FIELDS, grp ? 0u : 1u, 1, 48,
                           (encmax + 15) & ~15u, a.pt_stride, 4, 4,
                           any_one ? a.pt_stride : 0u, any_one ? a.aad_stride : 0u,
                           any_one ? 8u : 0u, any_one ? 1u : 0u};
  size_t per = 0;
  for (size_t b : rows) per += b;
  size_t chunk = std::min<size_t>(((size_t)n + 63) & ~(size_t)63, 65536);
  int rc = PRIO3_OK;
  Slab* slab = nullptr;
  for (;;) {  // all of a chunk's scratch or a smaller chunk
    slab = ws_acquire(e->device, per * chunk + 14 * 256, st, &rc);
    if (slab || chunk <= 64) break;
    chunk = std::max<size_t>(64, (chunk / 2) & ~(size_t)63);
  }
  if (!slab) return rc;
  uint8_t* arr[12];
  {
    uint8_t* b = slab->base + 256;  // the two list counters first
    for (int i = 0; i < 12; i++) {
      arr[i] = b;
      b += up256(rows[i] * chunk);
    }
  }
  a.cnt = grp ? c.cnt : (uint32_t*)slab->base;
  a.bad = arr[1];
  a.sel = arr[2];
  a.keys = (uint32_t*)arr[3];
  a.enc = arr[4];
  a.pt = arr[5];
  a.list[0] = (uint32_t*)arr[6];
  a.list[1] = (uint32_t*)arr[7];
  a.ct = arr[8];
  a.aad = arr[9];
  a.ct_len = (uint32_t*)arr[10];
  a.aad_len = a.ct_len + chunk;
  a.hst = arr[11];
  auto body = [&]() -> int {
    for (uint64_t off = 0; off < n; off += chunk) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
      a.n = m;
      a.rows = c.rows + (size_t)c.stride * off;
      a.ids = c.ids + 16 * off;
      a.times = c.times + off;
      a.lcfg = c.lcfg + off;
      a.hcfg = c.hcfg + off;
      a.henc = c.henc ? c.henc + (size_t)c.henc_len * off : nullptr;
      a.hct = c.hct ? c.hct + (size_t)c.hct_stride * off : nullptr;
      a.hct_len = c.hct_len + off;
      a.status = c.status + off;
      a.pub = c.pub ? c.pub + (size_t)psl * off : nullptr;
      a.shares = c.shares + (size_t)L * off;
      a.ext = c.ext ? c.ext + (size_t)c.ext_stride * off : nullptr;
      a.ext_len = c.ext_len + off;
      // the counters: the group's first chunk finds them zeroed by its DMA
      if (!grp || off) HIPCHK(hipMemsetAsync(a.cnt, 0, 8, st));
      if (grp) {
        a.meta = c.meta + off;
        a.fields = c.fields + (size_t)JANUS_DAP_REPORT_FIELDS * off;
        TIMED(e, st, "k_up_front", (k_up_front<<<(m + 3) / 4, 256, 0, st>>>(a)));
      } else {
        a.fields = (uint32_t*)arr[0];
        int drc = 0;
        TIMED(e, st, "k_rep_decode",
              drc = janus_dap_report_decode_device(m, a.rows, c.stride, c.len + off, a.ids, a.times,
                                                   a.fields, a.lcfg, a.hcfg, a.henc, c.henc_len,
                                                   a.hct, a.hct_len, c.hct_stride, a.bad, st));
        if (drc) return drc == JANUS_DAP_EDEVICE ? PRIO3_EDEVICE : PRIO3_EINVAL;
        TIMED(e, st, "k_up_pre", (k_up_pre<<<(m + 255) / 256, 256, 0, st>>>(a)));
      }
      const int orc = grp ? upload_open_finish<true>(e, a, c.op, wide, m, st)
                          : upload_open_finish<false>(e, a, c.op, wide, m, st);
      if (orc != PRIO3_OK) return orc;
    }
    return PRIO3_OK;
  };
  rc = body();
  ws_release(slab, st);
  return rc;
}

}  // namespace

extern "C" int prio3_device_leader_upload(
    prio3_engine* e, janus_hpke_opener* task_opener, uint8_t task_config_id,
    janus_hpke_opener* global_opener, uint8_t global_config_id, uint32_t n,
    const uint8_t task_id[32], uint64_t now, uint64_t report_deadline, uint64_t task_expiration,
    uint64_t report_expiry_age, const uint8_t* d_reports, uint32_t report_stride,
    const uint32_t* d_report_len, uint8_t* d_report_ids, uint64_t* d_times,
    uint8_t* d_public_shares, uint8_t* d_leader_input_shares, uint8_t* d_extensions,
    uint32_t* d_ext_len, uint32_t ext_stride, uint8_t* d_helper_config_ids, uint8_t* d_helper_enc,
    uint32_t helper_enc_len, uint8_t* d_helper_ct, uint32_t* d_helper_ct_len,
    uint32_t helper_ct_stride, uint8_t* d_leader_config_ids, uint8_t* d_status, void* stream) {
  if (!e) return PRIO3_EINVAL;
  if (e->dp.kind == PRIO3_FPVEC_BOUNDED_L2) return PRIO3_EUNSUPPORTED;
  janus_hpke_opener* op[2] = {task_opener, global_opener};
  if ((!op[0] && !op[1]) || !task_id || report_stride % 4 != 0 || ext_stride % 4 != 0 ||
      report_stride >= (1u << 31) || helper_enc_len > 0xFFFF || ((uintptr_t)d_reports & 3u))
    return PRIO3_EINVAL;
  for (auto* o : op)
    if (o && hpke_opener_device(o) != e->device) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  const uint32_t psl = e->sz.public_share_len;
  if (!d_reports || !d_report_len || !d_report_ids || !d_times || !d_leader_input_shares ||
      !d_ext_len || !d_helper_config_ids || !d_helper_ct_len || !d_leader_config_ids || !d_status ||
      (psl && !d_public_shares) || (ext_stride && !d_extensions) ||
      (helper_enc_len && !d_helper_enc) || (helper_ct_stride && !d_helper_ct))
    return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  UpCall c{};
  c.op[0] = op[0];
  c.op[1] = op[1];
  c.cfg[0] = task_config_id;
  c.cfg[1] = global_config_id;
  c.n = n;
  c.stride = report_stride;
  c.ext_stride = ext_stride;
  c.henc_len = helper_enc_len;
  c.hct_stride = helper_ct_stride;
  c.rows = d_reports;
  c.ids = d_report_ids;
  c.times = d_times;
  c.pub = d_public_shares;
  c.shares = d_leader_input_shares;
  c.ext = d_extensions;
  c.ext_len = d_ext_len;
  c.hcfg = d_helper_config_ids;
  c.hct_len = d_helper_ct_len;
  c.lcfg = d_leader_config_ids;
  c.status = d_status;
  c.task_id = task_id;
  c.now = now;
  c.deadline = report_deadline;
  c.task_exp = task_expiration;
  c.expiry_age = report_expiry_age;
  c.len = d_report_len;
  c.henc = d_helper_enc;
  c.hct = d_helper_ct;
  return upload_chain(e, c, (hipStream_t)stream);
}

extern "C" int prio3_leader_upload_batch(
    prio3_engine* e, janus_hpke_opener* task_opener, uint8_t task_config_id,
    janus_hpke_opener* global_opener, uint8_t global_config_id, uint32_t n,
    const uint8_t task_id[32], uint64_t now, uint64_t report_deadline, uint64_t task_expiration,
    uint64_t report_expiry_age, const uint8_t* reports, uint32_t report_stride,
    const uint32_t* report_len, uint8_t* report_ids, uint64_t* times, uint8_t* public_shares,
    uint8_t* leader_input_shares, uint8_t* extensions, uint32_t* ext_len, uint32_t ext_stride,
    uint8_t* helper_config_ids, uint8_t* helper_enc, uint32_t helper_enc_len, uint8_t* helper_ct,
    uint32_t* helper_ct_len, uint32_t helper_ct_stride, uint8_t* leader_config_ids,
    uint8_t* status) {
  if (!e) return PRIO3_EINVAL;
  if (e->dp.kind == PRIO3_FPVEC_BOUNDED_L2) return PRIO3_EUNSUPPORTED;
  if ((!task_opener && !global_opener) || !task_id || report_stride % 4 != 0 ||
      ext_stride % 4 != 0 || report_stride >= (1u << 31) || helper_enc_len > 0xFFFF)
    return PRIO3_EINVAL;
  for (auto* o : {task_opener, global_opener})
    if (o && hpke_opener_device(o) != e->device) return PRIO3_EINVAL;
  if (n == 0) return PRIO3_OK;
  const size_t psl = e->sz.public_share_len, L = e->sz.leader_input_share_len;
  if (!reports || !report_len || !report_ids || !times || !leader_input_shares || !ext_len ||
      !helper_config_ids || !helper_ct_len || !leader_config_ids || !status ||
      (psl && !public_shares) || (ext_stride && !extensions) || (helper_enc_len && !helper_enc) ||
      (helper_ct_stride && !helper_ct))
    return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = ws_stream_get(e->device);
  if (!st) return PRIO3_EDEVICE;
  // inputs 0-1, outputs 2-12
  const size_t sizes[13] = {(size_t)report_stride * n, 4 * (size_t)n, 16 * (size_t)n, 8 * (size_t)n,
                            psl * n, L * n, (size_t)ext_stride * n, 4 * (size_t)n, n,
                            (size_t)helper_enc_len * n, (size_t)helper_ct_stride * n, 4 * (size_t)n,
                            2 * (size_t)n};
  size_t offs[14] = {0};
  for (int i = 0; i < 13; i++) offs[i + 1] = offs[i] + up256(sizes[i]);
  int rc = PRIO3_OK;
  Slab* slab = ws_acquire(e->device, offs[13], st, &rc);
  if (slab) {
    uint8_t* b = slab->base;
    const void* src[2] = {reports, report_len};
    void* dst[11] = {report_ids, times, public_shares, leader_input_shares, extensions, ext_len,
                     helper_config_ids, helper_enc, helper_ct, helper_ct_len, nullptr};
    for (int i = 0; i < 2 && rc == PRIO3_OK; i++)
      if (hipMemcpyAsync(b + offs[i], src[i], sizes[i], hipMemcpyHostToDevice, st) != hipSuccess)
        rc = PRIO3_EDEVICE;
    uint8_t* tail = b + offs[12];  // leader config IDs [n], status [n]
    if (rc == PRIO3_OK)
      rc = prio3_device_leader_upload(
          e, task_opener, task_config_id, global_opener, global_config_id, n, task_id, now,
          report_deadline, task_expiration, report_expiry_age, b + offs[0],
          report_stride, (const uint32_t*)(b + offs[1]), b + offs[2], (uint64_t*)(b + offs[3]),
          psl ? b + offs[4] : nullptr, b + offs[5], ext_stride ? b + offs[6] : nullptr,
          (uint32_t*)(b + offs[7]), ext_stride, b + offs[8], helper_enc_len ? b + offs[9] : nullptr,
          helper_enc_len, helper_ct_stride ? b + offs[10] : nullptr, (uint32_t*)(b + offs[11]),
          helper_ct_stride, tail, tail + n, st);
    for (int i = 0; i < 10 && rc == PRIO3_OK; i++)
      if (sizes[2 + i] && hipMemcpyAsync(dst[i], b + offs[2 + i], sizes[2 + i],
                                         hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = PRIO3_EDEVICE;
    if (rc == PRIO3_OK &&
        (hipMemcpyAsync(leader_config_ids, tail, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipMemcpyAsync(status, tail + n, n, hipMemcpyDeviceToHost, st) != hipSuccess))
      rc = PRIO3_EDEVICE;
    if (hipStreamSynchronize(st) != hipSuccess && rc == PRIO3_OK) rc = PRIO3_EDEVICE;
    ws_release(slab, st);
  }
  ws_stream_put(e->device, st);
  return rc;
}

// ---- the upload executor's hooks (prio3_runtime.h) ----
bool upload_job_wide(prio3_engine* e, const janus_hpke_opener* o) {
  return upload_wide(e, o, upload_aead_option(e));
}

size_t upload_report_bytes(const UploadJob* j) {
  return (size_t)j->stride + sizeof(UploadMeta) + 4 * JANUS_DAP_REPORT_FIELDS + 8 + 16 + 4 + 4 +
         (size_t)j->e->sz.public_share_len + j->e->sz.leader_input_share_len + j->ext_stride + 3;
}

void upload_out_layout(const UploadLayout& L, uint32_t n, UploadOut* O) {
  size_t off = 0;
  auto take = [&](size_t per) {
    const size_t at = off;
    off += up256(per * n);
    return at;
  };
  O->fields = take(4 * JANUS_DAP_REPORT_FIELDS);
  O->times = take(8);
  O->ids = take(16);
  O->ext_len = take(4);
  O->hct_len = take(4);
  O->pub = take(L.psl);
  O->shares = take(L.share_len);
  O->ext = take(L.ext_stride);
  O->hcfg = take(1);
  O->lcfg = take(1);
  O->status = take(1);
  O->bytes = off;
}

void upload_layout(const UploadJob* j, uint32_t cap, UploadLayout* L) {
  L->cap = cap;
  L->stride = j->stride;
  L->psl = j->e->sz.public_share_len;
  L->share_len = j->e->sz.leader_input_share_len;
  L->ext_stride = j->ext_stride;
  L->tab_off = 256;  // the head: the chain's list counters
  L->meta_off = L->tab_off + up256(sizeof(UploadJobRow) * UPLOAD_MAX_JOBS);
  L->rows_off = L->meta_off + up256(sizeof(UploadMeta) * (size_t)cap);
  L->out_off = L->rows_off + up256((size_t)j->stride * cap);
  UploadOut O;
  upload_out_layout(*L, cap, &O);
  L->out_bytes = O.bytes;
  L->bytes = L->out_off + O.bytes;
}

uint64_t upload_group_key(const UploadJob* j) {
  uint64_t h = engine_group_key(j->e);
  auto mix = [&](uint64_t x) { h = (h ^ x) * 1099511628211ull; };
  for (int p = 0; p < 2; p++) {
    mix((uint64_t)(uintptr_t)j->op[p]);
    mix(j->op[p] ? hpke_opener_key(j->op[p]) : 0);
    mix(j->cfg[p]);
    mix(j->wide[p]);
  }
  mix(j->stride);
  mix(j->ext_stride);
  mix(j->henc_len);
  mix(j->hct_stride);
  return h;
}

int upload_group_issue(const UploadJob& pj, const UploadLayout& L, uint8_t* stg, uint32_t n,
                       uint32_t njobs, UploadRun* r, bool own_queue) {
  prio3_engine* e = pj.e;
  *r = UploadRun();
  if (n == 0 || n > L.cap || njobs == 0 || njobs > UPLOAD_MAX_JOBS) return PRIO3_EINVAL;
  DeviceGuard dg_(e->device);
  HIPCHK(dg_.rc);
  hipStream_t st = own_queue ? ws_exec_stream_get(e->device) : ws_stream_get(e->device);
  if (!st) return PRIO3_EDEVICE;
  UploadOut O;
  upload_out_layout(L, n, &O);
  // the device area: the staged head, table and meta as they lie in the staging, the rows, the
  // output block
  const size_t in_bytes = L.meta_off + sizeof(UploadMeta) * (size_t)n;
  const size_t d_rows = up256(in_bytes), row_bytes = (size_t)L.stride * n;
  const size_t d_out = d_rows + up256(row_bytes);
  int rc = PRIO3_OK;
  Slab* sl = ws_acquire(e->device, d_out + O.bytes, st, &rc);
  if (!sl) {
    ws_exec_stream_put(e->device, st);
    return rc;
  }
  uint8_t* b = sl->base;
  uint8_t* o = b + d_out;
  if (hipMemcpyAsync(b, stg, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
      (row_bytes && hipMemcpyAsync(b + d_rows, stg + L.rows_off, row_bytes, hipMemcpyHostToDevice,
                                   st) != hipSuccess))
    rc = PRIO3_EDEVICE;
  if (rc == PRIO3_OK) {
    UpCall c{};
    c.op[0] = pj.op[0];
    c.op[1] = pj.op[1];
    c.cfg[0] = pj.cfg[0];
    c.cfg[1] = pj.cfg[1];
    c.n = n;
    c.stride = L.stride;
    c.ext_stride = L.ext_stride;
    c.henc_len = pj.henc_len;
    c.hct_stride = pj.hct_stride;
    c.rows = b + d_rows;
    c.ids = o + O.ids;
    c.times = (uint64_t*)(o + O.times);
    c.pub = L.psl ? o + O.pub : nullptr;
    c.shares = o + O.shares;
    c.ext = L.ext_stride ? o + O.ext : nullptr;
    c.ext_len = (uint32_t*)(o + O.ext_len);
    c.hcfg = o + O.hcfg;
    c.hct_len = (uint32_t*)(o + O.hct_len);
    c.lcfg = o + O.lcfg;
    c.status = o + O.status;
    c.meta = (const UploadMeta*)(b + L.meta_off);
    c.jtab = (const UploadJobRow*)(b + L.tab_off);
    c.cnt = (uint32_t*)b;
    c.fields = (uint32_t*)(o + O.fields);
    c.wide[0] = pj.wide[0];
    c.wide[1] = pj.wide[1];
    rc = upload_chain(e, c, st);
  }
  if (rc == PRIO3_OK &&
      hipMemcpyAsync(stg + L.out_off, o, O.bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = PRIO3_EDEVICE;
  if (rc != PRIO3_OK) {
    (void)hipStreamSynchronize(st);
    ws_release(sl, st);
    ws_exec_stream_put(e->device, st);
    return rc;
  }
  r->device = e->device;
  r->st = st;
  r->slab = sl;
  r->lead = e;
  return PRIO3_OK;
}

void upload_group_collect(prio3_engine* lead) {
  if (lead && lead->timing) collect_times(lead, false);
}

// dap_codec.hip -- DAP-09 wire format <-> SoA marshaling for both roles' aggregation-job init
// on MI355X (gfx950); SURVEY 8(f) row 3.  See include/janus_dap.h for the encodings.
//
//  k_unpack_check / k_unpack_gather
//                 the speculative uniform layout (every PrepareInit has the first one's
//                 length): one lane per record validates its length and type fields; then one
//                 lane per OUTPUT DWORD gathers the byte fields (report ID, public share, enc,
//                 payload, leader prep share) into the SoA buffers the HPKE opener and the
//                 prio3 engine read -- coalesced reads of the body and coalesced writes.
//  k_resp_count / k_resp_scan / k_resp_write
//                 AggregationJobResp: per-block counts of the two PrepareResp sizes, an
//                 exclusive scan of the block totals, then each lane writes its record at its
//                 byte offset (block-local prefix via __syncthreads_count-style LDS scan).
//  k_req_count / k_req_scan / k_req_write
//                 leader: AggregationJobInitializeReq from the SoA buffers; records differ in
//                 length (ct_len) and failed reports are left out, so a scan over byte lengths
//                 gives each report its offset; one lane per aligned output dword.
//  k_runp_index / k_runp_check / k_runp_gather
//                 leader: AggregationJobResp into prepare messages and per-report errors; one
//                 workgroup indexes the three regular record shapes speculatively, then the
//                 parallel passes compare report IDs and gather the messages.
//  k_rep_write    client: one Report row per report from the SoA buffers and the sealer's rows.
//  k_rep_decode   leader upload: the inverse, one wave per Report row -- the field offsets and
//                 lengths, the small fields, the helper's ciphertext rows and a malformed flag.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/janus_dap.h"
#include "dap_report.h"
#include "prio3_runtime.h"

#define DEV __device__ __forceinline__

namespace {

// big-endian reads at an arbitrary byte offset of a device buffer (dword-aligned loads)
DEV uint32_t ld_be32(const uint8_t* base, uint64_t off) {
  const uint64_t a = off & ~3ull;
  const uint32_t sh = (uint32_t)(off & 3u);
  const uint32_t lo = *(const uint32_t*)(base + a);
  const uint32_t hi = sh ? *(const uint32_t*)(base + a + 4) : 0u;
  const uint32_t le = sh ? __builtin_amdgcn_alignbit(hi, lo, 8 * sh) : lo;
  return __builtin_bswap32(le);
}
DEV uint32_t ld_u8(const uint8_t* base, uint64_t off) { return base[off]; }
DEV uint32_t ld_be16(const uint8_t* base, uint64_t off) {
  return (ld_u8(base, off) << 8) | ld_u8(base, off + 1);
}
// little-endian word (memory order) at an arbitrary byte offset
DEV uint32_t ld_le32(const uint8_t* base, uint64_t off) {
  const uint64_t a = off & ~3ull;
  const uint32_t sh = (uint32_t)(off & 3u);
  const uint32_t lo = *(const uint32_t*)(base + a);
  if (!sh) return lo;
  const uint32_t hi = *(const uint32_t*)(base + a + 4);
  return __builtin_amdgcn_alignbit(hi, lo, 8 * sh);
}
struct UnpackArgs {
  const uint8_t* body;
  uint64_t list_off;
  uint32_t n, rec, psl, enc_len, pay_len, msg_len, ps_len;
  uint8_t *cfg, *msg_status;
  uint64_t* times;
  uint32_t *ct_len, *mismatch;
};

// The body buffer must be readable up to a dword past its end (the host pads the copy).
// k_unpack_check: one lane per record, only the length / type fields (a few scattered loads):
// validates the record against the first record's shape and writes the small per-report
// outputs (time, config id, payload length, message status).
__global__ __launch_bounds__(256) void k_unpack_check(UnpackArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const uint8_t* b = a.body;
  uint64_t o = a.list_off + (uint64_t)r * a.rec;
  const uint64_t end = o + a.rec;
  const uint64_t o_time = o + 16;
  o += 24;
  const uint32_t psl = ld_be32(b, o);
  o += 4 + (uint64_t)psl;
  bool ok = psl == a.psl && o + 3 <= end;
  const uint32_t cfg = ok ? ld_u8(b, o) : 0u;
  const uint32_t encl = ok ? ld_be16(b, o + 1) : 0u;
  o += 3 + (uint64_t)encl;
  ok = ok && encl == a.enc_len && o + 4 <= end;
  const uint32_t payl = ok ? ld_be32(b, o) : 0u;
  o += 4 + (uint64_t)payl;
  ok = ok && payl == a.pay_len && o + 4 <= end;
  const uint32_t msgl = ok ? ld_be32(b, o) : 0u;
  const uint64_t o_msg = o + 4;
  ok = ok && msgl == a.msg_len && o_msg + msgl == end;
  if (!ok) {
    atomicAdd(a.mismatch, 1u);
    a.msg_status[r] = 2;
    return;
  }
  // PingPongMessage: Initialize { u32-prefixed prep_share } expected (ping_pong.rs framing,
  // messages/src/tests/aggregation.rs:201-209)
  const uint32_t ty = ld_u8(b, o_msg);
  const uint32_t psl2 = msgl >= 5 ? ld_be32(b, o_msg + 1) : 0xffffffffu;
  // a message that does not decode rejects the whole request: leave it to the host parser
  bool wf = msgl >= 5 && ty <= 2;
  if (wf && ty != 1) wf = (uint64_t)msgl == 5 + (uint64_t)psl2;
  if (wf && ty == 1)
    wf = 9 + (uint64_t)psl2 <= msgl &&
         (uint64_t)msgl == 9 + (uint64_t)psl2 + ld_be32(b, o_msg + 5 + psl2);
  if (!wf) {
    atomicAdd(a.mismatch, 1u);
    a.msg_status[r] = 2;
    return;
  }
  uint8_t st = 0;
  if (ty != 0)
    st = 5;  // PeerMessageMismatch
  else if (psl2 != a.ps_len)
    st = 2;  // CodecPrepShare
  a.msg_status[r] = st;
  a.times[r] = ((uint64_t)ld_be32(b, o_time) << 32) | ld_be32(b, o_time + 4);
  a.cfg[r] = (uint8_t)cfg;
  a.ct_len[r] = a.pay_len;
}

// k_unpack_gather: the byte fields, one output dword per lane (grid.y = field): adjacent lanes
// read adjacent source bytes of the uniform records and write adjacent output dwords, so both
// sides are coalesced.  Output rows are `row` bytes, the field is `len` bytes at `off` within
// each record; bytes past `len` in a row are zeroed.  Rows that are not a multiple of 4 bytes
// (no Prio3 / X25519 field has one, but the ABI allows it) take a bytewise branch.
struct GatherField {
  uint8_t* dst;
  uint32_t row, len, off;
};
struct GatherArgs {
  const uint8_t* body;
  uint64_t list_off;
  uint32_t n, rec;
  GatherField f[5];
};
__global__ __launch_bounds__(256) void k_unpack_gather(GatherArgs g) {
  const GatherField F = g.f[blockIdx.y];
  if (!F.dst) return;
  const uint64_t total = (uint64_t)g.n * F.row;  // output bytes
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * i >= total) return;
  if ((F.row & 3u) == 0) {
    const uint32_t wpr = F.row >> 2;
    const uint32_t r = (uint32_t)(i / wpr), b = 4 * (uint32_t)(i - (uint64_t)r * wpr);
    uint32_t v = 0;
    if (b < F.len) {
      v = ld_le32(g.body, g.list_off + (uint64_t)r * g.rec + F.off + b);
      if (b + 4 > F.len) v &= (1u << (8 * (F.len - b))) - 1u;
    }
    ((uint32_t*)F.dst)[i] = v;
    return;
  }
  for (uint32_t k = 0; k < 4; k++) {
    const uint64_t j = 4 * i + k;
    if (j >= total) break;
    const uint32_t r = (uint32_t)(j / F.row), c = (uint32_t)(j - (uint64_t)r * F.row);
    F.dst[j] = c < F.len ? g.body[g.list_off + (uint64_t)r * g.rec + F.off + c] : 0;
  }
}

// ---- AggregationJobResp ----------------------------------------------------------------
// record sizes: Continue{Finish{prep_msg}} = 16 + 1 + 4 + 1 + 4 + pml; Reject = 16 + 1 + 1
DEV bool resp_ok(const uint8_t* pe, const uint8_t* st, uint32_t r) {
  return pe[r] == 0xFF && st[r] == 0;
}

__global__ __launch_bounds__(256) void k_resp_count(uint32_t n, const uint8_t* pe,
                                                    const uint8_t* st, uint32_t* blk) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const int ok = r < n && resp_ok(pe, st, r);
  const int c = __syncthreads_count(ok);
  if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)c;
}

// exclusive scan of the per-block ok counts (one block of 1024 threads, sequential chunks)
__global__ __launch_bounds__(1024) void k_resp_scan(uint32_t nb, uint32_t* blk, uint32_t n,
                                                    uint32_t pml, uint64_t* out_len,
                                                    uint8_t* out) {
  __shared__ uint32_t s[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? blk[i] : 0u;
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
      const uint32_t t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
      __syncthreads();
      s[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nb) blk[i] = carry + s[threadIdx.x] - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint64_t n_ok = carry;
    const uint64_t body = n_ok * (26ull + pml) + ((uint64_t)n - n_ok) * 18ull;
    *out_len = 4 + body;
    out[0] = (uint8_t)(body >> 24);  // u32-prefixed PrepareResp list
    out[1] = (uint8_t)(body >> 16);
    out[2] = (uint8_t)(body >> 8);
    out[3] = (uint8_t)body;
  }
}

__global__ __launch_bounds__(256) void k_resp_write(uint32_t n, const uint8_t* ids,
                                                    const uint8_t* pe, const uint8_t* st,
                                                    const uint8_t* pm, uint32_t pml,
                                                    const uint32_t* blk, uint8_t* out) {
  __shared__ uint32_t s[256];
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ok = (r < n && resp_ok(pe, st, r)) ? 1u : 0u;
  s[threadIdx.x] = ok;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if (r >= n) return;
  const uint64_t oks_before = (uint64_t)blk[blockIdx.x] + s[threadIdx.x] - ok;
  const uint64_t before = r;  // records before r
  uint64_t o = 4 + oks_before * (26ull + pml) + (before - oks_before) * 18ull;
  for (int i = 0; i < 16; i++) out[o + i] = ids[16 * (size_t)r + i];
  o += 16;
  if (ok) {
    const uint32_t ml = 5 + pml;  // PingPongMessage::Finish { prep_msg }
    out[o] = 0;                   // PrepareStepResult::Continue
    out[o + 1] = (uint8_t)(ml >> 24);
    out[o + 2] = (uint8_t)(ml >> 16);
    out[o + 3] = (uint8_t)(ml >> 8);
    out[o + 4] = (uint8_t)ml;
    out[o + 5] = 2;  // PingPongMessage type Finish
    out[o + 6] = (uint8_t)(pml >> 24);
    out[o + 7] = (uint8_t)(pml >> 16);
    out[o + 8] = (uint8_t)(pml >> 8);
    out[o + 9] = (uint8_t)pml;
    for (uint32_t i = 0; i < pml; i++) out[o + 10 + i] = pm[(size_t)pml * r + i];
  } else {
    out[o] = 2;  // PrepareStepResult::Reject
    out[o + 1] = pe[r] != 0xFF ? pe[r] : 5;  // PrepareError (VdafPrepError for prio3 failures)
  }
}

// ---- leader side: AggregationJobInitializeReq encode --------------------------------------
// record: id[16] time[8] psl[4] pub | cfg[1] enc_len[2] enc | ct_len[4] ct | ml[4] 0 ps[4] share
// = 44 + public_share_len + enc_len + ct_len + prep_share_len bytes.  A report takes part when
// its leader status is 0 and its ct_len fits the row.
constexpr uint32_t REQ_FIXED = 44;
constexpr uint32_t REQ_CHUNK = 256;   // records per block of the count / write kernels
constexpr uint32_t REQ_HDR_MAX = 4 + 256 + 1 + 32 + 4;

struct ReqHdr {  // the body's bytes before the first PrepareInit (list length filled on the device)
  uint8_t b[REQ_HDR_MAX];
  uint32_t len;
};
struct ReqArgs {
  uint32_t n, psl, enc_len, ct_stride, ps_len;
  const uint8_t *ids, *pub, *cfg, *enc, *ct, *ps, *status;
  const uint64_t* times;
  const uint32_t* ct_len;
  uint64_t* blk_bytes;  // [nb] per-chunk byte totals, then their exclusive scan
  uint32_t* blk_cnt;    // [nb] per-chunk record counts, then their exclusive scan
  uint32_t* rel;        // [n] chunk-local inclusive scan of the record lengths
  uint8_t* out;
  uint64_t* out_len;
  uint32_t *index, *n_included, *err;  // err[0]: reports left out for ct_len > ct_stride,
                                       // err[1]: the list does not fit a u32 (nothing written)
};

DEV uint32_t req_len(const ReqArgs& a, uint32_t r, bool count_oversize) {
  if (r >= a.n || a.status[r] != 0) return 0;
  const uint32_t cl = a.ct_len[r];
  if (cl > a.ct_stride) {
    if (count_oversize) atomicAdd(&a.err[0], 1u);
    return 0;
  }
  return REQ_FIXED + a.psl + a.enc_len + a.ps_len + cl;  // host checked: no u32 overflow
}

// k_req_count: the chunk-local inclusive scans of the record lengths and of the included
// reports (Hillis-Steele in LDS): rel[r] = bytes of the chunk up to and including report r,
// index[r] = its position among the chunk's included reports (the write kernel adds the chunk's
// base), and the chunk totals for k_req_scan
__global__ __launch_bounds__(256) void k_req_count(ReqArgs a) {
  __shared__ uint64_t s[256];
  __shared__ uint32_t c[256];
  const uint32_t t = threadIdx.x, r = blockIdx.x * REQ_CHUNK + t;
  const uint32_t len = req_len(a, r, true);
  s[t] = len;
  c[t] = len != 0;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t ts = t >= d ? s[t - d] : 0ull;
    const uint32_t tc = t >= d ? c[t - d] : 0u;
    __syncthreads();
    s[t] += ts;
    c[t] += tc;
    __syncthreads();
  }
  if (r < a.n) {
    a.rel[r] = (uint32_t)s[t];  // meaningless when the chunk passes 2^32: nothing is written then
    a.index[r] = len ? c[t] - 1 : 0xFFFFFFFFu;
  }
  if (t == 255) {
    a.blk_bytes[blockIdx.x] = s[255];
    a.blk_cnt[blockIdx.x] = c[255];
  }
}

// exclusive scans of the per-chunk byte totals and counts (one block, sequential 1024-chunk
// tiles, as k_resp_scan), then the header, the list length and the totals
__global__ __launch_bounds__(1024) void k_req_scan(uint32_t nb, ReqArgs a, ReqHdr h) {
  __shared__ uint64_t sb[1024];
  __shared__ uint32_t sc[1024];
  __shared__ uint64_t carry_b;
  __shared__ uint32_t carry_c;
  if (threadIdx.x == 0) {
    carry_b = 0;
    carry_c = 0;
  }
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t vb = i < nb ? a.blk_bytes[i] : 0ull;
    const uint32_t vc = i < nb ? a.blk_cnt[i] : 0u;
    sb[threadIdx.x] = vb;
    sc[threadIdx.x] = vc;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      const uint64_t tb = threadIdx.x >= d ? sb[threadIdx.x - d] : 0ull;
      const uint32_t tc = threadIdx.x >= d ? sc[threadIdx.x - d] : 0u;
      __syncthreads();
      sb[threadIdx.x] += tb;
      sc[threadIdx.x] += tc;
      __syncthreads();
    }
    if (i < nb) {
      a.blk_bytes[i] = carry_b + sb[threadIdx.x] - vb;
      a.blk_cnt[i] = carry_c + sc[threadIdx.x] - vc;
    }
    __syncthreads();
    if (threadIdx.x == 1023) {
      carry_b += sb[1023];
      carry_c += sc[1023];
    }
    __syncthreads();
  }
  const uint64_t list = carry_b;
  const bool fits = list <= 0xFFFFFFFFull;
  if (fits && threadIdx.x < h.len - 4) a.out[threadIdx.x] = h.b[threadIdx.x];
  if (threadIdx.x == 0) {
    a.err[1] = fits ? 0u : 1u;
    *a.out_len = fits ? h.len + list : 0ull;
    *a.n_included = fits ? carry_c : 0u;
    if (fits) {
      uint8_t* p = a.out + h.len - 4;
      p[0] = (uint8_t)(list >> 24);
      p[1] = (uint8_t)(list >> 16);
      p[2] = (uint8_t)(list >> 8);
      p[3] = (uint8_t)list;
    }
  }
}

// byte k (k < record length) of report r's PrepareInit; cl = its ct_len
DEV uint32_t req_byte(const ReqArgs& a, uint32_t r, uint32_t cl, uint32_t k) {
  if (k < 16) return a.ids[16 * (size_t)r + k];
  if (k < 24) return (uint32_t)(a.times[r] >> (8 * (23 - k))) & 0xFFu;
  if (k < 28) return (a.psl >> (8 * (27 - k))) & 0xFFu;
  k -= 28;
  if (k < a.psl) return a.pub[(size_t)a.psl * r + k];
  k -= a.psl;
  if (k == 0) return a.cfg[r];
  if (k < 3) return (a.enc_len >> (8 * (2 - k))) & 0xFFu;
  k -= 3;
  if (k < a.enc_len) return a.enc[(size_t)a.enc_len * r + k];
  k -= a.enc_len;
  if (k < 4) return (cl >> (8 * (3 - k))) & 0xFFu;
  k -= 4;
  if (k < cl) return a.ct[(size_t)a.ct_stride * r + k];
  k -= cl;
  if (k < 4) return ((5 + a.ps_len) >> (8 * (3 - k))) & 0xFFu;
  if (k == 4) return 0;  // PingPongMessage::Initialize
  if (k < 9) return (a.ps_len >> (8 * (8 - k))) & 0xFFu;
  return a.ps[(size_t)a.ps_len * r + (k - 9)];
}

// the four source bytes of record bytes [k, k + 4) when they lie inside one byte field whose
// array (base, `total` bytes, dword-aligned) covers the two aligned dwords ld_le32 reads
DEV bool req_field_dword(const uint8_t* base, uint64_t total, uint64_t row_off, uint32_t fs,
                         uint32_t flen, uint32_t k, uint32_t* v) {
  if (k < fs || k + 4 > fs + flen) return false;
  const uint64_t off = row_off + (k - fs);
  if (((uintptr_t)base & 3u) || (off & ~3ull) + ((off & 3u) ? 8 : 4) > total) return false;
  *v = ld_le32(base, off);
  return true;
}

// value of the aligned output dword holding record bytes [k, k + 4) of report r (k + 4 <= its
// length): a dword read of the field row when the four bytes lie in one byte field, else bytewise
DEV uint32_t req_dword(const ReqArgs& a, uint32_t r, uint32_t cl, uint32_t k) {
  const uint32_t f_pub = 28, f_enc = f_pub + a.psl + 3, f_ct = f_enc + a.enc_len + 4,
                 f_ps = f_ct + cl + 9;
  uint32_t v;
  if (req_field_dword(a.ps, (uint64_t)a.n * a.ps_len, (uint64_t)a.ps_len * r, f_ps, a.ps_len, k, &v) ||
      req_field_dword(a.ct, (uint64_t)a.n * a.ct_stride, (uint64_t)a.ct_stride * r, f_ct, cl, k, &v) ||
      req_field_dword(a.pub, (uint64_t)a.n * a.psl, (uint64_t)a.psl * r, f_pub, a.psl, k, &v) ||
      req_field_dword(a.enc, (uint64_t)a.n * a.enc_len, (uint64_t)a.enc_len * r, f_enc, a.enc_len, k, &v))
    return v;
  return req_byte(a, r, cl, k) | req_byte(a, r, cl, k + 1) << 8 | req_byte(a, r, cl, k + 2) << 16 |
         req_byte(a, r, cl, k + 3) << 24;
}

// k_req_write: a block writes the bytes of REQ_SUB consecutive reports (of one chunk), one lane
// per aligned dword of the output: the lane finds its report by a binary search of the block's
// offsets in LDS, so adjacent lanes write adjacent dwords across record boundaries and read
// adjacent bytes of the field rows.  Dwords that straddle two records are assembled bytewise; the
// block's first and last dword, which it may share with its neighbour (or with the header), are
// stored bytewise.
constexpr uint32_t REQ_SUB = 16;
__global__ __launch_bounds__(256) void k_req_write(ReqArgs a, uint32_t hdr_len) {
  __shared__ uint32_t s_off[REQ_SUB + 1];  // s_off[i + 1]: chunk bytes up to and including report i
  if (a.err[1]) return;  // the list does not fit a u32
  const uint32_t t = threadIdx.x, r0 = blockIdx.x * REQ_SUB, chunk = r0 / REQ_CHUNK;
  if (t <= REQ_SUB) {
    const uint32_t r = r0 + t;  // s_off[t] belongs to report r - 1
    uint32_t v = 0;
    if (r % REQ_CHUNK != 0 || t) v = a.rel[(r <= a.n ? r : a.n) - 1];
    s_off[t] = v;
    if (t && r <= a.n && a.index[r - 1] != 0xFFFFFFFFu) a.index[r - 1] += a.blk_cnt[chunk];
  }
  __syncthreads();
  const uint32_t b0 = s_off[0], b1 = s_off[REQ_SUB];
  if (b0 == b1) return;
  uint8_t* base = a.out + hdr_len + a.blk_bytes[chunk];
  const uint32_t fixed = REQ_FIXED + a.psl + a.enc_len + a.ps_len;
  // the report (of the block) that holds chunk byte x (b0 <= x < b1)
  auto find = [&](uint32_t x) {
    uint32_t lo = 0, hi = REQ_SUB - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_off[mid + 1] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  const uint32_t mis = (uint32_t)((uintptr_t)(base + b0) & 3u);
  const uint32_t nd = (mis + (b1 - b0) + 3) >> 2;
  for (uint32_t j = t; j < nd; j += 256) {
    const int64_t x0 = (int64_t)b0 - mis + 4 * (int64_t)j;  // dword j = chunk bytes [x0, x0 + 4)
    uint8_t* p = base + x0;
    const bool whole = x0 >= (int64_t)b0 && x0 + 4 <= (int64_t)b1;
    if (whole) {
      const uint32_t i = find((uint32_t)x0);
      const uint32_t start = s_off[i], L = s_off[i + 1] - start, k = (uint32_t)x0 - start;
      if (k + 4 <= L) {
        *(uint32_t*)p = req_dword(a, r0 + i, L - fixed, k);
        continue;
      }
    }
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
      const int64_t x = x0 + b;
      if (x < (int64_t)b0 || x >= (int64_t)b1) continue;
      const uint32_t i = find((uint32_t)x);
      const uint32_t start = s_off[i];
      const uint32_t byte = req_byte(a, r0 + i, s_off[i + 1] - start - fixed, (uint32_t)x - start);
      if (whole) v |= byte << (8 * b); else p[b] = (uint8_t)byte;
    }
    if (whole) *(uint32_t*)p = v;
  }
}

// ---- client side: Report encode -------------------------------------------------------------
// Report (messages/src/lib.rs, struct Report) = ReportMetadata { report_id[16], time u64 },
// u32-prefixed public share, HpkeCiphertext to the leader, HpkeCiphertext to the helper; each
// HpkeCiphertext { config_id u8, u16-prefixed enc, u32-prefixed payload }.  One report per output
// row (every report is its own upload body).
constexpr uint32_t REP_FIXED = 16 + 8 + 4 + 2 * (1 + 2 + 4);

struct RepCt {  // one aggregator's ciphertext rows
  const uint8_t *enc, *ct;
  const uint32_t* ct_len;
  uint32_t enc_len, ct_stride, cfg;
};
struct RepArgs {
  uint32_t n, psl, out_stride;
  const uint8_t *ids, *pub, *skip;
  const uint64_t* times;
  RepCt c[2];  // leader, helper
  uint8_t* out;
  uint32_t* out_len;
};

// byte k of one HpkeCiphertext (k < 7 + enc_len + cl)
DEV uint32_t rep_ct_byte(const RepCt& c, uint32_t r, uint32_t cl, uint32_t k) {
  if (k == 0) return c.cfg;
  if (k < 3) return (c.enc_len >> (8 * (2 - k))) & 0xFFu;
  k -= 3;
  if (k < c.enc_len) return c.enc[(size_t)c.enc_len * r + k];
  k -= c.enc_len;
  if (k < 4) return (cl >> (8 * (3 - k))) & 0xFFu;
  return c.ct[(size_t)c.ct_stride * r + (k - 4)];  // k - 4 < cl: nothing past ct_len is read
}

// byte k (k < the report's length) of report r; ll / hl = its two ct_len
DEV uint32_t rep_byte(const RepArgs& a, uint32_t r, uint32_t ll, uint32_t hl, uint32_t k) {
  if (k < 16) return a.ids[16 * (size_t)r + k];
  if (k < 24) return (uint32_t)(a.times[r] >> (8 * (23 - k))) & 0xFFu;
  if (k < 28) return (a.psl >> (8 * (27 - k))) & 0xFFu;
  k -= 28;
  if (k < a.psl) return a.pub[(size_t)a.psl * r + k];
  k -= a.psl;
  const uint32_t l0 = 7 + a.c[0].enc_len + ll;
  if (k < l0) return rep_ct_byte(a.c[0], r, ll, k);
  return rep_ct_byte(a.c[1], r, hl, k - l0);
}

// k_rep_write: one block per report, one lane per aligned dword of its output row (the row's first
// and last bytes, which may share a dword with the neighbouring rows, are stored bytewise); the
// row's bytes past the report are zero, and a report that is left out is a zero row of length 0.
__global__ __launch_bounds__(256) void k_rep_write(RepArgs a) {
  const uint32_t r = blockIdx.x, t = threadIdx.x;
  const uint32_t ll = a.c[0].ct_len[r], hl = a.c[1].ct_len[r];
  const bool out_ok = !(a.skip && a.skip[r]) && ll != 0 && ll <= a.c[0].ct_stride && hl != 0 &&
                      hl <= a.c[1].ct_stride;
  const uint32_t len = out_ok ? REP_FIXED + a.psl + a.c[0].enc_len + ll + a.c[1].enc_len + hl : 0u;
  if (t == 0) a.out_len[r] = len;
  uint8_t* row = a.out + (size_t)a.out_stride * r;
  const uint32_t mis = (uint32_t)((uintptr_t)row & 3u);
  const uint32_t nd = (mis + a.out_stride + 3) >> 2;
  for (uint32_t j = t; j < nd; j += 256) {
    const int64_t x0 = 4 * (int64_t)j - mis;  // dword j = row bytes [x0, x0 + 4)
    const bool whole = x0 >= 0 && x0 + 4 <= (int64_t)a.out_stride;
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
      const int64_t x = x0 + b;
      if (x < 0 || x >= (int64_t)a.out_stride) continue;
      const uint32_t byte = (uint32_t)x < len ? rep_byte(a, r, ll, hl, (uint32_t)x) : 0u;
      if (whole) v |= byte << (8 * b); else row[x] = (uint8_t)byte;
    }
    if (whole) *(uint32_t*)(row + x0) = v;
  }
}

// ---- leader side: AggregationJobResp decode -----------------------------------------------
// The three regular PrepareResp shapes: Continue { Finish { prep_msg[pml] } } = 26 + pml bytes,
// Finished = 17, Reject(e) = 18.  Record offsets depend on every earlier record, so one workgroup
// indexes the list first (k_runp_index) and the parallel passes read the index.
enum : uint32_t { RK_CONT = 0, RK_FINISHED = 1, RK_REJECT = 2 };
constexpr uint32_t RUNP_WIDTH = 1024;  // records speculated full-length per step
// classes a lane reports for the record at its speculated offset (low byte of the LDS key)
enum : uint32_t { RC_FINISHED = 1, RC_REJECT = 2, RC_BADCODE = 3, RC_IRREGULAR = 4,
                  RC_MALFORMED = 5, RC_END = 6 };

struct RunpArgs {
  const uint8_t* body;  // readable up to a dword past body_len
  uint64_t body_len;
  uint32_t n, n_included, pml;
  const uint32_t* index;
  const uint8_t* ids;
  uint8_t *msgs, *perr;
  uint32_t* flags;
  uint32_t* walked;  // scratch: records indexed
  uint32_t* off;     // scratch [n_included]: record offsets from the body's start
  uint8_t* kind;     // scratch [n_included]
};

// class of the record at byte o of a list ending at `end` (0: regular Continue-Finish)
DEV uint32_t runp_classify(const uint8_t* b, uint64_t o, uint64_t end, uint32_t pml) {
  if (o >= end) return RC_END;
  if (o + 17 > end) return RC_MALFORMED;
  const uint32_t ty = ld_u8(b, o + 16);
  if (ty == 1) return RC_FINISHED;
  if (ty == 2) {
    if (o + 18 > end) return RC_MALFORMED;
    return ld_u8(b, o + 17) <= 9 ? RC_REJECT : RC_BADCODE;
  }
  if (ty != 0 || o + 21 > end) return RC_MALFORMED;
  const uint64_t ml = ld_be32(b, o + 17);
  if (ml < 5 || o + 21 + ml > end) return RC_MALFORMED;
  const uint32_t pty = ld_u8(b, o + 21);
  const uint64_t x = ld_be32(b, o + 22);
  if (pty == 2 && ml == 5 + x && x == pml) return 0;
  if (pty == 0 || pty == 2) return ml == 5 + x ? RC_IRREGULAR : RC_MALFORMED;
  if (pty != 1 || 9 + x > ml) return RC_MALFORMED;
  return ml == 9 + x + ld_be32(b, o + 26 + x) ? RC_IRREGULAR : RC_MALFORMED;
}

// k_runp_index: one workgroup walks the list.  Per step lane i classifies the record that
// starts at o + i * (26 + pml) -- where record r + i starts if the records before it are all
// full-length; the first lane that does not see a regular Continue-Finish wins an LDS atomicMin
// of (i << 8 | class); lanes before it write offset and kind, the walk steps over the short
// record (Finished / Reject) and speculates again.  n / width + (short records) steps.
__global__ __launch_bounds__(1024) void k_runp_index(RunpArgs a) {
  __shared__ uint32_t first[3];
  const uint32_t F = 26 + a.pml, t = threadIdx.x;
  uint32_t fl = 0;
  uint64_t end = a.body_len;
  if (a.body_len < 4) {
    fl = JANUS_DAP_RESP_LISTLEN;
  } else {
    const uint64_t list = ld_be32(a.body, 0);
    if (4 + list > a.body_len) fl = JANUS_DAP_RESP_LISTLEN;
    if (4 + list < a.body_len) fl = JANUS_DAP_RESP_TRAILING;
    end = 4 + list;
  }
  uint32_t r = 0, slot = 0;
  uint64_t o = 4;
  if (t == 0) first[0] = 0xFFFFFFFFu;
  __syncthreads();
  while (!fl) {
    const uint64_t mine = o + (uint64_t)t * F;
    // a record past the expected count is the walk's end as well
    const uint32_t c = r + t >= a.n_included ? RC_END : runp_classify(a.body, mine, end, a.pml);
    if (c) atomicMin(&first[slot], t << 8 | c);
    // three slots, one barrier per step: the slot of the next step was last read two steps ago
    const uint32_t next = slot == 2 ? 0 : slot + 1;
    if (t == 0) first[next] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t f = first[slot];
    slot = next;
    const uint32_t k = f == 0xFFFFFFFFu ? RUNP_WIDTH : f >> 8, cls = f & 0xFFu;
    if (t < k) {
      a.off[r + t] = (uint32_t)mine;
      a.kind[r + t] = RK_CONT;
    }
    r += k;
    o += (uint64_t)k * F;
    if (k == RUNP_WIDTH) continue;
    if (cls == RC_FINISHED || cls == RC_REJECT) {
      if (t == 0) {
        a.off[r] = (uint32_t)o;
        a.kind[r] = cls == RC_FINISHED ? RK_FINISHED : RK_REJECT;
      }
      r += 1;
      o += cls == RC_FINISHED ? 17 : 18;
      continue;
    }
    if (cls == RC_BADCODE) fl = JANUS_DAP_RESP_REJECT_CODE;
    if (cls == RC_IRREGULAR) fl = JANUS_DAP_RESP_IRREGULAR;
    if (cls == RC_MALFORMED) fl = JANUS_DAP_RESP_IRREGULAR | JANUS_DAP_RESP_MALFORMED;
    if (cls == RC_END && (r != a.n_included || o != end)) fl = JANUS_DAP_RESP_COUNT;
    break;
  }
  if (t == 0) {
    *a.walked = r;
    if (fl) atomicOr(a.flags, fl);
  }
}

// k_runp_check: one lane per engine row: the record's report ID against the row's, and the
// row's PrepareError (0xFF: the helper continued)
__global__ __launch_bounds__(256) void k_runp_check(RunpArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  uint8_t pe = 0xFF;
  const uint32_t j = a.index[r];
  if (j != 0xFFFFFFFFu) {
    if (j >= a.n_included) {
      atomicOr(a.flags, (uint32_t)JANUS_DAP_RESP_COUNT);
    } else if (j < *a.walked) {
      const uint64_t o = a.off[j];
      bool same = true;
      for (uint32_t w = 0; w < 4; w++)
        same = same && ld_le32(a.body, o + 4 * w) == ld_le32(a.ids, 16 * (uint64_t)r + 4 * w);
      if (!same) atomicOr(a.flags, (uint32_t)JANUS_DAP_RESP_ID);
      const uint32_t kd = a.kind[j];
      if (kd == RK_FINISHED) pe = 5;  // VdafPrepError: the leader cannot be finished yet
      if (kd == RK_REJECT) pe = (uint8_t)ld_u8(a.body, o + 17);
    }
  }
  a.perr[r] = pe;
}

// k_runp_gather: one lane per dword of d_prep_msgs (rows of reports that did not continue are
// zeroed); consecutive Continue records are consecutive in the body, so both sides coalesce
__global__ __launch_bounds__(256) void k_runp_gather(RunpArgs a) {
  const uint64_t total = (uint64_t)a.n * a.pml;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * i >= total) return;
  const uint32_t walked = *a.walked;
  if ((a.pml & 3u) == 0) {
    const uint32_t wpr = a.pml >> 2;
    const uint32_t r = (uint32_t)(i / wpr), b = 4 * (uint32_t)(i - (uint64_t)r * wpr);
    const uint32_t j = a.index[r];
    uint32_t v = 0;
    if (j < a.n_included && j < walked && a.kind[j] == RK_CONT)
      v = ld_le32(a.body, (uint64_t)a.off[j] + 26 + b);
    ((uint32_t*)a.msgs)[i] = v;
    return;
  }
  for (uint32_t k = 0; k < 4; k++) {
    const uint64_t q = 4 * i + k;
    if (q >= total) break;
    const uint32_t r = (uint32_t)(q / a.pml), c = (uint32_t)(q - (uint64_t)r * a.pml);
    const uint32_t j = a.index[r];
    a.msgs[q] = (j < a.n_included && j < walked && a.kind[j] == RK_CONT)
                    ? a.body[(uint64_t)a.off[j] + 26 + c] : 0;
  }
}

// ---- host helpers -----------------------------------------------------------------------
struct Cur {
  const uint8_t* p;
  size_t len, o;
  bool ok = true;
  bool need(size_t k) {
    if (!ok || o + k > len) ok = false;
    return ok;
  }
  uint32_t u8() { return need(1) ? p[o++] : 0; }
  uint32_t u16() {
    if (!need(2)) return 0;
    const uint32_t v = (uint32_t)p[o] << 8 | p[o + 1];
    o += 2;
    return v;
  }
  uint32_t u32() {
    if (!need(4)) return 0;
    const uint32_t v = (uint32_t)p[o] << 24 | (uint32_t)p[o + 1] << 16 | (uint32_t)p[o + 2] << 8 |
                       p[o + 3];
    o += 4;
    return v;
  }
  uint64_t u64() {
    const uint64_t hi = u32();
    return hi << 32 | u32();
  }
};

struct RecShape {
  uint64_t o_id, o_pub, o_enc, o_pay, o_msg;
  uint32_t psl, cfg, enc_len, pay_len, msg_len;
  uint64_t time, end;
};

uint32_t be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// PingPongMessage framing (ping_pong.rs; messages/src/tests/aggregation.rs:201-268):
// 0 Initialize { prep_share<u32> }, 1 Continue { prep_msg<u32>, prep_share<u32> },
// 2 Finish { prep_msg<u32> }; the message must use every byte of its u32-prefixed field
bool pingpong_wellformed(const uint8_t* m, uint64_t len) {
  if (len < 5) return false;
  const uint64_t a = be32(m + 1);
  switch (m[0]) {
    case 0:
    case 2:
      return len == 5 + a;
    case 1:
      return 9 + a <= len && len == 9 + a + be32(m + 5 + a);
    default:
      return false;
  }
}

bool parse_record(Cur& c, RecShape& s) {
  s.o_id = c.o;
  c.need(16);
  c.o += 16;
  s.time = c.u64();
  s.psl = c.u32();
  s.o_pub = c.o;
  if (!c.need(s.psl)) return false;
  c.o += s.psl;
  s.cfg = c.u8();
  s.enc_len = c.u16();
  s.o_enc = c.o;
  if (!c.need(s.enc_len)) return false;
  c.o += s.enc_len;
  s.pay_len = c.u32();
  s.o_pay = c.o;
  if (!c.need(s.pay_len)) return false;
  c.o += s.pay_len;
  s.msg_len = c.u32();
  s.o_msg = c.o;
  if (!c.need(s.msg_len)) return false;
  c.o += s.msg_len;
  s.end = c.o;
  return c.ok;
}

}  // namespace

#define DCHK(x)                                                                       \
  do {                                                                                \
    hipError_t _e = (x);                                                              \
    if (_e != hipSuccess) {                                                           \
      fprintf(stderr, "janus_dap: HIP error %s at %s:%d\n", hipGetErrorString(_e),    \
              __FILE__, __LINE__);                                                    \
      return -2;                                                                      \
    }                                                                                 \
  } while (0)

extern "C" {

int janus_dap_agg_init_scan(const uint8_t* body, size_t len, janus_dap_agg_init_layout* L) {
  if (!body || !L) return -1;
  memset(L, 0, sizeof(*L));
  Cur c{body, len, 0};
  L->agg_param_len = c.u32();
  L->agg_param_off = c.o;
  if (!c.need(L->agg_param_len)) return -1;
  c.o += L->agg_param_len;
  L->query_type = (uint8_t)c.u8();
  if (L->query_type == JANUS_DAP_QUERY_FIXED_SIZE) {
    if (!c.need(32)) return -1;
    memcpy(L->batch_id, body + c.o, 32);
    c.o += 32;
  } else if (L->query_type != JANUS_DAP_QUERY_TIME_INTERVAL) {
    return -1;
  }
  L->list_len = c.u32();
  L->list_off = c.o;
  if (!c.ok || L->list_off + L->list_len != len) return -1;  // trailing bytes: decode error
  if (L->list_len == 0) {
    L->uniform = 1;
    return 0;
  }
  RecShape s;
  Cur r{body, L->list_off + L->list_len, L->list_off};
  if (!parse_record(r, s)) return -1;
  L->record_len = (uint32_t)(s.end - L->list_off);
  L->public_share_len = s.psl;
  L->enc_len = s.enc_len;
  L->payload_len = s.pay_len;
  L->message_len = s.msg_len;
  L->prep_share_len = (s.msg_len >= 5 && body[s.o_msg] == 0) ? s.msg_len - 5 : 0;
  L->uniform = L->list_len % L->record_len == 0;
  L->n = L->uniform ? (uint32_t)(L->list_len / L->record_len) : 0;
  return 0;
}

int janus_dap_agg_init_scan_ex(const uint8_t* body, size_t len, uint32_t public_share_len,
                               uint32_t enc_len, uint32_t prep_share_len,
                               janus_dap_agg_init_layout* L) {
  const int rc = janus_dap_agg_init_scan(body, len, L);
  if (rc || L->list_len == 0) return rc;
  // the task's expected lengths, not the first record's: a record whose public share, enc or
  // prep share has another length fails alone, and a body whose first record is off
  // is unpacked on the host, where every record is checked against these
  const bool fits = (public_share_len == JANUS_DAP_LEN_ANY || L->public_share_len == public_share_len) &&
                    (enc_len == JANUS_DAP_LEN_ANY || L->enc_len == enc_len) &&
                    (prep_share_len == JANUS_DAP_LEN_ANY || L->prep_share_len == prep_share_len);
  if (public_share_len != JANUS_DAP_LEN_ANY) L->public_share_len = public_share_len;
  if (enc_len != JANUS_DAP_LEN_ANY) L->enc_len = enc_len;
  if (prep_share_len != JANUS_DAP_LEN_ANY) L->prep_share_len = prep_share_len;
  if (!fits) {
    L->uniform = 0;
    L->n = 0;
  }
  return 0;
}

int janus_dap_agg_init_unpack_device(const janus_dap_agg_init_layout* L, const uint8_t* d_body,
                                     uint8_t* d_report_ids, uint64_t* d_times,
                                     uint8_t* d_public_shares, uint8_t* d_config_ids,
                                     uint8_t* d_enc, uint8_t* d_ct, uint32_t* d_ct_len,
                                     uint32_t ct_stride, uint8_t* d_prep_shares,
                                     uint8_t* d_msg_status, uint32_t* d_mismatch, void* stream) {
  if (!L || !d_mismatch || !L->uniform) return -1;
  hipStream_t st = (hipStream_t)stream;
  DCHK(hipMemsetAsync(d_mismatch, 0, 4, st));
  if (L->n == 0) return 0;
  if (!d_body || !d_report_ids || !d_times || !d_config_ids || !d_enc || !d_ct || !d_ct_len ||
      !d_prep_shares || !d_msg_status || (L->public_share_len && !d_public_shares) ||
      ct_stride < L->payload_len || ct_stride % 16)
    return -1;
  UnpackArgs a{};
  a.body = d_body;
  a.list_off = L->list_off;
  a.n = L->n;
  a.rec = L->record_len;
  a.psl = L->public_share_len;
  a.enc_len = L->enc_len;
  a.pay_len = L->payload_len;
  a.msg_len = L->message_len;
  a.ps_len = L->prep_share_len;
  a.cfg = d_config_ids;
  a.msg_status = d_msg_status;
  a.times = d_times;
  a.ct_len = d_ct_len;
  a.mismatch = d_mismatch;
  k_unpack_check<<<(L->n + 255) / 256, 256, 0, st>>>(a);
  DCHK(hipGetLastError());
  // field offsets within a record of the first record's shape
  const uint32_t o_pub = 28, o_enc = o_pub + L->public_share_len + 3,
                 o_pay = o_enc + L->enc_len + 4, o_ps = o_pay + L->payload_len + 4 + 5;
  GatherArgs g{};
  g.body = d_body;
  g.list_off = L->list_off;
  g.n = L->n;
  g.rec = L->record_len;
  g.f[0] = GatherField{d_report_ids, 16, 16, 0};
  g.f[1] = GatherField{L->public_share_len ? d_public_shares : nullptr, L->public_share_len,
                       L->public_share_len, o_pub};
  g.f[2] = GatherField{d_enc, L->enc_len, L->enc_len, o_enc};
  g.f[3] = GatherField{d_ct, ct_stride, L->payload_len, o_pay};
  g.f[4] = GatherField{L->prep_share_len ? d_prep_shares : nullptr, L->prep_share_len,
                       L->prep_share_len, o_ps};
  uint64_t maxw = 0;
  for (auto& f : g.f)
    if (f.dst && ((uint64_t)L->n * f.row + 3) / 4 > maxw) maxw = ((uint64_t)L->n * f.row + 3) / 4;
  const uint64_t blocks = (maxw + 255) / 256;
  k_unpack_gather<<<dim3((uint32_t)blocks, 5), 256, 0, st>>>(g);
  DCHK(hipGetLastError());
  return 0;
}

int64_t janus_dap_agg_init_unpack_host(const uint8_t* body, size_t len,
                                       const janus_dap_agg_init_layout* L, uint32_t cap,
                                       uint8_t* report_ids, uint64_t* times,
                                       uint8_t* public_shares, uint8_t* config_ids, uint8_t* enc,
                                       uint8_t* ct, uint32_t* ct_len, uint32_t ct_stride,
                                       uint8_t* prep_shares, uint8_t* msg_status) {
  if (!body || !L) return -1;
  Cur c{body, (size_t)(L->list_off + L->list_len), (size_t)L->list_off};
  uint32_t r = 0;
  while (c.o < c.len) {
    RecShape s;
    if (!parse_record(c, s)) return -1;
    if (r >= cap) return -1;
    memcpy(report_ids + 16 * (size_t)r, body + s.o_id, 16);
    times[r] = s.time;
    if (L->public_share_len) {
      uint8_t* pd = public_shares + (size_t)L->public_share_len * r;
      if (s.psl == L->public_share_len)
        memcpy(pd, body + s.o_pub, s.psl);
      else
        memset(pd, 0, L->public_share_len);
    }
    config_ids[r] = (uint8_t)s.cfg;
    uint8_t* ed = enc + (size_t)L->enc_len * r;
    if (s.enc_len == L->enc_len)
      memcpy(ed, body + s.o_enc, s.enc_len);
    else
      memset(ed, 0, L->enc_len);
    uint8_t* cd = ct + (size_t)ct_stride * r;
    memset(cd, 0, ct_stride);
    if (s.pay_len <= ct_stride && s.enc_len == L->enc_len) {
      memcpy(cd, body + s.o_pay, s.pay_len);
      ct_len[r] = s.pay_len;
    } else {
      ct_len[r] = 0;  // HPKE decrypt error for this report
    }
    // the PingPongMessage is decoded with the request: a malformed one rejects the request
    if (!pingpong_wellformed(body + s.o_msg, s.msg_len)) return -1;
    const uint32_t ty = body[s.o_msg];
    const uint32_t psl2 = be32(body + s.o_msg + 1);
    uint8_t stt = 0;
    if (s.psl != L->public_share_len)
      stt = 6;  // public share does not decode: InvalidMessage (aggregator.rs:1985-1999)
    else if (ty != 0)
      stt = 5;  // PeerMessageMismatch: Continue / Finish where Initialize is due
    else if (psl2 != L->prep_share_len)
      stt = 2;  // CodecPrepShare
    msg_status[r] = stt;
    uint8_t* pd = prep_shares + (size_t)L->prep_share_len * r;
    if (stt == 0)
      memcpy(pd, body + s.o_msg + 5, L->prep_share_len);
    else
      memset(pd, 0, L->prep_share_len);
    r++;
  }
  return r;
}

size_t janus_dap_agg_job_resp_max_len(uint32_t n, uint32_t pml) {
  return 4 + (size_t)n * (26 + pml > 18 ? 26 + pml : 18) + 8;
}

int janus_dap_agg_job_resp_encode_device(uint32_t n, const uint8_t* d_report_ids,
                                         const uint8_t* d_prepare_error,
                                         const uint8_t* d_prio3_status, const uint8_t* d_prep_msgs,
                                         uint32_t pml, uint8_t* d_out, uint64_t* d_out_len,
                                         uint32_t* d_scratch, void* stream) {
  if (!d_out || !d_out_len || !d_scratch || (n && (!d_report_ids || !d_prepare_error ||
                                                   !d_prio3_status || (pml && !d_prep_msgs))))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nb = (n + 255) / 256;
  if (n) {
    k_resp_count<<<nb, 256, 0, st>>>(n, d_prepare_error, d_prio3_status, d_scratch);
    DCHK(hipGetLastError());
  }
  k_resp_scan<<<1, 1024, 0, st>>>(nb, d_scratch, n, pml, d_out_len, d_out);
  DCHK(hipGetLastError());
  if (n) {
    k_resp_write<<<nb, 256, 0, st>>>(n, d_report_ids, d_prepare_error, d_prio3_status,
                                     d_prep_msgs, pml, d_scratch, d_out);
    DCHK(hipGetLastError());
  }
  return 0;
}

int64_t janus_dap_agg_job_resp_encode_host(uint32_t n, const uint8_t* ids, const uint8_t* pe,
                                           const uint8_t* st, const uint8_t* pm, uint32_t pml,
                                           uint8_t* out) {
  if (!out) return -1;
  size_t o = 4;
  for (uint32_t r = 0; r < n; r++) {
    memcpy(out + o, ids + 16 * (size_t)r, 16);
    o += 16;
    if (pe[r] == 0xFF && st[r] == 0) {
      const uint32_t ml = 5 + pml;
      const uint8_t hdr[10] = {0, (uint8_t)(ml >> 24), (uint8_t)(ml >> 16), (uint8_t)(ml >> 8),
                               (uint8_t)ml, 2, (uint8_t)(pml >> 24), (uint8_t)(pml >> 16),
                               (uint8_t)(pml >> 8), (uint8_t)pml};
      memcpy(out + o, hdr, 10);
      if (pml) memcpy(out + o + 10, pm + (size_t)pml * r, pml);
      o += 10 + pml;
    } else {
      out[o] = 2;
      out[o + 1] = pe[r] != 0xFF ? pe[r] : 5;
      o += 2;
    }
  }
  const size_t body = o - 4;
  out[0] = (uint8_t)(body >> 24);
  out[1] = (uint8_t)(body >> 16);
  out[2] = (uint8_t)(body >> 8);
  out[3] = (uint8_t)body;
  return (int64_t)o;
}

// ---- leader side --------------------------------------------------------------------------
namespace {
void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}
size_t req_hdr_len(uint32_t apl, uint8_t qt) {
  return 4 + (size_t)apl + 1 + (qt == JANUS_DAP_QUERY_FIXED_SIZE ? 32 : 0) + 4;
}
// the body up to the list length (which the caller fills at the returned offset)
size_t req_hdr_put(uint8_t* out, const uint8_t* ap, uint32_t apl, uint8_t qt, const uint8_t* bid) {
  size_t o = 0;
  put_be32(out, apl);
  o += 4;
  if (apl) memcpy(out + o, ap, apl);
  o += apl;
  out[o++] = qt;
  if (qt == JANUS_DAP_QUERY_FIXED_SIZE) {
    memcpy(out + o, bid, 32);
    o += 32;
  }
  return o;
}
bool req_args_ok(uint32_t n, const uint8_t* ap, uint32_t apl, uint8_t qt, const uint8_t* bid,
                 uint32_t psl, uint32_t enc_len, uint32_t ct_stride, uint32_t ps_len) {
  if (qt != JANUS_DAP_QUERY_TIME_INTERVAL && qt != JANUS_DAP_QUERY_FIXED_SIZE) return false;
  if ((apl && !ap) || (qt == JANUS_DAP_QUERY_FIXED_SIZE && !bid)) return false;
  if (enc_len > 0xFFFF) return false;
  // one record stays far below 2^32 bytes (the kernels index a record's bytes in 32 bits)
  return (uint64_t)REQ_FIXED + psl + enc_len + ct_stride + ps_len < (1ull << 31);
}
int device_of(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return at.device;
}
}  // namespace

size_t janus_dap_agg_init_req_max_len(uint32_t n, uint32_t apl, uint8_t qt, uint32_t psl,
                                      uint32_t enc_len, uint32_t ct_stride, uint32_t ps_len) {
  return req_hdr_len(apl, qt) +
         (size_t)n * ((size_t)REQ_FIXED + psl + enc_len + ct_stride + ps_len) + 8;
}

int64_t janus_dap_agg_init_req_encode_host(uint32_t n, const uint8_t* ap, uint32_t apl, uint8_t qt,
                                           const uint8_t* bid, const uint8_t* ids,
                                           const uint64_t* times, const uint8_t* pub, uint32_t psl,
                                           const uint8_t* cfg, const uint8_t* enc,
                                           uint32_t enc_len, const uint8_t* ct,
                                           const uint32_t* ct_len, uint32_t ct_stride,
                                           const uint8_t* ps, uint32_t ps_len,
                                           const uint8_t* status, uint8_t* out, uint32_t* index,
                                           uint32_t* n_included) {
  if (!out || !index || !n_included || !req_args_ok(n, ap, apl, qt, bid, psl, enc_len, ct_stride,
                                                    ps_len))
    return JANUS_DAP_EARG;
  if (n && (!ids || !times || !cfg || !ct_len || !status || (psl && !pub) || (enc_len && !enc) ||
            (ct_stride && !ct) || (ps_len && !ps)))
    return JANUS_DAP_EARG;
  uint64_t list = 0;
  for (uint32_t r = 0; r < n; r++) {
    if (status[r]) continue;
    if (ct_len[r] > ct_stride) return JANUS_DAP_EARG;
    list += (uint64_t)REQ_FIXED + psl + enc_len + ps_len + ct_len[r];
  }
  if (list > 0xFFFFFFFFull) return JANUS_DAP_ETOOLONG;
  size_t o = req_hdr_put(out, ap, apl, qt, bid);
  put_be32(out + o, (uint32_t)list);
  o += 4;
  uint32_t k = 0;
  for (uint32_t r = 0; r < n; r++) {
    if (status[r]) {
      index[r] = JANUS_DAP_INDEX_NONE;
      continue;
    }
    index[r] = k++;
    memcpy(out + o, ids + 16 * (size_t)r, 16);
    put_be32(out + o + 16, (uint32_t)(times[r] >> 32));
    put_be32(out + o + 20, (uint32_t)times[r]);
    put_be32(out + o + 24, psl);
    o += 28;
    if (psl) memcpy(out + o, pub + (size_t)psl * r, psl);
    o += psl;
    out[o] = cfg[r];
    out[o + 1] = (uint8_t)(enc_len >> 8);
    out[o + 2] = (uint8_t)enc_len;
    o += 3;
    if (enc_len) memcpy(out + o, enc + (size_t)enc_len * r, enc_len);
    o += enc_len;
    put_be32(out + o, ct_len[r]);
    o += 4;
    if (ct_len[r]) memcpy(out + o, ct + (size_t)ct_stride * r, ct_len[r]);
    o += ct_len[r];
    put_be32(out + o, 5 + ps_len);
    out[o + 4] = 0;  // PingPongMessage::Initialize
    put_be32(out + o + 5, ps_len);
    o += 9;
    if (ps_len) memcpy(out + o, ps + (size_t)ps_len * r, ps_len);
    o += ps_len;
  }
  *n_included = k;
  return (int64_t)o;
}

int janus_dap_agg_init_req_encode_device(uint32_t n, const uint8_t* ap, uint32_t apl, uint8_t qt,
                                         const uint8_t* bid, const uint8_t* d_ids,
                                         const uint64_t* d_times, const uint8_t* d_pub,
                                         uint32_t psl, const uint8_t* d_cfg, const uint8_t* d_enc,
                                         uint32_t enc_len, const uint8_t* d_ct,
                                         const uint32_t* d_ct_len, uint32_t ct_stride,
                                         const uint8_t* d_ps, uint32_t ps_len,
                                         const uint8_t* d_status, uint8_t* d_out,
                                         uint64_t* d_out_len, uint32_t* d_index,
                                         uint32_t* d_n_included, uint32_t* d_err, void* d_scratch,
                                         void* stream) {
  if (!d_out || !d_out_len || !d_n_included || !d_err || !d_scratch ||
      ((uintptr_t)d_scratch & 7u) || apl > JANUS_DAP_AGG_PARAM_MAX ||
      !req_args_ok(n, ap, apl, qt, bid, psl, enc_len, ct_stride, ps_len))
    return JANUS_DAP_EARG;
  if (n && (!d_ids || !d_times || !d_cfg || !d_ct_len || !d_status || !d_index ||
            (psl && !d_pub) || (enc_len && !d_enc) || (ct_stride && !d_ct) || (ps_len && !d_ps)))
    return JANUS_DAP_EARG;
  const int dev = device_of(d_out);
  if (dev < 0) return JANUS_DAP_EARG;
  DeviceGuard guard(dev);
  DCHK(guard.rc);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nb = (n + REQ_CHUNK - 1) / REQ_CHUNK;
  ReqHdr h;
  memset(&h, 0, sizeof(h));
  h.len = (uint32_t)req_hdr_put(h.b, ap, apl, qt, bid) + 4;
  ReqArgs a{};
  a.n = n;
  a.psl = psl;
  a.enc_len = enc_len;
  a.ct_stride = ct_stride;
  a.ps_len = ps_len;
  a.ids = d_ids;
  a.pub = d_pub;
  a.cfg = d_cfg;
  a.enc = d_enc;
  a.ct = d_ct;
  a.ps = d_ps;
  a.status = d_status;
  a.times = d_times;
  a.ct_len = d_ct_len;
  a.blk_bytes = (uint64_t*)d_scratch;
  a.blk_cnt = (uint32_t*)(a.blk_bytes + nb + 1);
  a.rel = a.blk_cnt + nb + 1;
  a.out = d_out;
  a.out_len = d_out_len;
  a.index = d_index;
  a.n_included = d_n_included;
  a.err = d_err;
  DCHK(hipMemsetAsync(d_err, 0, 8, st));
  if (n) {
    k_req_count<<<nb, 256, 0, st>>>(a);
    DCHK(hipGetLastError());
  }
  k_req_scan<<<1, 1024, 0, st>>>(nb, a, h);
  DCHK(hipGetLastError());
  if (n) {
    k_req_write<<<(n + REQ_SUB - 1) / REQ_SUB, 256, 0, st>>>(a, h.len);
    DCHK(hipGetLastError());
  }
  return 0;
}

int janus_dap_agg_job_resp_unpack_host(uint32_t n, const uint32_t* index, const uint8_t* ids,
                                       uint32_t n_included, const uint8_t* body, size_t body_len,
                                       uint32_t pml, uint8_t* msgs, uint8_t* perr) {
  if (!body || n_included > n || (n && (!index || !ids || !perr || (pml && !msgs))))
    return JANUS_DAP_EARG;
  if (body_len < 4) return JANUS_DAP_RESP_ELISTLEN;
  const uint64_t list = be32(body);
  if (4 + list > body_len) return JANUS_DAP_RESP_ELISTLEN;
  if (4 + list < body_len) return JANUS_DAP_RESP_ETRAILING;
  // the whole message decodes before the driver looks at it: count the records first
  const size_t end = body_len;
  uint64_t count = 0;
  for (size_t o = 4; o < end; count++) {
    if (o + 17 > end) return JANUS_DAP_RESP_EMALFORMED;
    const uint8_t ty = body[o + 16];
    if (ty == 1) {
      o += 17;
    } else if (ty == 2) {
      if (o + 18 > end) return JANUS_DAP_RESP_EMALFORMED;
      if (body[o + 17] > 9) return JANUS_DAP_RESP_EREJECT_CODE;
      o += 18;
    } else if (ty == 0) {
      if (o + 21 > end) return JANUS_DAP_RESP_EMALFORMED;
      const uint64_t ml = be32(body + o + 17);
      if (o + 21 + ml > end || !pingpong_wellformed(body + o + 21, ml))
        return JANUS_DAP_RESP_EMALFORMED;
      o += 21 + ml;
    } else {
      return JANUS_DAP_RESP_EMALFORMED;
    }
  }
  if (count != n_included) return JANUS_DAP_RESP_ECOUNT;
  // the row of each position of the request (index[] inverted)
  std::vector<uint32_t> row(n_included, JANUS_DAP_INDEX_NONE);
  for (uint32_t r = 0; r < n; r++) {
    if (index[r] == JANUS_DAP_INDEX_NONE) continue;
    if (index[r] >= n_included || row[index[r]] != JANUS_DAP_INDEX_NONE) return JANUS_DAP_EARG;
    row[index[r]] = r;
  }
  if (pml) memset(msgs, 0, (size_t)n * pml);
  if (n) memset(perr, 0xFF, n);
  size_t o = 4;
  for (uint32_t j = 0; j < n_included; j++) {
    const uint32_t r = row[j];
    if (r == JANUS_DAP_INDEX_NONE) return JANUS_DAP_EARG;
    if (memcmp(body + o, ids + 16 * (size_t)r, 16)) return JANUS_DAP_RESP_EID;
    const uint8_t ty = body[o + 16];
    if (ty == 1) {
      perr[r] = 5;  // VdafPrepError: a Prio3 leader is not finished before the helper's message
      o += 17;
    } else if (ty == 2) {
      perr[r] = body[o + 17];
      o += 18;
    } else {
      const uint32_t ml = be32(body + o + 17);
      const uint8_t* m = body + o + 21;
      if (m[0] == 2 && ml == 5 + (uint64_t)pml) {
        if (pml) memcpy(msgs + (size_t)pml * r, m + 5, pml);
      } else {
        perr[r] = 5;  // leader_continued fails: PeerMessageMismatch / a prepare message that
      }               // does not decode (handle_ping_pong_error -> VdafPrepError)
      o += 21 + (size_t)ml;
    }
  }
  return 0;
}

int janus_dap_agg_job_resp_unpack_device(uint32_t n, const uint32_t* d_index, const uint8_t* d_ids,
                                         uint32_t n_included, const uint8_t* d_body,
                                         size_t body_len, uint32_t pml, uint8_t* d_msgs,
                                         uint8_t* d_perr, uint32_t* d_flags, void* d_scratch,
                                         void* stream) {
  if (!d_body || !d_flags || !d_scratch || ((uintptr_t)d_scratch & 3u) || n_included > n ||
      body_len > 4ull + 0xFFFFFFFFull ||
      (n && (!d_index || !d_ids || !d_perr || (pml && !d_msgs))))
    return JANUS_DAP_EARG;
  const int dev = device_of(d_flags);
  if (dev < 0) return JANUS_DAP_EARG;
  DeviceGuard guard(dev);
  DCHK(guard.rc);
  hipStream_t st = (hipStream_t)stream;
  DCHK(hipMemsetAsync(d_flags, 0, 4, st));
  RunpArgs a{};
  a.body = d_body;
  a.body_len = body_len;
  a.n = n;
  a.n_included = n_included;
  a.pml = pml;
  a.index = d_index;
  a.ids = d_ids;
  a.msgs = d_msgs;
  a.perr = d_perr;
  a.flags = d_flags;
  a.walked = (uint32_t*)d_scratch;
  a.off = a.walked + 1;
  a.kind = (uint8_t*)(a.off + n_included);
  k_runp_index<<<1, 1024, 0, st>>>(a);
  DCHK(hipGetLastError());
  if (n) {
    k_runp_check<<<(n + 255) / 256, 256, 0, st>>>(a);
    DCHK(hipGetLastError());
    const uint64_t words = ((uint64_t)n * pml + 3) / 4;
    if (words) {
      k_runp_gather<<<(uint32_t)((words + 255) / 256), 256, 0, st>>>(a);
      DCHK(hipGetLastError());
    }
  }
  return 0;
}

// ---- client side ----------------------------------------------------------------------------
namespace {
bool rep_args_ok(uint32_t psl, uint32_t lenc, uint32_t lstride, uint32_t henc, uint32_t hstride,
                 uint32_t out_stride) {
  if (lenc > 0xFFFF || henc > 0xFFFF) return false;
  const uint64_t max_len = (uint64_t)REP_FIXED + psl + lenc + lstride + henc + hstride;
  return max_len < (1ull << 31) && out_stride >= max_len;
}
}  // namespace

size_t janus_dap_report_max_len(uint32_t psl, uint32_t lenc, uint32_t lstride, uint32_t henc,
                                uint32_t hstride) {
  return (size_t)REP_FIXED + psl + lenc + lstride + henc + hstride;
}

int janus_dap_report_encode_device(uint32_t n, const uint8_t* d_ids, const uint64_t* d_times,
                                   const uint8_t* d_pub, uint32_t psl, uint8_t leader_config_id,
                                   const uint8_t* d_lenc, uint32_t lenc, const uint8_t* d_lct,
                                   const uint32_t* d_lct_len, uint32_t lstride,
                                   uint8_t helper_config_id, const uint8_t* d_henc, uint32_t henc,
                                   const uint8_t* d_hct, const uint32_t* d_hct_len,
                                   uint32_t hstride, const uint8_t* d_skip, uint8_t* d_out,
                                   uint32_t out_stride, uint32_t* d_out_len, void* stream) {
  if (!rep_args_ok(psl, lenc, lstride, henc, hstride, out_stride)) return JANUS_DAP_EARG;
  if (n == 0) return 0;
  if (!d_ids || !d_times || !d_lct_len || !d_hct_len || !d_out || !d_out_len || (psl && !d_pub) ||
      (lenc && !d_lenc) || (henc && !d_henc) || (lstride && !d_lct) || (hstride && !d_hct))
    return JANUS_DAP_EARG;
  const int dev = device_of(d_out);
  if (dev < 0) return JANUS_DAP_EARG;
  DeviceGuard guard(dev);
  DCHK(guard.rc);
  RepArgs a{};
  a.n = n;
  a.psl = psl;
  a.out_stride = out_stride;
  a.ids = d_ids;
  a.pub = d_pub;
  a.skip = d_skip;
  a.times = d_times;
  a.c[0] = RepCt{d_lenc, d_lct, d_lct_len, lenc, lstride, leader_config_id};
  a.c[1] = RepCt{d_henc, d_hct, d_hct_len, henc, hstride, helper_config_id};
  a.out = d_out;
  a.out_len = d_out_len;
  k_rep_write<<<n, 256, 0, (hipStream_t)stream>>>(a);
  DCHK(hipGetLastError());
  return 0;
}

int64_t janus_dap_report_encode_host(uint32_t n, const uint8_t* ids, const uint64_t* times,
                                     const uint8_t* pub, uint32_t psl, uint8_t leader_config_id,
                                     const uint8_t* lenc_rows, uint32_t lenc, const uint8_t* lct,
                                     const uint32_t* lct_len, uint32_t lstride,
                                     uint8_t helper_config_id, const uint8_t* henc_rows,
                                     uint32_t henc, const uint8_t* hct, const uint32_t* hct_len,
                                     uint32_t hstride, const uint8_t* skip, uint8_t* out,
                                     uint32_t out_stride, uint32_t* out_len) {
  if (!rep_args_ok(psl, lenc, lstride, henc, hstride, out_stride)) return JANUS_DAP_EARG;
  if (n == 0) return 0;
  if (!ids || !times || !lct_len || !hct_len || !out || !out_len || (psl && !pub) ||
      (lenc && !lenc_rows) || (henc && !henc_rows) || (lstride && !lct) || (hstride && !hct))
    return JANUS_DAP_EARG;
  const uint8_t cfg[2] = {leader_config_id, helper_config_id};
  const uint8_t* encs[2] = {lenc_rows, henc_rows};
  const uint8_t* cts[2] = {lct, hct};
  const uint32_t* cls[2] = {lct_len, hct_len};
  const uint32_t enc_len[2] = {lenc, henc}, stride[2] = {lstride, hstride};
  int64_t emitted = 0;
  for (uint32_t r = 0; r < n; r++) {
    uint8_t* row = out + (size_t)out_stride * r;
    memset(row, 0, out_stride);
    out_len[r] = 0;
    if ((skip && skip[r]) || lct_len[r] == 0 || lct_len[r] > lstride || hct_len[r] == 0 ||
        hct_len[r] > hstride)
      continue;
    size_t o = 0;
    memcpy(row, ids + 16 * (size_t)r, 16);
    put_be32(row + 16, (uint32_t)(times[r] >> 32));
    put_be32(row + 20, (uint32_t)times[r]);
    put_be32(row + 24, psl);
    o = 28;
    if (psl) memcpy(row + o, pub + (size_t)psl * r, psl);
    o += psl;
    for (int c = 0; c < 2; c++) {
      const uint32_t cl = cls[c][r];
      row[o] = cfg[c];
      row[o + 1] = (uint8_t)(enc_len[c] >> 8);
      row[o + 2] = (uint8_t)enc_len[c];
      o += 3;
      if (enc_len[c]) memcpy(row + o, encs[c] + (size_t)enc_len[c] * r, enc_len[c]);
      o += enc_len[c];
      put_be32(row + o, cl);
      o += 4;
      memcpy(row + o, cts[c] + (size_t)stride[c] * r, cl);
      o += cl;
    }
    out_len[r] = (uint32_t)o;
    emitted++;
  }
  return emitted;
}

}  // extern "C"

// ---- leader side: Report decode ---------------------------------------------------------------
namespace {
struct RdecArgs {
  uint32_t n, stride, enc_len, ct_stride;
  const uint8_t* rows;
  const uint32_t* len;
  uint8_t *ids, *lcfg, *hcfg, *henc, *hct, *bad;
  uint64_t* times;
  uint32_t *fields, *hct_len;
};

// k_rep_decode: one wave per report.  Every lane walks the (at most five) length prefixes itself --
// the addresses are wave-uniform, so each is one broadcast load -- then the lanes share the small
// outputs and copy the helper's ciphertext rows.  The leader's fields stay in the row: the upload
// call reads them in place through fields[].
__global__ __launch_bounds__(256) void k_rep_decode(RdecArgs a) {
  const uint64_t r = 4ull * blockIdx.x + (threadIdx.x >> 6);
  const uint32_t l = threadIdx.x & 63u;
  if (r >= a.n) return;
  const uint8_t* row = a.rows + (size_t)a.stride * r;
  const uint32_t len = a.len[r];
  uint32_t f[JANUS_DAP_REPORT_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, cfg[2] = {0, 0};
  const bool ok = len <= a.stride && rep_parse(row, len, f, cfg);
  if (!ok) {
#pragma unroll
    for (int i = 0; i < JANUS_DAP_REPORT_FIELDS; i++) f[i] = 0;
    cfg[0] = cfg[1] = 0;
  }
  const bool hok = ok && f[7] == a.enc_len && f[9] <= a.ct_stride;
  if (l < 16) a.ids[16 * r + l] = ok ? row[l] : (uint8_t)0;
  if (l == 16) {
    uint64_t t = 0;
    if (ok)
      for (int i = 0; i < 8; i++) t = (t << 8) | row[16 + i];
    a.times[r] = t;
  }
  if (l == 17) {
#pragma unroll
    for (int i = 0; i < JANUS_DAP_REPORT_FIELDS; i++) a.fields[JANUS_DAP_REPORT_FIELDS * r + i] = f[i];
  }
  if (l == 18) {
    a.lcfg[r] = (uint8_t)cfg[0];
    a.hcfg[r] = (uint8_t)cfg[1];
    a.bad[r] = ok ? 0 : 1;
    a.hct_len[r] = hok ? f[9] : 0u;
  }
  for (uint32_t k = l; k < a.enc_len; k += 64)
    a.henc[(size_t)a.enc_len * r + k] = hok ? row[f[6] + k] : (uint8_t)0;  // f[6] + k < len
  for (uint32_t k = l; k < a.ct_stride; k += 64)
    a.hct[(size_t)a.ct_stride * r + k] = hok && k < f[9] ? row[f[8] + k] : (uint8_t)0;
}

bool rdec_args_ok(uint32_t n, const void* rows, uint32_t stride, const void* len, const void* ids,
                  const void* times, const void* fields, const void* lcfg, const void* hcfg,
                  const void* henc, uint32_t enc_len, const void* hct, const void* hct_len,
                  uint32_t ct_stride, const void* bad) {
  if (enc_len > 0xFFFF || stride >= (1u << 31)) return false;
  if (n == 0) return true;
  return len && ids && times && fields && lcfg && hcfg && hct_len && bad && (!stride || rows) &&
         (!enc_len || henc) && (!ct_stride || hct);
}
}  // namespace

extern "C" {

int64_t janus_dap_report_decode_host(uint32_t n, const uint8_t* reports, uint32_t stride,
                                     const uint32_t* report_len, uint8_t* ids, uint64_t* times,
                                     uint32_t* fields, uint8_t* lcfg, uint8_t* hcfg, uint8_t* henc,
                                     uint32_t enc_len, uint8_t* hct, uint32_t* hct_len,
                                     uint32_t ct_stride, uint8_t* bad) {
  if (!rdec_args_ok(n, reports, stride, report_len, ids, times, fields, lcfg, hcfg, henc, enc_len,
                    hct, hct_len, ct_stride, bad))
    return JANUS_DAP_EARG;
  int64_t decoded = 0;
  for (uint32_t r = 0; r < n; r++) {
    const uint8_t* row = reports + (size_t)stride * r;
    uint32_t f[JANUS_DAP_REPORT_FIELDS] = {0}, cfg[2] = {0, 0};
    const bool ok = report_len[r] <= stride && rep_parse(row, report_len[r], f, cfg);
    if (!ok) {
      memset(f, 0, sizeof f);
      cfg[0] = cfg[1] = 0;
    }
    const bool hok = ok && f[7] == enc_len && f[9] <= ct_stride;
    memset(ids + 16 * (size_t)r, 0, 16);
    times[r] = 0;
    if (ok) {
      memcpy(ids + 16 * (size_t)r, row, 16);
      for (int i = 0; i < 8; i++) times[r] = (times[r] << 8) | row[16 + i];
    }
    memcpy(fields + (size_t)JANUS_DAP_REPORT_FIELDS * r, f, sizeof f);
    lcfg[r] = (uint8_t)cfg[0];
    hcfg[r] = (uint8_t)cfg[1];
    bad[r] = ok ? 0 : 1;
    hct_len[r] = hok ? f[9] : 0u;
    if (enc_len) memset(henc + (size_t)enc_len * r, 0, enc_len);
    if (ct_stride) memset(hct + (size_t)ct_stride * r, 0, ct_stride);
    if (hok) {
      if (enc_len) memcpy(henc + (size_t)enc_len * r, row + f[6], enc_len);
      if (f[9]) memcpy(hct + (size_t)ct_stride * r, row + f[8], f[9]);
    }
    decoded += ok;
  }
  return decoded;
}

int janus_dap_report_decode_device(uint32_t n, const uint8_t* d_reports, uint32_t stride,
                                   const uint32_t* d_report_len, uint8_t* d_ids, uint64_t* d_times,
                                   uint32_t* d_fields, uint8_t* d_lcfg, uint8_t* d_hcfg,
                                   uint8_t* d_henc, uint32_t enc_len, uint8_t* d_hct,
                                   uint32_t* d_hct_len, uint32_t ct_stride, uint8_t* d_bad,
                                   void* stream) {
  if (!rdec_args_ok(n, d_reports, stride, d_report_len, d_ids, d_times, d_fields, d_lcfg, d_hcfg,
                    d_henc, enc_len, d_hct, d_hct_len, ct_stride, d_bad))
    return JANUS_DAP_EARG;
  if (n == 0) return 0;
  const int dev = device_of(d_bad);
  if (dev < 0) return JANUS_DAP_EARG;
  DeviceGuard guard(dev);
  DCHK(guard.rc);
  RdecArgs a{};
  a.n = n;
  a.stride = stride;
  a.enc_len = enc_len;
  a.ct_stride = ct_stride;
  a.rows = d_reports;
  a.len = d_report_len;
  a.ids = d_ids;
  a.lcfg = d_lcfg;
  a.hcfg = d_hcfg;
  a.henc = d_henc;
  a.hct = d_hct;
  a.bad = d_bad;
  a.times = d_times;
  a.fields = d_fields;
  a.hct_len = d_hct_len;
  k_rep_decode<<<(uint32_t)(((uint64_t)n + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
  DCHK(hipGetLastError());
  return 0;
}

}  // extern "C"

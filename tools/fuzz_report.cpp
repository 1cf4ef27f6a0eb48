// fuzz_report.cpp -- AddressSanitizer harness for the host form of the DAP `Report` decoder
// (janus_dap_report_decode_host): the leader's upload handler reads untrusted bytes, so the decoder
// is run here on mutated Report rows (bit flips, byte sets, truncations, length-field extremes,
// splices, a report_len above the row) under -fsanitize=address.  Every row lives in a heap buffer
// of exactly min(report_len, report_stride) meaningful bytes at the END of the allocation and every
// output buffer has exactly the size janus_dap.h specifies, so a read past a report or a write past
// a row is an ASan report.  The result is checked against an independent bounds-checked parse.
// Build + run: make -C janus_amd asan_report  (no GPU needed: only the host entry point is called).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/janus_dap.h"

namespace {

void put_be(std::vector<uint8_t>& b, uint64_t v, int n) {
  for (int i = n - 1; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i)));
}

// a well-formed Report of random field lengths
std::vector<uint8_t> make_report(std::mt19937_64& g) {
  std::vector<uint8_t> b;
  for (int i = 0; i < 24; i++) b.push_back((uint8_t)g());
  const uint32_t psl = (g() % 4 == 0) ? (uint32_t)(g() % 70) : 32;
  put_be(b, psl, 4);
  for (uint32_t i = 0; i < psl; i++) b.push_back((uint8_t)g());
  for (int c = 0; c < 2; c++) {
    b.push_back((uint8_t)g());
    const uint32_t el = (g() % 6 == 0) ? (uint32_t)(g() % 70) : 32;
    put_be(b, el, 2);
    for (uint32_t i = 0; i < el; i++) b.push_back((uint8_t)g());
    const uint32_t pl = (uint32_t)(g() % (c ? 80 : 300));
    put_be(b, pl, 4);
    for (uint32_t i = 0; i < pl; i++) b.push_back((uint8_t)g());
  }
  return b;
}

void mutate(std::mt19937_64& g, std::vector<uint8_t>& b) {
  const int k = 1 + (int)(g() % 4);
  for (int i = 0; i < k && !b.empty(); i++) {
    const size_t at = g() % b.size();
    switch (g() % 5) {
      case 0: b[at] ^= (uint8_t)(1u << (g() % 8)); break;
      case 1: b[at] = (uint8_t)g(); break;
      case 2: b.resize(at); break;                                     // truncate
      case 3: b[at] = (uint8_t)(g() % 2 ? 0xff : 0x00); break;          // length extremes
      default: {                                                        // splice a chunk
        const size_t from = g() % b.size(), len = std::min<size_t>(g() % 64, b.size() - from);
        std::vector<uint8_t> chunk(b.begin() + from, b.begin() + from + len);
        b.insert(b.begin() + at, chunk.begin(), chunk.end());
      }
    }
  }
}

// the independent parse: 64-bit cursor, every step bounds-checked
struct Parsed {
  bool ok;
  uint64_t f[JANUS_DAP_REPORT_FIELDS];
  uint8_t cfg[2];
};
Parsed parse(const uint8_t* p, uint64_t len) {
  Parsed r{};
  uint64_t o = 24;
  auto be = [&](int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[o + i];
    o += n;
    return v;
  };
  if (len < 28) return r;
  const uint64_t psl = be(4);
  if (o + psl > len) return r;
  r.f[0] = o, r.f[1] = psl, o += psl;
  for (int c = 0; c < 2; c++) {
    if (o + 3 > len) return r;
    r.cfg[c] = p[o++];
    const uint64_t el = be(2);
    if (o + el > len) return r;
    r.f[2 + 4 * c] = o, r.f[3 + 4 * c] = el, o += el;
    if (o + 4 > len) return r;
    const uint64_t pl = be(4);
    if (o + pl > len) return r;
    r.f[4 + 4 * c] = o, r.f[5 + 4 * c] = pl, o += pl;
  }
  r.ok = o == len;
  return r;
}

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "fuzz_report: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 g(argc > 2 ? strtoull(argv[2], nullptr, 10) : 0x4a414e5553ull);
  long decoded = 0, malformed = 0, helper_empty = 0;
  for (long it = 0; it < iters; it++) {
    std::vector<uint8_t> body = make_report(g);
    if (it % 8) mutate(g, body);
    // One row; the stride is the body's length, sometimes shorter (report_len > report_stride) or
    // longer.  The allocation ends where the readable bytes end.
    uint32_t stride = (uint32_t)body.size();
    uint32_t len = (uint32_t)body.size();
    const int shape = (int)(g() % 8);
    if (shape == 0 && stride) stride -= 1 + (uint32_t)(g() % stride);  // len > stride: malformed
    const uint32_t readable = stride < len ? stride : len;
    if (shape == 1) stride += 1 + (uint32_t)(g() % 16);  // a longer row whose tail is not allocated
    uint8_t* buf = (uint8_t*)malloc(readable ? readable : 1);
    memcpy(buf, body.data(), readable);
    const uint32_t enc_len = g() % 4 ? 32 : (uint32_t)(g() % 70);
    const uint32_t ct_stride = (uint32_t)(g() % 96);
    uint8_t* ids = (uint8_t*)malloc(16);
    uint64_t* times = (uint64_t*)malloc(8);
    uint32_t* fields = (uint32_t*)malloc(4 * JANUS_DAP_REPORT_FIELDS);
    uint8_t *lcfg = (uint8_t*)malloc(1), *hcfg = (uint8_t*)malloc(1), *bad = (uint8_t*)malloc(1);
    uint8_t* henc = (uint8_t*)malloc(enc_len ? enc_len : 1);
    uint8_t* hct = (uint8_t*)malloc(ct_stride ? ct_stride : 1);
    uint32_t* hcl = (uint32_t*)malloc(4);
    memset(henc, 0xEE, enc_len ? enc_len : 1);
    memset(hct, 0xEE, ct_stride ? ct_stride : 1);
    const int64_t rc = janus_dap_report_decode_host(1, buf, stride, &len, ids, times, fields, lcfg,
                                                    hcfg, henc, enc_len, hct, hcl, ct_stride, bad);
    const Parsed want = len <= stride ? parse(body.data(), len) : Parsed{};
    CHECK(rc == (want.ok ? 1 : 0));
    CHECK(*bad == (want.ok ? 0 : 1));
    for (int i = 0; i < JANUS_DAP_REPORT_FIELDS; i++) CHECK(fields[i] == (want.ok ? want.f[i] : 0));
    CHECK(*lcfg == (want.ok ? want.cfg[0] : 0) && *hcfg == (want.ok ? want.cfg[1] : 0));
    const bool hok = want.ok && want.f[7] == enc_len && want.f[9] <= ct_stride;
    CHECK(*hcl == (hok ? want.f[9] : 0));
    for (uint32_t k = 0; k < enc_len; k++) CHECK(henc[k] == (hok ? body[want.f[6] + k] : 0));
    for (uint32_t k = 0; k < ct_stride; k++)
      CHECK(hct[k] == (hok && k < want.f[9] ? body[want.f[8] + k] : 0));
    if (want.ok) {
      CHECK(memcmp(ids, body.data(), 16) == 0);
      uint64_t t = 0;
      for (int i = 0; i < 8; i++) t = (t << 8) | body[16 + i];
      CHECK(*times == t);
      decoded++;
      helper_empty += !hok;
    } else {
      for (int i = 0; i < 16; i++) CHECK(ids[i] == 0);
      CHECK(*times == 0);
      malformed++;
    }
    free(buf), free(ids), free(times), free(fields), free(lcfg), free(hcfg), free(bad);
    free(henc), free(hct), free(hcl);
  }
  // a batch: rows packed back to back in one exact allocation, the last row cut short
  {
    std::vector<std::vector<uint8_t>> reps;
    uint32_t stride = 0;
    for (int i = 0; i < 9; i++) {
      reps.push_back(make_report(g));
      stride = std::max<uint32_t>(stride, (uint32_t)reps.back().size());
    }
    const uint32_t n = (uint32_t)reps.size(), last = (uint32_t)reps[n - 1].size();
    uint8_t* rows = (uint8_t*)calloc((size_t)stride * (n - 1) + last, 1);
    std::vector<uint32_t> len(n);
    for (uint32_t i = 0; i < n; i++) {
      memcpy(rows + (size_t)stride * i, reps[i].data(), reps[i].size());
      len[i] = (uint32_t)reps[i].size();
    }
    std::vector<uint8_t> ids(16 * n), lcfg(n), hcfg(n), henc(32 * n), hct(80 * n), bad(n);
    std::vector<uint64_t> times(n);
    std::vector<uint32_t> fields(JANUS_DAP_REPORT_FIELDS * n), hcl(n);
    CHECK(janus_dap_report_decode_host(n, rows, stride, len.data(), ids.data(), times.data(),
                                       fields.data(), lcfg.data(), hcfg.data(), henc.data(), 32,
                                       hct.data(), hcl.data(), 80, bad.data()) == n);
    free(rows);
  }
  printf("fuzz_report: %ld reports, %ld decoded (%ld with empty helper rows), %ld malformed -- no "
         "ASan report\n", iters, decoded, helper_empty, malformed);
  return decoded && malformed && helper_empty ? 0 : 1;
}

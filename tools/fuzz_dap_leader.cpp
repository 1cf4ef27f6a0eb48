// fuzz_dap_leader.cpp -- sanitizer harness for the leader's host side of the DAP codec:
// janus_dap_agg_job_resp_unpack_host parses an untrusted AggregationJobResp body, and
// janus_dap_agg_init_req_encode_host writes into a buffer sized by
// janus_dap_agg_init_req_max_len.  Both run here under -fsanitize=address,undefined on exact-size
// heap buffers: mutated and truncated response bodies (bit flips, byte sets, truncations, length
// extremes, splices), and random jobs whose encoding is parsed back by the helper's host parser.
// Build + run: make -C janus_amd asan_leader  (no GPU needed: only host entry points are called).
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

// a well-formed response to a request of the reports ids[0 .. n): mostly Continue-Finish(pml),
// some Finished / Reject, now and then another ping-pong message
std::vector<uint8_t> make_resp(std::mt19937_64& g, const std::vector<uint8_t>& ids, int n,
                               uint32_t pml) {
  std::vector<uint8_t> recs;
  for (int r = 0; r < n; r++) {
    recs.insert(recs.end(), ids.begin() + 16 * r, ids.begin() + 16 * r + 16);
    const uint64_t k = g() % 16;
    if (k == 0) {
      recs.push_back(1);  // Finished
    } else if (k < 3) {
      recs.push_back(2);  // Reject
      recs.push_back((uint8_t)(g() % 10));
    } else {
      recs.push_back(0);
      std::vector<uint8_t> m;
      const uint32_t ty = k == 3 ? (uint32_t)(g() % 3) : 2u;
      const uint32_t len = k == 4 ? (uint32_t)(g() % 40) : pml;
      m.push_back((uint8_t)ty);
      put_be(m, len, 4);
      for (uint32_t i = 0; i < len; i++) m.push_back((uint8_t)g());
      if (ty == 1) {
        put_be(m, 7, 4);
        for (int i = 0; i < 7; i++) m.push_back((uint8_t)g());
      }
      put_be(recs, m.size(), 4);
      recs.insert(recs.end(), m.begin(), m.end());
    }
  }
  std::vector<uint8_t> b;
  put_be(b, recs.size(), 4);
  b.insert(b.end(), recs.begin(), recs.end());
  return b;
}

void mutate(std::mt19937_64& g, std::vector<uint8_t>& b) {
  const int k = 1 + (int)(g() % 4);
  for (int i = 0; i < k && !b.empty(); i++) {
    const size_t at = g() % b.size();
    switch (g() % 5) {
      case 0: b[at] ^= (uint8_t)(1u << (g() % 8)); break;
      case 1: b[at] = (uint8_t)g(); break;
      case 2: b.resize(at); break;
      case 3: b[at] = (uint8_t)(g() % 2 ? 0xff : 0x00); break;
      default: {
        const size_t from = g() % b.size(), len = std::min<size_t>(g() % 64, b.size() - from);
        std::vector<uint8_t> chunk(b.begin() + from, b.begin() + from + len);
        b.insert(b.begin() + at, chunk.begin(), chunk.end());
      }
    }
  }
}

uint8_t* exact(const std::vector<uint8_t>& v) {
  uint8_t* p = (uint8_t*)malloc(v.size() ? v.size() : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size());
  return p;
}

int fuzz_resp(std::mt19937_64& g, long* ok, long* rejected) {
  const int n = (int)(g() % 12), rows = n + (int)(g() % 4);
  const uint32_t pml = (uint32_t)(g() % 3 == 0 ? g() % 20 : 16);
  std::vector<uint8_t> ids(16 * (size_t)rows + 1);
  for (auto& x : ids) x = (uint8_t)g();
  // the first n rows are in the request, in a rotated order
  std::vector<uint32_t> index(rows + 1, JANUS_DAP_INDEX_NONE);
  std::vector<uint8_t> req_ids(16 * (size_t)n + 1);
  const int rot = n ? (int)(g() % n) : 0;
  for (int r = 0; r < n; r++) {
    index[r] = (uint32_t)((r + rot) % n);
    memcpy(&req_ids[16 * index[r]], &ids[16 * r], 16);
  }
  std::vector<uint8_t> body = make_resp(g, req_ids, n, pml);
  if (g() % 8) mutate(g, body);
  uint8_t* buf = exact(body);
  uint8_t* msgs = (uint8_t*)malloc((size_t)rows * pml + 1);
  uint8_t* perr = (uint8_t*)malloc(rows + 1);
  const int rc = janus_dap_agg_job_resp_unpack_host((uint32_t)rows, index.data(), ids.data(),
                                                    (uint32_t)n, buf, body.size(), pml, msgs, perr);
  int bad = 0;
  if (rc == 0) {
    (*ok)++;
    for (int r = 0; r < rows; r++) {
      if (perr[r] != 0xFF && perr[r] > 9) bad = 1;
      if (r >= n && perr[r] != 0xFF) bad = 1;
    }
  } else {
    (*rejected)++;
    if (rc < JANUS_DAP_RESP_EID || rc > JANUS_DAP_RESP_ELISTLEN) bad = 1;
  }
  if (bad) fprintf(stderr, "fuzz_resp: unexpected result rc=%d\n", rc);
  free(buf);
  free(msgs);
  free(perr);
  return bad;
}

int fuzz_req(std::mt19937_64& g, long* encoded) {
  const uint32_t n = (uint32_t)(g() % 20), psl = (uint32_t)(g() % 3) * 16, enc_len = 32,
                 stride = 16 * (1 + (uint32_t)(g() % 6)), ps_len = (uint32_t)(g() % 70),
                 apl = (uint32_t)(g() % 9);
  const uint8_t qt = (uint8_t)(1 + g() % 2);
  auto rnd = [&](size_t k) {
    std::vector<uint8_t> v(k);
    for (auto& x : v) x = (uint8_t)g();
    return v;
  };
  std::vector<uint8_t> ap = rnd(apl), bid = rnd(32), ids = rnd(16 * (size_t)n), pub = rnd((size_t)psl * n),
                       cfg = rnd(n), enc = rnd((size_t)enc_len * n), ct = rnd((size_t)stride * n),
                       ps = rnd((size_t)ps_len * n), st(n);
  std::vector<uint64_t> times(n);
  std::vector<uint32_t> cl(n);
  bool over = false;
  for (uint32_t r = 0; r < n; r++) {
    times[r] = g();
    st[r] = g() % 5 == 0 ? (uint8_t)(1 + g() % 6) : 0;
    cl[r] = g() % 50 == 0 ? stride + 1 + (uint32_t)(g() % 3) : (uint32_t)(g() % (stride + 1));
    over = over || (st[r] == 0 && cl[r] > stride);
  }
  const size_t cap = janus_dap_agg_init_req_max_len(n, apl, qt, psl, enc_len, stride, ps_len);
  uint8_t *a_ap = exact(ap), *a_ids = exact(ids), *a_pub = exact(pub), *a_cfg = exact(cfg),
          *a_enc = exact(enc), *a_ct = exact(ct), *a_ps = exact(ps), *a_st = exact(st);
  uint8_t* out = (uint8_t*)malloc(cap);
  std::vector<uint32_t> index(n + 1);
  uint32_t ninc = 0;
  const int64_t len = janus_dap_agg_init_req_encode_host(
      n, a_ap, apl, qt, bid.data(), a_ids, times.data(), a_pub, psl, a_cfg, a_enc, enc_len, a_ct,
      cl.data(), stride, a_ps, ps_len, a_st, out, index.data(), &ninc);
  int bad = 0;
  if (over) {
    bad = len != JANUS_DAP_EARG;
  } else if (len < 0 || (size_t)len > cap) {
    bad = 1;
  } else {
    (*encoded)++;
    // the helper's host parser reads the body back
    uint8_t* body = (uint8_t*)malloc((size_t)len);
    memcpy(body, out, (size_t)len);
    janus_dap_agg_init_layout L;
    if (janus_dap_agg_init_scan_ex(body, (size_t)len, psl, enc_len, ps_len, &L) != 0) bad = 1;
    if (!bad && ninc) {
      std::vector<uint8_t> o_ids(16 * (size_t)ninc), o_pub((size_t)psl * ninc + 1), o_cfg(ninc),
          o_enc((size_t)enc_len * ninc), o_ct((size_t)stride * ninc), o_ps((size_t)ps_len * ninc + 1),
          o_st(ninc);
      std::vector<uint64_t> o_t(ninc);
      std::vector<uint32_t> o_cl(ninc);
      const int64_t m = janus_dap_agg_init_unpack_host(
          body, (size_t)len, &L, ninc, o_ids.data(), o_t.data(), o_pub.data(), o_cfg.data(),
          o_enc.data(), o_ct.data(), o_cl.data(), stride, o_ps.data(), o_st.data());
      bad = m != (int64_t)ninc;
      for (uint32_t r = 0, k = 0; r < n && !bad; r++) {
        if (st[r]) {
          bad = index[r] != JANUS_DAP_INDEX_NONE;
          continue;
        }
        bad = index[r] != k || o_t[k] != times[r] || o_cl[k] != cl[r] || o_cfg[k] != cfg[r] ||
              o_st[k] != 0 || memcmp(&o_ids[16 * (size_t)k], &ids[16 * (size_t)r], 16) ||
              memcmp(&o_ct[(size_t)stride * k], &ct[(size_t)stride * r], cl[r]) ||
              (ps_len && memcmp(&o_ps[(size_t)ps_len * k], &ps[(size_t)ps_len * r], ps_len)) ||
              (psl && memcmp(&o_pub[(size_t)psl * k], &pub[(size_t)psl * r], psl));
        k++;
      }
    }
    free(body);
  }
  if (bad) fprintf(stderr, "fuzz_req: unexpected result len=%lld\n", (long long)len);
  free(a_ap), free(a_ids), free(a_pub), free(a_cfg), free(a_enc), free(a_ct), free(a_ps), free(a_st);
  free(out);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 g(argc > 2 ? strtoull(argv[2], nullptr, 10) : 0x4c45414445ull);
  long ok = 0, rejected = 0, encoded = 0;
  for (long it = 0; it < iters; it++)
    if (fuzz_resp(g, &ok, &rejected) || fuzz_req(g, &encoded)) return 1;
  printf("fuzz_dap_leader: %ld responses (%ld decoded, %ld rejected), %ld requests encoded and "
         "parsed back -- no sanitizer report\n", iters, ok, rejected, encoded);
  return 0;
}

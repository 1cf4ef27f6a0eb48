// dap_report.h -- the walk over one DAP `Report` body that the leader's upload decode shares:
// k_rep_decode and the host form (dap_codec.hip) and the front kernel of a coalesced upload group
// (prio3_upload.hip).
#pragma once
#include <cstdint>

// Walks one Report of `len` bytes: f[] = the JANUS_DAP_REPORT_* offsets and lengths, cfg[] = the two
// config IDs.  The cursor o never passes len and every read is below it; false = does not decode.
__host__ __device__ inline bool rep_parse(const uint8_t* row, uint32_t len, uint32_t* f,
                                          uint32_t* cfg) {
  if (len < 28) return false;
  const uint32_t psl = ((uint32_t)row[24] << 24) | ((uint32_t)row[25] << 16) |
                       ((uint32_t)row[26] << 8) | row[27];
  uint32_t o = 28;
  if (psl > len - o) return false;
  f[0] = o;
  f[1] = psl;
  o += psl;
  for (int c = 0; c < 2; c++) {
    if (len - o < 3) return false;
    cfg[c] = row[o];
    const uint32_t el = ((uint32_t)row[o + 1] << 8) | row[o + 2];
    o += 3;
    if (el > len - o) return false;
    f[2 + 4 * c] = o;
    f[3 + 4 * c] = el;
    o += el;
    if (len - o < 4) return false;
    const uint32_t pl = ((uint32_t)row[o] << 24) | ((uint32_t)row[o + 1] << 16) |
                        ((uint32_t)row[o + 2] << 8) | row[o + 3];
    o += 4;
    if (pl > len - o) return false;
    f[4 + 4 * c] = o;
    f[5 + 4 * c] = pl;
    o += pl;
  }
  return o == len;  // Report::get_decoded refuses trailing bytes
}

// Walk of the BGZF members of a file image (SAM specification 4.1): plain C++, no device runtime, shared by
// inflate_api.hip and the host check tests/native/inflate_core_check.cpp.
#pragma once
#include <stdint.h>

namespace gklinf {

enum BgzfScan { BGZF_OK = 0, BGZF_BAD_MAGIC = 1, BGZF_SHORT_HEADER = 2, BGZF_NO_BC = 3, BGZF_BAD_BSIZE = 4 };

inline const char* bgzf_scan_message(int r) {
  switch (r) {
    case BGZF_BAD_MAGIC: return "not a BGZF member (magic 1f 8b 08 04 expected)";
    case BGZF_SHORT_HEADER: return "the file ends inside a member's header";
    case BGZF_NO_BC: return "no BC subfield in the member's extra field";
    case BGZF_BAD_BSIZE: return "BSIZE points before the payload or past the end of the file";
    default: return "ok";
  }
}

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// Members from file[0] on, until the end of the file, max_members (when the arrays are given) or the first malformed
// member.  *n_members counts the well-formed ones, *bytes_used is the offset behind the last of them.  The arrays may
// all be NULL to count only.
inline int bgzf_scan(const uint8_t* file, int64_t len, int32_t max_members, int64_t* payload_off, int32_t* payload_len,
                     uint32_t* crc32, uint32_t* isize, int32_t* n_members, int64_t* bytes_used) {
  int64_t at = 0;
  int32_t m = 0;
  int r = BGZF_OK;
  while (at < len && (!payload_off || m < max_members) && m < INT32_MAX) {
    const uint8_t* p = file + at;
    const int64_t rest = len - at;
    if (rest < 4) { r = BGZF_SHORT_HEADER; break; }
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) { r = BGZF_BAD_MAGIC; break; }
    if (rest < 12) { r = BGZF_SHORT_HEADER; break; }
    const int64_t xlen = le16(p + 10);
    if (rest < 12 + xlen) { r = BGZF_SHORT_HEADER; break; }
    int64_t bsize = -1;
    for (int64_t x = 12; x + 4 <= 12 + xlen;) {
      const int64_t slen = le16(p + x + 2);
      if (x + 4 + slen > 12 + xlen) break;
      if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2) { bsize = le16(p + x + 4); break; }
      x += 4 + slen;
    }
    if (bsize < 0) { r = BGZF_NO_BC; break; }
    const int64_t total = bsize + 1;
    if (total < 12 + xlen + 8 || total > rest) { r = BGZF_BAD_BSIZE; break; }
    if (payload_off) {
      payload_off[m] = at + 12 + xlen;
      payload_len[m] = (int32_t)(total - 12 - xlen - 8);
      crc32[m] = le32(p + total - 8);
      isize[m] = le32(p + total - 4);
    }
    m++;
    at += total;
  }
  *n_members = m;
  *bytes_used = at;
  return r;
}

}  // namespace gklinf

// BGZF member framing (the SAM specification, section 4.1), host only and HIP-free: the 18-byte header with the BC
// subfield, the CRC32 / ISIZE trailer and the 28-byte end-of-file member.  deflate_api.hip frames the device's streams
// with it, tests/native/deflate_core_check.cpp the host core's.
#pragma once
#include <stdint.h>
#include <string.h>

namespace gkldef {

constexpr int kBgzfHeader = 18, kBgzfTrailer = 8, kBgzfEof = 28;
constexpr int kBgzfMaxBlock = 65498, kBgzfDefaultBlock = 65280;   // input bytes per member: 65498 + 5 + 26 <= 65536

// One member around `clen` bytes of raw deflate at p + kBgzfHeader (already in place).  Returns the member's size.
inline uint32_t bgzf_frame(uint8_t* p, uint32_t clen, uint32_t crc, uint32_t isize) {
  static const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  const uint32_t total = kBgzfHeader + clen + kBgzfTrailer;
  memcpy(p, head, 16);
  p[16] = (uint8_t)((total - 1) & 0xFF);
  p[17] = (uint8_t)((total - 1) >> 8);
  uint8_t* t = p + kBgzfHeader + clen;
  for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(isize >> (8 * i)); }
  return total;
}

inline void bgzf_eof(uint8_t* p) {
  p[kBgzfHeader] = 0x03; p[kBgzfHeader + 1] = 0x00;   // a final fixed block with the end-of-block code only
  bgzf_frame(p, 2, 0, 0);
}

inline int64_t bgzf_members(int64_t len, int32_t block_size) { return len <= 0 ? 0 : (len + block_size - 1) / block_size; }
// every member stored, plus the end-of-file member
inline int64_t bgzf_bound(int64_t len, int32_t block_size) {
  return (len < 0 ? 0 : len) + (5 + kBgzfHeader + kBgzfTrailer) * bgzf_members(len, block_size) + kBgzfEof;
}

}  // namespace gkldef

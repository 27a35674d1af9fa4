// Stand-alone host check of gkl_amd/csrc/inflate_core.h (the decoder the GPU kernel instantiates for a wavefront) and
// gkl_amd/csrc/bgzf_scan.h: the same core for ONE host thread, built with the address and undefined-behaviour
// sanitizers by tests/test_inflate_core_cpu.py.  Every source and every output sits in a heap block of exactly its
// size, so one byte read or written out of range is a report.
//   inflate_core_check run CASES RESULTS    CASES:   u32 n, then n x (u32 src_len, u32 capacity, src bytes)
//                                           RESULTS: n x (i32 status, i32 out_len, i32 consumed, u32 crc32, out bytes)
//   inflate_core_check scan FILE MAX        prints "rc n_members bytes_used", then "payload_off payload_len crc32 isize"
//                                           per member (MAX < 0: count only)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../gkl_amd/csrc/inflate_core.h"
#include "../../gkl_amd/csrc/bgzf_scan.h"

namespace {
struct HostExec {
  static constexpr int kLanes = 1;
  static int lane() { return 0; }
  static void sync() {}
};

std::unique_ptr<uint8_t[]> read_file(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  *len = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  std::unique_ptr<uint8_t[]> buf(new uint8_t[*len]);   // exactly sized
  if (*len && fread(buf.get(), 1, *len, f) != *len) { perror("fread"); exit(2); }
  fclose(f);
  return buf;
}

int run(const char* cases, const char* results) {
  size_t len = 0;
  const auto file = read_file(cases, &len);
  FILE* out = fopen(results, "wb");
  if (!out) { perror(results); return 2; }
  size_t at = 0;
  const auto u32 = [&] { uint32_t v; if (at + 4 > len) { fprintf(stderr, "case file truncated\n"); exit(2); } memcpy(&v, file.get() + at, 4); at += 4; return v; };
  const uint32_t n = u32();
  const std::unique_ptr<gklinf::Scratch> S(new gklinf::Scratch);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t src_len = u32(), cap = u32();
    if (at + src_len > len) { fprintf(stderr, "case file truncated\n"); return 2; }
    const std::unique_ptr<uint8_t[]> src(new uint8_t[src_len]), dst(new uint8_t[cap]);
    if (src_len) memcpy(src.get(), file.get() + at, src_len);
    at += src_len;
    memset(S.get(), 0xEE, sizeof(gklinf::Scratch));   // nothing may depend on what the last stream left
    int32_t res[3] = {0, 0, 0};
    res[0] = gklinf::inflate_stream<HostExec>(*S, src.get(), (int32_t)src_len, dst.get(), (int32_t)cap, &res[1], &res[2]);
    if (res[1] < 0 || (uint32_t)res[1] > cap) { fprintf(stderr, "case %u: out_len %d of %u\n", k, res[1], cap); return 1; }
    const uint32_t crc = gklinf::crc32_stream<HostExec>(*S, dst.get(), (uint32_t)res[1]);
    fwrite(res, 4, 3, out);
    fwrite(&crc, 4, 1, out);
    if (res[1]) fwrite(dst.get(), 1, (size_t)res[1], out);
  }
  fclose(out);
  printf("ok: %u streams\n", n);
  return 0;
}

int scan(const char* path, int max_members) {
  size_t len = 0;
  const auto file = read_file(path, &len);
  int32_t n = 0;
  int64_t used = 0;
  if (max_members < 0) {
    const int rc = gklinf::bgzf_scan(file.get(), (int64_t)len, 0, nullptr, nullptr, nullptr, nullptr, &n, &used);
    printf("%d %d %lld\n", rc, n, (long long)used);
    return 0;
  }
  const size_t m = (size_t)max_members;
  const std::unique_ptr<int64_t[]> off(new int64_t[m]);
  const std::unique_ptr<int32_t[]> plen(new int32_t[m]);
  const std::unique_ptr<uint32_t[]> crc(new uint32_t[m]), isize(new uint32_t[m]);
  const int rc = gklinf::bgzf_scan(file.get(), (int64_t)len, max_members, off.get(), plen.get(), crc.get(), isize.get(), &n, &used);
  printf("%d %d %lld\n", rc, n, (long long)used);
  for (int32_t k = 0; k < n; k++) printf("%lld %d %u %u\n", (long long)off[(size_t)k], plen[(size_t)k], crc[(size_t)k], isize[(size_t)k]);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "scan")) return scan(argv[2], atoi(argv[3]));
  fprintf(stderr, "usage: %s run CASES RESULTS | scan FILE MAX\n", argv[0]);
  return 2;
}

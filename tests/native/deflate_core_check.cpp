// Stand-alone host check of gkl_amd/csrc/deflate_core.h (the encoder the GPU kernel instantiates for a wavefront): the
// same core for ONE host thread, and a second time for FOUR lanes (threads that meet at every sync(), which shows that
// the loops are lane-strided correctly, nothing more).  tests/test_deflate_core_cpu.py builds it with the address and
// undefined-behaviour sanitizers, tests/test_deflate.py without them as the byte-exact reference of the GPU's streams.
// Every source and every output sits in a heap block of exactly its size.
//   deflate_core_check run INPUTS RESULTS LEVEL STRATEGY TYPES LANES
//        INPUTS:  u32 n, then n x (u32 len, u32 capacity, bytes)
//        RESULTS: n x (i32 status, i32 out_len, u32 crc32 of the input, out bytes)
//   deflate_core_check lengths INPUTS RESULTS     INPUTS: u32 n, then n x (u32 symbols, u32 limit, u32 counts[symbols])
//                                                 RESULTS: per case one byte per symbol, its code length
//   deflate_core_check bgzf DATA BLOCK_SIZE LEVEL EOF IMAGE    the BGZF image of DATA from the host core's streams
//   deflate_core_check bound LEN                  prints deflate_bound(LEN)
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../gkl_amd/csrc/deflate_core.h"
#include "../../gkl_amd/csrc/bgzf_frame.h"

namespace {
struct Barrier {
  std::atomic<int> waiting{0}, round{0};
  void wait(int n) {
    const int r = round.load();
    if (waiting.fetch_add(1) + 1 == n) { waiting.store(0); round.fetch_add(1); return; }
    for (int spin = 0; round.load() == r; spin++)
      if (spin > 200) std::this_thread::yield();
  }
};

template <int N>
struct HostExec {
  static constexpr int kLanes = N;
  static thread_local int lane_;
  static Barrier barrier;
  static uint32_t total_;
  static int lane() { return lane_; }
  static void sync() { if (N > 1) barrier.wait(N); }
  static uint32_t excl_scan64(uint32_t* a) {
    sync();
    if (lane() == 0) {
      uint32_t sum = 0;
      for (int i = 0; i < 64; i++) { const uint32_t v = a[i]; a[i] = sum; sum += v; }
      total_ = sum;
    }
    sync();
    return total_;
  }
  static uint64_t which64(const uint16_t* a) {
    uint64_t m = 0;
    for (int i = 0; i < 64; i++) m |= (uint64_t)(a[i] != 0) << i;
    return m;
  }
  static void atomic_add(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
  static void atomic_or(uint32_t* p, uint32_t v) { __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
  static void atomic_max16(uint16_t* p, uint16_t v) {
    uint16_t cur = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  }
  // runs body once per lane; the lanes meet at every sync()
  template <class F>
  static void lanes(F body) {
    if (N == 1) { lane_ = 0; body(); return; }
    std::vector<std::thread> t;
    for (int l = 0; l < N; l++) t.emplace_back([l, &body] { lane_ = l; body(); });
    for (auto& th : t) th.join();
  }
};
template <int N> thread_local int HostExec<N>::lane_ = 0;
template <int N> Barrier HostExec<N>::barrier;
template <int N> uint32_t HostExec<N>::total_ = 0;

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

struct Work {
  std::unique_ptr<gkldef::Scratch> S{new gkldef::Scratch};
  std::unique_ptr<uint32_t[]> toks{new uint32_t[gkldef::kTokensPerWave]};
};

// one stream through the core: status, length and the CRC-32 of the input
template <class X>
int one_stream(Work& w, const uint8_t* src, uint32_t len, uint8_t* dst, uint32_t cap, int level, int strategy, int types, int32_t* out_len, uint32_t* crc) {
  memset(w.S.get(), 0xEE, sizeof(gkldef::Scratch));   // nothing may depend on what the last stream left
  int status = 0;
  X::lanes([&] {
    const uint32_t c = gklinf::crc32_stream<X>(w.S->u.inf, src, len);
    int32_t n = 0;
    const int st = gkldef::deflate_stream<X>(*w.S, src, (int32_t)len, dst, (int32_t)cap, w.toks.get(), level, strategy, types, &n);
    if (X::lane() == 0) { status = st; *out_len = n; *crc = c; }
  });
  return status;
}

template <class X>
int run(const char* inputs, const char* results, int level, int strategy, int types) {
  size_t len = 0;
  const auto file = read_file(inputs, &len);
  FILE* out = fopen(results, "wb");
  if (!out) { perror(results); return 2; }
  size_t at = 0;
  const auto u32 = [&] { uint32_t v; if (at + 4 > len) { fprintf(stderr, "input file truncated\n"); exit(2); } memcpy(&v, file.get() + at, 4); at += 4; return v; };
  const uint32_t n = u32();
  Work w;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t src_len = u32(), cap = u32();
    if (at + src_len > len) { fprintf(stderr, "input file truncated\n"); return 2; }
    const std::unique_ptr<uint8_t[]> src(new uint8_t[src_len]), dst(new uint8_t[cap]);
    if (src_len) memcpy(src.get(), file.get() + at, src_len);
    at += src_len;
    int32_t res[2] = {0, 0};
    uint32_t crc = 0;
    res[0] = one_stream<X>(w, src.get(), src_len, dst.get(), cap, level, strategy, types, &res[1], &crc);
    if (res[1] < 0 || (uint32_t)res[1] > cap) { fprintf(stderr, "input %u: out_len %d of %u\n", k, res[1], cap); return 1; }
    fwrite(res, 4, 2, out);
    fwrite(&crc, 4, 1, out);
    if (res[1]) fwrite(dst.get(), 1, (size_t)res[1], out);
  }
  fclose(out);
  printf("ok: %u streams\n", n);
  return 0;
}

int lengths(const char* inputs, const char* results) {
  using X = HostExec<1>;
  size_t len = 0;
  const auto file = read_file(inputs, &len);
  FILE* out = fopen(results, "wb");
  if (!out) { perror(results); return 2; }
  size_t at = 0;
  const auto u32 = [&] { uint32_t v; if (at + 4 > len) { fprintf(stderr, "input file truncated\n"); exit(2); } memcpy(&v, file.get() + at, 4); at += 4; return v; };
  const uint32_t n = u32();
  Work w;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t symbols = u32(), limit = u32();
    if (symbols > 286 || limit > 15) { fprintf(stderr, "case %u: %u symbols, limit %u\n", k, symbols, limit); return 2; }
    const std::unique_ptr<uint32_t[]> freq(new uint32_t[symbols]);
    const std::unique_ptr<uint8_t[]> lens(new uint8_t[symbols]);
    for (uint32_t s = 0; s < symbols; s++) freq[s] = u32();
    memset(w.S.get(), 0xEE, sizeof(gkldef::Scratch));
    gkldef::build_lengths<X>(*w.S, freq.get(), symbols, limit, lens.get());
    fwrite(lens.get(), 1, symbols, out);
  }
  fclose(out);
  printf("ok: %u histograms\n", n);
  return 0;
}

int bgzf(const char* data_path, int block_size, int level, int eof, const char* image_path) {
  using X = HostExec<1>;
  size_t len = 0;
  const auto data = read_file(data_path, &len);
  if (block_size == 0) block_size = gkldef::kBgzfDefaultBlock;
  if (block_size < 1 || block_size > gkldef::kBgzfMaxBlock) return 2;
  FILE* out = fopen(image_path, "wb");
  if (!out) { perror(image_path); return 2; }
  Work w;
  for (size_t at = 0; at < len; at += (size_t)block_size) {
    const uint32_t n = (uint32_t)(len - at < (size_t)block_size ? len - at : (size_t)block_size);
    const uint32_t cap = (uint32_t)gkldef::deflate_bound(n);
    const std::unique_ptr<uint8_t[]> src(new uint8_t[n]), member(new uint8_t[gkldef::kBgzfHeader + cap + gkldef::kBgzfTrailer]);
    memcpy(src.get(), data.get() + at, n);
    int32_t clen = 0;
    uint32_t crc = 0;
    if (one_stream<X>(w, src.get(), n, member.get() + gkldef::kBgzfHeader, cap, level, 0, 0, &clen, &crc)) return 1;
    fwrite(member.get(), 1, gkldef::bgzf_frame(member.get(), (uint32_t)clen, crc, n), out);
  }
  if (eof) {
    uint8_t e[gkldef::kBgzfEof];
    gkldef::bgzf_eof(e);
    fwrite(e, 1, sizeof e, out);
  }
  fclose(out);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 8 && !strcmp(argv[1], "run")) {
    const int level = atoi(argv[4]), strategy = atoi(argv[5]), types = atoi(argv[6]), n_lanes = atoi(argv[7]);
    if (n_lanes == 1) return run<HostExec<1>>(argv[2], argv[3], level, strategy, types);
    if (n_lanes == 4) return run<HostExec<4>>(argv[2], argv[3], level, strategy, types);
  }
  if (argc == 4 && !strcmp(argv[1], "lengths")) return lengths(argv[2], argv[3]);
  if (argc == 7 && !strcmp(argv[1], "bgzf")) return bgzf(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6]);
  if (argc == 3 && !strcmp(argv[1], "bound")) { printf("%lld\n", (long long)gkldef::deflate_bound(atoll(argv[2]))); return 0; }
  fprintf(stderr, "usage: %s run INPUTS RESULTS LEVEL STRATEGY TYPES LANES(1|4) | lengths INPUTS RESULTS | bgzf DATA BLOCK_SIZE LEVEL EOF IMAGE | bound LEN\n", argv[0]);
  return 2;
}

// Stand-alone check of gkl_amd/csrc/pdhmm_gather_plan.h (tests/test_pdhmm_gather_plan_cpu.py builds it with
// -fsanitize=address,undefined and expects exit 0): for a few hundred seeded random sets of 1-64 regions -- K = 1 and
// K = 64, 1 x 1 regions, row strides of 1 and of 600, strides that are and are not multiples of 16, source arrays at
// every alignment -- the descriptor table is built and executed by a host loop over real buffers, with the kernel's own
// index functions (pd_gather_split, pd_gather_unit_at, pd_gather_tail_at), and
//   * the destination ranges of distinct (descriptor, row) pairs are disjoint and inside PdInputLayout::total;
//   * no source byte at or beyond n_items * src_row is read: every source array is a heap block of exactly that size
//     (plus the offset that sets its alignment), so AddressSanitizer faults on the first byte beyond it;
//   * every byte written lies inside its row's first src_row bytes, and nothing else of the block changes;
//   * the result equals what the host form's memcpy loop (pd_run_multi_locked) produces for the same regions.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../gkl_amd/csrc/pdhmm_gather_plan.h"

using namespace gklhip;

#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "set %d: %s failed: ", set, #cond);               \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      return 1;                                                              \
    }                                                                        \
  } while (0)

namespace {
struct Aligned16 {   // a heap block of exactly `bytes` bytes on a 16-byte boundary
  unsigned char* block = nullptr;
  Aligned16() = default;
  Aligned16(const Aligned16&) = delete;
  Aligned16& operator=(const Aligned16&) = delete;
  ~Aligned16() { std::free(block); }
  unsigned char* make(size_t bytes) {
    std::free(block);
    void* q = nullptr;
    if (posix_memalign(&q, 16, bytes) != 0) std::abort();
    return block = static_cast<unsigned char*>(q);
  }
};
// An array of exactly `bytes` bytes whose first byte lies `skew` bytes behind a 16-byte boundary: the end of the heap
// block is the end of the array.
struct Source {
  Aligned16 mem;
  unsigned char* p = nullptr;
  size_t bytes = 0;
  void make(size_t n, size_t skew, std::mt19937& rng) {
    p = mem.make(skew + n) + skew;
    bytes = n;
    for (size_t i = 0; i < n; i++) p[i] = (unsigned char)(rng() & 0xffu);
  }
};

struct Region {
  int n_haps, n_reads, max_hap, max_read;
  Source arrays[kPdGatherArrays];
};
}  // namespace

int main(int argc, char** argv) {
  const int n_sets = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937 rng(20240917u);
  auto pick = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  long long rows_seen = 0, units_seen = 0, tail_bytes_seen = 0;
  for (int set = 0; set < n_sets; set++) {
    const int K = set == 0 ? 1 : set == 1 ? 64 : set == 2 ? 2 : pick(1, kPdMaxRegions);
    // kinds of sets: every stride its own; every region the same strides (contiguous arrays); strides multiples of 16
    const int kind = set < 3 ? set : pick(0, 3);
    const int common_hap = 16 * pick(1, 12), common_read = 16 * pick(1, 12);
    std::vector<Region> R((size_t)K);
    for (int k = 0; k < K; k++) {
      Region& r = R[(size_t)k];
      const bool tiny = pick(0, 5) == 0;   // a 1 x 1 region
      r.n_haps = tiny ? 1 : pick(1, 9);
      r.n_reads = tiny ? 1 : pick(1, 40);
      auto stride = [&](int common) { return kind == 1 ? common : kind == 2 ? 16 * pick(1, 12) : pick(0, 7) == 0 ? 1 : pick(0, 7) == 0 ? 600 : pick(1, 200); };
      r.max_hap = stride(common_hap);
      r.max_read = stride(common_read);
      if (set == 2) { r.max_hap = k == 0 ? 1 : 600; r.max_read = k == 0 ? 600 : 1; }   // strides 1 and 600 next to each other
      for (int a = 0; a < kPdGatherArrays; a++) {
        const size_t bytes = a < 2 ? (size_t)r.n_haps * (size_t)r.max_hap : (size_t)r.n_reads * (size_t)r.max_read;
        // aligned sources in half of the aligned-stride sets (the 16-byte path), any skew elsewhere
        r.arrays[a].make(bytes, (kind == 1 || kind == 2) && pick(0, 1) ? 0 : (size_t)pick(0, 15), rng);
      }
    }
    size_t NH = 0, NR = 0, mh = 0, mr = 0;
    for (const Region& r : R) {
      NH += (size_t)r.n_haps; NR += (size_t)r.n_reads;
      mh = std::max(mh, (size_t)r.max_hap); mr = std::max(mr, (size_t)r.max_read);
    }
    const PdInputLayout in(NH, NR, mh, mr);
    const PdGatherTable T(in, K);
    CHECK(T.o_desc == in.total && T.o_results >= T.o_desc + (size_t)K * kPdGatherArrays * sizeof(PdGatherDesc) &&
              T.total >= T.o_results + (size_t)K * sizeof(PdRegionResults) && T.o_results % 256 == 0,
          "table at %zu / %zu / %zu", T.o_desc, T.o_results, T.total);
    std::vector<PdGatherRegion> G((size_t)K);
    for (int k = 0; k < K; k++) {
      for (int a = 0; a < kPdGatherArrays; a++) G[(size_t)k].arrays[a] = R[(size_t)k].arrays[a].p;
      G[(size_t)k].n_haps = R[(size_t)k].n_haps; G[(size_t)k].n_reads = R[(size_t)k].n_reads;
      G[(size_t)k].max_hap_len = R[(size_t)k].max_hap; G[(size_t)k].max_read_len = R[(size_t)k].max_read;
    }
    std::vector<PdGatherDesc> descs((size_t)K * kPdGatherArrays);
    pd_build_gather(G.data(), K, in, descs.data());

    // the destination block: 16-byte aligned like the device buffer, exactly in.total bytes (ASan guards its end too)
    Aligned16 dst_block;
    unsigned char* const dst = dst_block.make(in.total);
    memset(dst, 0xAB, in.total);
    std::vector<uint8_t> owner(in.total, 0);   // 1: inside some (descriptor, row)'s range

    for (size_t di = 0; di < descs.size(); di++) {
      const PdGatherDesc& d = descs[di];
      const Source& src = R[di / kPdGatherArrays].arrays[di % kPdGatherArrays];
      CHECK(d.src == src.p && (size_t)d.n_items * d.src_row == src.bytes, "descriptor %zu: %u x %u bytes of an array of %zu", di, d.n_items,
            d.src_row, src.bytes);
      CHECK(d.src_row >= 1 && d.src_row <= d.dst_row, "descriptor %zu: rows %u -> %u", di, d.src_row, d.dst_row);
      for (uint32_t i = 0; i < d.n_items; i++) {   // the row's destination range: its first src_row bytes
        const size_t lo = d.dst_off + (size_t)i * d.dst_row;
        CHECK(lo + d.src_row <= in.total, "descriptor %zu row %u ends at %zu of %zu", di, i, lo + d.src_row, in.total);
        for (size_t b = lo; b < lo + d.src_row; b++) { CHECK(owner[b] == 0, "byte %zu belongs to two rows", b); owner[b] = 1; }
        rows_seen++;
      }
      // execute, as pdhmm_gather_regions_kernel does
      uint32_t n_vec, tail;
      pd_gather_split(d, dst, &n_vec, &tail);
      CHECK(n_vec * 16u + tail == d.src_row, "descriptor %zu: %u units + %u bytes of %u", di, n_vec, tail, d.src_row);
      const unsigned char* s = static_cast<const unsigned char*>(d.src);
      for (uint32_t i = 0; i < d.n_items * n_vec; i++) {
        uint32_t sa, da;
        pd_gather_unit_at(d, n_vec, i, &sa, &da);
        CHECK((reinterpret_cast<uintptr_t>(s + sa) & 15u) == 0 && (reinterpret_cast<uintptr_t>(dst + d.dst_off + da) & 15u) == 0,
              "descriptor %zu unit %u is not aligned", di, i);
        CHECK(da % d.dst_row + 16u <= d.src_row, "descriptor %zu unit %u leaves its row", di, i);
        memcpy(dst + d.dst_off + da, s + sa, 16);   // (a read beyond the source array: ASan)
        units_seen++;
      }
      for (uint32_t i = 0; i < d.n_items * tail; i++) {
        uint32_t sa, da;
        pd_gather_tail_at(d, n_vec, tail, i, &sa, &da);
        CHECK(da % d.dst_row < d.src_row, "descriptor %zu tail byte %u leaves its row", di, i);
        dst[d.dst_off + da] = s[sa];
        tail_bytes_seen++;
      }
    }

    // what the host form's staging loop makes of the same regions
    std::vector<unsigned char> want(in.total, 0xAB);
    {
      const size_t at[kPdGatherArrays] = {in.o_hb, in.o_hp, in.o_rb, in.o_rq, in.o_ri, in.o_rd, in.o_gc};
      size_t hap_base = 0, read_base = 0;
      for (const Region& r : R) {
        for (int a = 0; a < kPdGatherArrays; a++) {
          const bool hap = a < 2;
          const size_t n = (size_t)(hap ? r.n_haps : r.n_reads), src_row = (size_t)(hap ? r.max_hap : r.max_read),
                       dst_row = hap ? in.hap_row : in.read_row;
          unsigned char* to = want.data() + at[a] + (hap ? hap_base : read_base) * dst_row;
          if (dst_row == src_row) { memcpy(to, r.arrays[a].p, n * src_row); continue; }
          for (size_t i = 0; i < n; i++) memcpy(to + i * dst_row, r.arrays[a].p + i * src_row, src_row);
        }
        hap_base += (size_t)r.n_haps; read_base += (size_t)r.n_reads;
      }
    }
    for (size_t b = 0; b < in.total; b++) {
      CHECK(dst[b] == want[b], "byte %zu is %02x, the host staging gives %02x", b, dst[b], want[b]);
      // (a byte outside every row still holds the fill -- in both)
    }
  }
  std::printf("ok: %d region sets, %lld rows, %lld 16-byte units, %lld tail bytes\n", n_sets, rows_seen, units_seen, tail_bytes_seen);
  return 0;
}

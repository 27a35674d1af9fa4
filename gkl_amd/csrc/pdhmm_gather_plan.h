// The input gather of a device-resident multi-region PDHMM call (gklhip_pdhmm_compute_cross_multi_device): the K regions'
// seven byte arrays lie in HBM at the regions' own row strides; the multi-region kernels need them concatenated at ONE
// common stride per side, in the PdInputLayout of the whole set.  One descriptor per (region, array) says where the
// array comes from and where its rows go; pdhmm_gather_regions_kernel (pdhmm_kernel.h) executes the table in one launch,
// device to device.  The table travels behind the set's inputs in the same device buffer and the same pinned block:
//   [ PdInputLayout of the set | 7 K descriptors | K pairs of result pointers ]
// so the ONE host-to-device copy that brings the regions' length arrays into o_hl / o_rl brings the table too.
//
// Plain C++ (tests/native/pdhmm_gather_plan_check.cpp compiles it for the host alone, under the sanitizers, and executes
// the descriptors with the same pd_gather_split / pd_gather_*_at that the kernel uses).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pdhmm_job_layout.h"   // pd_up, PdInputLayout
#include "pdhmm_multi_plan.h"   // GKL_PD_HD

namespace gklhip {

constexpr int kPdGatherArrays = 7;   // hap_bases, hap_pdbases, read_bases, read_qual, read_ins_qual, read_del_qual, gcp

// One array of one region: n_items rows of src_row bytes at src (HBM, any alignment) go to rows of dst_row >= src_row
// bytes from byte dst_off of the set's input block on.  Exactly src_row bytes of every row are copied: no source byte
// at or beyond n_items * src_row is read, nothing outside a row's first src_row bytes is written.  An array whose rows
// keep their stride is ONE row of all its bytes.
struct PdGatherDesc {
  const void* src;
  uint64_t dst_off;
  uint32_t n_items, src_row, dst_row, reserved;
};
static_assert(sizeof(PdGatherDesc) == 32, "the table is copied to the device as it stands");

// Where a device-resident multi-region call leaves region k's results: HBM addresses; sums may be NULL.
struct PdRegionResults {
  double* out;
  double* sums;
};

// A region as the gather sees it: the seven arrays in the order of kPdGatherArrays (the first two: one row per haplotype).
struct PdGatherRegion {
  const void* arrays[kPdGatherArrays];
  int32_t n_haps, n_reads, max_hap_len, max_read_len;
};

// The table's place behind the inputs, in bytes from the start of the input block.
struct PdGatherTable {
  size_t o_desc, o_results, total;
  PdGatherTable(const PdInputLayout& in, int K)
      : o_desc(in.total), o_results(o_desc + pd_up((size_t)K * kPdGatherArrays * sizeof(PdGatherDesc))),
        total(o_results + pd_up((size_t)K * sizeof(PdRegionResults))) {}
};

// out[7 k + a]: array a of region k.  Region k's rows follow those of the regions before it (the read_base / hap_base
// of pd_build_regions).  `in`: the layout of the whole set -- its row strides are at least every region's.
inline void pd_build_gather(const PdGatherRegion* R, int K, const PdInputLayout& in, PdGatherDesc* out) {
  const size_t at[kPdGatherArrays] = {in.o_hb, in.o_hp, in.o_rb, in.o_rq, in.o_ri, in.o_rd, in.o_gc};
  size_t hap_base = 0, read_base = 0;
  for (int k = 0; k < K; k++) {
    for (int a = 0; a < kPdGatherArrays; a++) {
      const bool hap = a < 2;
      const size_t n = (size_t)(hap ? R[k].n_haps : R[k].n_reads), src_row = (size_t)(hap ? R[k].max_hap_len : R[k].max_read_len),
                   dst_row = hap ? in.hap_row : in.read_row, base = hap ? hap_base : read_base;
      PdGatherDesc& d = out[k * kPdGatherArrays + a];
      d.src = R[k].arrays[a];
      d.dst_off = at[a] + base * dst_row;
      d.reserved = 0;
      if (src_row == dst_row) { d.n_items = 1; d.src_row = d.dst_row = (uint32_t)(n * src_row); }
      else { d.n_items = (uint32_t)n; d.src_row = (uint32_t)src_row; d.dst_row = (uint32_t)dst_row; }
    }
    hap_base += (size_t)R[k].n_haps;
    read_base += (size_t)R[k].n_reads;
  }
}

// How a row of the descriptor is copied: n_vec 16-byte units first, then `tail` single bytes (n_vec * 16 + tail ==
// src_row).  Units only where every row's source and destination start on a 16-byte boundary: both addresses aligned and,
// with more than one row, both strides multiples of 16; else the whole row goes byte by byte.  dst: the address that
// dst_off counts from.
GKL_PD_HD void pd_gather_split(const PdGatherDesc& d, const void* dst, uint32_t* n_vec, uint32_t* tail) {
  const uint64_t s = (uint64_t)(uintptr_t)d.src, t = (uint64_t)(uintptr_t)dst + d.dst_off;
  const bool vec = ((s | t) & 15u) == 0 && (d.n_items == 1 || ((d.src_row | d.dst_row) & 15u) == 0);
  *n_vec = vec ? d.src_row / 16u : 0u;
  *tail = d.src_row - *n_vec * 16u;
}
// Unit i of the descriptor's n_items * n_vec units, byte i of its n_items * tail tail bytes: offsets from d.src and from
// dst + d.dst_off.  (A set holds at most 4 MB: 32-bit arithmetic.)
GKL_PD_HD void pd_gather_unit_at(const PdGatherDesc& d, uint32_t n_vec, uint32_t i, uint32_t* src_at, uint32_t* dst_at) {
  const uint32_t item = i / n_vec, col = (i - item * n_vec) * 16u;
  *src_at = item * d.src_row + col;
  *dst_at = item * d.dst_row + col;
}
GKL_PD_HD void pd_gather_tail_at(const PdGatherDesc& d, uint32_t n_vec, uint32_t tail, uint32_t i, uint32_t* src_at, uint32_t* dst_at) {
  const uint32_t item = i / tail, col = n_vec * 16u + (i - item * tail);
  *src_at = item * d.src_row + col;
  *dst_at = item * d.dst_row + col;
}

}  // namespace gklhip

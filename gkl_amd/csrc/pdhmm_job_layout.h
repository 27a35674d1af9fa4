// Where a PDHMM call's blocks lie in its device buffers: the nine input arrays in `inputs`, a single call's job tables in
// `jobs`, the paired table route's scratch in `tabx`.  Every block starts on a 256-byte boundary; a layout is built from
// counts alone.
//
// Plain C++ (tests/native/pdhmm_multi_plan_check.cpp compiles it for the host alone, under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

#include "pairhmm_plan.h"  // PlanLane

namespace gklhip {

// What the kernels (pdhmm_kernel.h includes this header) and the host's planner (pdhmm_call_plan.h) both read: one
// definition, so a -DGKL_PD_RPL=... variant build reaches both.
// PD flag bits of hap_pdbases (reference MathUtils.h:66-75)
constexpr int kPdSnp = 1, kPdDelStart = 2, kPdDelEnd = 4, kPdA = 8, kPdC = 16, kPdG = 32, kPdT = 64;
// The most column classes of a table haplotype (pdhmm_kernel.h: "Table entries").
constexpr int kPdTabClasses = 6;
// Rows per lane (pdhmm_kernel.h: "Rows per lane" has the measurements behind the 6).
#ifndef GKL_PD_RPL
#define GKL_PD_RPL 6
#endif
constexpr int kPdRpl = GKL_PD_RPL;

inline size_t pd_up(size_t x) { return (x + 255) / 256 * 256; }
constexpr size_t kPdLaneRowBytes = 64 * sizeof(PlanLane);   // one job's lane row: 64 lanes of {item, block}

// The nine input arrays of a call (of a multi-region call: of all its regions, at the common row strides) in ONE block,
// each 256-byte aligned: the layout of the device buffer `inputs` and of the pinned block `stage_in`, and the size that
// decides whether a call is staged (kPdStageBytes) or fits a multi-region launch set.
struct PdInputLayout {
  size_t hap_row, read_row;   // bytes per item
  size_t hap_bytes, read_bytes;
  size_t o_hb, o_hp, o_rb, o_rq, o_ri, o_rd, o_gc, o_hl, o_rl, total;
  PdInputLayout(size_t n_hap_items, size_t n_read_items, size_t max_hap_len, size_t max_read_len)
      : hap_row(max_hap_len), read_row(max_read_len), hap_bytes(n_hap_items * max_hap_len), read_bytes(n_read_items * max_read_len),
        o_hb(0), o_hp(pd_up(hap_bytes)), o_rb(o_hp + pd_up(hap_bytes)), o_rq(o_rb + pd_up(read_bytes)), o_ri(o_rq + pd_up(read_bytes)),
        o_rd(o_ri + pd_up(read_bytes)), o_gc(o_rd + pd_up(read_bytes)), o_hl(o_gc + pd_up(read_bytes)),
        o_rl(o_hl + pd_up(n_hap_items * 8)), total(o_rl + pd_up(n_read_items * 8)) {}
};

// Where the job tables that the kernel arguments point at start in the device buffer `jobs`: the view that both launch
// paths fill (each lays its own block out).  jl .. js: the listed jobs' lane rows, first pairs, steps, striped flags;
// cl / cs / cr: the cross chunks' lane rows, steps, representative reads; nc / cc: the haplotypes' class counts and
// codes; jf / fj: the listed jobs' routing flags and the full launch's list; tg: the table groups; tl .. ts: the tail
// jobs' lane rows, pairs, steps, striped flags.
struct PdJobOffsets { size_t jl, jp, jn, js, cl, cs, cr, nc, cc, jf, fj, tg, tl, tp, tn, ts; };

// The counts that size a single call's job tables.
struct PdJobCounts {
  size_t n_general;        // listed jobs (paired: striped + packed chunks; cross: striped read x haplotype)
  size_t n_chunks_cross;   // cross layout: chunks of packed reads
  size_t n_haps_cross;     // cross layout: haplotypes (hap_order, hap_ncls, 8 class codes each); paired: 0
  size_t n_tail;           // reference-tail jobs
  size_t n_placed;         // paired layout: pairs (place_chunk, place_lane); cross: 0
  size_t n_chunks_paired;  // paired layout: packed chunks (chunk_used)
  size_t n_tab_starts;     // entries of tab_group_start (groups + 1, or 0)
};

// A single call's block in `jobs`, in this order (ho: the cross layout's haplotype order; pc / pl / cu: the paired
// layout's compact packing, expanded into jl on the device).
struct PdJobLayout : PdJobOffsets {
  size_t ho, pc, pl, cu, total;
  explicit PdJobLayout(const PdJobCounts& n) {
    size_t end = 0;
    auto block = [&end](size_t bytes) { const size_t at = end; end += pd_up(bytes); return at; };
    jl = block(n.n_general * kPdLaneRowBytes); jp = block(n.n_general * 4); jn = block(n.n_general * 4); js = block(n.n_general);
    cl = block(n.n_chunks_cross * kPdLaneRowBytes); ho = block(n.n_haps_cross * 4);
    cs = block(n.n_chunks_cross * 4); cr = block(n.n_chunks_cross * 4);
    tl = block(n.n_tail * kPdLaneRowBytes); tp = block(n.n_tail * 4); tn = block(n.n_tail * 4); ts = block(n.n_tail);
    nc = block(n.n_haps_cross); cc = block(n.n_haps_cross * 32); jf = block(n.n_general);
    pc = block(n.n_placed * 4); pl = block(n.n_placed); cu = block(n.n_chunks_paired);
    fj = block(n.n_general * 4); tg = block(n.n_tab_starts * 4);
    total = end;
  }
};

// The paired table route's scratch in `tabx` (PdArgs::hap_ncls_out, class_codes_out, special_bits, job_notab, the
// predicate launch's job list, job_ns -- the last only for the whole-job asm program).
struct PdTabxLayout {
  size_t nc, cc, sb, nt, hj, ns, total;
  PdTabxLayout(size_t n_hap_items, size_t n_general, size_t entry_stride, bool with_job_ns)
      : nc(0), cc(pd_up(n_hap_items)), sb(cc + pd_up(n_hap_items * 32)), nt(sb + pd_up(n_hap_items * (entry_stride / 64) * 8)),
        hj(nt + pd_up(n_general)), ns(hj + pd_up(n_general * 4)), total(ns + (with_job_ns ? pd_up(n_general * entry_stride * 4) : 0)) {}
};

}  // namespace gklhip

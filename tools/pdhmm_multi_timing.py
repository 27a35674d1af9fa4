#!/usr/bin/env python3
"""K copies of the reference's 276 reads x 48 haplotypes holders fixture as ONE gklhip_pdhmm_compute_cross_multi call against
K consecutive gklhip_pdhmm_compute_cross_batched calls on the same context: median host-to-host time and kernel time
(gklhip_pdhmm_last_kernel_ms; for the consecutive calls: their sum) of each, K in --counts, alternating arm by arm.
Both arms are made on prebuilt arguments: nothing but the C ABI is timed.  Checks that both give the same bytes.

usage: tools/pdhmm_multi_timing.py [--counts 1,2,4,8] [--reps 50] [--warmup 20] [--out FILE]
(nine copies are the most that fit the 131 072-pair limit of a shared launch set: K = 16 would time the region-by-region
fallback against itself, so it is reported as such when asked for)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from gkl_amd import native
    from tools.pdhmm_server_scaling import fixture
    reads, haps = fixture()
    ctx = native.PdhmmContext(device=0)
    lib, h = ctx.lib, ctx.handle
    keep = [np.ascontiguousarray(x, np.int8) for x in (haps.hap_bases, haps.hap_pdbases, reads.read_bases, reads.read_qual,
                                                       reads.read_ins_qual, reads.read_del_qual, reads.gcp)]
    hl, rl = np.ascontiguousarray(haps.hap_lengths, np.int64), np.ascontiguousarray(reads.read_lengths, np.int64)
    cross = native.CPdhmmCross(reads.batch, haps.batch, haps.max_hap_len, reads.max_read_len, *[x.ctypes.data for x in keep],
                               hl.ctypes.data, rl.ctypes.data)
    n = reads.batch * haps.batch
    cells = int(rl.sum()) * int(hl.sum())
    result = {"pairs_per_region": n, "cells_per_region": cells, "reps": a.reps, "rows": []}
    for K in (int(x) for x in a.counts.split(",")):
        crosses = (native.CPdhmmCross * K)(*[cross] * K)
        outs_m = [np.empty(n) for _ in range(K)]
        outs_s = [np.empty(n) for _ in range(K)]
        ptrs = (C.c_void_p * K)(*[o.ctypes.data for o in outs_m])
        status = (C.c_int32 * K)()

        def multi():
            if lib.gklhip_pdhmm_compute_cross_multi(h, K, crosses, None, ptrs, status) != 0:
                raise SystemExit("multi call failed: " + lib.gklhip_pdhmm_last_error().decode())
            return lib.gklhip_pdhmm_last_kernel_ms(h)

        def singles():
            ms = 0.0
            for o in outs_s:
                if lib.gklhip_pdhmm_compute_cross_batched(h, C.byref(cross), C.c_int64(0), o.ctypes.data) != 0:
                    raise SystemExit("single call failed: " + lib.gklhip_pdhmm_last_error().decode())
                ms += lib.gklhip_pdhmm_last_kernel_ms(h)
            return ms

        for _ in range(a.warmup):
            multi()
            singles()
        before = native.pdhmm_combine_counts()
        multi()
        shared = native.pdhmm_combine_counts()[2] - before[2] == 1
        t = {"multi": [], "singles": []}
        k = {"multi": [], "singles": []}
        for _ in range(a.reps):
            for name, fn in (("multi", multi), ("singles", singles)):
                t0 = time.perf_counter()
                kms = fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
                k[name].append(kms)
        same = all(m.tobytes() == s.tobytes() for m, s in zip(outs_m, outs_s))
        row = {"K": K, "one_launch_set": bool(shared), "same_bytes": bool(same)}
        for name in ("multi", "singles"):
            row[name] = {"host_ms_p50": round(float(np.median(t[name])), 4), "host_ms_p10": round(float(np.percentile(t[name], 10)), 4),
                         "host_ms_p90": round(float(np.percentile(t[name], 90)), 4),
                         "kernel_ms_p50": round(float(np.median(k[name])), 4),
                         "tcups_host": round(K * cells / (float(np.median(t[name])) * 1e-3) / 1e12, 4)}
        row["host_speedup"] = round(row["singles"]["host_ms_p50"] / row["multi"]["host_ms_p50"], 3)
        row["kernel_speedup"] = round(row["singles"]["kernel_ms_p50"] / row["multi"]["kernel_ms_p50"], 3)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("the multi call and the single calls differ")
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

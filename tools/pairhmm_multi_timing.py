#!/usr/bin/env python3
"""K distinct seeded `hc` regions of READS x HAPS (--region, default 100 reads x 10 haplotypes) as ONE gklhip_compute_multi
call against K consecutive gklhip_compute calls on the same context: median host-to-host time of each, K in --counts, the
two arms alternating in one process.  Both arms are made on prebuilt arguments: nothing but the C ABI is timed.  Checks that
both give the same bytes and reports how many sets of launches the multi call took (gklhip_small_call_counts: calls,
combined calls, sets).  A mid-size shape (400x40, 250x128, 1000x50) measures the mid-size sets of docs/NOTES.md 69.
--double: the same on a double-precision context (gklhip_config.use_double, GATK's --native-pair-hmm-use-double-precision):
docs/NOTES.md 70; with a mid-size --region: the mid-size fp64 sets of docs/NOTES.md 71.  --read-len LO-HI / --hap-len LO-HI:
the length ranges of the regions' reads and haplotypes (default: make_batch's 50-250 / 100-500); --limit 383|511: the
context's small-read limit (gklhip_set_small_read_limit) -- long-read regions under both limits: docs/NOTES.md 72.
--device: the regions resident in HBM, three arms alternating on one context, host to host: (a) K gklhip_compute_device
calls on one stream and one stream synchronise, (b) one host gklhip_compute_multi of the same regions, (c) one
gklhip_compute_multi_device (left out when the library loaded with --lib has no such symbol); checks that (a) and (c) give
the same bytes and prints the combiner's counts for (c): docs/NOTES.md 78.  --lib FILE: development only -- another build of libgklhip_pairhmm.so (A/B against an earlier commit's, same process layout).

usage: tools/pairhmm_multi_timing.py [--device] [--double] [--region 100x10] [--read-len 384-511] [--hap-len 520-600] [--limit 511]
                                      [--counts 1,2,4,8,16,64] [--reps 30] [--warmup 10] [--lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_row(a, native, ctx, K, batches, cbs, ptrs, cells):
    """One K of --device: the three arms on prebuilt arguments, alternating."""
    import torch
    lib, h = ctx.lib, ctx.handle
    dbs = [native.DeviceBatch.upload(b) for b in batches]
    dcbs = (native.CBatch * K)(*[d.c_batch() for d in dbs])
    outs_a = [torch.empty(b.n_pairs, dtype=torch.float64, device="cuda:0") for b in batches]
    outs_c = [torch.zeros(b.n_pairs, dtype=torch.float64, device="cuda:0") for b in batches]
    dptrs = (C.c_void_p * K)(*[o.data_ptr() for o in outs_c])
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    single_args = [(C.byref(dcbs[k]), outs_a[k].data_ptr()) for k in range(K)]
    have_c = hasattr(lib, "gklhip_compute_multi_device")
    torch.cuda.synchronize()

    def device_singles():
        for cb, out in single_args:
            if lib.gklhip_compute_device(h, cb, out, sp) != 0:
                raise SystemExit("single device call failed: " + lib.gklhip_last_error().decode())
        stream.synchronize()

    def host_multi():
        if lib.gklhip_compute_multi(h, K, cbs, ptrs, None) != 0:
            raise SystemExit("multi call failed: " + lib.gklhip_last_error().decode())

    def device_multi():
        if lib.gklhip_compute_multi_device(h, K, dcbs, dptrs, None, sp) != 0:
            raise SystemExit("device multi call failed: " + lib.gklhip_last_error().decode())

    arms = [("device_singles", device_singles), ("host_multi", host_multi)] + ([("device_multi", device_multi)] if have_c else [])
    for _ in range(a.warmup):
        for _, fn in arms:
            fn()
    counts = None
    if have_c:
        native.small_call_counts(0, reset=True)
        device_multi()
        counts = native.small_call_counts(0)
    t = {name: [] for name, _ in arms}
    for _ in range(a.reps):
        for name, fn in arms:
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    same = not have_c or all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(outs_a, outs_c))
    row = {"K": K, "device_multi_call_counts": list(counts) if counts else None, "same_bytes": bool(same)}
    for name, _ in arms:
        p50 = float(np.median(t[name]))
        row[name] = {"host_ms_p50": round(p50, 4), "host_ms_p10": round(float(np.percentile(t[name], 10)), 4),
                     "host_ms_p90": round(float(np.percentile(t[name], 90)), 4), "gcups_host": round(cells / (p50 * 1e-3) / 1e9, 1)}
    if have_c:
        row["speedup_over_device_singles"] = round(row["device_singles"]["host_ms_p50"] / row["device_multi"]["host_ms_p50"], 3)
        row["speedup_over_host_multi"] = round(row["host_multi"]["host_ms_p50"] / row["device_multi"]["host_ms_p50"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region", default="100x10", help="READSxHAPS of every region")
    ap.add_argument("--counts", default="1,2,4,8,16,64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--double", action="store_true", help="a use_double context")
    ap.add_argument("--lib", default="", help="the libgklhip_pairhmm.so to load (default: the tree's)")
    ap.add_argument("--read-len", default="", help="LO-HI: read lengths (default: make_batch's)")
    ap.add_argument("--hap-len", default="", help="LO-HI: haplotype lengths (default: make_batch's)")
    ap.add_argument("--limit", type=int, default=0, help="383 or 511: the context's small-read limit (default: the library's, not set)")
    ap.add_argument("--device", action="store_true", help="regions resident in HBM: K compute_device calls, the host multi call, the device multi call")
    a = ap.parse_args()
    lens = {}
    for key, val in (("read_len", a.read_len), ("hap_len", a.hap_len)):
        if val:
            try:
                lo, hi = (int(x) for x in val.split("-"))
            except ValueError:
                raise SystemExit(f"--{key.replace('_', '-')} wants LO-HI, e.g. 384-511")
            if not 1 <= lo <= hi:
                raise SystemExit(f"--{key.replace('_', '-')} wants 1 <= LO <= HI")
            lens[key] = (lo, hi)
    if a.reps < 30:
        raise SystemExit("at least 30 repetitions")
    try:
        n_reads, n_haps = (int(x) for x in a.region.lower().split("x"))
    except ValueError:
        raise SystemExit("--region wants READSxHAPS, e.g. 400x40")
    if n_reads < 1 or n_haps < 1:
        raise SystemExit("--region wants at least one read and one haplotype")
    from gkl_amd import native
    from gkl_amd.synth import make_batch
    if a.lib:
        native.LIB_PATH = os.path.abspath(a.lib)   # (before the first load: the counters below come from the same library)
    ctx = native.PairHmmContext(device=0, use_double=a.double, small_read_limit=a.limit or None)
    lib, h = ctx.lib, ctx.handle
    result = {"region": f"hc {n_reads} x {n_haps}", "read_len": a.read_len or "default", "hap_len": a.hap_len or "default", "limit": a.limit or "default",
              "use_double": bool(a.double), "lib": a.lib or "tree", "reps": a.reps, "warmup": a.warmup, "rows": []}
    for K in (int(x) for x in a.counts.split(",")):
        batches = [make_batch("hc", n_reads, n_haps, seed=1000 + k, **lens) for k in range(K)]
        keep, cbs = [], (native.CBatch * K)()
        for k, b in enumerate(batches):
            arrs = [np.ascontiguousarray(x, np.uint8) for x in (b.read_bases, b.read_quals, b.ins_gop, b.del_gop, b.gcp, b.hap_bases)]
            ro, ho = np.ascontiguousarray(b.read_off, np.int64), np.ascontiguousarray(b.hap_off, np.int64)
            keep.append((arrs, ro, ho))
            cbs[k] = native.CBatch(b.n_reads, b.n_haps, ro.ctypes.data_as(native._i64p), ho.ctypes.data_as(native._i64p),
                                   *[x.ctypes.data for x in arrs])
        cells = sum(int(b.read_off[-1]) * int(b.hap_off[-1]) for b in batches)
        outs_m = [np.empty(b.n_pairs) for b in batches]
        outs_s = [np.empty(b.n_pairs) for b in batches]
        ptrs = (C.c_void_p * K)(*[o.ctypes.data for o in outs_m])
        if a.device:
            row = device_row(a, native, ctx, K, batches, cbs, ptrs, cells)
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            if not row["same_bytes"]:
                raise SystemExit("the device multi call and the single device calls differ")
            continue
        single_args = [(C.byref(cbs[k]), outs_s[k].ctypes.data) for k in range(K)]

        def multi():
            if lib.gklhip_compute_multi(h, K, cbs, ptrs, None) != 0:
                raise SystemExit("multi call failed: " + lib.gklhip_last_error().decode())

        def singles():
            for cb, out in single_args:
                if lib.gklhip_compute(h, cb, out) != 0:
                    raise SystemExit("single call failed: " + lib.gklhip_last_error().decode())

        for _ in range(a.warmup):
            multi()
            singles()
        native.small_call_counts(0, reset=True)
        multi()
        counts = native.small_call_counts(0)
        t = {"multi": [], "singles": []}
        for _ in range(a.reps):
            for name, fn in (("multi", multi), ("singles", singles)):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        same = all(m.tobytes() == s.tobytes() for m, s in zip(outs_m, outs_s))
        row = {"K": K, "multi_call_counts": list(counts), "same_bytes": bool(same)}
        for name in ("multi", "singles"):
            p50 = float(np.median(t[name]))
            row[name] = {"host_ms_p50": round(p50, 4), "host_ms_p10": round(float(np.percentile(t[name], 10)), 4),
                         "host_ms_p90": round(float(np.percentile(t[name], 90)), 4), "gcups_host": round(cells / (p50 * 1e-3) / 1e9, 1)}
        row["host_speedup"] = round(row["singles"]["host_ms_p50"] / row["multi"]["host_ms_p50"], 3)
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

#!/usr/bin/env python3
"""Timing of the batch deflate (docs/NOTES.md, "Deflate"): nothing here is a pass/fail bar.

Workload: the payload of tests/golden/HiSeq.1mb.1RG.2k_lines.bam in its own member sizes, repeated to 4096 members
(267 MB of input) -- the counterpart of tools/inflate_timing.py's "fixture" workload.  Measured, p50 / p10 / p90 of
--reps repetitions in one process: the kernel alone (HIP events), the device-resident call host to host, the host call
host to host; the yardstick is Python's zlib at the same level (raw, wbits = -15) over the same members on one thread
and on 16 (zlib releases the GIL).  One 64 KB member alone is timed too: that call is expected to lose to the CPU.
--level N (default 1; 0, 1 and 3 to 8 are built) sets the level of both sides; zlib's higher levels are slow, so
--zlib-reps bounds the repetitions of the yardstick alone.  --lib PATH times another build of libgklhip_deflate.so.

    python tools/deflate_timing.py [--level 1] [--reps 30] [--zlib-reps REPS] [--members 4096] [--lib PATH] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BAM = os.path.join(ROOT, "tests", "golden", "HiSeq.1mb.1RG.2k_lines.bam")


def pcts(ms):
    a = np.sort(np.asarray(ms, float))
    return {"p50": float(np.percentile(a, 50)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def zlib_raw(data, level=1):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def workload(n_members):
    from gkl_amd import native
    image = open(BAM, "rb").read()
    off, plen, _, isize, _ = native.bgzf_scan(image)
    pieces = [zlib.decompress(image[o:o + l], -15) for o, l, n in zip(off, plen, isize) if n > 0]
    return [pieces[k % len(pieces)] for k in range(n_members)]


def measure(ctx, inputs, reps, level=1, zlib_reps=None):
    import torch
    from gkl_amd import native
    n = len(inputs)
    so, do = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.cumsum([len(s) for s in inputs], out=so[1:])
    np.cumsum([native.deflate_bound(len(s)) for s in inputs], out=do[1:])
    src = np.frombuffer(b"".join(inputs), dtype=np.uint8)
    dst = np.zeros(int(do[-1]), np.uint8)
    in_bytes = int(so[-1])
    res = {"workload": "fixture", "members": n, "in_bytes": in_bytes}
    if level != 1:   # level 1's keys are what they were
        res["level"] = level
    zlib_reps = zlib_reps or reps
    # correctness of what is timed, once
    out_len, crc, status = ctx.deflate_batch_raw(src, so, dst, do, level)
    assert not status.any()
    for k in range(0, n, max(1, n // 16)):
        assert zlib.decompress(dst[do[k]:do[k] + out_len[k]].tobytes(), -15) == inputs[k] and int(crc[k]) == zlib.crc32(inputs[k])
    res["out_bytes"] = int(out_len.sum())
    distinct = {id(s): s for s in inputs}
    z = {i: len(zlib_raw(s, level)) for i, s in distinct.items()}
    res[f"zlib_level{level}_out_bytes"] = sum(z[id(s)] for s in inputs)
    res[f"size_over_zlib_level{level}"] = res["out_bytes"] / res[f"zlib_level{level}_out_bytes"]
    d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.zeros(int(do[-1]), dtype=torch.uint8, device="cuda")
    kernel_ms, call_ms = [], []
    for r in range(reps + 2):   # two unrecorded calls first: buffers grow, clocks rise
        t0 = time.perf_counter()
        ctx.deflate_batch_device(d_src, so, d_dst, do, level)
        t1 = time.perf_counter()
        if r >= 2:
            call_ms.append((t1 - t0) * 1e3)
            kernel_ms.append(ctx.last_kernel_ms())
    res["kernel_ms"], res["device_call_ms"] = pcts(kernel_ms), pcts(call_ms)
    ctx.deflate_batch_raw(src, so, dst, do, level)
    res["host_call_ms"] = pcts(timed(lambda: ctx.deflate_batch_raw(src, so, dst, do, level), reps))
    res["zlib_1_thread_ms"] = pcts(timed(lambda: [zlib_raw(s, level) for s in inputs], zlib_reps))
    slices = [inputs[i::16] for i in range(16)]
    with ThreadPoolExecutor(16) as pool:
        res["zlib_16_threads_ms"] = pcts(timed(lambda: list(pool.map(lambda sl: [len(zlib_raw(s, level)) for s in sl], slices)), zlib_reps))
    for key in ("kernel_ms", "device_call_ms", "host_call_ms", "zlib_1_thread_ms", "zlib_16_threads_ms"):
        res[key.replace("_ms", "_GBps_in")] = in_bytes / res[key]["p50"] / 1e6
    return res


def one_member(ctx, data, reps, level=1):
    ctx.deflate_batch([data], level)
    gpu = timed(lambda: ctx.deflate_batch([data], level), reps)
    kernel = ctx.last_kernel_ms()
    cpu = timed(lambda: zlib_raw(data, level), reps)
    return {"workload": "one_64KB_member", "in_bytes": len(data), "host_call_ms": pcts(gpu), "kernel_ms_last": kernel,
            "zlib_1_thread_ms": pcts(cpu), "gpu_over_cpu": pcts(gpu)["p50"] / pcts(cpu)["p50"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--level", type=int, default=1, help="of the batch deflate and of the zlib yardstick")
    ap.add_argument("--zlib-reps", type=int, default=None, help="repetitions of the zlib yardstick (default: --reps)")
    ap.add_argument("--lib", help="another build of libgklhip_deflate.so to time")
    ap.add_argument("--out")
    a = ap.parse_args()
    from gkl_amd import native
    if a.lib:
        native._deflate_lib = native.load_deflate_library(a.lib)
    results = []
    with native.DeflateContext(device=0) as ctx:
        inputs = workload(a.members)
        results.append(measure(ctx, inputs, a.reps, a.level, a.zlib_reps))
        print(json.dumps(results[-1]), flush=True)
        results.append(one_member(ctx, inputs[0], a.reps, a.level))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

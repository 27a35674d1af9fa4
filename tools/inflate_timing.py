#!/usr/bin/env python3
"""Timing of the batch inflate (docs/NOTES.md, "Inflate"): nothing here is a pass/fail bar.

Workloads: the data members of tests/golden/HiSeq.1mb.1RG.2k_lines.bam repeated to 4096 members (about 260 MB of
output), and the same bytes recompressed at levels 1 and 9 in 64 KB members.  Measured per workload, p50 / p10 / p90 of
--reps repetitions in one process: the kernel alone (HIP events), the device-resident call host to host, the host call
host to host; the yardstick is Python's zlib.decompress over the same members on one thread and on 16 (zlib releases
the GIL).  One 64 KB member alone is timed too: that call is expected to lose to the CPU.

    python tools/inflate_timing.py [--reps 30] [--members 4096] [--out FILE.json]
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


def raw_deflate(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def workloads(n_members):
    from gkl_amd import native
    image = open(BAM, "rb").read()
    off, plen, _, isize, _ = native.bgzf_scan(image)
    members = [image[o:o + l] for o, l, n in zip(off, plen, isize) if n > 0]
    plain = b"".join(zlib.decompress(m, -15) for m in members)
    pieces = [plain[i:i + 65536] for i in range(0, len(plain), 65536)]
    sets = {"fixture": members, "level1": [raw_deflate(p, 1) for p in pieces], "level9": [raw_deflate(p, 9) for p in pieces]}
    return {name: [ms[k % len(ms)] for k in range(n_members)] for name, ms in sets.items()}


def measure(ctx, name, streams, reps):
    import torch
    size_of = {}   # the members repeat: one oracle run per distinct member
    for s in streams:
        if id(s) not in size_of:
            size_of[id(s)] = len(zlib.decompress(s, -15))
    sizes = [size_of[id(s)] for s in streams]
    n = len(streams)
    so, do = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=so[1:])
    np.cumsum(sizes, out=do[1:])
    src = np.frombuffer(b"".join(streams), dtype=np.uint8)
    dst = np.zeros(int(do[-1]), np.uint8)
    out_bytes = int(do[-1])
    res = {"workload": name, "members": n, "in_bytes": int(so[-1]), "out_bytes": out_bytes}
    # correctness of what is timed, once
    out_len, _, crc, status = ctx.inflate_batch_raw(src, so, dst, do)
    assert not status.any() and int(out_len.sum()) == out_bytes
    for k in range(0, n, max(1, n // 16)):
        want = zlib.decompress(streams[k], -15)
        assert dst[do[k]:do[k + 1]].tobytes() == want and int(crc[k]) == zlib.crc32(want)
    d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    kernel_ms, call_ms = [], []
    for r in range(reps + 2):   # two unrecorded calls first: buffers grow, clocks rise
        t0 = time.perf_counter()
        ctx.inflate_batch_device(d_src, so, d_dst, do)
        t1 = time.perf_counter()
        if r >= 2:
            call_ms.append((t1 - t0) * 1e3)
            kernel_ms.append(ctx.last_kernel_ms())
    res["kernel_ms"], res["device_call_ms"] = pcts(kernel_ms), pcts(call_ms)
    ctx.inflate_batch_raw(src, so, dst, do)
    res["host_call_ms"] = pcts(timed(lambda: ctx.inflate_batch_raw(src, so, dst, do), reps))
    res["zlib_1_thread_ms"] = pcts(timed(lambda: [zlib.decompress(s, -15) for s in streams], reps))
    slices = [streams[i::16] for i in range(16)]
    with ThreadPoolExecutor(16) as pool:
        res["zlib_16_threads_ms"] = pcts(timed(lambda: list(pool.map(lambda sl: [len(zlib.decompress(s, -15)) for s in sl], slices)), reps))
    for key in ("kernel_ms", "device_call_ms", "host_call_ms", "zlib_1_thread_ms", "zlib_16_threads_ms"):
        res[key.replace("_ms", "_GBps_out")] = out_bytes / res[key]["p50"] / 1e6
    return res


def one_stream(ctx, stream, reps):
    want = zlib.decompress(stream, -15)
    ctx.inflate_batch([stream], [len(want)])
    gpu = timed(lambda: ctx.inflate_batch([stream], [len(want)]), reps)
    kernel = ctx.last_kernel_ms()
    cpu = timed(lambda: zlib.decompress(stream, -15), reps)
    return {"workload": "one_64KB_member", "out_bytes": len(want), "host_call_ms": pcts(gpu), "kernel_ms_last": kernel,
            "zlib_1_thread_ms": pcts(cpu), "gpu_over_cpu": pcts(gpu)["p50"] / pcts(cpu)["p50"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--out")
    a = ap.parse_args()
    from gkl_amd import native
    results = []
    with native.InflateContext(device=0) as ctx:
        sets = workloads(a.members)
        for name, streams in sets.items():
            results.append(measure(ctx, name, streams, a.reps))
            print(json.dumps(results[-1]), flush=True)
        results.append(one_stream(ctx, sets["fixture"][0], a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

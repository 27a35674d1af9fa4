#!/usr/bin/env python3
"""P one-caller processes of PDHMM region calls -- the reference's 276 reads x 48 haplotypes holders fixture
(tests/golden/pdhmm_new.txt) as ONE gklhip_pdhmm_compute_cross_batched call per iteration -- run DIRECTLY (every process
opens the GPU) and THROUGH ONE SERVER (every process a client: GKL_HIP_SERVER; only the server opens the GPU), on
device 0, and THROUGH ONE SERVER THAT COMBINES concurrent calls into shared launches (GKL_HIP_PDHMM_COMBINE=1 in the server's
environment; --combine-min / --combine-wait-us set the leader's hold), the three arms alternating count by count.  Per arm: aggregate TCUPS, calls per second, median, p99 and slowest
call.  Also the per-call cost of one client over one direct caller (the P = 1 rows).

This parent never opens the GPU, and at most 16 processes hold it at once (the server is stopped before the next direct
arm starts).  Every child runs under its own `timeout`; an arm with a child that exits non-zero ends the script.

usage: tools/pdhmm_server_scaling.py [--counts 1,4,8,16] [--seconds 1.5] [--combine-min K] [--combine-wait-us T] [--out FILE]
Prints one JSON line per arm; --out FILE also writes the whole record there."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fixture():
    from gkl_amd.pdhmm_batch import PdhmmBatch
    from tests.golden_io import load_pdhmm_holders_file
    reads, haps, _ = load_pdhmm_holders_file()
    one = b"\0"
    return (PdhmmBatch.from_pairs([(one, one, r[0], r[1], r[2], r[3], r[4]) for r in reads]),
            PdhmmBatch.from_pairs([(h[0], h[1], one, one, one, one, one) for h in haps]))


def child(a):
    """One caller: a context (a client context when GKL_HIP_SERVER is set), warm-up calls, then timed calls for
    --seconds once the go file exists.  The call is made on prebuilt arguments: nothing but the C ABI is timed."""
    from gkl_amd import native
    reads, haps = fixture()
    ctx = native.PdhmmContext()
    keep = [np.ascontiguousarray(x, np.int8) for x in (haps.hap_bases, haps.hap_pdbases, reads.read_bases, reads.read_qual,
                                                       reads.read_ins_qual, reads.read_del_qual, reads.gcp)]
    hl, rl = np.ascontiguousarray(haps.hap_lengths, np.int64), np.ascontiguousarray(reads.read_lengths, np.int64)
    cb = native.CPdhmmCross(reads.batch, haps.batch, haps.max_hap_len, reads.max_read_len, *[x.ctypes.data for x in keep],
                            hl.ctypes.data, rl.ctypes.data)
    out = np.empty(reads.batch * haps.batch)
    fn, h, ref, dst = ctx.lib.gklhip_pdhmm_compute_cross_batched, ctx.handle, C.c_int64(0), out.ctypes.data

    def once():
        if fn(h, C.byref(cb), ref, dst) != 0:
            raise SystemExit("call failed: " + ctx.lib.gklhip_pdhmm_last_error().decode())
    for _ in range(30):
        once()
    first = out.copy()
    open(a.out + ".ready", "w").close()
    t_end = time.monotonic() + 120
    while not os.path.exists(a.go):
        if time.monotonic() > t_end:
            raise SystemExit("no go file")
        time.sleep(0.001)
    ms = []
    t0 = time.perf_counter()
    t = t0
    while t - t0 < a.seconds:
        once()
        t1 = time.perf_counter()
        ms.append((t1 - t) * 1e3)
        t = t1
    rec = {"remote": ctx.is_remote, "ms": ms, "t0": t0, "t1": t, "same": bool(out.tobytes() == first.tobytes()),
           "cells": int(rl.sum()) * int(hl.sum())}
    ctx.close()
    with open(a.out + ".json", "w") as f:
        json.dump(rec, f)


def run_arm(n, seconds, env, tmp, tag):
    go = os.path.join(tmp, f"{tag}.go")
    outs = [os.path.join(tmp, f"{tag}_{i}") for i in range(n)]
    limit = str(int(seconds + 180))
    procs = [subprocess.Popen(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child", "--seconds",
                               str(seconds), "--go", go, "--out", o], env=env) for o in outs]
    t_end = time.monotonic() + 170
    while not all(os.path.exists(o + ".ready") for o in outs):
        if any(p.poll() is not None for p in procs) or time.monotonic() > t_end:
            break
        time.sleep(0.01)
    open(go, "w").close()
    codes = [p.wait() for p in procs]
    if any(codes):
        raise SystemExit(f"{tag}: a child exited with {codes}")
    recs = [json.load(open(o + ".json")) for o in outs]
    ms = np.concatenate([np.asarray(r["ms"]) for r in recs])
    wall = max(r["t1"] for r in recs) - min(r["t0"] for r in recs)   # (perf_counter: one clock for all processes)
    assert all(r["same"] for r in recs)
    return {"processes": n, "remote": all(r["remote"] for r in recs), "calls": int(ms.size), "calls_per_s": round(ms.size / wall, 1),
            "aggregate_tcups": round(float(ms.size) * recs[0]["cells"] / wall / 1e12, 4), "p50_ms": round(float(np.median(ms)), 4),
            "p99_ms": round(float(np.percentile(ms, 99)), 4), "max_ms": round(float(ms.max()), 4),
            "calls_over_5ms": int((ms > 5).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,4,8,16")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--combine-min", type=int, default=1)
    ap.add_argument("--combine-wait-us", type=int, default=0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--go", default="")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    from gkl_amd import server
    counts = tuple(int(x) for x in a.counts.split(","))
    if max(counts) > 16:
        raise SystemExit("at most 16 processes may hold the GPU at once")
    env = dict(os.environ)
    env.pop("GKL_HIP_SERVER", None)
    for k in [k for k in env if k.startswith("GKL_HIP_PDHMM_COMBINE")]:
        del env[k]
    combine_env = dict(env, GKL_HIP_PDHMM_COMBINE="1", GKL_HIP_PDHMM_COMBINE_MIN=str(a.combine_min),
                       GKL_HIP_PDHMM_COMBINE_WAIT_US=str(a.combine_wait_us))
    tmp = tempfile.mkdtemp(prefix="gklpdsrv")
    result = {"counts": counts, "seconds": a.seconds, "direct": {}, "server": {}, "server_combined": {},
              "combine_min": a.combine_min, "combine_wait_us": a.combine_wait_us}
    for n in counts:
        result["direct"][n] = run_arm(n, a.seconds, env, tmp, f"direct{n}")
        print(json.dumps({"direct": result["direct"][n]}), flush=True)
        sock = os.path.join(tmp, f"s{n}.sock")
        h = server.start(sock, env=env, timeout=120)
        try:
            result["server"][n] = run_arm(n, a.seconds, dict(env, GKL_HIP_SERVER=sock), tmp, f"server{n}")
            result["server"][n]["server_calls"] = h.pdhmm_stats()["calls_served"]
            arenas = h.stats()
            result["server"][n]["arenas"] = {k: arenas[k] for k in ("arenas_registered", "arenas_copied")}
        finally:
            if h.stop() != 0:
                raise SystemExit("the server did not stop cleanly")
        print(json.dumps({"server": result["server"][n]}), flush=True)
        sock = os.path.join(tmp, f"sc{n}.sock")
        h = server.start(sock, env=combine_env, timeout=120)
        try:
            result["server_combined"][n] = run_arm(n, a.seconds, dict(env, GKL_HIP_SERVER=sock), tmp, f"combined{n}")
            st = h.pdhmm_stats()
            result["server_combined"][n]["server_calls"] = st["calls_served"]
            result["server_combined"][n]["combine_counts"] = list(st["combine_counts"])   # calls, calls that shared a launch set, launch sets
        finally:
            if h.stop() != 0:
                raise SystemExit("the server did not stop cleanly")
        print(json.dumps({"server_combined": result["server_combined"][n]}), flush=True)
    if 1 in counts:
        d, s = result["direct"][1]["p50_ms"], result["server"][1]["p50_ms"]
        result["single_client_per_call_us"] = {"direct_p50_ms": d, "server_p50_ms": s, "overhead_us": round((s - d) * 1e3, 1)}
        print(json.dumps(result["single_client_per_call_us"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

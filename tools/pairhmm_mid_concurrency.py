#!/usr/bin/env python3
"""T threads, each with a context and a pinned batch of its own, calling gklhip_compute on an `hc` region of READS x HAPS
back to back (prebuilt arguments: nothing but the C ABI is timed): aggregate calls/s and TCUPS, the per-call p50 / p10 /
p90 over all threads, and the combiner's three counters (gklhip_small_call_counts: calls, combined calls, sets of
launches) -- for the mid-size switch of docs/NOTES.md 75 (gklhip_set_mid_combine / GKL_HIP_COMBINE_MID), which lets the
mid-size calls (2049 - 65 536 pairs) of concurrent callers share sets of launches.  One process is one arm: --mid 0|1 sets
the switch on every context (a library without the setter, e.g. an earlier commit's loaded with --lib, only runs --mid
0).  --mixed: T/2 threads of 100 x 10 regions beside T/2 of the --regions' first one; the small calls' p50 / p99 and the
mid-size calls' p50 are reported apart (what kMidFlights is for).  --server P1,P2: P one-caller client processes of the
first region through ONE PairHMM server, started here with or without GKL_HIP_COMBINE_MID=1 by --mid (this process and
the clients never open the GPU).  --double: use_double contexts.  --lib FILE: development
only -- another build of libgklhip_pairhmm.so (A/B against an earlier commit's, same process layout).

usage: tools/pairhmm_mid_concurrency.py [--mid 0|1] [--double] [--regions 400x40,250x128,1000x50] [--threads 1,4,8,16]
                                         [--calls 300] [--warmup 20] [--mixed] [--server 4,16] [--lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def client(a):
    """One client process of the server on a.client: its calls' latencies as one JSON line."""
    from gkl_amd import native
    from gkl_amd.synth import make_batch
    n_reads, n_haps = (int(x) for x in a.regions.split(",")[0].lower().split("x"))
    b = make_batch("hc", n_reads, n_haps, seed=a.seed)
    out = np.empty(b.n_pairs)
    with native.PairHmmContext(server=a.client, use_double=a.double) as ctx:
        for _ in range(a.warmup):
            ctx.compute(b, out)
        while not os.path.exists(a.go):
            time.sleep(0.001)
        lat = np.zeros(a.calls)
        t_begin = time.time()
        for i in range(a.calls):
            t0 = time.perf_counter()
            ctx.compute(b, out)
            lat[i] = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"begin": t_begin, "end": time.time(), "lat": [round(float(x), 4) for x in lat], "remote": ctx.is_remote,
                          "cells": int(b.read_off[-1]) * int(b.hap_off[-1])}), flush=True)


def through_the_server(a, result):
    from gkl_amd import server
    me = os.path.abspath(__file__)
    for P in (int(x) for x in a.server.split(",")):
        with tempfile.TemporaryDirectory() as d:
            env = dict(os.environ)
            env.pop("GKL_HIP_COMBINE_MID", None)
            if a.mid:
                env["GKL_HIP_COMBINE_MID"] = "1"
            h = server.start(os.path.join(d, "s.sock"), env=env, timeout=120)
            try:
                go = os.path.join(d, "go")
                cmd = [sys.executable, me, "--client", h.socket_path, "--go", go, "--regions", a.regions, "--calls", str(a.calls), "--warmup", str(a.warmup)]
                procs = [subprocess.Popen(cmd + ["--seed", str(1000 + k)] + (["--double"] if a.double else []), stdout=subprocess.PIPE, text=True)
                         for k in range(P)]
                t_end = time.monotonic() + 120
                while h.stats()["live_connections"] < P and time.monotonic() < t_end and all(p.poll() is None for p in procs):
                    time.sleep(0.01)
                time.sleep(0.5)   # (the warm-up calls)
                open(go, "w").close()
                recs = [json.loads(p.communicate(timeout=300)[0].strip().splitlines()[-1]) for p in procs]
                counts = h.stats()["small_call_counts"][0]
            finally:
                h.stop()
        lat = np.concatenate([r["lat"] for r in recs])
        dt = max(r["end"] for r in recs) - min(r["begin"] for r in recs)
        row = {"region": "hc " + a.regions.split(",")[0].replace("x", " x "), "clients": P, "calls_per_s": round(P * a.calls / dt, 1),
               "tcups": round(sum(r["cells"] for r in recs) * a.calls / dt / 1e12, 4), "counts_with_warmup": list(counts),
               "ms": {"p50": round(float(np.percentile(lat, 50)), 4), "p10": round(float(np.percentile(lat, 10)), 4),
                      "p90": round(float(np.percentile(lat, 90)), 4), "p99": round(float(np.percentile(lat, 99)), 4)}}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", type=int, default=0, help="the mid-size switch of every context")
    ap.add_argument("--double", action="store_true", help="use_double contexts")
    ap.add_argument("--regions", default="400x40,250x128,1000x50", help="READSxHAPS, comma-separated")
    ap.add_argument("--threads", default="1,4,8,16")
    ap.add_argument("--calls", type=int, default=300, help="timed calls per thread")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mixed", action="store_true", help="half the threads call 100 x 10 regions")
    ap.add_argument("--lib", default="", help="the libgklhip_pairhmm.so to load (default: the tree's)")
    ap.add_argument("--out", default="")
    ap.add_argument("--server", default="", help="P1,P2: client processes through one server instead of threads")
    ap.add_argument("--client", default="", help=argparse.SUPPRESS)   # (a client process of --server: the socket)
    ap.add_argument("--go", default="", help=argparse.SUPPRESS)
    ap.add_argument("--seed", type=int, default=1000, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.client:
        return client(a)
    from gkl_amd import native
    from gkl_amd.synth import make_batch
    if a.lib:
        native.LIB_PATH = os.path.abspath(a.lib)   # (before the first load: the counters below come from the same library)
    lib = native.load_library()
    if a.mid and not hasattr(lib, "gklhip_set_mid_combine"):
        raise SystemExit("this library has no gklhip_set_mid_combine: --mid 0 only")
    shapes = []
    for item in a.regions.split(","):
        try:
            r, h = (int(x) for x in item.lower().split("x"))
        except ValueError:
            raise SystemExit("--regions wants READSxHAPS, e.g. 400x40")
        shapes.append((r, h))
    result = {"lib": a.lib or "tree", "mid": a.mid, "use_double": bool(a.double), "mixed": bool(a.mixed), "calls": a.calls, "warmup": a.warmup, "rows": []}
    if a.server:
        through_the_server(a, result)
        shapes = []
    for n_reads, n_haps in (shapes[:1] if a.mixed else shapes):
        for T in (int(x) for x in a.threads.split(",")):
            # thread k's region: its own seed; --mixed: the even threads call 100 x 10 regions
            small = [a.mixed and k % 2 == 0 for k in range(T)]
            batches = [make_batch("hc", 100 if small[k] else n_reads, 10 if small[k] else n_haps, seed=1000 + k) for k in range(T)]
            ctxs = [native.PairHmmContext(device=0, use_double=a.double) for _ in range(T)]
            if hasattr(lib, "gklhip_set_mid_combine"):
                for c in ctxs:
                    c.set_mid_combine(bool(a.mid))
            pins = [native.PinnedBatch(b) for b in batches]
            outs = [np.empty(b.n_pairs) for b in batches]
            keep, args = [], []
            for k, p in enumerate(pins):
                pb = p.batch
                ro, ho = np.ascontiguousarray(pb.read_off, np.int64), np.ascontiguousarray(pb.hap_off, np.int64)
                cb = native.CBatch(pb.n_reads, pb.n_haps, ro.ctypes.data_as(native._i64p), ho.ctypes.data_as(native._i64p),
                                   *[x.ctypes.data for x in (pb.read_bases, pb.read_quals, pb.ins_gop, pb.del_gop, pb.gcp, pb.hap_bases)])
                keep.append((ro, ho, cb))
                args.append((ctxs[k].handle, C.byref(cb), outs[k].ctypes.data))
            lat = [np.zeros(a.calls) for _ in range(T)]
            failed = []
            start = threading.Barrier(T + 1)

            def work(k):
                h, cb, out = args[k]
                for _ in range(a.warmup):
                    if lib.gklhip_compute(h, cb, out) != 0:
                        failed.append(lib.gklhip_last_error().decode())
                start.wait()
                start.wait()   # (the counters are reset between the two)
                for i in range(a.calls):
                    t0 = time.perf_counter()
                    if lib.gklhip_compute(h, cb, out) != 0:
                        failed.append(lib.gklhip_last_error().decode())
                    lat[k][i] = (time.perf_counter() - t0) * 1e3

            th = [threading.Thread(target=work, args=(k,)) for k in range(T)]
            for t in th:
                t.start()
            start.wait()
            native.small_call_counts(0, reset=True)
            start.wait()
            t0 = time.perf_counter()
            for t in th:
                t.join()
            dt = time.perf_counter() - t0
            counts = native.small_call_counts(0)
            if failed:
                raise SystemExit("a call failed: " + failed[0])
            cells = sum(int(b.read_off[-1]) * int(b.hap_off[-1]) for b in batches) * a.calls

            def pct(x, q):
                return round(float(np.percentile(x, q)), 4)

            row = {"region": f"hc {n_reads} x {n_haps}", "threads": T, "calls_per_s": round(T * a.calls / dt, 1), "tcups": round(cells / dt / 1e12, 4),
                   "counts": list(counts)}
            groups = {"ms": list(range(T))} if not a.mixed else {"small_ms": [k for k in range(T) if small[k]], "mid_ms": [k for k in range(T) if not small[k]]}
            for name, ks in groups.items():
                if ks:
                    x = np.concatenate([lat[k] for k in ks])
                    row[name] = {"p50": pct(x, 50), "p10": pct(x, 10), "p90": pct(x, 90), "p99": pct(x, 99)}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            for c, p in zip(ctxs, pins):
                p.close()
                c.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""P one-caller processes of 100 x 10 PairHMM regions (bench.process_records), run DIRECTLY (every process opens the GPU)
and THROUGH ONE PairHMM SERVER (every process a client: GKL_HIP_SERVER; only the server opens the GPU), on device 0.
Also: one client's round trip against one direct caller (the P = 1 rows), and the eight-busy-plus-one-idle scenario of
tools/idle_parent.py with every process a client -- this parent, a client, once sends big batches and then stays idle
while eight clients loop.  This parent never opens the GPU.

usage: tools/server_scaling.py [--counts 1,4,8,16] [--seconds 1.5] [--out FILE]
Prints one JSON line per run; --out FILE also writes the whole record there."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gkl_amd import native, server  # noqa: E402
from gkl_amd.synth import make_batch  # noqa: E402

KEYS = ("aggregate_gcups", "calls_per_s", "p50_ms", "p99_ms", "max_ms", "calls_over_5ms", "first_call_after_idle_ms")


def summary(rec):
    return {k: {x: v[x] for x in KEYS} for k, v in rec.items() if isinstance(v, dict)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,4,8,16")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    counts = tuple(int(x) for x in a.counts.split(","))
    os.environ.pop("GKL_HIP_SERVER", None)
    result = {"counts": counts, "seconds": a.seconds}

    direct = bench.process_records(0, "hc", counts=counts, duration_s=a.seconds)
    result["direct"] = summary(direct)
    print(json.dumps({"direct": result["direct"]}), flush=True)

    sock = os.path.join(tempfile.mkdtemp(prefix="gklsrv"), "pairhmm.sock")
    h = server.start(sock, timeout=120)
    try:
        os.environ["GKL_HIP_SERVER"] = sock          # the children of process_records become clients
        via = bench.process_records(0, "hc", counts=counts, duration_s=a.seconds)
        result["server"] = summary(via)
        st = h.stats()
        result["server_stats"] = {k: st[k] for k in ("calls_served", "arenas_registered", "arenas_copied", "small_call_counts")}
        print(json.dumps({"server": result["server"], "server_stats": result["server_stats"]}), flush=True)
        if 1 in counts:
            d, s = direct["processes_1"]["p50_ms"], via["processes_1"]["p50_ms"]
            result["single_client_round_trip_us"] = {"direct_p50_ms": d, "server_p50_ms": s, "overhead_us": round((s - d) * 1e3, 1)}
            print(json.dumps(result["single_client_round_trip_us"]), flush=True)

        # 8 + 1: this process (a client) has run big batches through two contexts and then idles, as in tools/idle_parent.py
        big = make_batch("hc", 3200, 128)
        out = np.empty(big.n_pairs)
        ctxs = [native.PairHmmContext(server=sock) for _ in range(2)]
        for c in ctxs:
            for _ in range(3):
                c.compute(big, out)
        idle = bench.process_records(0, "hc", counts=(8,), duration_s=a.seconds)
        result["eight_plus_idle_client"] = summary(idle)
        result["eight_plus_idle_client"]["longest_child_s"] = idle["processes_8"]["longest_child_s"]
        print(json.dumps({"eight_plus_idle_client": result["eight_plus_idle_client"]}), flush=True)
        for c in ctxs:
            c.close()
    finally:
        os.environ.pop("GKL_HIP_SERVER", None)
        h.stop()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""PDHMM host calls against device-resident calls (gklhip_pdhmm_compute_device / _cross_device), one machine, one
session, one context per library: the x32 fixture as paired pairs (423 936 padded pairs, 498 MB of input), the x32 fixture
as a cross call (8832 reads x 48 haplotypes) and one 276 x 48 region.  p50 / p10 / p90 of --reps calls after --warmup
calls, host to host (the device-resident call is synchronous), plus last_kernel_ms of the last call.

--parent-lib PATH: a libgklhip_pdhmm.so built from the parent commit; its HOST calls are timed in the same session on
the same three problems (it has no device-resident calls), and the tool says whether this tree's p50 lies inside the
parent's own p10-p90 band (the criterion of docs/NOTES.md 73).

usage: tools/pdhmm_device_timing.py [--reps 30] [--warmup 5] [--parent-lib PATH] [--json OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gkl_amd import native  # noqa: E402
from gkl_amd.pdhmm_batch import PdhmmBatch  # noqa: E402
from tests.golden_io import load_pdhmm_holders_file  # noqa: E402

DEV = "cuda:0"


def problems(fixture_x=32):
    """(name, kind, payload) of the three problems, built as bench.py builds them."""
    reads, haps, _ = load_pdhmm_holders_file()
    one = b"\0"
    r1 = PdhmmBatch.from_pairs([(one, one, r[0], r[1], r[2], r[3], r[4]) for r in reads])
    hb = PdhmmBatch.from_pairs([(h[0], h[1], one, one, one, one, one) for h in haps])
    rx = r1.subset(np.tile(np.arange(r1.batch), fixture_x))
    ri, hi = np.repeat(np.arange(r1.batch), hb.batch), np.tile(np.arange(hb.batch), r1.batch)
    hsub, rsub = hb.subset(hi), r1.subset(ri)
    p1 = PdhmmBatch(rsub.batch, hb.max_hap_len, r1.max_read_len, hsub.hap_bases, hsub.hap_pdbases, rsub.read_bases, rsub.read_qual,
                    rsub.read_ins_qual, rsub.read_del_qual, rsub.gcp, hsub.hap_lengths, rsub.read_lengths)
    px = p1.subset(np.tile(np.arange(p1.batch), fixture_x))
    return [(f"paired x{fixture_x} ({px.batch} pairs)", "paired", px), (f"cross x{fixture_x} ({rx.batch} x {hb.batch})", "cross", (rx, hb)),
            (f"region {r1.batch} x {hb.batch}", "cross", (r1, hb))]


def timed(call, kernel_ms, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"p50": round(float(np.percentile(ts, 50)), 4), "p10": round(float(np.percentile(ts, 10)), 4),
            "p90": round(float(np.percentile(ts, 90)), 4), "last_kernel_ms": round(kernel_ms(), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    rows = []
    ctx = native.PdhmmContext(device=0, fma_mode=1)
    parent = native.PdhmmContext(device=0, fma_mode=1, lib_path=a.parent_lib) if a.parent_lib else None
    for name, kind, payload in problems():
        row = {"problem": name}
        if kind == "paired":
            host = lambda c: (lambda: c.compute(payload))  # noqa: E731
            db = native.PdhmmDeviceBatch.upload(payload, DEV)
            out = torch.empty(payload.batch, dtype=torch.float64, device=DEV)
            device = lambda: ctx.compute_device(db, out=out)  # noqa: E731
        else:
            reads, haps = payload
            host = lambda c: (lambda: c.compute_cross(reads, haps))  # noqa: E731
            rdb, hdb = native.PdhmmDeviceBatch.upload_cross(reads, haps, DEV)
            out = torch.empty(reads.batch * haps.batch, dtype=torch.float64, device=DEV)
            device = lambda: ctx.compute_cross_device(rdb, hdb, out=out)  # noqa: E731
        torch.cuda.synchronize()
        # interleaved: parent's host call, this tree's host call, this tree's device-resident call
        if parent is not None:
            row["parent_host"] = timed(host(parent), parent.last_kernel_ms, a.reps, a.warmup)
        row["host"] = timed(host(ctx), ctx.last_kernel_ms, a.reps, a.warmup)
        row["device"] = timed(device, ctx.last_kernel_ms, a.reps, a.warmup)
        # sanity: the device-resident result is the host call's to the last bits
        ref, got = host(ctx)(), out.cpu().numpy()
        row["max_abs_diff_vs_host"] = float(np.max(np.abs(got - ref)))
        if parent is not None:
            p = row["parent_host"]
            row["host_p50_inside_parent_band"] = bool(p["p10"] <= row["host"]["p50"] <= p["p90"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        db = rdb = hdb = out = None   # free the HBM copies before the next problem
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()
    if parent is not None:
        parent.close()


if __name__ == "__main__":
    main()

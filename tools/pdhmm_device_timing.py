#!/usr/bin/env python3
"""PDHMM host calls against device-resident calls (gklhip_pdhmm_compute_device / _cross_device), one machine, one
session, one context per library: the x32 fixture as paired pairs (423 936 padded pairs, 498 MB of input), the x32 fixture
as a cross call (8832 reads x 48 haplotypes) and one 276 x 48 region.  p50 / p10 / p90 of --reps calls after --warmup
calls, host to host (the device-resident call is synchronous), plus last_kernel_ms of the last call.

--parent-lib PATH: a libgklhip_pdhmm.so built from the parent commit; its HOST calls are timed in the same session on
the same three problems (it has no device-resident calls), and the tool says whether this tree's p50 lies inside the
parent's own p10-p90 band (the criterion of docs/NOTES.md 73).

--multi: the multi arm instead.  K = 1, 2, 4, 8, 16 copies of the 276 x 48 region, every copy with its own arrays in HBM, as
(a) K single gklhip_pdhmm_compute_cross_device calls, (b) one host gklhip_pdhmm_compute_cross_multi call, (c) one
gklhip_pdhmm_compute_cross_multi_device call: the same percentiles, the kernel times (a: summed over the K calls) and
the ratios c / a and c / b of the p50s.  With --parent-lib: the parent's (a) and (b) in the same session, and whether this
tree's p50 of each lies inside, below or above the parent's p10-p90 band.

usage: tools/pdhmm_device_timing.py [--reps 30] [--warmup 5] [--parent-lib PATH] [--multi] [--json OUT]"""
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


MULTI_K = (1, 2, 4, 8, 16)


def multi_rows(a, ctx, parent):
    """The multi arm: K copies of the 276 x 48 region, each with its own arrays in HBM, as (a) K single device-resident
    calls, (b) one host multi call, (c) one device-resident multi call; with a parent library, its (a) and (b) too."""
    import torch
    _, _, (reads, haps) = problems()[2]
    n = reads.batch * haps.batch
    for K in MULTI_K:
        regions = [(reads, haps)] * K
        dbs = [native.PdhmmDeviceBatch.upload_cross(reads, haps, DEV) for _ in range(K)]
        outs = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(K)]
        torch.cuda.synchronize()
        kernel_ms = [0.0]

        def singles(c):
            def call():
                kernel_ms[0] = 0.0
                for k in range(K):
                    c.compute_cross_device(*dbs[k], out=outs[k])
                    kernel_ms[0] += c.last_kernel_ms()
            return call

        row = {"problem": f"{K} x region {reads.batch} x {haps.batch}", "K": K}
        if parent is not None:
            row["parent_a_single_device_calls"] = timed(singles(parent), lambda: kernel_ms[0], a.reps, a.warmup)
        row["a_single_device_calls"] = timed(singles(ctx), lambda: kernel_ms[0], a.reps, a.warmup)
        want = [o.cpu().numpy().tobytes() for o in outs]
        if parent is not None:
            row["parent_b_host_multi"] = timed(lambda: parent.compute_cross_multi(regions), parent.last_kernel_ms, a.reps, a.warmup)
        row["b_host_multi"] = timed(lambda: ctx.compute_cross_multi(regions), ctx.last_kernel_ms, a.reps, a.warmup)
        for o in outs:
            o.zero_()
        row["c_multi_device"] = timed(lambda: ctx.compute_cross_multi_device(dbs, outs=outs), ctx.last_kernel_ms, a.reps, a.warmup)
        row["c_bytes_equal_a"] = bool([o.cpu().numpy().tobytes() for o in outs] == want)
        row["c_over_a_p50"] = round(row["c_multi_device"]["p50"] / row["a_single_device_calls"]["p50"], 4)
        row["c_over_b_p50"] = round(row["c_multi_device"]["p50"] / row["b_host_multi"]["p50"], 4)
        if parent is not None:
            for arm in ("a_single_device_calls", "b_host_multi"):
                p = row["parent_" + arm]
                p50 = row[arm]["p50"]
                row[arm + "_p50_vs_parent_band"] = "below" if p50 < p["p10"] else "above" if p50 > p["p90"] else "inside"
        yield row
        dbs = outs = None
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--multi", action="store_true", help="only the multi arm: K regions as single device calls, host multi, device multi")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    rows = []
    ctx = native.PdhmmContext(device=0, fma_mode=1)
    parent = native.PdhmmContext(device=0, fma_mode=1, lib_path=a.parent_lib) if a.parent_lib else None
    if a.multi:
        for row in multi_rows(a, ctx, parent):
            rows.append(row)
            print(json.dumps(row), flush=True)
    for name, kind, payload in ([] if a.multi else problems()):
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

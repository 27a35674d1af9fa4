"""Child process of tests/test_pairhmm_small_long_reads.py: one gklhip_compute_multi call of the named pool regions on a
plain fp32 context -- no setter --, under whatever process-wide knobs the parent put into the environment
(GKL_HIP_SMALL_READ_LIMIT and GKL_HIP_COMBINE are read once per process).  Writes the outputs (OUT.npz) and the combiner's
counters and the call's statistics (OUT.json).

usage: python -m tests.pairhmm_small_long_reads_child --out PREFIX --names a,b,c [--fma 1]"""
import argparse
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--names", required=True)
    ap.add_argument("--fma", type=int, default=1)
    a = ap.parse_args()
    from gkl_amd import native
    from tests.test_pairhmm_small_long_reads import build_pool
    pool = build_pool()
    names = a.names.split(",")
    with native.PairHmmContext(fma_mode=a.fma) as ctx:
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([pool[n] for n in names])
        counts = native.small_call_counts(0)
        st = ctx.stats()
    np.savez(a.out + ".npz", **{f"out{k}": o for k, o in enumerate(got)})
    with open(a.out + ".json", "w") as f:
        json.dump({"counts": list(counts), "n_pairs": int(st["n_pairs"]), "n_fallback": int(st["n_fallback"])}, f)


if __name__ == "__main__":
    main()

"""Child process of tests/test_pdhmm_combine_gpu.py:

    python -m tests.pd_combine_child --out PREFIX --shapes 61:41,20:7,... --seed S

One thread per shape, each with a PDHMM context of its own; behind a barrier every thread makes ONE cross call of its
region (tests.pd_server_client.region(seed + i, shape)).  Whether the calls are combined is the environment's business
(GKL_HIP_PDHMM_COMBINE*).  Writes the outputs to PREFIX.npz (out0, out1, ...) and, to PREFIX.json, the process's
gklhip_pdhmm_combine_counts after the calls and each thread's routing.
"""
import argparse
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.pd_server_client import region  # noqa: E402
from tests.server_client import write_json  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--shapes", required=True)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    from gkl_amd import native
    shapes = [tuple(map(int, s.split(":"))) for s in a.shapes.split(",")]
    n = len(shapes)
    ctxs = [native.PdhmmContext(device=0) for _ in range(n)]
    regions = [region(a.seed + i, *shapes[i]) for i in range(n)]
    outs, routing, errors = [None] * n, [None] * n, [None] * n
    barrier = threading.Barrier(n)

    def work(i):
        try:
            barrier.wait(60)
            outs[i] = ctxs[i].compute_cross(*regions[i])
            routing[i] = ctxs[i].last_routing()
        except Exception as e:  # noqa: BLE001  (reported to the parent)
            errors[i] = repr(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    counts = native.pdhmm_combine_counts()
    for c in ctxs:
        c.close()
    if all(o is not None for o in outs):
        np.savez(a.out + ".npz", **{f"out{i}": o for i, o in enumerate(outs)})
    write_json(a.out, {"counts": list(counts), "routing": routing, "errors": errors})


if __name__ == "__main__":
    main()

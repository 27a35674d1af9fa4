"""A client process of the PairHMM server, for tests/test_server_cpu.py and tests/test_server_gpu.py:

    python -m tests.server_client MODE --socket PATH --out PREFIX [options]

MODE random: `--calls` calls of random shapes (seeded), each checked here against what the stub C ABI computes
(tests/mockjni.py: stub_expected) -- CPU suite.  MODE batches: the synth batches of `--spec` (kind:n_reads:n_haps:seed,
comma-separated) with `--double` / `--fma`; the doubles go to PREFIX.npz for the parent to compare.  MODE loop: the same
small call over and over until killed (PREFIX.json appears after the first one).  MODE jni: computeLikelihoodsNative of
the first `--spec` batch through the mock JVM and libgkl_pairhmm.so (GKL_HIP_SERVER comes from the environment).

Every mode writes PREFIX.json: what it did, and the targets of its open file descriptors (/proc/self/fd) -- a client
must never have opened the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def open_files():
    out = []
    for fd in os.listdir("/proc/self/fd"):
        try:
            out.append(os.readlink(os.path.join("/proc/self/fd", fd)))
        except OSError:
            pass
    return out


def batches_of(spec):
    from gkl_amd.synth import make_batch
    out = []
    for item in spec.split(","):
        kind, n_reads, n_haps, seed = item.split(":")
        out.append(make_batch(kind, int(n_reads), int(n_haps), seed=int(seed)))
    return out


def wait_for(path, timeout=60.0):
    t_end = time.monotonic() + timeout
    while path and not os.path.exists(path):
        if time.monotonic() > t_end:
            raise TimeoutError(path)
        time.sleep(0.002)


def write_json(prefix, rec):
    rec["open_files"] = open_files()
    with open(prefix + ".json.tmp", "w") as f:
        json.dump(rec, f)
    os.replace(prefix + ".json.tmp", prefix + ".json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["random", "batches", "loop", "jni"])
    ap.add_argument("--socket", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--spec", default="hc:100:10:1")
    ap.add_argument("--double", type=int, default=0)
    ap.add_argument("--fma", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--go", default="", help="wait until this file exists before the timed / concurrent calls")
    a = ap.parse_args()

    if a.mode == "jni":
        from tests import mockjni
        b = batches_of(a.spec)[0]
        rc, out, cls, msg, _ = mockjni.run(b, use_double=bool(a.double), max_threads=1)
        np.savez(a.out + ".npz", out0=out)
        write_json(a.out, {"rc": rc, "exception": cls, "message": msg})
        return

    from gkl_amd import native
    ctx = native.PairHmmContext(server=a.socket, use_double=bool(a.double), fma_mode=a.fma, max_threads=1)
    rec = {"remote": ctx.is_remote}
    if a.mode == "random":
        from gkl_amd.synth import random_batch
        from tests.mockjni import stub_expected
        rng = np.random.RandomState(a.seed)
        wait_for(a.go)
        good = bad = 0
        for _ in range(a.calls):
            b = random_batch(rng, int(rng.randint(1, 80)), int(rng.randint(1, 16)), read_len=(1, 300), hap_len=(1, 400))
            if np.array_equal(ctx.compute(b), stub_expected(b)):
                good += 1
            else:
                bad += 1
        rec.update(good=good, bad=bad)
    elif a.mode == "batches":
        bs = batches_of(a.spec)
        ctx.compute(bs[0])   # (arena)
        wait_for(a.go)
        outs = {}
        for i, b in enumerate(bs):
            for k in range(a.repeat):
                o = ctx.compute(b)
                if k == 0:
                    outs[f"out{i}"] = o.copy()
                elif o.tobytes() != outs[f"out{i}"].tobytes():
                    rec["unstable"] = i
        np.savez(a.out + ".npz", **outs)
        rec["stats"] = {k: float(v) for k, v in ctx.stats().items()}
    else:  # loop
        b = batches_of(a.spec)[0]
        ctx.compute(b)
        write_json(a.out, rec)
        while True:
            ctx.compute(b)
    ctx.close()
    write_json(a.out, rec)


if __name__ == "__main__":
    main()

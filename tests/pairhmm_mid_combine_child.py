"""Child process of tests/test_pairhmm_mid_combine.py, under the process-wide knobs the parent put into the environment
(GKL_HIP_COMBINE_MID, GKL_HIP_COMBINE_MIN, GKL_HIP_COMBINE_WAIT_US: read once per process).

MODE threads: the threads of --plan (a JSON list; per thread {"pool": "f32" | "f64", "double": 0 | 1, "fma": 0 | 1,
"names": [...], "rot": k}) each make a context of their own and, round by round behind a barrier, call gklhip_compute on
their regions -- `names` rotated by `rot`.  A name with colons is a synth batch kind:n_reads:n_haps:seed, any other a region
of the named pool (build_pool of tests/test_pairhmm_multi_mid.py / tests/test_pairhmm_double_mid.py).  Every output of
every round is compared with the thread's first one for that region; the first ones go to OUT.npz as t<thread>_<position
in names> for the parent to compare with the oracle.  OUT.json: the combiner's counts over all rounds, the calls made, and
which (thread, region) ever changed its bytes.

MODE jni: mockjni.run_concurrent of the --spec batch through libgkl_pairhmm.so; OUT.npz: out0; OUT.json: rc, the
exception, and that library's own small-call counts.

usage: python -m tests.pairhmm_mid_combine_child threads --out PREFIX --plan JSON [--rounds 20]
       python -m tests.pairhmm_mid_combine_child jni --out PREFIX --spec hc:560:30:7 --threads 8 --iters 10 [--double 1]"""
import argparse
import ctypes as C
import json
import threading

import numpy as np


def region(pools, pool, name):
    if ":" in name:
        from gkl_amd.synth import make_batch
        kind, n_reads, n_haps, seed = name.split(":")
        return make_batch(kind, int(n_reads), int(n_haps), seed=int(seed))
    if pool not in pools:
        if pool == "f32":
            from tests.test_pairhmm_multi_mid import build_pool
        else:
            from tests.test_pairhmm_double_mid import build_pool
        pools[pool] = build_pool()
    return pools[pool][name]


def run_threads(a):
    from gkl_amd import native
    plan = json.loads(a.plan)
    pools = {}
    batches = [[region(pools, t["pool"], n) for n in t["names"]] for t in plan]
    ctxs = [native.PairHmmContext(use_double=bool(t["double"]), fma_mode=int(t["fma"])) for t in plan]
    barrier = threading.Barrier(len(plan))
    first = [[None] * len(t["names"]) for t in plan]
    changed, errors = [], []
    calls = [0] * len(plan)

    def work(i):
        try:
            n = len(batches[i])
            for r in range(a.rounds):
                barrier.wait(timeout=120)
                for j in range(n):
                    k = (j + plan[i]["rot"]) % n
                    out = ctxs[i].compute(batches[i][k])
                    calls[i] += 1
                    if first[i][k] is None:
                        first[i][k] = out
                    elif out.tobytes() != first[i][k].tobytes():
                        changed.append((i, plan[i]["names"][k], r))
        except Exception as e:  # noqa: BLE001  (reported to the parent; the other threads' barrier breaks)
            errors.append(f"thread {i}: {type(e).__name__}: {e}")
            barrier.abort()

    native.small_call_counts(0, reset=True)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(plan))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    counts = native.small_call_counts(0)
    for c in ctxs:
        c.close()
    np.savez(a.out + ".npz", **{f"t{i}_{k}": o for i, outs in enumerate(first) for k, o in enumerate(outs) if o is not None})
    with open(a.out + ".json", "w") as f:
        json.dump({"counts": list(counts), "calls": sum(calls), "changed": changed, "errors": errors}, f)
    return 1 if errors else 0


def run_jni(a):
    from gkl_amd.synth import make_batch
    from tests import mockjni
    kind, n_reads, n_haps, seed = a.spec.split(":")
    b = make_batch(kind, int(n_reads), int(n_haps), seed=int(seed))
    try:
        import torch  # noqa: F401  (HIP runtime load order, as mockjni.run_concurrent)
    except ImportError:
        pass
    lib = C.CDLL(mockjni.JNI_LIB)   # (held from before the mock JVM loads it: the same handle, and the combiner its calls go through)
    rc, out, cls, msg, _ = mockjni.run_concurrent(b, n_threads=a.threads, iters=a.iters, use_double=bool(a.double))
    k = (C.c_int64 * 3)()
    lib.gklhip_small_call_counts.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int]
    assert lib.gklhip_small_call_counts(0, k, 0) == 0
    np.savez(a.out + ".npz", out0=out)
    with open(a.out + ".json", "w") as f:
        json.dump({"rc": int(rc), "exception": cls, "message": msg, "counts": [int(x) for x in k]}, f)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["threads", "jni"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--plan", default="[]")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--spec", default="hc:560:30:7")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--double", type=int, default=0)
    a = ap.parse_args()
    return run_threads(a) if a.mode == "threads" else run_jni(a)


if __name__ == "__main__":
    raise SystemExit(main())

"""A PDHMM client process of the server, for tests/test_pdhmm_server_cpu.py and tests/test_pdhmm_server_gpu.py:

    python -m tests.pd_server_client MODE --socket PATH --out PREFIX [options]

MODE random: `--calls` calls of random shapes, layouts and modes (seeded), each checked here against what the stub PDHMM
library computes (tests/test_pdhmm_server_cpu.py: stub_pd_expected) -- CPU suite.  MODE loop: the same small call over
and over until killed (PREFIX.json appears after the first one).  MODE once: GKL_HIP_SERVER comes from the environment;
init, one checked call, done.  MODE region: `--calls` times the reads x haplotypes product of `--shape` (seeded) as
one cross call each; the first result goes to PREFIX.npz, a later one that differs is reported.  MODE jniload: what
System.load does to libgkl_pdhmm.so (dlopen, JNI_OnLoad; GKL_HIP_SERVER from the environment), and with `--run 1`
computePDHMMNative and computeLikelihoodsNative of the seeded batches through the mock JVM, results to PREFIX.npz.

Every mode writes PREFIX.json: what it did, and the targets of its open file descriptors (/proc/self/fd) -- a client
must never have opened the GPU.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.server_client import wait_for, write_json  # noqa: E402

JNI_VERSION_1_8 = 0x00010008


def region(seed, n_reads, n_haps):
    """The reads and the haplotypes of one region-sized call (both as PdhmmBatch-like halves).  Read bases are A, C, G
    and T only: in the default reference-tail mode any other read base under a SNP column is an input error, as in GKL,
    when its pair falls into a batch's scalar tail."""
    from tests.test_pdhmm import random_pd_batch
    rng = np.random.RandomState(seed)
    reads = random_pd_batch(rng, n_reads, read_len=(30, 151), hap_len=(1, 2), with_n=False, lower=False)
    haps = random_pd_batch(rng, n_haps, read_len=(1, 2), hap_len=(100, 260), flag_rate=0.05, with_n=False, lower=False)
    return reads, haps


def random_stub_call(rng):
    """(reads, haps, cross, fma_mode, tail_mode, ref_batch_pairs) of random shape for the stub library."""
    from tests.test_pdhmm import random_pd_batch
    cross = bool(rng.randint(0, 2))
    if cross:
        reads = random_pd_batch(rng, int(rng.randint(1, 30)), read_len=(1, 120), hap_len=(1, 2))
        haps = random_pd_batch(rng, int(rng.randint(1, 9)), read_len=(1, 2), hap_len=(1, 160))
    else:
        reads = haps = random_pd_batch(rng, int(rng.randint(1, 60)), read_len=(1, 120), hap_len=(1, 160))
    return reads, haps, cross, int(rng.randint(0, 2)), int(rng.randint(0, 2)), int(rng.randint(0, 50)) if cross else 0


def stub_call(ctx, reads, haps, cross, fma, tail, ref_batch_pairs):
    ctx.lib.gklhip_pdhmm_set_fma_mode(ctx.handle, fma)
    ctx.lib.gklhip_pdhmm_set_tail_mode(ctx.handle, tail)
    return ctx.compute_cross(reads, haps, ref_batch_pairs) if cross else ctx.compute(reads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["random", "loop", "once", "region", "jniload"])
    ap.add_argument("--socket", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shape", default="61:41")
    ap.add_argument("--run", type=int, default=0)
    ap.add_argument("--go", default="", help="wait until this file exists before the concurrent calls")
    a = ap.parse_args()

    if a.mode == "jniload":
        from tests import mockjni
        lib = C.CDLL(mockjni.PD_JNI_LIB)
        lib.JNI_OnLoad.argtypes = [C.c_void_p, C.c_void_p]
        lib.JNI_OnLoad.restype = C.c_int
        rec = {"onload": int(lib.JNI_OnLoad(None, None))}
        if a.run and rec["onload"] == JNI_VERSION_1_8:
            from tests.golden_io import load_pdhmm_file
            flat, _ = load_pdhmm_file("pdhmm_syn_199_68_51.txt")
            reads, haps = region(a.seed, *map(int, a.shape.split(":")))
            rc0, out0, cls0, msg0 = mockjni.run_pdhmm(flat)
            rc1, out1, cls1, msg1 = mockjni.run_pdhmm(None, holders=(reads, haps))
            np.savez(a.out + ".npz", flat=out0, holders=out1)
            rec.update(rc=[rc0, rc1], exception=[cls0, cls1], message=[msg0, msg1])
        write_json(a.out, rec)
        return

    from gkl_amd import native
    if a.mode == "once":
        assert os.environ.get("GKL_HIP_SERVER") == a.socket
        ctx = native.PdhmmContext()          # (gklhip_pdhmm_init: client mode comes from the environment)
    else:
        ctx = native.PdhmmContext(server=a.socket)
    rec = {"remote": ctx.is_remote}
    if a.mode in ("random", "once"):
        from tests.test_pdhmm_server_cpu import stub_pd_expected
        rng = np.random.RandomState(a.seed)
        wait_for(a.go)
        good = bad = 0
        for _ in range(1 if a.mode == "once" else a.calls):
            call = random_stub_call(rng)
            if np.array_equal(stub_call(ctx, *call), stub_pd_expected(*call)):
                good += 1
            else:
                bad += 1
        rec.update(good=good, bad=bad)
    elif a.mode == "region":
        reads, haps = region(a.seed, *map(int, a.shape.split(":")))
        first = ctx.compute_cross(reads, haps)   # (arena)
        wait_for(a.go)
        for k in range(a.calls):
            if ctx.compute_cross(reads, haps).tobytes() != first.tobytes():
                rec["unstable"] = k
        np.savez(a.out + ".npz", out=first)
    else:  # loop
        call = random_stub_call(np.random.RandomState(a.seed))
        stub_call(ctx, *call)
        write_json(a.out, rec)
        while True:
            stub_call(ctx, *call)
    ctx.close()
    write_json(a.out, rec)


if __name__ == "__main__":
    main()

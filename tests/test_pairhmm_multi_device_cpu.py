"""What gklhip_compute_multi_device (include/gkl_hip_pairhmm.h) promises without a GPU: every product library that
exports gklhip_compute_multi exports it, and a client context of the PairHMM server -- here the stub server of
tests/test_server_cpu.py -- refuses device-resident regions before anything else."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

from gkl_amd import native
from gkl_amd.synth import random_batch
from tests.test_server_cpu import sockdir, srv, stub_exe  # noqa: F401  (fixtures: the stub server)


def exported(path):
    listed = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in listed.splitlines() if line.split()[-2:-1] == ["T"]}


def test_every_library_with_the_multi_call_exports_the_device_form():
    libs = sorted(glob.glob(os.path.join(native.LIB_DIR, "*.so")))
    with_multi = [p for p in libs if "gklhip_compute_multi" in exported(p)]
    names = {os.path.basename(p) for p in with_multi}
    assert {"libgklhip_pairhmm.so", "libgklhip_pairhmm_cxxfast.so", "libgkl_pairhmm.so"} <= names
    for p in with_multi:
        assert "gklhip_compute_multi_device" in exported(p), p
    lib = native.load_library()
    assert lib.gklhip_compute_multi_device.restype is C.c_int and len(lib.gklhip_compute_multi_device.argtypes) == 6


def test_client_context_refuses_device_resident_regions(srv):  # noqa: F811
    rng = np.random.RandomState(5)
    regions = [random_batch(rng, 6, 3), random_batch(rng, 2, 2)]
    keep, cbs = [], (native.CBatch * 2)()
    for k, b in enumerate(regions):
        arrs = [np.ascontiguousarray(a, np.uint8) for a in (b.read_bases, b.read_quals, b.ins_gop, b.del_gop, b.gcp, b.hap_bases)]
        ro, ho = np.ascontiguousarray(b.read_off, np.int64), np.ascontiguousarray(b.hap_off, np.int64)
        keep.append((arrs, ro, ho))
        # host arrays stand in for device pointers: never read
        cbs[k] = native.CBatch(b.n_reads, b.n_haps, ro.ctypes.data_as(C.POINTER(C.c_int64)), ho.ctypes.data_as(C.POINTER(C.c_int64)), *[a.ctypes.data for a in arrs])
    outs = [np.full(b.n_pairs, 7.0) for b in regions]
    out_ptrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    status = (C.c_int32 * 2)(-5, -5)
    with native.PairHmmContext(server=srv.socket_path) as c:
        assert c.is_remote
        served = srv.stats()["calls_served"]
        st = c.lib.gklhip_compute_multi_device(c.handle, 2, cbs, out_ptrs, status, None)
        assert st == native.ERR_UNSUPPORTED and b"gklhip_compute_multi_device" in c.lib.gklhip_last_error()
        # before anything else: arguments that every other check refuses still answer "unsupported"
        assert c.lib.gklhip_compute_multi_device(c.handle, 0, None, None, None, None) == native.ERR_UNSUPPORTED
        assert c.lib.gklhip_compute_multi_device(c.handle, -1, cbs, None, None, None) == native.ERR_UNSUPPORTED
        assert b"gklhip_compute_multi_device" in c.lib.gklhip_last_error()
        assert srv.stats()["calls_served"] == served
        assert all(np.all(o == 7.0) for o in outs) and list(status) == [-5, -5]
        c.compute(regions[0])   # the context goes on: a host call reaches the server
        assert srv.stats()["calls_served"] == served + 1

"""What the device-resident PDHMM calls (gklhip_pdhmm_compute_device / _cross_device / _finalise_host,
include/gkl_hip_pdhmm.h) promise without a GPU: the host finalisation is libm's log10, a client context of the server
refuses device-resident batches before anything else, and both product builds export the symbols."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from gkl_amd import native
from tests.test_pdhmm import random_pd_batch
from tests.test_pdhmm_server_cpu import sockdir, srv, stub_exe, stub_pd_lib  # noqa: F401  (fixtures: the stub server)

LIB_DIR = os.path.dirname(native.PDHMM_LIB_PATH)
NEW_SYMBOLS = ("gklhip_pdhmm_compute_device", "gklhip_pdhmm_compute_cross_device", "gklhip_pdhmm_finalise_host")


def test_finalise_host_is_the_host_libms_log10():
    rng = np.random.RandomState(76)
    # 0, the smallest subnormal, 1, the scale itself, and 1000 positives spread over 600 decades
    x = np.concatenate([[0.0, 5e-324, 1.0, 2.0 ** 1020], 10.0 ** rng.uniform(-300.0, 300.0, 1000) * rng.uniform(1.0, 10.0, 1000)])
    assert x[1] > 0.0 and x[1] < np.finfo(np.float64).tiny and np.all(x[4:] > 0.0) and np.all(np.isfinite(x))
    got = native.pdhmm_finalise_host(x)
    scale = math.log10(2.0 ** 1020)
    exp = np.array([(-math.inf if v == 0.0 else math.log10(v)) - scale for v in x.tolist()], np.float64)   # CPython: the same libm
    assert got[0] == -math.inf
    assert got[3] == 0.0
    assert got.tobytes() == exp.tobytes()
    assert native.pdhmm_finalise_host(np.empty(0)).size == 0


def test_finalise_host_takes_a_cpu_tensor():
    torch = pytest.importorskip("torch")
    x = np.array([1.0, 3.5e200, 2.0 ** 1000])
    assert native.pdhmm_finalise_host(torch.from_numpy(x)).tobytes() == native.pdhmm_finalise_host(x).tobytes()


def test_client_context_refuses_device_resident_calls(srv):  # noqa: F811
    b = random_pd_batch(np.random.RandomState(3), 6)
    keep = [np.ascontiguousarray(a, np.int8) for a in (b.hap_bases, b.hap_pdbases, b.read_bases, b.read_qual, b.read_ins_qual,
                                                       b.read_del_qual, b.gcp)]
    hl, rl = np.ascontiguousarray(b.hap_lengths, np.int64), np.ascontiguousarray(b.read_lengths, np.int64)
    ptrs = [a.ctypes.data for a in keep] + [hl.ctypes.data, rl.ctypes.data]   # host arrays stand in for device pointers: never read
    out, sums = np.full(b.batch * b.batch, 7.0), np.full(b.batch * b.batch, 7.0)
    with native.PdhmmContext(server=srv.socket_path) as c:
        assert c.is_remote
        served = srv.pdhmm_stats()["calls_served"]
        paired = native.CPdhmmBatch(b.batch, b.max_hap_len, b.max_read_len, *ptrs)
        st = c.lib.gklhip_pdhmm_compute_device(c.handle, C.byref(paired), out.ctypes.data, sums.ctypes.data, None)
        assert st == native.ERR_UNSUPPORTED and b"gklhip_pdhmm_compute_device" in c.lib.gklhip_pdhmm_last_error()
        cross = native.CPdhmmCross(b.batch, b.batch, b.max_hap_len, b.max_read_len, *ptrs)
        st = c.lib.gklhip_pdhmm_compute_cross_device(c.handle, C.byref(cross), 0, out.ctypes.data, None, None)
        assert st == native.ERR_UNSUPPORTED and b"gklhip_pdhmm_compute_cross_device" in c.lib.gklhip_pdhmm_last_error()
        # before anything else: arguments that every other check refuses still answer "unsupported"
        assert c.lib.gklhip_pdhmm_compute_device(c.handle, None, None, None, None) == native.ERR_UNSUPPORTED
        assert c.lib.gklhip_pdhmm_compute_cross_device(c.handle, None, -1, None, None, None) == native.ERR_UNSUPPORTED
        assert srv.pdhmm_stats()["calls_served"] == served
        assert np.all(out == 7.0) and np.all(sums == 7.0)
        c.compute(b)   # the context goes on: a host call reaches the server
        assert srv.pdhmm_stats()["calls_served"] == served + 1


@pytest.mark.parametrize("name", ["libgklhip_pdhmm.so", "libgklhip_pdhmm_cxx.so"])
def test_both_builds_export_the_new_symbols(name):
    listed = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, name)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listed.splitlines() if line.split()[-2:-1] == ["T"]}
    assert set(NEW_SYMBOLS) <= exported
    lib = native.load_pdhmm_library(os.path.join(LIB_DIR, name))
    assert lib.gklhip_pdhmm_finalise_host.argtypes is not None and lib.gklhip_pdhmm_compute_device.restype is C.c_int

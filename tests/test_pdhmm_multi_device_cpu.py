"""What the device-resident multi-region PDHMM call (gklhip_pdhmm_compute_cross_multi_device, include/gkl_hip_pdhmm.h)
promises without a GPU: a client context of the server refuses it before anything else, and both product builds export
the symbol.  (The stub server of tests/test_pdhmm_server_cpu.py, as in tests/test_pdhmm_device_cpu.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gkl_amd import native
from tests.test_pdhmm import random_pd_batch
from tests.test_pdhmm_server_cpu import sockdir, srv, stub_exe, stub_pd_lib  # noqa: F401  (fixtures: the stub server)

LIB_DIR = os.path.dirname(native.PDHMM_LIB_PATH)
SYMBOL = "gklhip_pdhmm_compute_cross_multi_device"


def test_client_context_refuses_the_multi_device_call(srv):  # noqa: F811
    b = random_pd_batch(np.random.RandomState(3), 6)
    keep = [np.ascontiguousarray(a, np.int8) for a in (b.hap_bases, b.hap_pdbases, b.read_bases, b.read_qual, b.read_ins_qual,
                                                       b.read_del_qual, b.gcp)]
    hl, rl = np.ascontiguousarray(b.hap_lengths, np.int64), np.ascontiguousarray(b.read_lengths, np.int64)
    ptrs = [a.ctypes.data for a in keep] + [hl.ctypes.data, rl.ctypes.data]   # host arrays stand in for device pointers: never read
    out, sums = np.full(b.batch * b.batch, 7.0), np.full(b.batch * b.batch, 7.0)
    crosses = (native.CPdhmmCross * 2)(*[native.CPdhmmCross(b.batch, b.batch, b.max_hap_len, b.max_read_len, *ptrs)] * 2)
    outs, sums_ptrs = (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data), (C.c_void_p * 2)(sums.ctypes.data, None)
    status = (C.c_int32 * 2)(-1, -1)
    with native.PdhmmContext(server=srv.socket_path) as c:
        assert c.is_remote
        served = srv.pdhmm_stats()["calls_served"]
        st = c.lib.gklhip_pdhmm_compute_cross_multi_device(c.handle, 2, crosses, None, outs, sums_ptrs, status, None)
        assert st == native.ERR_UNSUPPORTED
        text = c.lib.gklhip_pdhmm_last_error().decode()
        assert text.startswith(SYMBOL + ": ") and "client context" in text
        # before anything else: arguments that every other check refuses still answer "unsupported"
        assert c.lib.gklhip_pdhmm_compute_cross_multi_device(c.handle, 0, None, None, None, None, None, None) == native.ERR_UNSUPPORTED
        assert srv.pdhmm_stats()["calls_served"] == served
        assert np.all(out == 7.0) and np.all(sums == 7.0) and list(status) == [-1, -1]
        # the host multi call of the same context goes to the server, region by region
        got = c.compute_cross_multi([(b, b), (b, b)])
        assert len(got) == 2 and srv.pdhmm_stats()["calls_served"] == served + 2


@pytest.mark.parametrize("name", ["libgklhip_pdhmm.so", "libgklhip_pdhmm_cxx.so"])
def test_both_builds_export_the_symbol(name):
    listed = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB_DIR, name)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in listed.splitlines() if line.split()[-2:-1] == ["T"]}
    assert SYMBOL in exported
    lib = native.load_pdhmm_library(os.path.join(LIB_DIR, name))
    assert lib.gklhip_pdhmm_compute_cross_multi_device.restype is C.c_int

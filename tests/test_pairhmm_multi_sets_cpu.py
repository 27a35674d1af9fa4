"""The sets of a multi-region PairHMM call (gkl_amd/csrc/pairhmm_multi_sets.h: the set-cutting rule, the block prefix sums
and the block -> (region, local block) lookup that the host and the *_multi_kernel families share), checked on the host:
tests/native/pairhmm_multi_sets_check.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers, cuts 300 random region lists into sets and maps every block of every launch there and back.  And the new
C-ABI entry points' argument checks, which need no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairhmm_multi_sets_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_multi_sets.h")


def test_set_cutting_and_block_lookup_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pairhmm_multi_sets_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 300 region lists"), r.stdout


def test_multi_entry_points_exist_and_check_their_arguments():
    from gkl_amd import native
    lib = native.load_library()
    assert hasattr(lib, "gklhip_compute_multi") and hasattr(lib, "gklhip_get_raw_region")

    def err():
        return (lib.gklhip_last_error() or b"").decode()

    regions = (native.CBatch * 1)()
    outs = (C.c_void_p * 1)()
    status = (C.c_int32 * 1)(7)
    assert lib.gklhip_compute_multi(None, 1, regions, outs, status) == native.ERR_INVALID_ARG
    assert "context is NULL" in err()
    # (the remaining checks come before the context is looked at: any non-NULL pointer stands in for one)
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    for n in (0, -3):
        assert lib.gklhip_compute_multi(ctx, n, regions, outs, status) == native.ERR_INVALID_ARG
        assert err() == "no regions to process"
    assert lib.gklhip_compute_multi(ctx, 1, None, outs, status) == native.ERR_INVALID_ARG
    assert err() == "regions / out_host is NULL"
    assert lib.gklhip_compute_multi(ctx, 1, regions, None, status) == native.ERR_INVALID_ARG
    assert err() == "regions / out_host is NULL"
    assert status[0] == 7   # a refused call writes no status
    assert lib.gklhip_get_raw_region(None, 0, None, None, None) == native.ERR_INVALID_ARG
    assert "context is NULL" in err()

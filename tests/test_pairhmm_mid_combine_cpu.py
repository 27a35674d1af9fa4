"""The mid-size switch of the small-call combiner (gklhip_set_mid_combine / GKL_HIP_COMBINE_MID), as far as it can be
checked without a device.  The rule by which a leader of concurrent callers picks its set -- gkl_amd/csrc/
pairhmm_multi_sets.h: CombinePick, kCombineMidPairs, kMidFlights -- runs in tests/native/pairhmm_mid_combine_check.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers.  And the setter's argument checks: a NULL
context, and a client context of the (stub) PairHMM server.  (At the parent of this change the symbol does not exist.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairhmm_mid_combine_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_multi_sets.h")


def test_the_pick_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pairhmm_mid_combine_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 400 queues"), r.stdout


def test_the_setter_exists_and_refuses_a_null_context():
    from gkl_amd import native
    lib = native.load_library()
    assert hasattr(lib, "gklhip_set_mid_combine")
    for on in (0, 1):
        assert lib.gklhip_set_mid_combine(None, on) == native.ERR_INVALID_ARG
        assert "context is NULL" in (lib.gklhip_last_error() or b"").decode()


def test_a_client_context_cannot_set_it(tmp_path):
    """The server's contexts follow the server process's environment; the client is told so."""
    from gkl_amd import native
    from gkl_amd.errors import RuntimeException
    from tests.test_server_cpu import build_stub_server, start_stub
    h = start_stub(build_stub_server(str(tmp_path / "gklhip_server_stub")), tmp_path / "s.sock")
    try:
        with native.PairHmmContext(server=h.socket_path) as c:
            assert c.is_remote
            for on in (True, False):
                with pytest.raises(RuntimeException, match="unsupported") as e:
                    c.set_mid_combine(on)
                assert "GKL_HIP_COMBINE_MID" in str(e.value)
            assert c.lib.gklhip_set_mid_combine(c.handle, 1) == native.ERR_UNSUPPORTED
    finally:
        assert h.stop() == 0

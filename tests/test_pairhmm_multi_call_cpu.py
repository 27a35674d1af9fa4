"""The decisions of one multi-region PairHMM call (gkl_amd/csrc/pairhmm_multi_call.h: which regions are staged on which
lane and when, which sets run in which order, what becomes of a region that fails or finds no set), checked on the host:
tests/native/pairhmm_multi_call_check.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers, runs the driver over fake operations that record every call and fail where they are told to -- the failure
paths that no GPU test can reach."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairhmm_multi_call_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_multi_call.h")


def test_multi_call_driver_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pairhmm_multi_call_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout
    lists, held, failed = (int(r.stdout.split(" " + word)[0].split()[-1]) for word in ("region lists", "held plans", "failed"))
    assert lists >= 400 and held > 0 and failed > 0, r.stdout

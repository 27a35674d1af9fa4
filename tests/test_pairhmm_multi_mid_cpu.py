"""The mid-size sets of a multi-region PairHMM call, checked on the host (gkl_amd/csrc/pairhmm_multi_sets.h: the two-kind
cut -- small regions with multi_cut_sets, mid-size regions among themselves with multi_cut_mid_sets -- and the grids of a
mid-size region's two policy launches): tests/native/pairhmm_multi_mid_check.cpp, a stand-alone program built with the
address and undefined-behaviour sanitizers, cuts 300 random region lists and walks every list of flagged pairs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairhmm_multi_mid_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_multi_sets.h")


def test_two_kind_cut_and_list_walk_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pairhmm_multi_mid_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 300 region lists"), r.stdout

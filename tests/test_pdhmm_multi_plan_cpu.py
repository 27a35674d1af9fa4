"""The region table of the multi-region PDHMM launches (gkl_amd/csrc/pdhmm_multi_plan.h) and its index mappings, checked
on the host: tests/native/pdhmm_multi_plan_check.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers, maps every unit of every launch and every pair of a few hundred random region sets there and back."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pdhmm_multi_plan_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pdhmm_multi_plan.h")


def test_region_table_and_index_mappings_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pdhmm_multi_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 300 region sets"), r.stdout

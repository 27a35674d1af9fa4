"""The descriptor table of the device-resident multi-region PDHMM call's input gather (gkl_amd/csrc/pdhmm_gather_plan.h),
checked on the host: tests/native/pdhmm_gather_plan_check.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers, builds the table for a few hundred random region sets, executes it over exact-size buffers
with the index functions the kernel uses, and compares with the host form's staging loop."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pdhmm_gather_plan_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pdhmm_gather_plan.h")


def test_gather_descriptors_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pdhmm_gather_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 300 region sets"), r.stdout
    rows, units, tail = (int(r.stdout.split(", ")[i].split()[0]) for i in (1, 2, 3))
    assert rows > 0 and units > 0 and tail > 0   # both copy forms were exercised

"""The row tiers and launch forms of the one-pair-per-wavefront PairHMM kernels, checked on the host
(gkl_amd/csrc/pairhmm_pair_forms.h: rows per lane by read length, the kernel form of each family for a single call and
for a set, the occupancy rules, the run-time to compile-time dispatcher): tests/native/pairhmm_pair_forms_check.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers, holds the table of forms written out and
walks every read length of 1 to 511 bases and every set of member tiers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairhmm_pair_forms_check.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_pair_forms.h")


def test_tiers_forms_and_dispatch_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    assert os.path.exists(HEADER)
    exe = str(tmp_path / "pairhmm_pair_forms_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 32 table entries, 511 read lengths, 320 sets"), r.stdout

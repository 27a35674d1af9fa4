"""The PDHMM call planner (gkl_amd/csrc/pdhmm_call_plan.h: packing, striped and tail jobs, haplotype routing, table groups,
slices, the multi-region plan and the host side of table staging), checked on the host:
tests/native/pdhmm_call_plan_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers,
re-derives every plan naively for a few hundred regions and region sets, in both arithmetic modes and both tail modes,
and fills the job tables into blocks of exactly the layouts' sizes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pdhmm_call_plan_check.cpp")
PLAN_SRC = os.path.join(ROOT, "gkl_amd", "csrc", "pairhmm_plan.cpp")
HEADER = os.path.join(ROOT, "gkl_amd", "csrc", "pdhmm_call_plan.h")


def test_planner_header_is_free_of_the_device_runtime():
    text = open(HEADER).read()
    assert "gklhip_pdhmm_ctx" not in text
    # no HIP name and no HIP header; the project's own namespace is the one word that contains the letters
    assert "hip" not in text.replace("namespace gklhip", "")
    assert "g_err" not in text and "fail(" not in text


def test_call_plans_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    exe = str(tmp_path / "pdhmm_call_plan_check")
    # no ROCm include path: the header and pairhmm_plan.cpp are plain C++
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC, PLAN_SRC], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout
    seen = {name: int(n) for n, name in re.findall(r"(\d+) ([a-z ]+?)(?:,|\n|$)", r.stdout[4:])}
    assert seen["multi sets"] == 300, r.stdout
    # every kind of case was exercised: a generator that stops producing one fails here
    for name in ("regions", "striped reads", "table haplotypes", "odd haplotypes", "tail jobs", "striped tails", "sliced plans",
                 "paired plans", "shared unions", "kept lists", "groups of several"):
        assert seen[name] > 0, (name, r.stdout)

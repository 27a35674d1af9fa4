#!/usr/bin/env python3
"""Writes tests/golden/deflate_parent_digests.json: per setting of tests/deflate_inputs.SETTINGS (levels 0 and 1) one
SHA-256 over the (status, length, stream) records that the one-lane host build of gkl_amd/csrc/deflate_core.h gives on
tests/deflate_inputs.INPUTS.  It was run on the commit before levels 3-8 were added, so the file pins the bytes of
levels 0 and 1; tests/test_deflate_levels_cpu.py recomputes the digests with `digests()` below.  Run it again only when
a change means to move those bytes.
    python3 tests/golden/make_deflate_parent_digests.py"""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import deflate_inputs as di  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "deflate_core_check.cpp")
OUT = os.path.join(ROOT, "tests", "golden", "deflate_parent_digests.json")


def digest(results) -> str:
    h = hashlib.sha256()
    for status, stream, _ in results:
        h.update(struct.pack("<ii", status, len(stream)) + stream)
    return h.hexdigest()


def digests(exe, tmp) -> dict:
    datas = [d for _, d in di.INPUTS]
    inputs = os.path.join(tmp, "digest_inputs.bin")
    results = os.path.join(tmp, "digest_results.bin")
    with open(inputs, "wb") as f:
        f.write(di.input_file(datas, [di.roomy(len(d)) for d in datas]))
    out = {}
    for name, level, strategy, types in di.SETTINGS:
        subprocess.run([exe, "run", inputs, results, str(level), str(strategy), str(types), "1"], check=True, capture_output=True, timeout=600)
        with open(results, "rb") as f:
            out[name] = digest(di.parse_results(f.read(), len(datas)))
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "deflate_core_check")
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O2", "-pthread", "-o", exe, SRC], check=True, timeout=300)
        d = digests(exe, tmp)
    with open(OUT, "w") as f:
        json.dump({"inputs": len(di.INPUTS), "sha256": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(d, indent=1))


if __name__ == "__main__":
    main()

"""The decoder core of the batch inflate (gkl_amd/csrc/inflate_core.h, the one copy of the deflate decoding logic, which
the GPU kernel instantiates for a wavefront) checked on the host: tests/native/inflate_core_check.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers, runs the whole case list of tests/deflate_cases.py
through the same core for one thread, every source and output in a heap block of exactly its size.  Also: the BGZF
member walk (gkl_amd/csrc/bgzf_scan.h, gklhip_bgzf_scan) and the argument checks of the IntelInflater mirror."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from tests import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "inflate_core_check.cpp")
CORE = os.path.join(ROOT, "gkl_amd", "csrc", "inflate_core.h")
BAM = os.path.join(ROOT, "tests", "golden", "HiSeq.1mb.1RG.2k_lines.bam")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    exe = str(tmp_path_factory.mktemp("inflate_core") / "inflate_core_check")
    # no ROCm include path: the core and the member walk are plain C++
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-o", exe, SRC], check=True, timeout=300)
    return exe


def test_core_is_free_of_the_device_runtime():
    text = open(CORE).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "__device__" not in code and "threadIdx" not in code and "__shared__" not in code
    assert "#include <stdint.h>" in text and code.count("#include") == 1


def test_case_list_covers_every_family_and_status():
    assert set(dc.FAMILIES) == {"stored", "fixed", "match", "dynamic", "zlib", "capacity", "truncation", "mutation"}
    assert {c.status for c in dc.CASES} == set(range(6))
    assert sum(c.family == "mutation" for c in dc.CASES) == 300
    assert all(len(c.output) <= c.capacity for c in dc.CASES)


def test_whole_case_list_under_sanitizers(check_exe, tmp_path):
    cases = dc.CASES + dc.CRC_CASES
    (tmp_path / "cases.bin").write_bytes(dc.case_file(cases))
    r = subprocess.run([check_exe, "run", str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"ok: {len(cases)} streams"), r.stdout
    results = dc.parse_results((tmp_path / "results.bin").read_bytes(), len(cases))
    bad = [m for m in (dc.mismatch(c, *res) for c, res in zip(cases, results)) if m]
    assert not bad, f"{len(bad)} of {len(cases)} differ from the oracle:\n" + "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------- BGZF member walk
def bgzf_member(payload, crc, isize, extra=b"", bc=True, bsize=None):
    sub = extra
    xlen = len(extra) + (6 if bc else 0)
    total = 12 + xlen + len(payload) + 8
    if bc:
        sub = extra + b"BC" + struct.pack("<HH", 2, (total - 1) if bsize is None else bsize)
    return b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", xlen) + sub + payload + struct.pack("<II", crc, isize)


def run_scan(exe, tmp_path, image, max_members):
    (tmp_path / "image.bgzf").write_bytes(image)
    r = subprocess.run([exe, "scan", str(tmp_path / "image.bgzf"), str(max_members)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    return lines[0], lines[1:]


def test_bgzf_scan_of_the_fixture(check_exe, tmp_path):
    image = open(BAM, "rb").read()
    assert len(image) == 222075
    (rc, n, used), members = run_scan(check_exe, tmp_path, image, 64)
    assert (rc, n, used) == (0, 12, len(image))
    total = 0
    for off, plen, crc, isize in members:
        out = zlib.decompress(image[off:off + plen], -15)
        assert (zlib.crc32(out), len(out)) == (crc, isize)
        total += isize
    assert total == 717156 and max(m[3] for m in members) == 65498 and members[-1][3] == 0
    assert run_scan(check_exe, tmp_path, image, -1)[0] == (0, 12, len(image))        # counting only
    (rc, n, used), some = run_scan(check_exe, tmp_path, image, 5)                      # a caller with room for five
    assert (rc, n) == (0, 5) and some == members[:5] and used == members[5][0] - 18


def test_bgzf_scan_of_malformed_members(check_exe, tmp_path):
    good = bgzf_member(b"\x03\x00", 0, 0)
    assert run_scan(check_exe, tmp_path, good + good, 8)[0] == (0, 2, 2 * len(good))
    # extra subfields in front of BC
    padded = bgzf_member(b"\x03\x00", 0, 0, extra=b"XY" + struct.pack("<H", 3) + b"abc")
    head, members = run_scan(check_exe, tmp_path, good + padded, 8)
    assert head == (0, 2, len(good) + len(padded)) and members[1][:2] == (len(good) + 12 + 7 + 6, 2)
    bad_magic = b"\x1f\x8b\x08\x00" + good[4:]
    assert run_scan(check_exe, tmp_path, good + bad_magic, 8)[0] == (1, 1, len(good))
    assert run_scan(check_exe, tmp_path, good + good[:10], 8)[0] == (2, 1, len(good))
    no_bc = bgzf_member(b"\x03\x00", 0, 0, extra=b"XY" + struct.pack("<H", 2) + b"ab", bc=False)
    assert run_scan(check_exe, tmp_path, good + no_bc, 8)[0] == (3, 1, len(good))
    past_end = bgzf_member(b"\x03\x00", 0, 0, bsize=len(good))   # one byte more than there is
    assert run_scan(check_exe, tmp_path, good + past_end, 8)[0] == (4, 1, len(good))
    too_small = bgzf_member(b"\x03\x00", 0, 0, bsize=20)
    assert run_scan(check_exe, tmp_path, too_small, 8)[0] == (4, 0, 0)
    assert run_scan(check_exe, tmp_path, b"", 8)[0] == (0, 0, 0)


def test_bgzf_scan_through_the_c_abi():
    """gklhip_bgzf_scan itself (no device needed): the same answers, and the refusals as exceptions."""
    from gkl_amd import native
    image = open(BAM, "rb").read()
    off, plen, crc, isize, used = native.bgzf_scan(image)
    assert len(off) == 12 and used == len(image) and int(isize.sum()) == 717156
    assert all(zlib.crc32(zlib.decompress(image[o:o + l], -15)) == c for o, l, c in zip(off, plen, crc))
    assert len(native.bgzf_scan(image, 5)[0]) == 5
    good = bgzf_member(b"\x03\x00", 0, 0)
    with pytest.raises(native.BgzfError) as e:
        native.bgzf_scan(good + b"\x1f\x8b\x08\x00" + good[4:])
    assert e.value.bad_member == 1 and "magic" in str(e.value)
    with pytest.raises(native.BgzfError) as e:
        native.bgzf_scan(bgzf_member(b"\x03\x00", 0, 0, bsize=4000))
    assert e.value.bad_member == 0 and "BSIZE" in str(e.value)


def test_every_symbol_of_the_header_is_exported():
    import ctypes
    import re
    try:
        import torch  # noqa: F401  (HIP runtime load order, see gkl_amd.native.load_library)
    except ImportError:
        pass
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflate", "gkl_hip_inflate.h")).read(), flags=re.S)
    symbols = sorted(set(re.findall(r"\b(gklhip_\w+)\s*\(", text)))
    assert len(symbols) == 8, symbols
    lib = ctypes.CDLL(os.path.join(ROOT, "gkl_amd", "lib", "libgklhip_inflate.so"))
    for s in symbols:
        assert hasattr(lib, s), f"{s} is declared but not exported by libgklhip_inflate.so"


# ---------------------------------------------------------------------------------------------- the mirror's checks
def test_mirror_argument_checks():
    from gkl_amd.errors import ArrayIndexOutOfBoundsException, IllegalArgumentException, NullPointerException
    from gkl_amd.inflate import IntelInflater
    with pytest.raises(IllegalArgumentException, match="ZLIB format is not supported at this time with Intel GKL"):
        IntelInflater(nowrap=False)
    inf = IntelInflater()
    inf._ctx = object()   # the checks come before any use of the device
    data = bytes(10)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        inf.setInput(None, 0, 0)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Offset value is less than zero"):
        inf.setInput(data, -1, 1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value is less than zero"):
        inf.setInput(data, 0, -1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value exceeds permissible range"):
        inf.setInput(data, 5, 6)
    out = bytearray(10)
    with pytest.raises(NullPointerException, match="Output buffer is null"):
        inf.inflate(None, 0, 0)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Offset value is less than zero"):
        inf.inflate(out, -1, 1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value is less than zero"):
        inf.inflate(out, 0, -1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value exceeds permissible range"):
        inf.inflate(out, 5, 6)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        inf.inflate(out, 0, 10)   # no input set
    inf.setInput(data, 3, 0)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        inf.inflate(out, 0, 10)   # an empty input
    assert not inf.finished()
    inf._ctx = None

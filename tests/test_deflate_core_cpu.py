"""The encoder core of the batch deflate (gkl_amd/csrc/deflate_core.h, the one copy of the deflate encoding logic, which
the GPU kernel instantiates for a wavefront) checked on the host: tests/native/deflate_core_check.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers, runs the input list of tests/deflate_inputs.py
through the same core for one thread and for four lanes, every source and output in a heap block of exactly its size.
The oracle is Python's zlib.  Also: the code construction alone, the ratio condition against zlib level 1, the BGZF
framing, the exported symbols and the argument checks of the IntelDeflater mirror."""
import heapq
import os
import re
import shutil
import subprocess
import zlib

import pytest

from tests import deflate_inputs as di

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deflate_core_check.cpp")
CORE = os.path.join(ROOT, "gkl_amd", "csrc", "deflate_core.h")
HEADER = os.path.join(ROOT, "include", "deflate", "gkl_hip_deflate.h")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    exe = str(tmp_path_factory.mktemp("deflate_core") / "deflate_core_check")
    # no ROCm include path: the core and the framing are plain C++
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-pthread", "-o", exe, SRC], check=True, timeout=300)
    return exe


def run_core(exe, tmp_path, inputs, capacities, level, strategy, types, lanes=1):
    (tmp_path / "inputs.bin").write_bytes(di.input_file(inputs, capacities))
    r = subprocess.run([exe, "run", str(tmp_path / "inputs.bin"), str(tmp_path / "results.bin"), str(level), str(strategy), str(types), str(lanes)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.startswith(f"ok: {len(inputs)} streams"), r.stdout
    return di.parse_results((tmp_path / "results.bin").read_bytes(), len(inputs))


_one_lane = {}


def one_lane(exe, tmp_path, setting):
    """The one-lane results of the whole list under a setting, computed once."""
    name, level, strategy, types = setting
    if name not in _one_lane:
        datas = [d for _, d in di.INPUTS]
        _one_lane[name] = run_core(exe, tmp_path, datas, [di.roomy(len(d)) for d in datas], level, strategy, types)
    return _one_lane[name]


def test_core_is_free_of_the_device_runtime():
    text = open(CORE).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "__device__" not in code and "threadIdx" not in code and "__shared__" not in code
    assert set(re.findall(r"#include\s+(\S+)", code)) == {"<stdint.h>", '"inflate_core.h"'}
    assert "crc32_stream" not in code   # the CRC-32 is inflate_core.h's, used by the callers, not copied


def test_input_list_is_what_the_tests_expect():
    names = [n for n, _ in di.INPUTS]
    assert len(names) == len(set(names)) and sum(n.startswith("case_output_") for n in names) == 459
    sizes = {len(d) for _, d in di.INPUTS}
    assert {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 258, 259, 260, 261, 517, 65280, 1 << 20} <= sizes
    assert {di.BLOCK_LEN - 1, di.BLOCK_LEN, di.BLOCK_LEN + 1, 2 * di.BLOCK_LEN + 1, 2 * 32767, 2 * 32768, 2 * 32769} <= sizes
    assert sum(n.startswith("fixture_65280_") for n in names) == 11 and sum(n.startswith("fixture_65498_") for n in names) == 11


@pytest.mark.parametrize("setting", di.SETTINGS, ids=[s[0] for s in di.SETTINGS])
def test_whole_list_round_trips_under_sanitizers(check_exe, tmp_path, setting):
    name, level, strategy, types = setting
    results = one_lane(check_exe, tmp_path, setting)
    bad = []
    for (iname, data), (status, stream, crc) in zip(di.INPUTS, results):
        m = None
        if status != 0:
            m = f"{iname}: status {status}"
        m = m or di.round_trip_fault(iname, data, stream)
        if m is None and crc != zlib.crc32(data):
            m = f"{iname}: CRC-32 {crc:08x}, zlib says {zlib.crc32(data):08x}"
        if m is None and name in ("default", "huffman_only", "level0") and len(stream) > di.bound(len(data)):
            m = f"{iname}: {len(stream)} bytes exceed the bound {di.bound(len(data))}"
        if m is None and name in ("stored", "level0") and len(stream) != di.bound(len(data)):
            m = f"{iname}: {len(stream)} bytes, stored blocks take {di.bound(len(data))}"
        if m:
            bad.append(m)
    assert not bad, f"{len(bad)} of {len(di.INPUTS)}:\n" + "\n".join(bad[:20])


def test_the_settings_drive_the_block_types(check_exe, tmp_path):
    """The first block's type bits are what the mask allows; random bytes fall back to stored, len + 5."""
    for setting, allowed in zip(di.SETTINGS, ({0, 1, 2}, {0, 1, 2}, {1}, {2}, {0}, {0})):
        types = {(stream[0] >> 1) & 3 for _, stream, _ in one_lane(check_exe, tmp_path, setting)}
        assert types <= allowed and (len(allowed) == 1 or len(types) == 3), (setting[0], types)
    by_name = {n: r for (n, _), r in zip(di.INPUTS, one_lane(check_exe, tmp_path, di.SETTINGS[0]))}
    assert len(by_name["random_65280"][1]) == 65280 + 5
    assert len(by_name["len_0"][1]) <= 5 and len(by_name["run_65280"][1]) < 400


def test_bound_matches_the_formula(check_exe):
    from gkl_amd import native
    for n in (0, 1, 65534, 65535, 65536, 131070, 131071, 1 << 20, (1 << 31) - 1):
        r = subprocess.run([check_exe, "bound", str(n)], capture_output=True, text=True, timeout=60)
        assert int(r.stdout) == di.bound(n) == native.deflate_bound(n), n


def test_capacity_exact_and_one_short(check_exe, tmp_path):
    """At its exact size a stream fits, one byte short and at 0 it is OUT_OVERFLOW with out_len 0; the sanitizers see
    every byte of the exactly sized output block."""
    picks = ("len_0", "len_1", "len_5", "chunk_seam_65", "run_259", "period_63", "random_300", "random_65280", "skewed_4_symbols",
             "block_seam_65536", "block_seam_131071", "distance_32768", "fibonacci_counts", "fixture_65280_3")
    datas = dict(di.INPUTS)
    for setting in (di.SETTINGS[0], di.SETTINGS[2], di.SETTINGS[3], di.SETTINGS[5]):
        _, level, strategy, types = setting
        exact = {n: len(r[1]) for (n, _), r in zip(di.INPUTS, one_lane(check_exe, tmp_path, setting))}
        inputs = [datas[p] for p in picks]
        fit = run_core(check_exe, tmp_path, inputs, [exact[p] for p in picks], level, strategy, types)
        short = run_core(check_exe, tmp_path, inputs, [exact[p] - 1 for p in picks], level, strategy, types)
        none = run_core(check_exe, tmp_path, inputs, [0] * len(picks), level, strategy, types)
        for p, a, b, c in zip(picks, fit, short, none):
            assert a[0] == 0 and di.round_trip_fault(p, datas[p], a[1]) is None, (setting[0], p)
            assert (b[0], b[1]) == (1, b"") and (c[0], c[1]) == (1, b""), (setting[0], p)


@pytest.mark.parametrize("setting", di.SETTINGS, ids=[s[0] for s in di.SETTINGS])
def test_four_lanes_write_the_one_lane_bytes(check_exe, tmp_path, setting):
    _, level, strategy, types = setting
    datas = [d for _, d in di.INPUTS]
    four = run_core(check_exe, tmp_path, datas, [di.roomy(len(d)) for d in datas], level, strategy, types, lanes=4)
    one = one_lane(check_exe, tmp_path, setting)
    differ = [n for (n, _), a, b in zip(di.INPUTS, one, four) if a != b]
    assert not differ, differ[:20]


# ---------------------------------------------------------------------------------------------- code construction alone
def huffman_cost(freq):
    """The cost and the longest code of a plain Huffman code (two or more used symbols)."""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    cost, tie = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tie, max(a[2], b[2]) + 1))
        tie += 1
    return cost, heap[0][2]


def histograms():
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    hs = []
    for n in range(20, 41):
        hs.append((286, 15, fib[:n] + [0] * (286 - n)))
        hs.append((286, 15, [0] * (286 - n) + fib[:n][::-1]))
    for n in range(10, 20):
        hs.append((19, 7, fib[:n] + [0] * (19 - n)))
        hs.append((19, 7, ([0] * (19 - n) + fib[:n])[::-1]))
    for symbols, limit in ((286, 15), (30, 15), (19, 7)):
        hs.append((symbols, limit, [0] * 5 + [9] + [0] * (symbols - 6)))                 # one symbol
        hs.append((symbols, limit, [3] + [0] * (symbols - 2) + [1000]))                  # two symbols
        hs.append((symbols, limit, [5] * symbols))                                       # all equal
        hs.append((symbols, limit, [1] * (symbols - 1) + [1 << 30]))                     # one huge count
        hs.append((symbols, limit, [(i * 7919) % 97 for i in range(symbols)]))           # mixed, some zeros
    return hs


def test_code_construction_alone(check_exe, tmp_path):
    import struct
    hs = histograms()
    blob = struct.pack("<I", len(hs)) + b"".join(struct.pack(f"<II{s}I", s, lim, *f) for s, lim, f in hs)
    (tmp_path / "hist.bin").write_bytes(blob)
    r = subprocess.run([check_exe, "lengths", str(tmp_path / "hist.bin"), str(tmp_path / "lens.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    out, at = (tmp_path / "lens.bin").read_bytes(), 0
    limited = 0
    for k, (symbols, limit, freq) in enumerate(hs):
        lens = list(out[at:at + symbols])
        at += symbols
        used = [i for i, f in enumerate(freq) if f]
        assert all((lens[i] > 0) == (freq[i] > 0) for i in range(symbols)), k
        assert max(lens) <= limit, (k, max(lens))
        if len(used) == 1:
            assert lens[used[0]] == 1
            continue
        assert sum(2 ** (limit - lens[i]) for i in used) == 2 ** limit, f"histogram {k}: the Kraft sum is not 1"
        assert all(lens[i] <= lens[j] for i in used for j in used if freq[i] > freq[j]), f"histogram {k}: a more frequent symbol has a longer code"
        cost, longest = huffman_cost(freq)
        mine = sum(freq[i] * lens[i] for i in used)
        if longest <= limit:
            assert mine == cost, (k, mine, cost)
        else:
            limited += 1
            assert mine > cost
    assert at == len(out) and limited >= 20


# ---------------------------------------------------------------------------------------------- ratio condition
def test_ratio_against_zlib_level_1(check_exe, tmp_path):
    """The fixture payload in 65280-byte blocks at level 1: no more than 1.05 x zlib level 1 on the same blocks (the
    bound of a prototype of the plainest design: 64-position chunks, 8192 one-entry slots, minimum match 4, which gave
    1.034 x), and below the fixed-Huffman-only total of the same tokens: dynamic codes must pay on BAM data."""
    rows = {s[0]: one_lane(check_exe, tmp_path, s) for s in (di.SETTINGS[0], di.SETTINGS[2])}
    idx = [k for k, (n, _) in enumerate(di.INPUTS) if n.startswith("fixture_65280_")]
    ours = sum(len(rows["default"][k][1]) for k in idx)
    fixed = sum(len(rows["fixed"][k][1]) for k in idx)
    ref = 0
    for k in idx:
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(z.compress(di.INPUTS[k][1]) + z.flush())
    print(f"fixture payload, 65280-byte blocks: {ours} bytes, zlib level 1 {ref} ({ours / ref:.4f} x), fixed codes only {fixed}")
    assert ours <= 1.05 * ref, (ours, ref, ours / ref)
    assert ours < fixed, (ours, fixed)


# ---------------------------------------------------------------------------------------------- BGZF framing
@pytest.mark.parametrize("block_size", (0, 65498, 1000))
def test_bgzf_framing_of_the_host_cores_streams(check_exe, tmp_path, block_size):
    from gkl_amd import native
    payload = di.fixture_payload() if block_size != 1000 else di.fixture_payload()[:70001]
    (tmp_path / "payload.bin").write_bytes(payload)
    r = subprocess.run([check_exe, "bgzf", str(tmp_path / "payload.bin"), str(block_size), "1", "1", str(tmp_path / "image.bgzf")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    image = (tmp_path / "image.bgzf").read_bytes()
    off, plen, crc, isize, used = native.bgzf_scan(image)
    cut = block_size or 65280
    assert used == len(image) and len(off) == -(-len(payload) // cut) + 1 and len(image) <= native.bgzf_bound(len(payload), block_size)
    at = 0
    for o, l, c, n in zip(off, plen, crc, isize):
        part = payload[at:at + cut] if at < len(payload) else b""
        assert zlib.decompress(image[o:o + l], -15) == part and (zlib.crc32(part), len(part)) == (c, n)
        assert 18 + l + 8 <= 65536
        at += len(part)
    assert at == len(payload)
    assert image[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert native.bgzf_bound(0, 0) == 28 and native.bgzf_bound(10, 65499) == -1 and native.bgzf_bound(65498, 65498) == 65498 + 31 + 28


def test_every_symbol_of_the_header_is_exported():
    import ctypes
    try:
        import torch  # noqa: F401  (HIP runtime load order, see gkl_amd.native.load_library)
    except ImportError:
        pass
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    symbols = sorted(set(re.findall(r"\b(gklhip_\w+)\s*\(", text)))
    assert len(symbols) == 10, symbols
    lib = ctypes.CDLL(os.path.join(ROOT, "gkl_amd", "lib", "libgklhip_deflate.so"))
    for s in symbols:
        assert hasattr(lib, s), f"{s} is declared but not exported by libgklhip_deflate.so"


# ---------------------------------------------------------------------------------------------- the mirror's checks
def test_mirror_argument_checks():
    from gkl_amd.deflate import IntelDeflater
    from gkl_amd.errors import ArrayIndexOutOfBoundsException, IllegalArgumentException, NullPointerException, RuntimeException
    for level in (-2, 10):
        with pytest.raises(IllegalArgumentException, match="Illegal compression level"):
            IntelDeflater(level)
    for level in (1, 2):
        with pytest.raises(IllegalArgumentException, match="Compression configuration requested not supported"):
            IntelDeflater(level, nowrap=False)
    for level in (-1, 2, 9):
        with pytest.raises(RuntimeException, match="is not built"):
            IntelDeflater(level).reset()
    d = IntelDeflater(1)
    d._ctx = object()   # the checks come before any use of the device
    data = bytes(10)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        d.setInput(None, 0, 0)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Offset value is less than zero"):
        d.setInput(data, -1, 1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value is less than zero"):
        d.setInput(data, 0, -1)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value exceeds permissible range"):
        d.setInput(data, 5, 6)
    out = bytearray(10)
    with pytest.raises(NullPointerException, match="Output buffer is null"):
        d.deflate(None, 0, 0)
    with pytest.raises(IllegalArgumentException, match="The only accepted offset value is 0"):
        d.deflate(out, 1, 5)
    with pytest.raises(ArrayIndexOutOfBoundsException, match="Length value is less or equal than zero"):
        d.deflate(out, 0, 0)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        d.deflate(out, 0, 10)   # no input set
    d.setInput(data, 3, 0)
    with pytest.raises(NullPointerException, match="Input buffer is null"):
        d.deflate(out, 0, 10)   # an empty input
    assert not d.finished()
    d._ctx = None

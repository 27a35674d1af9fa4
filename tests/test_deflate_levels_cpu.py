"""Deflate levels 3-8 (hash chains, bounded walks, minimum match 3, lazy selection: gkl_amd/csrc/deflate_core.h) checked
on the host: tests/native/deflate_core_check.cpp, the stand-alone program of tests/test_deflate_core_cpu.py, built with
the address and undefined-behaviour sanitizers, runs tests/deflate_inputs.INPUTS plus tests/deflate_level_inputs.INPUTS
through the core for one thread and for four lanes.  The oracle is Python's zlib.  Also: guards that the new inputs
reach their paths, the digests that pin the bytes of levels 0 and 1, the ratio conditions on the BAM fixture and the
levels the IntelDeflater mirror accepts."""
import importlib.util
import json
import os
import shutil
import subprocess
import zlib

import pytest

from tests import deflate_inputs as di
from tests import deflate_level_inputs as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deflate_core_check.cpp")
DIGESTS = os.path.join(ROOT, "tests", "golden", "deflate_parent_digests.json")
ALL = list(di.INPUTS) + list(dl.INPUTS)
DATAS = [d for _, d in ALL]
INDEX = {n: k for k, (n, _) in enumerate(ALL)}
# (name, level, strategy, block-type mask), as tests/deflate_inputs.SETTINGS
ROUND_TRIP = (("level3", 3, 0, 0), ("level5", 5, 0, 0), ("level8", 8, 0, 0), ("level5_fixed", 5, 0, di.FIXED),
              ("level5_dynamic", 5, 0, di.DYNAMIC), ("level5_huffman_only", 5, 1, 0))
FIXED = {level: (f"level{level}_fixed", level, 0, di.FIXED) for level in (1, 3, 5, 8)}


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the stand-alone check")
    exe = str(tmp_path_factory.mktemp("deflate_levels") / "deflate_core_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-pthread", "-o", exe, SRC], check=True, timeout=300)
    return exe


def run_core(exe, tmp_path, inputs, capacities, level, strategy, types, lanes=1):
    (tmp_path / "inputs.bin").write_bytes(di.input_file(inputs, capacities))
    r = subprocess.run([exe, "run", str(tmp_path / "inputs.bin"), str(tmp_path / "results.bin"), str(level), str(strategy), str(types), str(lanes)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert r.stdout.startswith(f"ok: {len(inputs)} streams"), r.stdout
    return di.parse_results((tmp_path / "results.bin").read_bytes(), len(inputs))


_one_lane = {}


def one_lane(exe, tmp_path, setting):
    """The one-lane results of both lists under a setting, computed once."""
    name, level, strategy, types = setting
    if name not in _one_lane:
        _one_lane[name] = run_core(exe, tmp_path, DATAS, [di.roomy(len(d)) for d in DATAS], level, strategy, types)
    return _one_lane[name]


def test_new_inputs_are_what_the_tests_expect():
    names = [n for n, _ in dl.INPUTS]
    assert len(names) == len(set(names)) and not set(names) & {n for n, _ in di.INPUTS}
    assert all(len(d) <= dl.BLOCK_LEN for n, d in dl.INPUTS if n != "repeat_over_block_seam")
    assert len(dict(dl.INPUTS)["key_every_4096"]) == dl.BLOCK_LEN
    a, b = dl.colliding_keys()
    assert a[:3] != b[:3] and dl.hash3(a) == dl.hash3(b)
    assert dict(dl.INPUTS)["interleaved_collision"].count(a) == 40 == dict(dl.INPUTS)["interleaved_collision"].count(b)
    assert dl.repeated_trigrams(dict(dl.INPUTS)["three_byte_far"], dl.FAR3) == 0
    assert set(dl.LEVELS) == {3, 4, 5, 6, 7, 8} and all(depth < 300 for depth, _, _ in dl.LEVELS.values())


@pytest.mark.parametrize("setting", ROUND_TRIP, ids=[s[0] for s in ROUND_TRIP])
def test_both_lists_round_trip_under_sanitizers(check_exe, tmp_path, setting):
    name, level, strategy, types = setting
    results = one_lane(check_exe, tmp_path, setting)
    bad = []
    for (iname, data), (status, stream, crc) in zip(ALL, results):
        m = None
        if status != 0:
            m = f"{iname}: status {status}"
        m = m or di.round_trip_fault(iname, data, stream)
        if m is None and crc != zlib.crc32(data):
            m = f"{iname}: CRC-32 {crc:08x}, zlib says {zlib.crc32(data):08x}"
        if m is None and types == 0 and len(stream) > di.bound(len(data)):
            m = f"{iname}: {len(stream)} bytes exceed the bound {di.bound(len(data))}"
        if m:
            bad.append(m)
    assert not bad, f"{len(bad)} of {len(ALL)}:\n" + "\n".join(bad[:20])


def test_huffman_only_is_the_same_at_every_level(check_exe, tmp_path):
    picks = [k for k, d in enumerate(DATAS) if len(d) <= 70000]
    datas = [DATAS[k] for k in picks]
    five = one_lane(check_exe, tmp_path, ROUND_TRIP[5])
    one = run_core(check_exe, tmp_path, datas, [di.roomy(len(d)) for d in datas], 1, 1, 0)
    eight = run_core(check_exe, tmp_path, datas, [di.roomy(len(d)) for d in datas], 8, 1, 0)
    assert one == eight == [five[k] for k in picks]


@pytest.mark.parametrize("setting", ROUND_TRIP[:3], ids=[s[0] for s in ROUND_TRIP[:3]])
def test_four_lanes_write_the_one_lane_bytes(check_exe, tmp_path, setting):
    _, level, strategy, types = setting
    four = run_core(check_exe, tmp_path, DATAS, [di.roomy(len(d)) for d in DATAS], level, strategy, types, lanes=4)
    one = one_lane(check_exe, tmp_path, setting)
    differ = [n for (n, _), a, b in zip(ALL, one, four) if a != b]
    assert not differ, differ[:20]


def test_capacity_exact_and_one_short_at_level_5(check_exe, tmp_path):
    """The picks of test_capacity_exact_and_one_short and two of the new inputs: at its exact size a stream fits, one
    byte short and at 0 it is OUT_OVERFLOW with out_len 0."""
    picks = ("len_0", "len_1", "len_5", "chunk_seam_65", "run_259", "period_63", "random_300", "random_65280", "skewed_4_symbols",
             "block_seam_65536", "block_seam_131071", "distance_32768", "fibonacci_counts", "fixture_65280_3", "chain_of_300",
             "repeat_over_block_seam")
    results = one_lane(check_exe, tmp_path, ROUND_TRIP[1])
    inputs = [DATAS[INDEX[p]] for p in picks]
    exact = [len(results[INDEX[p]][1]) for p in picks]
    fit = run_core(check_exe, tmp_path, inputs, exact, 5, 0, 0)
    short = run_core(check_exe, tmp_path, inputs, [e - 1 for e in exact], 5, 0, 0)
    none = run_core(check_exe, tmp_path, inputs, [0] * len(picks), 5, 0, 0)
    for p, d, a, b, c in zip(picks, inputs, fit, short, none):
        assert a[0] == 0 and a == results[INDEX[p]] and di.round_trip_fault(p, d, a[1]) is None, p
        assert (b[0], b[1]) == (1, b"") and (c[0], c[1]) == (1, b""), p


def test_the_new_inputs_reach_their_paths(check_exe, tmp_path):
    """Under the fixed-only mask the size follows the tokens."""
    size = {level: {n: len(r[1]) for (n, _), r in zip(ALL, one_lane(check_exe, tmp_path, FIXED[level]))} for level in (1, 3, 5, 8)}
    for level in (1, 3, 5, 8):
        for (n, d), r in zip(ALL, one_lane(check_exe, tmp_path, FIXED[level])):
            assert r[0] == 0 and di.round_trip_fault(n, d, r[1]) is None, (level, n)
    show = ["three_byte_near", "three_byte_far", "chain_of_300", "key_every_4096"] + [f"lazy_trigger_{o}" for o in dl.LAZY_OFFSETS]
    for n in show:
        print(n, {level: size[level][n] for level in (1, 3, 5, 8)})
    # minimum match 3: level 1 finds nothing in either input; the far repeats are dropped, so level 5 finds nothing either
    assert size[5]["three_byte_near"] < size[1]["three_byte_near"]
    assert size[5]["three_byte_far"] == size[1]["three_byte_far"]
    # lazy (level 5) against greedy (level 3) over the same candidates; at offset 63 the chunk's last position does not look ahead
    assert not dl.LEVELS[3][2] and dl.LEVELS[5][2]
    for o in (0, 31, 62):
        assert size[5][f"lazy_trigger_{o}"] < size[3][f"lazy_trigger_{o}"], o
    assert size[5]["lazy_trigger_63"] == size[3]["lazy_trigger_63"]
    # the last occurrence: depth 128 reaches number 200, 100 back, and its 5-byte match; depth 4 only 4-byte prefixes;
    # neither reaches the oldest's 6 bytes, 300 back
    assert size[8]["chain_of_300"] <= size[3]["chain_of_300"]


def test_level_0_and_1_bytes_are_the_parents(check_exe, tmp_path):
    """tests/golden/deflate_parent_digests.json was written by tests/golden/make_deflate_parent_digests.py on the commit
    before levels 3-8: one SHA-256 per setting over the (status, length, stream) records of the whole list."""
    spec = importlib.util.spec_from_file_location("make_deflate_parent_digests", os.path.join(ROOT, "tests", "golden", "make_deflate_parent_digests.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(DIGESTS) as f:
        golden = json.load(f)
    assert golden["inputs"] == len(di.INPUTS) and set(golden["sha256"]) == {s[0] for s in di.SETTINGS}
    assert gen.digests(check_exe, str(tmp_path)) == golden["sha256"]


def test_ratio_on_the_fixture(check_exe, tmp_path):
    """The fixture payload (717 156 bytes) in 65 280-byte blocks, totals of the eleven streams.  Measured once on the
    host core: level 1 251 601, level 3 231 147, level 5 221 302, level 8 218 131; zlib (raw, same blocks) level 1
    243 374, level 5 221 992, level 8 217 091.  So level 5 is 0.9969 x zlib level 5, bound B = 1.00, and level 8 is
    1.0048 x zlib level 8, bound 1.01 (the measured ratio rounded up to the next 0.01)."""
    idx = [k for k, (n, _) in enumerate(ALL) if n.startswith("fixture_65280_")]
    assert len(idx) == 11
    ours = {1: sum(len(one_lane(check_exe, tmp_path, di.SETTINGS[0])[k][1]) for k in idx)}
    for setting in ROUND_TRIP[:3]:
        ours[setting[1]] = sum(len(one_lane(check_exe, tmp_path, setting)[k][1]) for k in idx)
    ref = {}
    for level in (1, 5, 8):
        ref[level] = 0
        for k in idx:
            z = zlib.compressobj(level, zlib.DEFLATED, -15)
            ref[level] += len(z.compress(DATAS[k]) + z.flush())
    print(f"fixture payload, 65280-byte blocks: ours {ours}, zlib {ref}; level 5 {ours[5] / ref[5]:.4f} x, level 8 {ours[8] / ref[8]:.4f} x")
    assert ours[5] < ours[1]
    assert ours[5] < ref[1]
    assert ours[8] <= ours[5] <= ours[3]
    assert ours[5] <= 1.00 * ref[5], (ours[5], ref[5])
    assert ours[8] <= 1.01 * ref[8], (ours[8], ref[8])


def test_mirror_accepts_levels_3_to_8():
    from gkl_amd import deflate
    from gkl_amd.errors import RuntimeException
    assert deflate.BUILT_LEVELS == (0, 1, 3, 4, 5, 6, 7, 8)
    for level in range(3, 9):
        d = deflate.IntelDeflater(level)
        d._ctx = object()   # reset() checks the level before any use of the device
        d.reset()
        assert not d.finished()
        d._ctx = None
    for level in (-1, 2, 9):
        with pytest.raises(RuntimeException, match="is not built"):
            deflate.IntelDeflater(level).reset()

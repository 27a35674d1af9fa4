"""Batch deflate on the GPU (include/deflate/gkl_hip_deflate.h, gkl_amd/csrc/deflate_kernel.h).  The contract under test:
a stream's bytes depend on its input, the level, the strategy and the block-type mask only -- so the wavefront's bytes
must EQUAL those of the same core run by one host thread (tests/native/deflate_core_check.cpp, built here with plain
g++), which is what catches a lane race, a missing sync() or a nondeterministic table insert.  Every stream also round
trips through Python's zlib.  Then: the device-resident call with sentinel-filled gaps, the pull loop over many more
streams than the grid, BGZF both ways on the device, two contexts on two threads, the IntelDeflater mirror, refusals."""
import os
import shutil
import subprocess
import threading
import zlib

import numpy as np
import pytest

from tests import deflate_inputs as di

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deflate_core_check.cpp")
GAP, SENTINEL = 32, 0xA5
DATAS = [d for _, d in di.INPUTS]
NAMES = [n for n, _ in di.INPUTS]


@pytest.fixture(scope="module")
def ctx():
    from gkl_amd import native
    with native.DeflateContext(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def host_core(tmp_path_factory):
    """setting -> [(status, stream, crc)] of the whole list from the one-lane host build of the core, computed once."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the host reference of the encoder")
    tmp = tmp_path_factory.mktemp("deflate_ref")
    exe = str(tmp / "deflate_core_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-o", exe, SRC], check=True, timeout=300)
    (tmp / "inputs.bin").write_bytes(di.input_file(DATAS, [di.roomy(len(d)) for d in DATAS]))
    cache = {}

    def get(setting):
        name, level, strategy, types = setting
        if name not in cache:
            r = subprocess.run([exe, "run", str(tmp / "inputs.bin"), str(tmp / "results.bin"), str(level), str(strategy), str(types), "1"],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            cache[name] = di.parse_results((tmp / "results.bin").read_bytes(), len(DATAS))
        return cache[name]
    return get


def layout(datas, capacities, gap=GAP):
    """Flat arrays of one call: behind every stream's capacity a sentinel-filled gap (an empty input of its own, whose
    stream of at most 12 bytes -- the dynamic-only one -- lands in the gap's first bytes)."""
    src_lens, caps = [], []
    for d, c in zip(datas, capacities):
        src_lens += [len(d), 0]
        caps += [c, gap]
    so, do = np.zeros(len(src_lens) + 1, np.int64), np.zeros(len(caps) + 1, np.int64)
    np.cumsum(src_lens, out=so[1:])
    np.cumsum(caps, out=do[1:])
    src = np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)
    dst = np.full(max(int(do[-1]), 1), SENTINEL, np.uint8)
    return src, so, dst, do


def streams_of(dst, do, out_len):
    return [dst[int(do[2 * k]):int(do[2 * k]) + int(out_len[2 * k])].tobytes() for k in range(len(out_len) // 2)]


def gaps_fault(dst, do, out_len, status):
    """None, or the first stream with a byte written behind its stream or outside the gap stream's own bytes.  A stream
    of several blocks that overflows in a later block has written the earlier ones: inside its capacity, never behind."""
    for k in range(len(out_len) // 2):
        lo, hi = int(do[2 * k]) + int(out_len[2 * k]), int(do[2 * k + 1])
        if int(status[2 * k]) == 1:
            lo = hi
        if not (dst[lo:hi] == SENTINEL).all():
            return f"stream {k}: bytes behind its {int(out_len[2 * k])} were written"
        g = int(out_len[2 * k + 1])
        if int(status[2 * k + 1]) != 0 or not 0 < g <= 12 or not (dst[hi + g:int(do[2 * k + 2])] == SENTINEL).all():
            return f"gap {k}: status {int(status[2 * k + 1])}, {g} bytes"
    return None


@pytest.mark.parametrize("setting", di.SETTINGS, ids=[s[0] for s in di.SETTINGS])
def test_whole_list_host_call_equals_the_host_core(ctx, host_core, setting):
    _, level, strategy, types = setting
    ref = host_core(setting)
    src, so, dst, do = layout(DATAS, [di.roomy(len(d)) for d in DATAS])
    ctx.set_strategy(strategy, types)
    try:
        out_len, crc, status = ctx.deflate_batch_raw(src, so, dst, do, level)
    finally:
        ctx.set_strategy(0, 0)
    got = streams_of(dst, do, out_len)
    bad = []
    for k, (name, data) in enumerate(di.INPUTS):
        m = None
        if int(status[2 * k]) != 0 or ref[k][0] != 0:
            m = f"{name}: status {int(status[2 * k])}, the host core's {ref[k][0]}"
        elif got[k] != ref[k][1]:
            first = next((i for i, (a, b) in enumerate(zip(got[k], ref[k][1])) if a != b), min(len(got[k]), len(ref[k][1])))
            m = f"{name}: {len(got[k])} bytes, the host core's {len(ref[k][1])}; first difference at byte {first}"
        m = m or di.round_trip_fault(name, data, got[k])
        if m is None and int(crc[2 * k]) != zlib.crc32(data):
            m = f"{name}: CRC-32 {int(crc[2 * k]):08x}"
        if m:
            bad.append(m)
    assert not bad, f"{len(bad)} of {len(DATAS)}:\n" + "\n".join(bad[:20])
    assert gaps_fault(dst, do, out_len, status) is None


def test_device_resident_call(ctx, host_core):
    """Byte-identical to the host core (hence to the host call); the sentinel gaps come back untouched, also at
    capacity = exact size, and at exact size - 1 nothing but OUT_OVERFLOW comes back."""
    import torch
    ref = host_core(di.SETTINGS[0])
    exact = [len(r[1]) for r in ref]
    for caps, fits in (([di.roomy(len(d)) for d in DATAS], True), (exact, True), ([e - 1 for e in exact], False)):
        src, so, dst, do = layout(DATAS, caps)
        d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst).cuda()
        out_len, crc, status = ctx.deflate_batch_device(d_src, so, d_dst, do, 1)
        out_len, status, back = out_len.cpu().numpy(), status.cpu().numpy(), d_dst.cpu().numpy()
        crc = crc.cpu().numpy().view(np.uint32)
        if fits:
            assert (status == 0).all()
            got = streams_of(back, do, out_len)
            differ = [NAMES[k] for k in range(len(DATAS)) if got[k] != ref[k][1] or int(crc[2 * k]) != ref[k][2]]
            assert not differ, differ[:20]
        else:
            assert (status[0::2] == 1).all() and (out_len[0::2] == 0).all()
        assert gaps_fault(back, do, out_len, status) is None


def test_pull_loop_over_many_times_the_grid(ctx):
    rng = np.random.default_rng(5)
    n = 20480
    base = rng.integers(0, 6, 4096, dtype=np.uint8).tobytes()
    datas = [base[(37 * k) % 3900:(37 * k) % 3900 + 100] for k in range(n)]
    outs, crcs, statuses = ctx.deflate_batch(datas, 1)
    assert statuses == [0] * n
    assert all(zlib.decompress(o, -15) == d and c == zlib.crc32(d) for o, d, c in zip(outs, datas, crcs))
    first = {}
    for d, o in zip(datas, outs):   # the same input, whichever wavefront took it, the same bytes
        assert first.setdefault(d, o) == o


@pytest.mark.parametrize("block_size", (0, 65498))
def test_bgzf_both_ways_on_the_device(ctx, block_size):
    from gkl_amd import native
    payload = di.fixture_payload()
    image, members = ctx.bgzf_deflate(payload, block_size)
    cut = block_size or 65280
    off, plen, crc, isize, used = native.bgzf_scan(image)
    assert used == len(image) and len(off) == members == -(-len(payload) // cut) + 1
    assert all(18 + int(l) + 8 <= 65536 for l in plen)
    assert b"".join(zlib.decompress(image[o:o + l], -15) for o, l in zip(off, plen)) == payload
    assert image[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    with native.InflateContext(device=0) as inf:
        assert inf.bgzf_inflate(image) == payload
    assert ctx.bgzf_deflate(b"", block_size) == (image[-28:], 1) and ctx.bgzf_deflate(b"", block_size, append_eof=False) == (b"", 0)
    stored, _ = ctx.bgzf_deflate(payload[:100000], block_size, level=0, append_eof=False)
    assert len(stored) == 100000 + 31 * 2 and native.bgzf_scan(stored)[4] == len(stored)


def test_two_contexts_on_two_threads(ctx, host_core):
    from gkl_amd import native
    ref = host_core(di.SETTINGS[0])
    picks = [k for k, d in enumerate(DATAS) if len(d) <= 4096][:60]
    datas, expect = [DATAS[k] for k in picks], [ref[k][1] for k in picks]
    faults = []

    def work():
        try:
            with native.DeflateContext(device=0) as c:
                for _ in range(50):
                    outs, _, statuses = c.deflate_batch(datas, 1)
                    if outs != expect or any(statuses):
                        faults.append("streams differ from the single-threaded bytes")
                        return
        except Exception as e:   # a thread's exception would otherwise be lost
            faults.append(repr(e))
    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not faults, faults


def test_mirror_round_trip_and_overflow_message():
    from gkl_amd.deflate import IntelDeflater
    from gkl_amd.errors import RuntimeException
    data = di.fixture_payload()[:65280]
    for level in (0, 1):
        d = IntelDeflater(level)
        d.reset()
        buf = bytearray(10) + bytearray(data)
        d.setInput(buf, 10, len(data))   # the mirror honours the offset
        d.finish()
        out = bytearray(65536)
        n = d.deflate(out, 0, len(out))
        assert d.finished() and zlib.decompress(bytes(out[:n]), -15) == data and (n < len(data) // 2 if level else n == len(data) + 5)
        d.reset()
        assert not d.finished()
        d.setInput(data, 0, len(data))
        d.finish()
        with pytest.raises(RuntimeException, match="Output buffer too small."):
            d.deflate(bytearray(n - 1), 0, n - 1)
        d.end()


def test_refusals_are_statuses(ctx):
    import ctypes as C
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException, RuntimeException
    src, so, dst, do = layout([b"abc"], [16])
    with pytest.raises(RuntimeException, match="level 2 is not built"):
        ctx.deflate_batch_raw(src, so, dst, do, 2)
    with pytest.raises(RuntimeException, match="level 2 is not built"):
        ctx.bgzf_deflate(b"abc", level=2)
    lib, h = ctx.lib, ctx.handle
    n1 = np.zeros(1, np.int32)
    assert lib.gklhip_deflate_batch(h, 0, None, None, None, None, 1, None, None, None) == native.OK        # n == 0 touches nothing
    assert lib.gklhip_deflate_batch(h, -1, None, None, None, None, 1, None, None, None) == native.ERR_INVALID_ARG
    assert lib.gklhip_deflate_batch(None, 1, src.ctypes.data, so.ctypes.data, dst.ctypes.data, do.ctypes.data, 1, n1.ctypes.data, None, n1.ctypes.data) == native.ERR_INVALID_ARG
    assert lib.gklhip_deflate_batch(h, 2, src.ctypes.data, None, dst.ctypes.data, do.ctypes.data, 1, n1.ctypes.data, None, n1.ctypes.data) == native.ERR_INVALID_ARG
    assert lib.gklhip_deflate_batch(h, 2, None, so.ctypes.data, dst.ctypes.data, do.ctypes.data, 1, n1.ctypes.data, None, n1.ctypes.data) == native.ERR_INVALID_ARG
    assert lib.gklhip_deflate_batch(h, 2, src.ctypes.data, so.ctypes.data, dst.ctypes.data, do.ctypes.data, 1, None, None, n1.ctypes.data) == native.ERR_INVALID_ARG
    with pytest.raises(IllegalArgumentException, match="offsets decrease"):
        ctx.deflate_batch_raw(src, np.array([0, 3, 2], np.int64), dst, do, 1)
    with pytest.raises(IllegalArgumentException, match="offsets decrease"):
        ctx.deflate_batch_raw(src, so, dst, np.array([0, 16, 8], np.int64), 1)
    with pytest.raises(IllegalArgumentException, match="strategy"):
        ctx.set_strategy(2, 0)
    with pytest.raises(IllegalArgumentException, match="mask"):
        ctx.set_strategy(0, 8)
    with pytest.raises(IllegalArgumentException, match="block_size"):
        ctx.bgzf_deflate(b"abc", block_size=65499)
    n64, m32 = C.c_int64(0), C.c_int32(0)
    assert lib.gklhip_bgzf_deflate(h, None, 5, 0, 1, 1, dst.ctypes.data, 64, C.byref(n64), C.byref(m32)) == native.ERR_INVALID_ARG
    assert lib.gklhip_bgzf_deflate(h, src.ctypes.data, 3, 0, 1, 1, dst.ctypes.data, 20, C.byref(n64), C.byref(m32)) == native.ERR_INVALID_ARG   # out_cap too small
    assert lib.gklhip_deflate_init(0, None) == native.ERR_INVALID_ARG
    # the context still works
    outs, _, statuses = ctx.deflate_batch([b"abcabcabcabc"], 1)
    assert statuses == [0] and zlib.decompress(outs[0], -15) == b"abcabcabcabc"

"""Deflate levels 3-8 on the GPU (the SEARCH_CHAINS instantiation of gkl_amd/csrc/deflate_kernel.h).  As in
tests/test_deflate.py the wavefront's bytes must EQUAL those of the same core run by one host thread
(tests/native/deflate_core_check.cpp, built here with plain g++): the chain links of a chunk, the walks over the ring
in global memory and the lazy selection leave no room for a lane race that this comparison would not show.  Level 5
runs both input lists, levels 3 and 8 about 40 picks.  Then: the device-resident call, more streams than wavefronts
(no link of a wavefront's previous stream is seen), level 1 before and after level 5 on one context, BGZF at level 5,
the levels that are refused, the IntelDeflater mirror."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_inputs as di
from tests import deflate_level_inputs as dl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "deflate_core_check.cpp")
GAP, SENTINEL = 32, 0xA5
ALL = list(di.INPUTS) + list(dl.INPUTS)
NEW = {n for n, _ in dl.INPUTS}
PICKS = [(n, d) for n, d in ALL if n in NEW or n.startswith(("chunk_seam_", "block_seam_", "run_", "distance_"))
         or n in ("fixture_65280_0", "fixture_65280_5", "fixture_65280_10")]


@pytest.fixture(scope="module")
def ctx():
    from gkl_amd import native
    with native.DeflateContext(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def host_core(tmp_path_factory):
    """(level, datas) -> [(status, stream, crc)] from the one-lane host build of the core, roomy capacities; the two
    lists are computed once per level."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the host reference of the encoder")
    tmp = tmp_path_factory.mktemp("deflate_levels_ref")
    exe = str(tmp / "deflate_core_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-o", exe, SRC], check=True, timeout=300)
    cache = {}

    def get(level, items, key=None):
        if key is not None and (level, key) in cache:
            return cache[(level, key)]
        datas = [d for _, d in items]
        (tmp / "inputs.bin").write_bytes(di.input_file(datas, [di.roomy(len(d)) for d in datas]))
        r = subprocess.run([exe, "run", str(tmp / "inputs.bin"), str(tmp / "results.bin"), str(level), "0", "0", "1"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res = di.parse_results((tmp / "results.bin").read_bytes(), len(datas))
        if key is not None:
            cache[(level, key)] = res
        return res
    return get


def layout(datas, capacities, gap=GAP):
    """Flat arrays of one call, a sentinel-filled gap (an empty input of its own) behind every stream's capacity."""
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
    """None, or the first stream with a byte written behind its stream or outside the gap stream's own bytes."""
    for k in range(len(out_len) // 2):
        lo, hi = int(do[2 * k]) + int(out_len[2 * k]), int(do[2 * k + 1])
        if not (dst[lo:hi] == SENTINEL).all():
            return f"stream {k}: bytes behind its {int(out_len[2 * k])} were written"
        g = int(out_len[2 * k + 1])
        if int(status[2 * k + 1]) != 0 or not 0 < g <= 12 or not (dst[hi + g:int(do[2 * k + 2])] == SENTINEL).all():
            return f"gap {k}: status {int(status[2 * k + 1])}, {g} bytes"
    return None


def differences(items, ref, got, status, crc):
    bad = []
    for k, (name, data) in enumerate(items):
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
    return bad


@pytest.mark.parametrize("level,which", ((5, "all"), (3, "picks"), (8, "picks")))
def test_host_call_equals_the_host_core(ctx, host_core, level, which):
    items = ALL if which == "all" else PICKS
    assert which == "all" or 35 <= len(items) <= 50
    ref = host_core(level, items, which)
    datas = [d for _, d in items]
    src, so, dst, do = layout(datas, [di.roomy(len(d)) for d in datas])
    out_len, crc, status = ctx.deflate_batch_raw(src, so, dst, do, level)
    bad = differences(items, ref, streams_of(dst, do, out_len), status, crc)
    assert not bad, f"{len(bad)} of {len(items)}:\n" + "\n".join(bad[:20])
    assert gaps_fault(dst, do, out_len, status) is None


def test_device_resident_call_at_level_5(ctx, host_core):
    import torch
    ref = host_core(5, PICKS, "picks")
    datas = [d for _, d in PICKS]
    src, so, dst, do = layout(datas, [len(r[1]) for r in ref])   # capacity = the exact size
    d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst).cuda()
    out_len, crc, status = ctx.deflate_batch_device(d_src, so, d_dst, do, 5)
    out_len, status, back = out_len.cpu().numpy(), status.cpu().numpy(), d_dst.cpu().numpy()
    crc = crc.cpu().numpy().view(np.uint32)
    bad = differences(PICKS, ref, streams_of(back, do, out_len), status, crc)
    assert not bad, bad[:20]
    assert [int(n) for n in out_len[0::2]] == [len(r[1]) for r in ref] and [int(c) for c in crc[0::2]] == [r[2] for r in ref]
    assert gaps_fault(back, do, out_len, status) is None


def test_more_streams_than_wavefronts(ctx, host_core):
    """5000 inputs of at most 2 KB, 50 distinct: every copy gives the host core's bytes, whichever wavefront took it and
    whatever stream left its links in that wavefront's ring before."""
    rng = np.random.default_rng(6)
    base = rng.integers(0, 6, 8192, dtype=np.uint8).tobytes()
    distinct = [(f"slice_{k}", base[(131 * k) % 6000:(131 * k) % 6000 + 40 * k + 48]) for k in range(50)]
    assert max(len(d) for _, d in distinct) <= 2048 and len({d for _, d in distinct}) == 50
    ref = {d: r for (_, d), r in zip(distinct, host_core(5, distinct))}
    datas = [distinct[int(k)][1] for k in rng.integers(0, 50, 5000)]
    outs, crcs, statuses = ctx.deflate_batch(datas, 5)
    assert statuses == [0] * 5000
    wrong = [k for k, (d, o, c) in enumerate(zip(datas, outs, crcs)) if (o, c) != (ref[d][1], ref[d][2])]
    assert not wrong, wrong[:20]


def test_no_state_across_levels(ctx, host_core):
    datas = [d for _, d in PICKS]
    first = ctx.deflate_batch(datas, 1)
    five = ctx.deflate_batch(datas, 5)
    again = ctx.deflate_batch(datas, 1)
    assert first == again
    assert first[0] == [r[1] for r in host_core(1, PICKS, "picks")] and first[2] == [0] * len(datas)
    assert five[0] == [r[1] for r in host_core(5, PICKS, "picks")] and five[2] == [0] * len(datas)


def test_bgzf_at_level_5(ctx):
    from gkl_amd import native
    payload = di.fixture_payload()
    image, members = ctx.bgzf_deflate(payload, level=5)
    one, _ = ctx.bgzf_deflate(payload, level=1)
    off, plen, crc, isize, used = native.bgzf_scan(image)
    assert used == len(image) and len(off) == members == -(-len(payload) // 65280) + 1
    assert all(18 + int(l) + 8 <= 65536 for l in plen)
    assert b"".join(zlib.decompress(image[o:o + l], -15) for o, l in zip(off, plen)) == payload
    with native.InflateContext(device=0) as inf:
        assert inf.bgzf_inflate(image) == payload
    print(f"BGZF image of the fixture payload: level 5 {len(image)} bytes, level 1 {len(one)}")
    assert len(image) < len(one)


def test_levels_accepted_and_refused(ctx):
    from gkl_amd.errors import RuntimeException
    for level in range(3, 9):
        outs, crcs, statuses = ctx.deflate_batch([b"abc"], level)
        assert statuses == [0] and zlib.decompress(outs[0], -15) == b"abc" and crcs == [zlib.crc32(b"abc")]
    src, so, dst, do = layout([b"abc"], [16])
    for level in (9, 10, -1):
        with pytest.raises(RuntimeException, match=f"level {level} is not built"):
            ctx.deflate_batch_raw(src, so, dst, do, level)
        with pytest.raises(RuntimeException, match="is not built"):
            ctx.bgzf_deflate(b"abc", level=level)


def test_mirror_round_trip_at_level_5():
    from gkl_amd.deflate import IntelDeflater
    from gkl_amd.errors import RuntimeException
    data = di.fixture_payload()[:65280]
    d = IntelDeflater(5)
    d.reset()
    buf = bytearray(10) + bytearray(data)
    d.setInput(buf, 10, len(data))
    d.finish()
    out = bytearray(65536)
    n = d.deflate(out, 0, len(out))
    assert d.finished() and zlib.decompress(bytes(out[:n]), -15) == data and n < len(data) // 2
    d.reset()
    assert not d.finished()
    d.setInput(data, 0, len(data))
    d.finish()
    with pytest.raises(RuntimeException, match="Output buffer too small."):
        d.deflate(bytearray(n - 1), 0, n - 1)
    d.end()

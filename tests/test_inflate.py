"""Batch inflate on the GPU (include/inflate/gkl_hip_inflate.h, gkl_amd/csrc/inflate_kernel.h) against Python's zlib: the case
list of tests/deflate_cases.py through the host call, the device-resident call and the IntelInflater mirror; the
reference's BAM test resource through the BGZF call; batch shapes; the device CRC-32; two contexts on two threads.
In the calls on flat arrays a sentinel-filled gap stands behind each stream's output and must come back untouched; it is
the device-resident calls that show this of the kernel (the host call copies back only what a stream reports written)."""
import os
import threading
import zlib

import numpy as np
import pytest

from tests import deflate_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = os.path.join(ROOT, "tests", "golden", "HiSeq.1mb.1RG.2k_lines.bam")
GAP, SENTINEL = 32, 0xA5


@pytest.fixture(scope="module")
def ctx():
    from gkl_amd import native
    with native.InflateContext(device=0) as c:
        yield c


def layout(cases):
    """Flat arrays of one call: behind every case an empty stream whose capacity is the sentinel gap."""
    src_lens, caps = [], []
    for c in cases:
        src_lens += [len(c.stream), 0]
        caps += [c.capacity, GAP]
    so, do = np.zeros(len(src_lens) + 1, np.int64), np.zeros(len(caps) + 1, np.int64)
    np.cumsum(src_lens, out=so[1:])
    np.cumsum(caps, out=do[1:])
    src = np.frombuffer(b"".join(c.stream for c in cases) or b"\0", dtype=np.uint8)
    dst = np.full(max(int(do[-1]), 1), SENTINEL, np.uint8)
    return src, so, dst, do


def check(cases, dst, do, out_len, consumed, crc, status):
    """Every stream's status, valid prefix, consumed count and CRC are the oracle's; nothing else was written."""
    bad = []
    for k, c in enumerate(cases):
        n, lo, hi = int(out_len[2 * k]), int(do[2 * k]), int(do[2 * k + 2])
        assert 0 <= n <= c.capacity, c.name
        m = dc.mismatch(c, int(status[2 * k]), dst[lo:lo + n].tobytes(), int(consumed[2 * k]), int(crc[2 * k]) & 0xFFFFFFFF)
        if m is None and not (dst[lo + n:hi] == SENTINEL).all():
            m = f"{c.name}: bytes behind the valid prefix were written"
        if m is None and (int(status[2 * k + 1]), int(out_len[2 * k + 1])) != (dc.END_INPUT, 0):
            m = f"{c.name}: the empty stream behind it ended {int(status[2 * k + 1])}"
        if m:
            bad.append(m)
    assert not bad, f"{len(bad)} of {len(cases)} differ from the oracle:\n" + "\n".join(bad[:20])


def family(name):
    return dc.CASES if name == "all" else [c for c in dc.CASES if c.family == name]


_host = {}


def host_call(ctx, name):
    if name not in _host:
        src, so, dst, do = layout(family(name))
        _host[name] = (dst, do) + ctx.inflate_batch_raw(src, so, dst, do)
    return _host[name]


@pytest.mark.parametrize("name", dc.FAMILIES + ("all",))
def test_case_list_host_call(ctx, name):
    dst, do, out_len, consumed, crc, status = host_call(ctx, name)
    check(family(name), dst, do, out_len, consumed, crc, status)


@pytest.mark.parametrize("name", dc.FAMILIES + ("all",))
def test_case_list_device_call(ctx, name):
    import torch
    cases = family(name)
    src, so, dst, do = layout(cases)
    d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst).cuda()
    res = ctx.inflate_batch_device(d_src, so, d_dst, do)
    out_len, consumed, crc, status = (t.cpu().numpy() for t in res)
    got = d_dst.cpu().numpy()
    check(cases, got, do, out_len, consumed, crc, status)
    # byte-identical to the host call
    h_dst, _, h_len, h_consumed, h_crc, h_status = host_call(ctx, name)
    assert got.tobytes() == h_dst.tobytes()
    assert np.array_equal(out_len, h_len) and np.array_equal(status, h_status) and np.array_equal(crc.view(np.uint32), h_crc)
    ok = h_status == dc.OK
    assert np.array_equal(consumed[ok], h_consumed[ok])


def test_case_list_through_the_mirror():
    from gkl_amd.errors import RuntimeException
    from gkl_amd.inflate import IntelInflater
    messages = {dc.INVALID_BLOCK: "Invalid deflate block found.", dc.INVALID_SYMBOL: "Invalid deflate symbol found.",
                dc.INVALID_LOOKBACK: "Invalid lookback distance found."}
    inf = IntelInflater(True)
    assert inf.load()
    seen = set()
    for name in dc.FAMILIES:
        cases = [c for c in family(name) if 0 < len(c.stream) < 70000]
        sample = [c for st in range(6) for c in [c for c in cases if c.status == st][:2]]   # two of every status the family has
        for c in sample:
            inf.reset()
            framed = b"xy" + c.stream + b"z"   # offsets into a larger array, as htsjdk passes them
            inf.setInput(framed, 2, len(c.stream))
            out = bytearray([SENTINEL]) * (c.capacity + 5)
            if c.status in messages:
                with pytest.raises(RuntimeException, match=messages[c.status]):
                    inf.inflate(out, 3, c.capacity)
            else:
                n = inf.inflate(out, 3, c.capacity)
                assert n == len(c.output) and bytes(out[3:3 + n]) == c.output, c.name
                assert set(out[:3]) | set(out[3 + n:]) <= {SENTINEL}, c.name
                assert inf.finished() == (c.status == dc.END_INPUT or (c.status == dc.OK and c.consumed == len(c.stream))), c.name
            seen.add(c.status)
    inf.end()
    assert seen == set(range(6))


# ---------------------------------------------------------------------------------------------- the BAM fixture
def test_bam_fixture_through_bgzf_inflate(ctx):
    image = open(BAM, "rb").read()
    off, plen, crc, isize, used = ctx.bgzf_scan(image)
    assert len(off) == 12 and used == len(image) == 222075
    expected = [zlib.decompress(image[o:o + l], -15) for o, l in zip(off, plen)]
    assert [len(e) for e in expected] == [int(v) for v in isize] and [zlib.crc32(e) for e in expected] == [int(v) for v in crc]
    got = ctx.bgzf_inflate(image)
    assert len(got) == 717156 and got == b"".join(expected)
    # the members as a plain batch: every CRC and every length from the device
    outs, crcs, statuses, consumed = ctx.inflate_batch([image[o:o + l] for o, l in zip(off, plen)], [int(v) for v in isize])
    assert statuses == [0] * 12 and outs == expected
    assert crcs == [int(v) for v in crc] and consumed == [int(v) for v in plen]


def test_bam_fixture_with_one_payload_bit_flipped(ctx):
    from gkl_amd import native
    image = bytearray(open(BAM, "rb").read())
    off, plen, _, _, _ = ctx.bgzf_scan(bytes(image))
    image[int(off[3]) + int(plen[3]) // 2] ^= 0x10
    with pytest.raises(native.BgzfError) as e:
        ctx.bgzf_inflate(bytes(image))
    assert e.value.bad_member == 3
    image[int(off[3]) + int(plen[3]) // 2] ^= 0x10
    image[int(off[7]) - 18] = 0x1e   # a member's magic
    with pytest.raises(native.BgzfError) as e:
        ctx.bgzf_inflate(bytes(image))
    assert e.value.bad_member == 7


# ---------------------------------------------------------------------------------------------- batch shapes
def test_no_stream_and_one_stream(ctx):
    assert ctx.inflate_batch([], []) == ([], [], [], [])
    data = dc.content("text", 1000, 41)
    assert ctx.inflate_batch([dc.deflate(data)], [1000]) == ([data], [zlib.crc32(data)], [0], [len(dc.deflate(data))])


def test_more_tiny_streams_than_resident_wavefronts(ctx):
    datas = [dc.content(dc.CONTENT_KINDS[k % 4], k % 37, k) for k in range(5000)]
    streams = [dc.deflate(d, ("level6", "fixed", "level0")[k % 3]) for k, d in enumerate(datas)]
    outs, crcs, statuses, consumed = ctx.inflate_batch(streams, [len(d) for d in datas])
    assert statuses == [0] * 5000 and outs == datas
    assert crcs == [zlib.crc32(d) for d in datas] and consumed == [len(s) for s in streams]


def test_many_times_more_streams_than_the_grid_has_wavefronts(ctx):
    """40 000 streams (20 000 tiny cases of every block type and status, an empty stream behind each) on a grid of 16
    wavefronts per CU: every wavefront takes stream after stream from the counter, so tables, bit reader and pending
    literals of one stream meet the leftovers of the last."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count * 16 * 4 < 40000
    tiny = [c for c in dc.CASES if len(c.stream) <= 400 and c.capacity <= 400]
    # the error cases of the list have roomy outputs: the same streams with eight bytes of room behind their valid prefix
    for c in dc.CASES:
        if len(c.stream) <= 400 and c.capacity > 400 and len(c.output) <= 400:
            cap = len(c.output) + 8
            tiny.append(dc.Case(c.name, c.family, c.stream, cap, *dc.classify(c.stream, cap)))
    assert {c.status for c in tiny} == set(range(6)) and {c.family for c in tiny} == set(dc.FAMILIES)
    cases = [tiny[k % len(tiny)] for k in range(20000)]
    src, so, dst, do = layout(cases)
    d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst).cuda()
    out_len, consumed, crc, status = (t.cpu().numpy() for t in ctx.inflate_batch_device(d_src, so, d_dst, do))
    check(cases, d_dst.cpu().numpy(), do, out_len, consumed, crc, status)
    h_len, h_consumed, h_crc, h_status = ctx.inflate_batch_raw(src, so, dst, do)
    check(cases, dst, do, h_len, h_consumed, h_crc, h_status)
    assert dst.tobytes() == d_dst.cpu().numpy().tobytes()


def test_sizes_mixed_with_a_bad_stream_between_good_ones(ctx):
    sizes = [0, 65536, 1, 40000, 17, 65535, 300, 9000, 64, 65, 20000, 5]
    cases = []
    for k, n in enumerate(sizes):
        data = dc.content(dc.CONTENT_KINDS[k % 4], n, 50 + k)
        s = dc.deflate(data, ("level6", "level1", "rle", "level9")[k % 4])
        cases.append(dc.Case(f"mixed/{n}", "mixed", s, n, *dc.classify(s, n)))
    good = cases[3]
    broken = bytearray(good.stream)
    broken[len(broken) // 2] ^= 0x04
    broken = bytes(broken)
    bad = dc.Case("mixed/broken", "mixed", broken, good.capacity, *dc.classify(broken, good.capacity))
    assert bad.status != dc.OK or bad.output != good.output
    cases.insert(4, bad)
    src, so, dst, do = layout(cases)
    check(cases, dst, do, *ctx.inflate_batch_raw(src, so, dst, do))


# ---------------------------------------------------------------------------------------------- CRC-32
def test_crc32_on_the_device(ctx):
    big = next(c for c in dc.CASES if c.name == "zlib/one_megabyte_several_blocks")
    cases = dc.CRC_CASES + [big]
    assert [len(c.output) for c in cases] == list(dc.CRC_SIZES) + [1048576]
    outs, crcs, statuses, _ = ctx.inflate_batch([c.stream for c in cases], [c.capacity for c in cases])
    assert statuses == [0] * len(cases) and outs == [c.output for c in cases]
    assert crcs == [zlib.crc32(c.output) for c in cases]


# ---------------------------------------------------------------------------------------------- threads
def test_two_threads_on_two_contexts():
    from gkl_amd import native
    picks = [[c for c in dc.CASES if len(c.stream) < 4096][i::2][::9] for i in (0, 1)]
    errors = []

    def work(cases):
        try:
            with native.InflateContext(device=0) as c:
                for _ in range(50):
                    src, so, dst, do = layout(cases)
                    check(cases, dst, do, *c.inflate_batch_raw(src, so, dst, do))
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(p,)) for p in picks]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(len(p) > 20 and len({c.status for c in p}) >= 4 for p in picks)

"""The input list of the deflate tests (tests/test_deflate_core_cpu.py on the host core, tests/test_deflate.py on the
GPU): deterministic, seeded, each entry (name, bytes).  Also the file formats of tests/native/deflate_core_check.cpp and
the settings the list is run under."""
import gzip
import io
import os
import random
import struct
import zlib

import numpy as np

from tests import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = os.path.join(ROOT, "tests", "golden", "HiSeq.1mb.1RG.2k_lines.bam")
BLOCK_LEN = 65535   # gkldef::kBlockLen
STORED, FIXED, DYNAMIC = 1, 2, 4

# (name, level, strategy, block-type mask)
SETTINGS = (("default", 1, 0, 0), ("huffman_only", 1, 1, 0), ("fixed", 1, 0, FIXED), ("dynamic", 1, 0, DYNAMIC),
            ("stored", 1, 0, STORED), ("level0", 0, 0, 0))


def fixture_payload() -> bytes:
    with open(BAM, "rb") as f:
        data = gzip.GzipFile(fileobj=io.BytesIO(f.read())).read()
    assert len(data) == 717156
    return data


def _rand(rng, n, symbols=256) -> bytes:
    return rng.integers(0, symbols, n, dtype=np.uint8).tobytes()


def _build():
    rng = np.random.default_rng(20261021)
    out = []
    seen = set()
    for c in dc.CASES:   # the distinct outputs of the inflate case list, the 1 MB one included
        if c.output not in seen:
            seen.add(c.output)
            out.append((f"case_output_{len(seen)}", c.output))
    assert len(out) == 459
    text = _rand(rng, 400, 7)
    for n in (0, 1, 2, 3, 4, 5):
        out.append((f"len_{n}", b"abcab"[:n]))
    for n in (63, 64, 65, 127, 128, 129):   # chunk seams
        out.append((f"chunk_seam_{n}", (text * 2)[:n]))
    long_text = (_rand(rng, 3000, 12) * 50)
    for n in (BLOCK_LEN - 1, BLOCK_LEN, BLOCK_LEN + 1, 2 * BLOCK_LEN + 1):   # block seams
        out.append((f"block_seam_{n}", long_text[:n]))
    for n in (258, 259, 260, 261, 517, 65280):   # runs: the maximum match, distance 1, overlap
        out.append((f"run_{n}", b"\x5a" * n))
    for p in (2, 3, 4, 5, 63, 64, 65):
        out.append((f"period_{p}", (_rand(rng, p) * (2000 // p + 2))[:2000]))
    for half in (32767, 32768, 32769):   # a distance of exactly 32768 is legal, 32769 is not; the far half crosses a block
        h = _rand(rng, half)
        out.append((f"distance_{half}", h + h))
    head = _rand(rng, 500)
    out.append(("match_ends_on_last_byte", head + _rand(rng, 40) + head[100:140]))
    out.append(("candidate_runs_past_end", head + head[200:205]))
    for n in (4, 300, 65280):   # the last is the stored fallback: out_len == len + 5
        out.append((f"random_{n}", _rand(rng, n)))
    for k in (4, 16):
        out.append((f"skewed_{k}_symbols", _rand(rng, 65280, k)))
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    buf = bytearray(b"".join(bytes([40 + i]) * f for i, f in enumerate(fib)))   # 121392 bytes: Huffman-only needs 15-bit limiting
    random.Random(7).shuffle(buf)
    out.append(("fibonacci_counts", bytes(buf)))
    out.append(("all_values_once", bytes(range(256))))
    eq = bytearray(bytes(range(256)) * 16)
    random.Random(8).shuffle(eq)
    out.append(("all_values_equal", bytes(eq)))
    payload = fixture_payload()
    for cut in (65280, 65498):
        for i in range(0, len(payload), cut):
            out.append((f"fixture_{cut}_{i // cut}", payload[i:i + cut]))
    return out


INPUTS = _build()


def bound(n: int) -> int:
    """gklhip_deflate_bound, written out: the stored size."""
    return n + 5 * max(1, -(-n // BLOCK_LEN))


def roomy(n: int) -> int:
    """A capacity no setting overflows: fixed codes cost at most 9 bits a byte, a dynamic header under 300 bytes a block."""
    return n + n // 8 + 400 * max(1, -(-n // BLOCK_LEN))


def input_file(inputs, capacities) -> bytes:
    """The INPUTS file of `deflate_core_check run`."""
    parts = [struct.pack("<I", len(inputs))]
    for data, cap in zip(inputs, capacities):
        parts.append(struct.pack("<II", len(data), cap) + data)
    return b"".join(parts)


def parse_results(blob: bytes, n: int):
    """[(status, stream, crc32 of the input)] of `deflate_core_check run`'s RESULTS file."""
    res, at = [], 0
    for _ in range(n):
        status, out_len, crc = struct.unpack_from("<iiI", blob, at)
        at += 12
        res.append((status, blob[at:at + out_len], crc))
        at += out_len
    assert at == len(blob)
    return res


def round_trip_fault(name, data, stream):
    """None, or what is wrong with `stream` as the raw-deflate stream of `data`."""
    z = zlib.decompressobj(-15)
    try:
        got = z.decompress(stream)
    except zlib.error as e:
        return f"{name}: zlib refuses the stream: {e}"
    if got != data:
        return f"{name}: inflates to {len(got)} bytes that differ from the {len(data)} of the input"
    if not z.eof or z.unused_data:
        return f"{name}: eof {z.eof}, {len(z.unused_data)} unused bytes"
    return None

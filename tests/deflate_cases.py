"""The one list of raw-deflate cases that the host check of the decoder core (test_inflate_core_cpu.py) and the GPU tests
(test_inflate.py) share.  Every case's expected status, bytes and consumed count come from Python's zlib
(`zlib.decompressobj(-15).decompress(stream, capacity + 1)`); the streams zlib's compressor never emits are put together
bit by bit with the small assembler below, and are classified by the same oracle when the list is built."""
import random
import zlib
from collections import namedtuple

OK, INVALID_BLOCK, INVALID_SYMBOL, INVALID_LOOKBACK, END_INPUT, OUT_OVERFLOW = range(6)
STATUS_NAMES = ("OK", "INVALID_BLOCK", "INVALID_SYMBOL", "INVALID_LOOKBACK", "END_INPUT", "OUT_OVERFLOW")

_MESSAGES = {
    "invalid block type": INVALID_BLOCK, "invalid stored block lengths": INVALID_BLOCK,
    "too many length or distance symbols": INVALID_BLOCK, "invalid code lengths set": INVALID_BLOCK,
    "invalid bit length repeat": INVALID_BLOCK, "invalid code -- missing end-of-block": INVALID_BLOCK,
    "invalid literal/lengths set": INVALID_BLOCK, "invalid distances set": INVALID_BLOCK,
    "invalid literal/length code": INVALID_SYMBOL, "invalid distance code": INVALID_SYMBOL,
    "invalid distance too far back": INVALID_LOOKBACK,
}

# name, family, the stream, the output capacity, and what the oracle says: status, the valid prefix of the output,
# input bytes consumed (None where the status leaves it open: every error and OUT_OVERFLOW)
Case = namedtuple("Case", "name family stream capacity status output consumed")


# ---------------------------------------------------------------------------------------------- the oracle
def _raises(stream, max_length=0):
    try:
        zlib.decompressobj(-15).decompress(stream, max_length)
    except zlib.error as e:
        for text, status in _MESSAGES.items():
            if text in str(e):
                return status
        raise AssertionError(f"the oracle's message is not in the table: {e}")
    return None


def _error_prefix(stream):
    """The bytes zlib wrote before it met the error of `stream`: the output of the longest prefix of the input that
    does not raise, confirmed by the smallest output limit at which the whole stream raises."""
    lo, hi = 0, len(stream)   # stream[:lo] passes, stream[:hi] raises
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _raises(stream[:mid]) is None:
            lo = mid
        else:
            hi = mid
    out = zlib.decompressobj(-15).decompress(stream[:lo])
    # With a limit of m bytes zlib reaches an error iff it lies before the write of byte m + 1 -- except a distance too far
    # back, which it only looks for once the match has room for a byte (inflate.c, case MATCH).  So the smallest limit that
    # raises is the prefix length (or 1 for an empty prefix), plus 1 for that one error.
    late = 1 if _raises(stream) == INVALID_LOOKBACK else 0
    lo_m, hi_m = 0, max(len(out) + late, 1)   # hi_m raises
    assert _raises(stream, hi_m) is not None, "the error lies in the input byte that also completes an output byte"
    while hi_m - lo_m > 1:
        mid = (lo_m + hi_m) // 2
        if _raises(stream, mid) is None:
            lo_m = mid
        else:
            hi_m = mid
    assert hi_m == max(len(out) + late, 1), "the oracle cannot say where the valid prefix ends"
    return out


def classify(stream, capacity):
    """(status, valid prefix, consumed) of one stream with room for `capacity` bytes, by the oracle."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, capacity + 1)
    except zlib.error:
        status = _raises(stream, capacity + 1)
        out = _error_prefix(stream)
        # an error right behind byte capacity + 1 would be OUT_OVERFLOW in stream order: no case may sit there
        assert len(out) <= capacity, "ambiguous case: the error follows the first byte that does not fit"
        return status, out, None
    if len(out) == capacity + 1:
        return OUT_OVERFLOW, out[:capacity], None
    if d.eof:
        return OK, out, len(stream) - len(d.unused_data)
    return END_INPUT, out, len(stream)


# ---------------------------------------------------------------------------------------------- bit-level assembler
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):   # LSB first
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code_len):   # a Huffman code goes in MSB first
        code, length = code_len
        self.put(int(format(code, f"0{length}b")[::-1], 2) if length else 0, length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths."""
    codes, code = {}, 0
    for length in range(1, 16):
        for sym, l in enumerate(lens):
            if l == length:
                codes[sym] = (code, length)
                code += 1
        code <<= 1
    return codes


LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# complete sets over every symbol a dynamic block may use
FULL_LIT = [8] * 226 + [9] * 60
FULL_DIST = [4] * 2 + [5] * 28
PLAIN_CL = [4] * 13 + [5] * 6   # a complete code-length code with every symbol in it


def match(length, dist):
    """The token of a match, with the symbols zlib's tables give it."""
    ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
    ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return ("L", ls, length - LEN_BASE[ls], ds, dist - DIST_BASE[ds])


def tokens_to(b, tokens, lit_lens, dist_lens, eob=True):
    """Tokens: an int is a literal; ("L", length symbol - 257, extra, distance symbol, extra) a match by its raw symbols
    (extra bits of symbols 30 / 31 are not written); ("S", symbol) one raw literal/length symbol."""
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            b.huff(lit[t])
        elif t[0] == "S":
            b.huff(lit[t[1]])
        else:
            _, ls, le, ds, de = t
            b.huff(lit[257 + ls])
            b.put(le, LEN_EXTRA[ls])
            b.huff(dist[ds])
            if ds < 30:
                b.put(de, DIST_EXTRA[ds])
    if eob:
        b.huff(lit[256])


def fixed_block(b, tokens, final=True, eob=True):
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    tokens_to(b, tokens, FIXED_LIT, FIXED_DIST, eob)


def stored_block(b, data, final=True, nlen=None):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    b.out += data


def dynamic_header(b, hlit, hdist, cl_lens, seq, hclen=19, final=True):
    """seq: (code-length symbol, extra-bits value) in stream order."""
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens[CL_ORDER[i]], 3)
    codes = canonical(cl_lens)
    for sym, extra in seq:
        b.huff(codes[sym])
        if sym >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[sym])


def dynamic_block(b, tokens, lit_lens=FULL_LIT, dist_lens=FULL_DIST, final=True, eob=True):
    """A dynamic block whose header spells every code length out (no repeat codes)."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    lit_lens += [0] * (257 - len(lit_lens))
    dynamic_header(b, len(lit_lens), len(dist_lens), PLAIN_CL, [(l, 0) for l in lit_lens + dist_lens], final=final)
    tokens_to(b, tokens, lit_lens, dist_lens, eob)


# ---------------------------------------------------------------------------------------------- content
def content(kind, n, seed=7):
    if kind == "random":
        return random.Random(seed * 1000 + n).randbytes(n)
    if kind == "zeros":
        return bytes(n)
    if kind == "period3":
        return (b"abc" * (n // 3 + 1))[:n]
    words = [b"read", b"chr1", b"ACGTTGCA", b"GGATCC", b"\t", b"60", b"101M", b"=", b"NM:i:0", b"FFFFFJJJJ", b"\n", b"HISEQ:1:"]
    r, out = random.Random(seed * 77 + n), bytearray()
    while len(out) < n:
        out += r.choice(words)
    return bytes(out[:n])


CONTENT_KINDS = ("random", "zeros", "period3", "text")
ZLIB_MODES = {"level0": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY),
              "level9": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "rle": (6, zlib.Z_RLE),
              "huffman": (6, zlib.Z_HUFFMAN_ONLY)}


def deflate(data, mode="level6"):
    level, strategy = ZLIB_MODES[mode]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


# ---------------------------------------------------------------------------------------------- the list
def _build():
    cases = []

    def add(family, name, stream, capacity=None, expect=None, says=None):
        stream = bytes(stream)
        if capacity is None:   # exact for a stream that ends well, roomy otherwise
            try:
                capacity = len(zlib.decompressobj(-15).decompress(stream))
            except zlib.error:
                capacity = 1 << 16
        status, out, consumed = classify(stream, capacity)
        # every assembled case is first shown to mean what it claims
        if expect is not None:
            assert status == expect, (name, STATUS_NAMES[status], STATUS_NAMES[expect])
        if says is not None:
            assert status == OK and out == says, name
        cases.append(Case(f"{family}/{name}", family, stream, capacity, status, out, consumed))

    def one(build, *a, **kw):
        b = Bits()
        build(b, *a, **kw)
        return b.bytes()

    rnd = random.Random(20240521)

    # ---- stored blocks
    for n in (0, 1, 65535):
        data = content("random", n)
        add("stored", f"{n}_bytes", one(stored_block, data), says=data)
    for phase in range(8):   # an empty stored block behind a fixed block whose end falls on every bit phase
        k = (phase - 2) % 8   # header 3 + 'A' 8 + end-of-block 7 bits end at phase 2; every 9-bit literal moves it by one
        b = Bits()
        fixed_block(b, [65] + [200] * k, final=False)
        assert b.n == phase
        stored_block(b, b"", final=False)
        fixed_block(b, [66])
        add("stored", f"empty_at_phase_{phase}", b.bytes(), says=b"A" + b"\xc8" * k + b"B")
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    flushed = c.compress(b"first part ") + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(b"second part ") + c.flush(zlib.Z_FULL_FLUSH) + \
        c.compress(b"third part") + c.flush()
    add("stored", "sync_and_full_flush", flushed, says=b"first part second part third part")
    add("stored", "nlen_mismatch", one(stored_block, b"abc", nlen=0x1234), expect=INVALID_BLOCK)
    add("stored", "block_type_3", bytes([0x07]), expect=INVALID_BLOCK)

    # ---- fixed blocks
    add("fixed", "immediate_eob", bytes([0x03, 0x00]), says=b"")
    add("fixed", "all_literals", one(fixed_block, list(range(256))), says=bytes(range(256)))
    seed = list(content("random", 300, 3))
    for ls in range(29):
        for le in {0, (1 << LEN_EXTRA[ls]) - 1}:
            add("fixed", f"length_symbol_{257 + ls}_extra_{le}", one(fixed_block, seed + [("L", ls, le, 10, 1)]), expect=OK)
    far = list(content("random", 32768, 4))
    for ds in range(30):
        for de in {0, (1 << DIST_EXTRA[ds]) - 1}:
            add("fixed", f"distance_symbol_{ds}_extra_{de}", one(fixed_block, far + [("L", 2, 0, ds, de)]), expect=OK)
    for sym in (286, 287):
        add("fixed", f"length_symbol_{sym}", one(fixed_block, [1, 2, 3, ("S", sym)]), expect=INVALID_SYMBOL)
    for ds in (30, 31):
        add("fixed", f"distance_symbol_{ds}", one(fixed_block, [1, 2, 3, ("L", 0, 0, ds, 0)]), expect=INVALID_SYMBOL)

    # ---- match copies
    base = list(content("random", 259, 5))
    for dist in (1, 2, 3, 63, 64, 65, 257, 258, 259):
        for length in (3, 64, 65, 258):
            add("match", f"dist_{dist}_len_{length}", one(fixed_block, base + [match(length, dist), 7]), expect=OK)
    for dist in (32767, 32768):
        body = list(content("random", dist, dist))
        add("match", f"dist_{dist}_behind_as_much", one(fixed_block, body + [match(5, dist)]), expect=OK)
        add("match", f"dist_{dist}_behind_one_less", one(fixed_block, body[1:] + [match(5, dist)]), expect=INVALID_LOOKBACK)
    add("match", "first_token", one(fixed_block, [match(3, 1)]), expect=INVALID_LOOKBACK)
    big = content("text", 65536 + 700, 9)
    b = Bits()
    stored_block(b, big[:40000], final=False)
    stored_block(b, big[40000:], final=False)
    fixed_block(b, [match(258, 32768), 1, match(258, 32768)])
    add("match", "max_distance_behind_64k", b.bytes(), expect=OK)

    # ---- dynamic headers
    text = list(b"GATTACA" * 5)
    add("dynamic", "plain_hclen_19", one(dynamic_block, text + [match(20, 7)]), expect=OK)
    b = Bits()   # HCLEN 4: only 16, 17, 18 and 0 have a code, so no literal can: no end-of-block code
    cl = [0] * 19
    for s in (16, 17, 18, 0):
        cl[s] = 2
    dynamic_header(b, 257, 1, cl, [(18, 127), (18, 109)], hclen=4)
    add("dynamic", "hclen_4", b.bytes() + b"\0\0", expect=INVALID_BLOCK)
    chain = [0] * 258
    for i in range(14):
        chain[65 + i] = i + 1
    chain[256] = chain[257] = 15
    dchain = list(range(1, 16)) + [15]
    long_codes = [65, 66, 70, 78, 78, 77, ("L", 0, 0, 0, 0), ("L", 0, 0, 15, 3), ("L", 0, 0, 14, 0), 72]   # 15-bit codes of both sets
    b = Bits()
    stored_block(b, content("random", 300, 6), final=False)
    dynamic_block(b, long_codes, chain, dchain)
    long_stream = b.bytes()
    add("dynamic", "max_length_15", long_stream, expect=OK)

    def header_case(name, seq, hlit=257, hdist=1, expect=None, tail=b"\0\0\0\0"):
        b = Bits()
        dynamic_header(b, hlit, hdist, PLAIN_CL, seq)
        add("dynamic", name, b.bytes() + tail, expect=expect)

    header_case("repeat_16_first", [(16, 0)] + [(8, 0)] * 260, expect=INVALID_BLOCK)
    # 16 running across the literal/distance boundary: end-of-block and symbol 257 have length 1, so have both distance codes
    b = Bits()
    stored_block(b, b"abc", final=False)
    dynamic_header(b, 258, 2, PLAIN_CL, [(18, 127), (18, 107), (1, 0), (16, 0)])
    tokens_to(b, [("L", 0, 0, 0, 0)], [0] * 256 + [1, 1], [1, 1])
    add("dynamic", "repeat_16_across_boundary", b.bytes(), says=b"abcccc")
    # 18 with 138 repeats, the rest spelled out; no distance code
    late = [0] * 138 + [6] * 9 + [7] * 110
    b = Bits()
    dynamic_header(b, 257, 1, PLAIN_CL, [(18, 127)] + [(l, 0) for l in late[138:]] + [(0, 0)])
    tokens_to(b, [140, 200, 255], late, [0])
    add("dynamic", "code_18_138_repeats", b.bytes(), says=bytes([140, 200, 255]))
    header_case("repeat_overshoots", [(18, 127), (18, 127)], expect=INVALID_BLOCK)
    one_dist = one(dynamic_block, text + [("L", 0, 0, 0, 0)], FULL_LIT, [1])
    add("dynamic", "one_distance_code_of_length_1", one_dist, expect=OK)
    b = Bits()   # the other pattern of that incomplete set: distance bit 1
    dynamic_header(b, 286, 1, PLAIN_CL, [(l, 0) for l in FULL_LIT + [1]])
    lit = canonical(FULL_LIT)
    b.huff(lit[65]); b.huff(lit[257]); b.put(1, 1)
    add("dynamic", "unused_pattern_of_one_distance_code", b.bytes() + b"\0\0", expect=INVALID_SYMBOL)
    add("dynamic", "no_distance_code_literals_only", one(dynamic_block, text, FULL_LIT, [0]), expect=OK)
    b = Bits()
    dynamic_header(b, 286, 1, PLAIN_CL, [(l, 0) for l in FULL_LIT + [0]])
    b.huff(lit[65]); b.huff(lit[257]); b.put(0, 1)
    add("dynamic", "no_distance_code_match", b.bytes() + b"\0\0", expect=INVALID_SYMBOL)
    no_eob = list(FULL_LIT)
    no_eob[256] = 0
    header_case("missing_eob", [(l, 0) for l in no_eob + [1]], hlit=286, expect=INVALID_BLOCK)
    header_case("oversubscribed_literals", [(l, 0) for l in [7] * 257 + [1]], expect=INVALID_BLOCK)
    header_case("incomplete_literals", [(l, 0) for l in [9] * 257 + [1]], expect=INVALID_BLOCK)
    header_case("oversubscribed_distances", [(l, 0) for l in FULL_LIT + [1, 1, 1]], hlit=286, hdist=3, expect=INVALID_BLOCK)
    header_case("incomplete_distances", [(l, 0) for l in FULL_LIT + [2, 2]], hlit=286, hdist=2, expect=INVALID_BLOCK)
    header_case("hlit_287", [(8, 0)] * 300, hlit=287, expect=INVALID_BLOCK)
    header_case("hdist_31", [(8, 0)] * 300, hdist=31, expect=INVALID_BLOCK)
    b = Bits()   # no code-length code at all: zlib reads every pattern as length 0, then misses the end-of-block code
    dynamic_header(b, 257, 1, [0] * 19, [])
    add("dynamic", "empty_code_length_code", b.bytes() + b"\0" * 40, expect=INVALID_BLOCK)
    b = Bits()
    dynamic_header(b, 257, 1, [1] + [0] * 18, [])
    add("dynamic", "incomplete_code_length_code", b.bytes() + b"\0" * 40, expect=INVALID_BLOCK)

    # ---- zlib's own output
    for mode in ZLIB_MODES:
        for i, n in enumerate((0, 1, 63, 64, 65, 65279, 65536)):
            kinds = CONTENT_KINDS if n <= 65 else (CONTENT_KINDS[(i + len(mode)) % 4],)
            for kind in kinds:
                data = content(kind, n)
                add("zlib", f"{mode}_{kind}_{n}", deflate(data, mode), says=data)
    for kind in CONTENT_KINDS:
        for mode in ("level6", "rle"):
            data = content(kind, 65536, 11)
            add("zlib", f"{mode}_{kind}_65536_b", deflate(data, mode), says=data)
    mb = content("text", 700000, 13) + content("random", 100000, 13) + content("period3", 248576, 13)
    add("zlib", "one_megabyte_several_blocks", deflate(mb, "level6"), says=mb)

    # ---- capacity
    lit_stream = one(fixed_block, list(b"0123456789"))
    match_stream = one(fixed_block, list(b"0123") + [match(12, 4)])
    add("capacity", "exact", lit_stream, 10, expect=OK)
    add("capacity", "one_short_at_a_literal", lit_stream, 9, expect=OUT_OVERFLOW)
    add("capacity", "one_short_inside_a_match", match_stream, 15, expect=OUT_OVERFLOW)
    add("capacity", "short_in_the_middle_of_a_match", match_stream, 9, expect=OUT_OVERFLOW)
    add("capacity", "zero_with_output", lit_stream, 0, expect=OUT_OVERFLOW)
    add("capacity", "zero_without_output", bytes([0x03, 0x00]), 0, expect=OK)
    add("capacity", "stored_one_short", one(stored_block, b"abcdefgh"), 7, expect=OUT_OVERFLOW)
    add("capacity", "trailing_bytes_are_not_an_error", lit_stream + b"trailer", 10, expect=OK)
    add("capacity", "empty_input", b"", 8, expect=END_INPUT)

    # ---- truncation: every prefix of three short streams, one per block type
    short_text = b"to be or not to be, that is the question; to be or not"
    for kind, whole in (("stored", one(stored_block, short_text[:20])), ("fixed", deflate(short_text, "fixed")),
                        ("dynamic", one(dynamic_block, list(short_text[:20]) + [match(9, 13)], FULL_LIT, FULL_DIST))):
        full = zlib.decompressobj(-15).decompress(whole)
        for cut in range(len(whole)):
            add("truncation", f"{kind}_{cut}_of_{len(whole)}", whole[:cut], len(full), expect=END_INPUT)

    # ---- mutation: 300 seeded single-bit and single-byte changes of valid streams under 2 KB
    bases = [deflate(content("text", 3000, 21), "level9"), deflate(content("text", 1500, 22), "fixed"),
             one(stored_block, content("random", 40, 23), final=False) + deflate(content("period3", 900, 24) + content("random", 300, 24), "level6"),
             one_dist, long_stream]
    assert all(len(s) < 2048 and classify(s, 1 << 16)[0] == OK for s in bases)
    n_mut = 0
    while n_mut < 300:
        which = rnd.randrange(len(bases))
        s = bytearray(bases[which])
        at = rnd.randrange(len(s))
        if rnd.random() < 0.5:
            s[at] ^= 1 << rnd.randrange(8)
            how = "bit"
        else:
            s[at] = (s[at] + rnd.randrange(1, 256)) & 255
            how = "byte"
        add("mutation", f"{n_mut}_base{which}_{how}_at_{at}", s, 1 << 16)
        n_mut += 1
    return cases


CASES = _build()
FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))
# the output sizes the CRC-32 is compared at
CRC_SIZES = (0, 1, 63, 64, 65, 4095, 65535, 65536)
CRC_CASES = [Case(f"crc/{n}", "crc", s, n, *classify(s, n)) for n in CRC_SIZES for s in (deflate(content("text", n, 31), "level1"),)]


def case_file(cases):
    """The cases in the form tests/native/inflate_core_check.cpp reads."""
    import struct
    out = bytearray(struct.pack("<I", len(cases)))
    for c in cases:
        out += struct.pack("<II", len(c.stream), c.capacity) + c.stream
    return bytes(out)


def parse_results(blob, n):
    """What inflate_core_check writes: [(status, output, consumed, crc32)] of n streams."""
    import struct
    at, res = 0, []
    for _ in range(n):
        status, out_len, consumed, crc = struct.unpack_from("<iiiI", blob, at)
        at += 16
        res.append((status, bytes(blob[at:at + out_len]), consumed, crc))
        at += out_len
    assert at == len(blob)
    return res


def mismatch(case, status, output, consumed, crc):
    """None if one stream's results are the oracle's, else what differs.  `output` is the valid prefix."""
    if status != case.status:
        return f"{case.name}: status {STATUS_NAMES[status]}, the oracle says {STATUS_NAMES[case.status]}"
    if len(output) != len(case.output):
        return f"{case.name}: {len(output)} bytes, the oracle wrote {len(case.output)}"
    if output != case.output:
        return f"{case.name}: bytes differ from the oracle's"
    if case.consumed is not None and consumed != case.consumed:
        return f"{case.name}: consumed {consumed}, the oracle {case.consumed}"
    if crc is not None and crc != zlib.crc32(case.output):
        return f"{case.name}: CRC-32 {crc:08x}, zlib.crc32 says {zlib.crc32(case.output):08x}"
    return None

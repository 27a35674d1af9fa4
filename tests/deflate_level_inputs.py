"""Inputs that reach the paths of deflate levels 3-8 (gkl_amd/csrc/deflate_core.h, tokenize_chains): 3-byte matches near
and far, lazy triggers at fixed chunk offsets, candidates in the lane's own chunk, chains longer than any depth, the
link ring's wrap, colliding keys, the distance limit and a block seam.  Deterministic and seeded, each (name, bytes),
in the format of tests/deflate_inputs.INPUTS, whose file formats and helpers the tests share."""
import numpy as np

BLOCK_LEN = 65535     # gkldef::kBlockLen
HASH_BITS = 13        # gkldef::kHashBits
FAR3 = 4096           # gkldef::kFar3
LAZY_OFFSETS = (0, 31, 62, 63)
LEVELS = {3: (4, 32, False), 4: (8, 32, True), 5: (16, 64, True), 6: (32, 128, True), 7: (64, 258, True), 8: (128, 258, True)}   # depth, nice, lazy


def hash3(b: bytes) -> int:
    """gkldef::hash3 of the three bytes at b[0:3]."""
    v = b[0] | (b[1] << 8) | (b[2] << 16)
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def repeated_trigrams(data: bytes, window: int) -> int:
    """The positions whose three bytes also start at most `window` positions earlier."""
    last, n = {}, 0
    for i in range(len(data) - 2):
        t = data[i:i + 3]
        j = last.get(t)
        n += j is not None and i - j <= window
        last[t] = i
    return n


def _rand(rng, n) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _seeded(make, designed, window, seed):
    """make(rng) from the first seed at or after `seed` whose input repeats only the trigrams it was designed to."""
    while True:
        data = make(np.random.default_rng(seed))
        if repeated_trigrams(data, window) == designed:
            return data
        seed += 1


def three_byte_near(rng) -> bytes:
    """150 x (3 bytes, 5 others, the same 3 bytes, a byte that ends the match, 6 others): repeats at distance 8."""
    out = bytearray()
    for _ in range(150):
        t = _rand(rng, 3)
        out += t + _rand(rng, 5) + t + _rand(rng, 7)
    return bytes(out)


def three_byte_far(rng) -> bytes:
    """6000 bytes, then 150 x (3 of them from 5250 or more back, a byte that differs from their successor, one other)."""
    a = _rand(rng, 6000)
    out = bytearray(a)
    for k in range(150):
        out += a[10 * k:10 * k + 3] + bytes([a[10 * k + 3] ^ 0xFF]) + _rand(rng, 1)
    return bytes(out)


def lazy_trigger(rng, offset: int, triggers: int = 24) -> bytes:
    """Per 256 bytes: `abcd` + z at 0, q + `bcdefghijk` at 20, and `a` + `bcdefghijk` at 128 + offset -- a 4-byte match at
    chunk offset `offset` whose successor has a 10-byte match."""
    out = bytearray()
    for _ in range(triggers):
        seg = bytearray(_rand(rng, 256))
        x, tail = _rand(rng, 4), _rand(rng, 7)
        y = x[1:] + tail
        seg[0:4] = x
        seg[4] = tail[0] ^ 0xFF
        seg[20] = x[0] ^ 0xFF
        seg[21:31] = y
        p = 128 + offset
        seg[p] = x[0]
        seg[p + 1:p + 11] = y
        out += seg
    return bytes(out)


LAZY_DESIGNED = 10   # repeated trigrams per trigger: `bcd` at 21, then the nine from `abc` to `ijk`


def chain_of_300(rng) -> bytes:
    """One 4-byte prefix 301 times, each with a 4-byte tail of its own.  The last shares two tail bytes with the first,
    300 back (its longest match, 6 bytes), one with number 200 (5 bytes) and none with the others (4 bytes).  The
    shared part is shorter than 3 bytes, so no chain but the prefix's leads to it."""
    prefix, tail = _rand(rng, 4), _rand(rng, 2)
    out = bytearray()
    for k in range(301):
        if k in (0, 300):
            out += prefix + tail + k.to_bytes(2, "little")
        elif k == 200:
            out += prefix + tail[:1] + bytes([tail[1] ^ 0xFF]) + k.to_bytes(2, "little")
        else:
            out += prefix + bytes([tail[0] ^ (1 + k % 255)]) + k.to_bytes(2, "little") + _rand(rng, 1)
    return bytes(out)


def key_every_4096(rng) -> bytes:
    """A full block of random bytes with one 4-byte key at every multiple of 4096: at 61440 the chain's 8th candidate
    is 32768 back, and its ring slot is the one 61440 itself has just written."""
    out = bytearray(_rand(rng, BLOCK_LEN))
    key = _rand(rng, 4)
    for at in range(0, BLOCK_LEN - 4, 4096):
        out[at:at + 4] = key
    return bytes(out)


def colliding_keys():
    """Two 4-byte keys whose first three bytes differ and share a hash slot (the first pair in counting order)."""
    seen = {}
    for v in range(1 << 24):
        k = v.to_bytes(3, "little")
        h = hash3(k)
        if h in seen:
            return seen[h] + b"\x11", k + b"\x22"
        seen[h] = k
    raise AssertionError("no collision")


def interleaved_collision(rng) -> bytes:
    a, b = colliding_keys()
    out = bytearray()
    for _ in range(40):
        out += a + _rand(rng, 4) + b + _rand(rng, 4)
    return bytes(out)


def at_distance(rng, near: bool, far: bool) -> bytes:
    """A position 32 769 whose next 8 bytes also stand 32 768 back (`near`), 32 769 back (`far`) or, as nine equal
    bytes from 0, both."""
    out = bytearray(_rand(rng, 32769 + 40))
    p = 32769
    if near and far:
        out[0:9] = b"\xAB" * 9
        out[9] = 0x01
        out[p:p + 8] = b"\xAB" * 8
        out[p - 1], out[p + 8] = 0x02, 0x03
    else:
        pre = _rand(rng, 8)
        at = p - 32768 if near else p - 32769
        out[at:at + 8] = pre
        out[p:p + 8] = pre
    return bytes(out)


def repeat_over_block_seam(rng) -> bytes:
    """40 bytes that start 10 bytes before the end of the first block, and once more in the second."""
    r = _rand(rng, 40)
    return _rand(rng, BLOCK_LEN - 10) + r + _rand(rng, 5) + r + _rand(rng, 20)


def _build():
    out = [("three_byte_near", _seeded(three_byte_near, 150, 1 << 20, 100)),
           ("three_byte_far", _seeded(three_byte_far, 0, FAR3, 200))]
    for o in LAZY_OFFSETS:
        out.append((f"lazy_trigger_{o}", _seeded(lambda rng, o=o: lazy_trigger(rng, o), 24 * LAZY_DESIGNED, 1 << 20, 300 + o)))
    rng = np.random.default_rng(20261022)
    for p in range(2, 8):
        out.append((f"own_chunk_period_{p}", (_rand(rng, p) * 80)[:150]))
    out.append(("chain_of_300", chain_of_300(rng)))
    out.append(("key_every_4096", key_every_4096(rng)))
    out.append(("interleaved_collision", interleaved_collision(rng)))
    out.append(("at_distance_32768", at_distance(rng, True, False)))
    out.append(("at_distance_32769", at_distance(rng, False, True)))
    out.append(("at_distance_both", at_distance(rng, True, True)))
    out.append(("repeat_over_block_seam", repeat_over_block_seam(rng)))
    return out


INPUTS = _build()

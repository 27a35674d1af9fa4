"""Deterministic batches that drive the planned fp64 pass (plan_policy_kernel, plan_pack_kernel, plan_jobs_kernel and
the packed fp64 job kernel) through the branches its planner has, and the reference of the device finalisation.

A non-double call takes the planned pass when it has more than 65 536 pairs or a read too long for the per-pair
kernels (pairhmm_device_pass.h: plan_call).  Reads and haplotypes of a few tens of bases make a 100 000-pair call a
few 10^7 cells, so every batch here costs the CPU oracle a fraction of a second.

Fallback is made on purpose.  A read whose qualities, gap-open and gap-continuation penalties are all 100 .. 127 loses
ten or more decimal digits per base that does not match, so ten unmatched bases underflow fp32 (the policy's bar is
1e-28 on a sum scaled by 2^120: a likelihood below 7.5e-65) and stay far above the fp64 floor (2^1020 scaling).  Such a
read that is a copy of a piece of a haplotype is kept; against a haplotype that does not hold the piece it is flagged.

tests/test_pairhmm_planned_pass_cpu.py asserts, on the oracle's flags, that every batch has the property it is built
for; tests/test_pairhmm_planned_pass.py runs them on the GPU.
"""
from __future__ import annotations

import functools
import hashlib
import math

import numpy as np

from gkl_amd.batch import FlatBatch
from gkl_amd.synth import random_batch

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_ACG = np.frombuffer(b"ACG", dtype=np.uint8)

DIRECT_PAIRS = 65536       # kDirectPairs: calls above take the planned pass
HOST_SHARD_PAIRS = 400000  # kHostShardPairs: host calls from here on run as two half-batches
FORCING_READ_LEN = 512     # a read this long fits no per-pair kernel, whichever small-read limit is set
CHUNK_READ_LEN_MAX = 639   # the longest read a chunk of the packed fp64 pass holds (64 lanes x 10 rows - 1)
PACK_WINDOW = 96           # kPackWindow: reads per packing window
PACK_GRID_WAVES = 1024     # wavefronts of the packing launch's largest grid (64 blocks x 16)


# ---------------------------------------------------------------------------------------------- pieces
def _seq(rng, n, alpha=_ACGT):
    return alpha[rng.randint(0, alpha.size, size=int(n))]


def _quals(rng, n, lo, hi):
    return rng.randint(lo, hi + 1, size=int(n)).astype(np.uint8)


def _read(bases, q, ins, dele, gcp):
    n = bases.size
    full = lambda x: np.full(n, x, np.uint8) if np.isscalar(x) else np.asarray(x, np.uint8)  # noqa: E731
    return (np.asarray(bases, np.uint8), full(q), full(ins), full(dele), full(gcp))


def _sharp(rng, bases, lo=100, hi=127):
    """A read that loses >= 10 digits per base it cannot match: all four penalties in lo .. hi."""
    n = bases.size
    return _read(bases.copy(), _quals(rng, n, lo, hi), _quals(rng, n, lo, hi), _quals(rng, n, lo, hi), _quals(rng, n, lo, hi))


def _soft(rng, bases, q=(20, 30), sub=0.0):
    """A sequencer-like read: qualities q, gap-open 40 .. 45, gap-continuation 10, a fraction `sub` of bases replaced."""
    n = bases.size
    b = bases.copy()
    if sub > 0:
        flip = rng.random_sample(n) < sub
        b[flip] = _ACGT[(np.searchsorted(_ACGT, b[flip]) + 1 + rng.randint(0, 3, size=int(flip.sum()))) % 4]
    return _read(b, _quals(rng, n, q[0], q[1]), _quals(rng, n, 40, 45), _quals(rng, n, 40, 45), 10)


def _assemble(reads, haps, meta=None) -> FlatBatch:
    lens = [r[0].size for r in reads]
    assert min(lens) > 0 and min(h.size for h in haps) > 0
    read_off = np.zeros(len(reads) + 1, np.int64)
    read_off[1:] = np.cumsum(lens)
    hap_off = np.zeros(len(haps) + 1, np.int64)
    hap_off[1:] = np.cumsum([h.size for h in haps])
    cat = lambda k: np.ascontiguousarray(np.concatenate([r[k] for r in reads]), np.uint8)  # noqa: E731
    return FlatBatch(len(reads), len(haps), read_off, hap_off, cat(0), cat(1), cat(2), cat(3), cat(4),
                     np.ascontiguousarray(np.concatenate(haps), np.uint8), dict(meta or {}))


def stream_order(b: FlatBatch) -> np.ndarray:
    """Caller's haplotype index at every position of the haplotype stream (pairhmm_plan.cpp: by length, stable)."""
    return np.argsort(b.hap_lens, kind="stable")


# ---------------------------------------------------------------------------------------------- A: many reads, few haplotypes
def batch_a1(n_reads=120000, seed=101) -> FlatBatch:
    """120 000 unrelated reads of 20 .. 30 bases, qualities 60 .. 93, against ONE haplotype of 30: more than 1024
    packing windows (the packing grid has 1024 wavefronts), and a wavefront of the policy spans 64 reads."""
    rng = np.random.RandomState(seed)
    b = random_batch(rng, n_reads, 1, read_len=(20, 30), hap_len=(30, 30), qual_range=(60, 93), related=False)
    b.meta = {"case": "A1"}
    return b


def batch_a2(n_reads, n_haps, seed) -> FlatBatch:
    """n_haps of 3 or 5: every fail count 0 .. n_haps occurs in >= 1000 reads, and the pairs a read fails against lie
    anywhere among its n_haps (not a nested pattern).  Unrelated 30-base windows S_0 .. S_{n-1}; S_i is part of n - i of the
    haplotypes (chosen at random), a read is a sharp copy of 20 .. 30 bases of one window -- it fails against the i
    haplotypes without S_i -- or unrelated to all of them."""
    rng = np.random.RandomState(seed)
    segs = [_seq(rng, 30) for _ in range(n_haps)]
    member = np.zeros((n_haps, n_haps), bool)   # member[i, h]: haplotype h holds S_i
    member[0, :] = True
    for i in range(1, n_haps):
        member[i, rng.permutation(n_haps)[: n_haps - i]] = True
    haps = []
    for h in range(n_haps):
        mine = [i for i in rng.permutation(n_haps) if member[i, h]]
        haps.append(np.concatenate([segs[i] for i in mine]))
    reads, klass = [], rng.randint(0, n_haps + 1, size=n_reads)
    for r in range(n_reads):
        L = int(rng.randint(20, 31))
        if klass[r] == n_haps:
            reads.append(_sharp(rng, _seq(rng, L)))
        else:
            off = int(rng.randint(0, 30 - L + 1))
            reads.append(_sharp(rng, segs[klass[r]][off:off + L]))
    return _assemble(reads, haps, {"case": "A2", "klass": klass})


# ---------------------------------------------------------------------------------------------- B: histogram and scan width
_B_SHARE = (0.85, 0.08, 0.04, 0.03)   # graded shares of the four windows among the haplotypes


def batch_b(n_haps, n_reads, seed) -> FlatBatch:
    """n_haps of 1025 / 4094 / 4095 (one count per scan thread and the LDS histogram end at 1024 and 4094): haplotypes
    are prefixes of 20 .. 45 bases of four unrelated windows in graded shares, in random order.  A sharp read that is
    the first L bases of window w is kept against the haplotypes of w with at least L bases and flagged against all
    others, so read lengths of 10 .. 40 spread the fail counts over the range; a soft short read fails nowhere, a sharp
    unrelated one everywhere."""
    rng = np.random.RandomState(seed)
    wins = [_seq(rng, 45) for _ in _B_SHARE]
    which = rng.choice(len(wins), size=n_haps, p=_B_SHARE)
    haps = [wins[w][: int(rng.randint(20, 46))] for w in which]
    reads = [_read(wins[0][:10].copy(), 8, 45, 45, 10),   # fails nowhere
             _sharp(rng, _seq(rng, 36))]                  # fails everywhere
    lens0 = (10, 22, 27, 31, 34, 37, 39, 40)
    plan = [(0, L) for L in lens0] + [(1, 12), (1, 30), (1, 40), (2, 15), (2, 35), (3, 20), (3, 38)]
    for k in range(n_reads - 2):
        w, L = plan[k % len(plan)]
        if k >= len(plan):
            L = int(rng.randint(10, 41))
        reads.append(_sharp(rng, wins[w][:L]))
    return _assemble(reads, haps, {"case": "B"})


# ---------------------------------------------------------------------------------------------- C: run detection
def c_family_of_position(pos: int) -> int:
    """Family (0 A, 1 B, 2 C) of the haplotype at stream position pos: B at 62 and 63, all of 64 .. 127 are A."""
    if pos < 62:
        return pos % 3
    if pos < 64:
        return 1
    if pos < 128:
        return 0
    return 1 + pos % 2


C_READ_FAMILIES = (0, 1, 2, 3)   # the reads of a call: copies of window A / B / C, or (3) unrelated to all


def batch_c(n_haps, read_family, seed=303) -> FlatBatch:
    """Haplotypes of 30 .. 60 bases, prefixes of three unrelated windows; the family of a haplotype follows from its
    position in the stream (c_family_of_position).  330 sharp reads of 20 .. 30 bases from the first 30 bases of ONE
    window: each is flagged against exactly the haplotypes of the other families, so every chunk of the fp64 pass needs
    the same set -- runs that cross the 64-haplotype segments of the run detection, stop at them, start at them, or
    skip a whole segment.  read_family 3: unrelated reads, every haplotype needed.  Calls of at most 65 536 pairs get
    one soft read of 520 .. 639 bases from window A, which no per-pair kernel holds."""
    rng = np.random.RandomState(seed + n_haps)   # (the haplotypes of an n_haps are the same for every read family)
    wins = [_seq(rng, 640) for _ in range(4)]   # (the fourth: what the unrelated reads are copies of)
    lens = rng.randint(30, 61, size=n_haps)
    order = np.argsort(lens, kind="stable")
    fam = np.empty(n_haps, np.int64)
    fam[order] = [c_family_of_position(p) for p in range(n_haps)]
    haps = [wins[fam[h]][: lens[h]] for h in range(n_haps)]
    rng = np.random.RandomState(seed * 7 + n_haps * 4 + read_family)
    reads = []
    for _ in range(330):
        L = int(rng.randint(20, 31))
        off = int(rng.randint(0, 30 - L + 1))
        reads.append(_sharp(rng, wins[read_family][off:off + L]))
    if 330 * n_haps <= DIRECT_PAIRS:
        reads.append(_soft(rng, wins[0][: int(rng.randint(520, 640))], q=(10, 20)))
    return _assemble(reads, haps, {"case": "C", "fam": fam, "read_family": read_family, "n_short": 330})


def c_needed_mask(b: FlatBatch) -> np.ndarray:
    """needed[p]: the short reads of a batch_c call are flagged against the haplotype at stream position p."""
    fam = b.meta["fam"][stream_order(b)]
    return fam != b.meta["read_family"]


# ---------------------------------------------------------------------------------------------- D: packing windows
def batch_d(seed=404) -> FlatBatch:
    """8 haplotypes of 300 .. 700 bases (prefixes of one window over A, C, G; the last one ends in nine T); reads of the
    lane counts the packing meets at its edges, at 10 rows per lane: 110 of 320 .. 329 bases (33 lanes: no two share a
    chunk), 34 of 630 .. 639 (all 64 lanes), one of 639 and one of 640 (the first pseudo-chunk), 36 of 6 .. 9 bases (one
    lane; all T at quality 127: flagged against the seven haplotypes without a T), 60 spread over 10 .. 300.  The long
    ones are copies with 8 % substitutions at quality 40: flagged against all eight in fp32, finite in fp64.  The
    planner orders the flagged reads by fail count, in no fixed order within a count: the reads that fail against all
    eight are nearly all of 33 lanes or more, so its first window of 96 opens more than 64 bins whatever the order."""
    rng = np.random.RandomState(seed)
    win = _seq(rng, 700, _ACG)
    haps = [win[:L].copy() for L in (300, 420, 540, 610, 650, 680, 700, 691)]
    for h in haps[1:7:2]:
        h[rng.randint(0, h.size, size=3)] = _ACG[rng.randint(0, 3, size=3)]
    haps[7] = np.concatenate([haps[7], np.full(9, ord("T"), np.uint8)])
    reads = []

    def noisy(L):
        off = int(rng.randint(0, 691 - L + 1))
        return _soft(rng, win[off:off + L], q=(40, 40), sub=0.08)

    for _ in range(110):
        reads.append(noisy(int(rng.randint(320, 330))))
    for _ in range(34):
        reads.append(noisy(int(rng.randint(630, 640))))
    reads.append(noisy(639))
    reads.append(noisy(640))
    for _ in range(36):
        reads.append(_read(np.full(int(rng.randint(6, 10)), ord("T"), np.uint8), 127, 127, 127, 127))
    for k in range(60):
        L = 10 + (290 * k) // 59
        # (a sharp copy of the bases behind the shortest haplotype's end: kept against the haplotypes that reach its end)
        reads.append(noisy(L) if k % 2 else _sharp(rng, win[300:300 + L]))
    perm = rng.permutation(len(reads))
    return _assemble([reads[i] for i in perm], haps, {"case": "D"})


# ---------------------------------------------------------------------------------------------- E: degenerate fallback counts
def _region(rng, n_reads, n_haps, extra):
    """All haplotypes span one 560-base window (0 .. 3 substitutions each); soft reads of 50 .. 250 bases from its first
    520 bases, and one of 520 bases that forces the planned pass."""
    win = _seq(rng, 560)
    haps = []
    for _ in range(n_haps):
        h = win.copy()
        k = int(rng.randint(0, 4))
        h[rng.randint(0, 520, size=k)] = _ACGT[rng.randint(0, 4, size=k)]
        haps.append(h)
    reads = []
    for _ in range(n_reads):
        L = int(rng.randint(50, 251))
        off = int(rng.randint(0, 520 - L + 1))
        reads.append(_soft(rng, win[off:off + L], q=(20, 40), sub=0.003))
    reads.append(_soft(rng, win[:520], q=(25, 35), sub=0.003))
    return win, haps, reads + extra(win, haps)


def batch_e_none(seed=505) -> FlatBatch:
    """A planned call in which nothing fails: the plan's launches leave at n_fail == 0."""
    rng = np.random.RandomState(seed)
    _, haps, reads = _region(rng, 60, 8, lambda win, haps: [])
    return _assemble(reads, haps, {"case": "E-none"})


def batch_e_one(seed=506) -> FlatBatch:
    """... and one in which exactly one pair fails: the last 40 bases of haplotype 3 are replaced, and one sharp read is
    a copy of the window's last 40 bases (no other read reaches them)."""
    rng = np.random.RandomState(seed)

    def extra(win, haps):
        haps[3] = haps[3].copy()
        haps[3][520:] = (np.searchsorted(_ACGT, win[520:]) + 1 + rng.randint(0, 3, size=40)) % 4
        haps[3][520:] = _ACGT[haps[3][520:]]
        return [_sharp(rng, win[520:])]

    _, haps, reads = _region(rng, 60, 8, extra)
    return _assemble(reads, haps, {"case": "E-one"})


def batch_e_all(seed=507) -> FlatBatch:
    """Every pair fails: 300 sharp reads of 20 .. 40 bases over G, T x 220 haplotypes of 30 .. 60 over A, C."""
    rng = np.random.RandomState(seed)
    gt, ac = np.frombuffer(b"GT", dtype=np.uint8), np.frombuffer(b"AC", dtype=np.uint8)
    haps = [_seq(rng, rng.randint(30, 61), ac) for _ in range(220)]
    reads = [_sharp(rng, _seq(rng, rng.randint(20, 41), gt)) for _ in range(300)]
    return _assemble(reads, haps, {"case": "E-all"})


# ---------------------------------------------------------------------------------------------- F: pseudo-chunks, many haplotypes
def batch_f(seed=606) -> FlatBatch:
    """130 haplotypes: 30 of 700 .. 720 bases from window A, 30 from window B (lengths interleaved in the stream), 70 short
    prefixes of 30 .. 100 bases of either; 6 soft reads of 640 .. 700 bases from window A -- too long for a chunk of the
    packed fp64 pass, each its own pseudo-chunk of the striped kernel, whose jobs never cross a stream group -- are kept
    against A's long haplotypes and flagged against the rest; 40 sharp reads of 20 .. 30 bases from either window."""
    rng = np.random.RandomState(seed)
    wins = [_seq(rng, 720), _seq(rng, 720)]
    haps = []
    for k in range(60):
        h = wins[k % 2][: int(rng.randint(700, 721))].copy()
        n_sub = int(rng.randint(0, 3))
        h[rng.randint(0, h.size, size=n_sub)] = _ACGT[rng.randint(0, 4, size=n_sub)]
        haps.append(h)
    for k in range(70):
        haps.append(wins[k % 2][: int(rng.randint(30, 101))].copy())
    haps = [haps[i] for i in rng.permutation(len(haps))]
    reads = []
    for _ in range(6):
        L = int(rng.randint(640, 701))
        off = int(rng.randint(0, 700 - L + 1))
        reads.append(_soft(rng, wins[0][off:off + L], q=(28, 35)))
    for k in range(40):
        L = int(rng.randint(20, 31))
        off = int(rng.randint(0, 30 - L + 1))
        reads.append(_sharp(rng, wins[k % 2][off:off + L]))
    perm = rng.permutation(len(reads))
    long_reads = np.nonzero(perm < 6)[0]
    return _assemble([reads[i] for i in perm], haps, {"case": "F", "long_reads": long_reads})


# ---------------------------------------------------------------------------------------------- the list
@functools.lru_cache(maxsize=None)
def batch(name: str) -> FlatBatch:
    """The batches by name; built once per process and never changed."""
    kind, _, arg = name.partition(":")
    if kind == "A1":
        return batch_a1()
    if kind == "A2":
        return {"3": lambda: batch_a2(30000, 3, 202), "5": lambda: batch_a2(20000, 5, 203)}[arg]()
    if kind == "B":
        n_haps, _, seed = arg.partition("/")
        n_reads = 70 if n_haps == "1025" else 17
        return batch_b(int(n_haps), n_reads, 3000 + int(n_haps) + 17 * int(seed or 0))
    if kind == "C":
        n_haps, fam = arg.split("/")
        return batch_c(int(n_haps), int(fam))
    if kind == "D":
        return batch_d()
    if kind == "E":
        return {"none": batch_e_none, "one": batch_e_one, "all": batch_e_all}[arg]()
    if kind == "F":
        return batch_f()
    raise KeyError(name)


C_N_HAPS = (200, 63, 64, 65, 129)
# name -> fma modes the GPU test runs it in
CASES = {"A1": (1,), "A2:3": (1, 0), "A2:5": (1, 0),
         "B:1025": (1,), "B:4094": (1,), "B:4095": (1, 0),
         **{f"C:{n}/{f}": (1, 0) for n in C_N_HAPS for f in C_READ_FAMILIES},
         "D": (1, 0), "E:none": (1,), "E:one": (1,), "E:all": (1,), "F": (1, 0)}
SEQUENCE_G = ("B:4095", "E:none", "A1", "C:200/0", "B:4095/1", "E:one")   # one context, many shapes
SMALLEST_GRIDS_H = ("B:1025", "C:200/1", "D")                              # GKLHIP_PLAN_BLOCKS=1


def takes_planned_pass(b: FlatBatch) -> bool:
    """The routing rule: more pairs than the per-pair kernels take, or a read that none of them holds under either
    small-read limit; and a single pass on the host side."""
    return (b.n_pairs > DIRECT_PAIRS or int(b.read_lens.max()) >= FORCING_READ_LEN) and b.n_pairs < HOST_SHARD_PAIRS


_REFERENCE = {}


def reference(oracle, name: str, fma_mode: int = 1):
    """The oracle's (out, raw32, raw64, used64) of a batch: computed once per process, read-only."""
    key = (name, int(fma_mode))
    if key not in _REFERENCE:
        res = oracle.batch(batch(name), fma_mode=fma_mode, want_raw=True, n_threads=8)
        for a in res:
            a.setflags(write=False)
        _REFERENCE[key] = res
    return _REFERENCE[key]


def digests(out, r32, r64, u) -> dict:
    """SHA-256 of a call's output, raw fp32 sums, raw fp64 sums of the flagged pairs and flags."""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    return {"out": sha(out), "raw32": sha(r32), "raw64": sha(np.where(np.asarray(u) == 1, r64, 0.0)), "used64": sha(u)}


# ---------------------------------------------------------------------------------------------- device finalisation
# The device finalisation modes write log10(sum) - log10(scale) with the device's log10.  The reference below takes the
# logarithm in numpy.longdouble (x87: 64 bits of mantissa) from the ORACLE's raw sums.
LOG10_INIT32 = math.log10(math.ldexp(1.0, 120))    # as doubles: what the library subtracts from a kept pair
LOG10_INIT64 = math.log10(math.ldexp(1.0, 1020))   # ... from a flagged pair
ULP_BOUND = 2.0   # one ulp for the device's double log10 (the bound ROCm documents), one for the subtraction
MAX_EXEMPT_SHARE = 1e-4


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


class Finalised:
    """What a device finalisation mode must write for the oracle's raw sums (o32, o64, used64)."""

    def __init__(self, oracle, o32, o64, used64):
        assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than double here"
        flagged = np.asarray(used64) != 0
        v = np.where(flagged, np.asarray(o64, np.float64), np.asarray(o32, np.float32).astype(np.float64))
        self.flagged = flagged
        self.valid = ~np.isnan(v)                      # pairs whose oracle sum is NaN are left out
        self.zero = self.valid & (v == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.L = np.log10(v.astype(np.longdouble))
        c = np.where(flagged, np.longdouble(LOG10_INIT64), np.longdouble(LOG10_INIT32))
        with np.errstate(invalid="ignore"):
            self.E = (self.L - c).astype(np.float64)   # mode 1, and the flagged pairs of mode 2
            self.scale = _ulp(np.maximum(np.abs(self.L).astype(np.float64), np.abs(self.E)))
        # mode 2, kept pairs: double(float(L) - log10f(2^120)), float subtraction; the constant is the host libm's
        self.c32 = np.float32(-oracle.finalize_f32(1.0))
        with np.errstate(invalid="ignore", over="ignore"):
            L32 = self.L.astype(np.float32)
            self.E32 = (L32 - self.c32).astype(np.float64)
            lo, hi = np.nextafter(L32, np.float32(-np.inf)), np.nextafter(L32, np.float32(np.inf))
            self.E32_lo, self.E32_hi = (lo - self.c32).astype(np.float64), (hi - self.c32).astype(np.float64)
            # a pair is exempt where L lies within two double ulps of the midpoint of two adjacent floats
            mid_lo = (L32.astype(np.longdouble) + lo.astype(np.longdouble)) / 2
            mid_hi = (L32.astype(np.longdouble) + hi.astype(np.longdouble)) / 2
            near = np.minimum(np.abs(self.L - mid_lo), np.abs(self.L - mid_hi))
            self.exempt = self.valid & ~flagged & np.isfinite(self.L.astype(np.float64)) & (near <= 2 * _ulp(self.L.astype(np.float64)))

    def n_exempt(self) -> int:
        return int(self.exempt.sum())

    def distance_ulps(self, out, mask):
        """|out - E| in ulps of max(|L|, |E|) over `mask` (finite expectations only)."""
        m = mask & self.valid & np.isfinite(self.E)
        if not m.any():
            return np.zeros(0)
        with np.errstate(invalid="ignore"):
            return np.abs(np.asarray(out, np.float64)[m] - self.E[m]) / self.scale[m]

    def check(self, out, mode: int) -> dict:
        """Asserts the finalisation rule on `out`; returns the observed figures."""
        out = np.asarray(out, np.float64)
        wide = self.valid if mode == 1 else (self.valid & self.flagged)   # pairs under the ulp bound
        inf = wide & ~np.isfinite(self.E)
        assert np.array_equal(out[inf], self.E[inf]), "a zero (infinite) sum must give exactly -inf (+inf)"
        assert np.all(out[self.zero & wide] == -np.inf)
        d = self.distance_ulps(out, wide)
        worst = float(d.max()) if d.size else 0.0
        print(f"finalisation mode {mode}: {int(wide.sum())} pairs under the ulp bound, max distance {worst:.3f} ulp; "
              f"{self.n_exempt()} exempt of {int((self.valid & ~self.flagged).sum())} kept")
        assert not np.isnan(d).any() and worst <= ULP_BOUND, f"mode {mode}: {worst} ulp from the long-double reference (bound {ULP_BOUND})"
        res = {"max_ulp": worst, "n_exempt": self.n_exempt()}
        if mode == 2:
            kept = self.valid & ~self.flagged
            exact = kept & ~self.exempt
            bad = exact & (out != self.E32) & ~(np.isnan(out) & np.isnan(self.E32))
            assert not bad.any(), f"mode 2: {int(bad.sum())} kept pairs differ from double(float(L) - c32), first at {int(np.argmax(bad))}"
            ex = self.exempt
            ok = (out[ex] == self.E32[ex]) | (out[ex] == self.E32_lo[ex]) | (out[ex] == self.E32_hi[ex])
            assert ok.all(), "mode 2: an exempt pair is more than one float ulp away"
            assert self.n_exempt() <= MAX_EXEMPT_SHARE * out.size, "too many exempt pairs"
        return res

"""Deterministic Smith-Waterman case families for tests/test_sw_edges.py, tests/fuzz.py and the fixture generator
tests/golden/make_sw_edge_fixtures.py.  No HIP and no reference in here: sequences, recipes, and one-comparison mutants
of oracle/sw_oracle.c that say whether a set of cases can tell a wrong tie break from a right one.

A family is a function (seed, *ints) -> (ref, alt); a `Case` is the recipe (family, ints, seed, params, strategy,
cigar_len), so a fixture stores a few integers and not the sequence.  `expand(case)` gives (ref, alt, params, strategy).

What the families aim at (gkl_amd/csrc/sw_kernel.h):
  low       homopolymers, AC against CA repeats, CAG repeats, a two-letter alphabet, a sequence against itself: scores
            that tie, in the cell rule and in the maximum over the last row and column (nrow == ncol: cell (nrow, ncol)
            is a candidate of both on one anti-diagonal); lengths around the 64-candidate blocks of sw_find_max
  longgap   one indel of 15..100 bases: the 16-cell look-ahead of the walker inside a gap and its n > 16 clamp
  rowtie    two last-row candidates with the maximum score at the same distance from the diagonal: the strict "<"
            of the last-row rule keeps the first (the other families never tell it from "<=")
  twogaps   two single-base deletions k bases apart: match runs at the edges of the 32-cell diagonal window
  seam      a 33-row deletion / a 33-column insertion across row 64 * rpl, where a stripe hands over to the next
  tier      both ends of every single-stripe rows-per-lane tier, with no steady phase, one step of it, one past it
  floor     gap penalties of -1e6 under INDEL / LEADING_INDEL: the border crosses MATRIX_MIN_CUTOFF (-1e8)
  params    zero penalties, extension dearer than opening, a positive mismatch, the largest match value
  bytes     sequences over all 256 byte values, 0x00 and bytes >= 0x80 among them
  smallbuf  gap cases with a CIGAR buffer of 1..9 bytes: the skip-what-does-not-fit rule"""
import collections
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from oracle.sw import IGNORE, INDEL, LEADING_INDEL, SOFTCLIP, STRATEGIES, _call
from tests.test_sw import PARAM_SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_PARAMS = [(5, -4, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0), (2, -1, -1, -3), (1, 1, -1, -1), (65536, -65536, -3, -1)]
FLOOR_PARAMS = (10, -5, -1000000, -1000000)
ROWTIE_PARAMS = (10, -50, -100, -100)     # a changed base costs six matches, a gap ten and more: fam_rowtie
ALL_PARAMS = list(dict.fromkeys(list(PARAM_SETS) + EXTRA_PARAMS))
LOW_PARAMS = [PARAM_SETS[0], (3, -1, -4, -3), (1, -1, -1, -1), (5, -4, 0, 0), (0, 0, 0, 0), (1, 1, -1, -1)]
LOW_L = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513)
GAPS = (15, 16, 17, 31, 32, 33, 48, 49, 100)
GAP_RUNS = (15, 16, 17, 31, 32, 33, 48, 49)      # the lengths the guards ask for, as I runs and as D runs
SPACINGS = (31, 32, 33, 63, 64, 65)
SEAM_ROWS = (513, 640, 641, 1024, 1025)
SMALL_BUFFERS = (1, 2, 3, 5, 9)
MAX_ROWS, MAX_COLS = 1025, 1403
KLANES = 64

Case = collections.namedtuple("Case", "family ints seed params strategy cigar_len")


def rows_per_lane(nrow):
    """The rule of gklhip_sw_align_batch (sw_api.hip), restated: as many stripes as 8 rows per lane would need, the rows
    spread evenly over them, the fewest rows per lane that hold such a stripe."""
    n_stripes = (nrow + 8 * KLANES - 1) // (8 * KLANES)
    per_stripe = (nrow + n_stripes - 1) // n_stripes
    return max(1, (per_stripe + KLANES - 1) // KLANES)


def lanes_used(nrow):
    """Lanes of the first stripe that hold a row."""
    rpl = rows_per_lane(nrow)
    return (min(nrow, KLANES * rpl) + rpl - 1) // rpl


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(bytes(alphabet), np.uint8)[rng.randint(0, len(alphabet), n)])


def _rand_no_repeat(rng, n):
    """ACGT with no two equal neighbours: a single-base deletion has one place to go."""
    out = bytearray([b"ACGT"[rng.randint(0, 4)]])
    while len(out) < n:
        out.append([c for c in b"ACGT" if c != out[-1]][rng.randint(0, 3)])
    return bytes(out)


def _substitute(rng, s, n):
    b = bytearray(s)
    for _ in range(n):
        k = int(rng.randint(0, len(b)))
        b[k] = [c for c in b"ACGT" if c != b[k]][rng.randint(0, 3)]
    return bytes(b)


# ------------------------------------------------------------------ families: (seed, *ints) -> (ref, alt)
def fam_low(seed, kind, L, M):
    rng = np.random.RandomState(seed)
    if kind == 0:
        return b"A" * L, b"A" * M
    if kind == 1:
        return (b"AC" * (L // 2 + 1))[:L], (b"CA" * (M // 2 + 1))[:M]
    if kind == 2:
        return (b"CAG" * (L // 3 + 1))[:L], (b"CAG" * (M // 3 + 1))[:M]
    if kind == 3:
        return _rand(rng, L, b"AC"), _rand(rng, M, b"AC")
    x = _rand(rng, L)                # kind 4: a sequence against itself (M is not used)
    return x, x


def fam_longgap(seed, g, pos, ins):
    """x against x without g bases (ins = 0: a deletion) or the reverse (ins = 1: an insertion).  pos 0: mid-sequence,
    1: the gap starts at base 2, 2: it ends one base before the end."""
    rng = np.random.RandomState(seed)
    n = 260
    x = _rand(rng, n)
    start = ((n - g) // 2, 1, n - 1 - g)[pos]
    y = x[:start] + x[start + g:]
    return (y, x) if ins else (x, y)


def fam_twogaps(seed, k, ins):
    rng = np.random.RandomState(seed)
    p = 50
    x = _rand_no_repeat(rng, p + 1 + k + 1 + 50)
    y = x[:p] + x[p + 1:p + 1 + k] + x[p + 2 + k:]
    return (y, x) if ins else (x, y)


def fam_seam(seed, nrow, which, kind, window):
    """kind 0: rows s-15 .. s+17 are missing from alt (a 33-row deletion across the hand-over s = which * 64 * rpl);
    kind 1..3: 33 columns inserted behind row s-1, s, s+1.  window > 0: alt is cut to that many bases on either side."""
    rng = np.random.RandomState(seed)
    x = _rand(rng, nrow)
    s = which * KLANES * rows_per_lane(nrow)
    assert s + 17 < nrow
    if kind == 0:
        a, b, mid = s - 16, s + 17, b""
    else:
        a = b = s + kind - 2
        mid = _rand(rng, 33)
    lo, hi = (max(0, a - window), min(nrow, b + window)) if window else (0, nrow)
    return x, x[lo:a] + mid + x[b:hi]


def fam_tier(seed, nrow, ncol):
    rng = np.random.RandomState(seed)
    x = _rand(rng, nrow)
    a = (nrow - ncol) // 2 if nrow > ncol else 0
    alt = (x + _rand(rng, ncol))[a:a + ncol]
    return x, _substitute(rng, alt, 1) if ncol >= 3 else alt


def fam_floor(seed, kind, nrow, ncol):
    rng = np.random.RandomState(seed)
    if kind == 2:
        return b"A" * nrow, b"A" * ncol
    x = _rand(rng, nrow)
    if kind == 0:
        return x, _rand(rng, ncol)
    return x, _substitute(rng, (x * (ncol // nrow + 2))[5:5 + ncol], 4)


def fam_params(seed, kind, L, M):
    if kind < 4:
        return fam_low(seed, kind, L, M)
    rng = np.random.RandomState(seed)   # kind 4: related ACGT, one base missing and two changed
    x = _rand(rng, L)
    y = _substitute(rng, x, 2)
    return x, (y[:L // 2] + y[L // 2 + 1:])[:M] or b"A"


def fam_bytes(seed, kind, L):
    rng = np.random.RandomState(seed)
    if kind == 2:
        few = bytes([0x00, 0x80, 0xff, 0x41])
        return _rand(rng, L, few), _rand(rng, L + 3, few)
    if kind == 3:                       # every byte value once (L is 256), three of them missing from alt
        x = bytes(rng.permutation(256).astype(np.uint8))
        return x, x[:100] + x[103:]
    x = bytearray(_rand(rng, L, bytes(range(256))))
    x[0], x[-1] = 0x00, 0xff
    y = bytearray(x)
    if kind == 0:
        for k in (L // 3, 2 * L // 3):
            y[k] = (y[k] + 0x80) & 0xff
    else:
        del y[L // 2:L // 2 + 3]
    return bytes(x), bytes(y) or b"\0"


def fam_rowtie(seed, n, t, tail, match, mismatch):
    """Two last-row cells with the same score at the same distance from the diagonal, (n, n - t) before (n, n + t):
    alt begins with the last n - t bases of ref (n - t matches from the border of column 0) and holds, from base t on,
    all of ref with t * match / (match - mismatch) bases changed (the same score from the border of row 0); t >= n / 2
    keeps the two apart, `tail` more bases keep (n, n + t) out of the last column."""
    rng = np.random.RandomState(seed)
    changed, rest = divmod(t * match, match - mismatch)
    assert rest == 0 and 2 * t >= n and changed <= n
    x = _rand(rng, n)
    y = bytearray(x)
    for q in range(changed):            # evenly spread: no cluster that a gap would bridge for less
        k = (2 * q + 1) * n // (2 * changed)
        y[k] = [c for c in b"ACGT" if c != y[k]][rng.randint(0, 3)]
    return x, x[t:] + _rand(rng, 2 * t - n) + bytes(y) + _rand(rng, tail)


FAMILIES = {"rowtie": fam_rowtie, "low": fam_low, "longgap": fam_longgap, "twogaps": fam_twogaps, "seam": fam_seam, "tier": fam_tier,
            "floor": fam_floor, "params": fam_params, "bytes": fam_bytes, "smallbuf": fam_longgap}


_SEQ = {}


def expand(case):
    key = (case.family, case.seed, case.ints)
    if key not in _SEQ:
        _SEQ[key] = FAMILIES[case.family](case.seed, *case.ints)
    ref, alt = _SEQ[key]
    return ref, alt, tuple(case.params), case.strategy


def case_from_json(d):
    return Case(d["family"], tuple(d["ints"]), d["seed"], tuple(d["params"]), d["strategy"], d["cigar_len"])


def case_to_json(c):
    return {"family": c.family, "ints": list(c.ints), "seed": c.seed, "params": list(c.params), "strategy": c.strategy,
            "cigar_len": c.cigar_len}


# ------------------------------------------------------------------ the set
_ALL = []


def all_cases():
    """The whole set, in a fixed order.  cigar_len None = the Java side's 2 * max(len)."""
    if _ALL:
        return _ALL
    out = []

    def add(family, ints, seed, params_list, strategies=STRATEGIES, cigar_len=None):
        for p in params_list:
            for s in strategies:
                out.append(Case(family, tuple(int(v) for v in ints), int(seed), tuple(p), s, cigar_len))

    for L in LOW_L:
        for M in sorted({m for m in (1, 17, 64, 65, L - 1, L, L + 1) if m >= 1}):
            for kind in range(4):
                add("low", (kind, L, M), 1000 + L * 7 + M, LOW_PARAMS)
        add("low", (4, L, L), 2000 + L, LOW_PARAMS)
    gap_params = [PARAM_SETS[0], PARAM_SETS[2], (1, -1, -1, -1)]
    for g in GAPS:
        for pos in range(3):
            for ins in range(2):
                add("longgap", (g, pos, ins), 3000 + g, gap_params)
    for k in SPACINGS:
        for ins in range(2):
            add("twogaps", (k, ins), 4000 + k, [PARAM_SETS[0], (3, -1, -4, -3)])
    for nrow in SEAM_ROWS:
        rpl = rows_per_lane(nrow)
        for which in range(1, (nrow - 18) // (KLANES * rpl) + 1):
            for kind in range(4):
                add("seam", (nrow, which, kind, 160), 5000 + nrow, [PARAM_SETS[0]])
                if nrow in (640, 1025):
                    add("seam", (nrow, which, kind, 0), 5000 + nrow, [PARAM_SETS[0]], strategies=(SOFTCLIP, INDEL))
    for k in range(1, 9):
        for nrow in (64 * k, 64 * k + 1):
            lu = lanes_used(nrow)
            for ncol in sorted({c for c in (1, lu - 1, lu, lu + 1) if c >= 1}):
                add("tier", (nrow, ncol), 6000 + nrow, [PARAM_SETS[0], (3, -1, -4, -3)])
    for nrow, ncol in ((100, 100), (101, 300), (300, 101), (150, 150), (300, 300), (200, 257), (129, 128),
                       (256, 256), (257, 129), (120, 300), (300, 120), (250, 251)):
        for kind in range(3):
            add("floor", (kind, nrow, ncol), 7000 + nrow + ncol, [FLOOR_PARAMS])
    for kind in range(5):
        for L, M in ((33, 33), (65, 64), (129, 130)):
            add("params", (kind, L, M), 8000 + L, ALL_PARAMS)
    for kind in range(3):
        for L in (5, 64, 200):
            add("bytes", (kind, L), 9000 + L, [PARAM_SETS[0], (3, -1, -4, -3), (1, 0, 0, 0)])
    add("bytes", (3, 256), 9256, [PARAM_SETS[0], (3, -1, -4, -3), (1, 0, 0, 0)])
    for n, t, tail, p in ((100, 60, 10, ROWTIE_PARAMS), (40, 24, 3, ROWTIE_PARAMS), (100, 60, 12, PARAM_SETS[2]),
                          (300, 180, 20, ROWTIE_PARAMS), (513, 342, 30, PARAM_SETS[2])):
        for k in range(4):
            add("rowtie", (n, t, tail, p[0], p[1]), 10000 + k, [p])
    for cl in SMALL_BUFFERS:
        for g, ins in ((17, 0), (33, 1)):
            add("smallbuf", (g, 0, ins), 3000 + g, [PARAM_SETS[0]], cigar_len=cl)
    for c in out:   # neither side wraps: the bound holds for every parameter set and shape
        ref, alt = expand(c)[:2]
        assert 1 <= len(ref) <= MAX_ROWS and 1 <= len(alt) <= MAX_COLS, c
        assert (len(ref) + len(alt)) * abs(c.params[3]) + abs(c.params[2]) < 2 ** 30, c
    _ALL.extend(out)
    return _ALL


def one_per_family():
    seen = {}
    for c in all_cases():
        seen.setdefault(c.family, c)
    return list(seen.values())


def draw(rng):
    """One random member of a random family, for tests/fuzz.py: (ref, alt, params, strategy)."""
    fam = ("low", "longgap", "twogaps", "seam", "tier", "floor", "params", "bytes")[rng.randint(0, 8)]
    seed = int(rng.randint(0, 2 ** 31 - 1))
    params = ALL_PARAMS[rng.randint(0, len(ALL_PARAMS))]
    strategy = STRATEGIES[rng.randint(0, 4)]
    if fam == "low":
        L = int(rng.randint(1, 600))
        ints = (int(rng.randint(0, 5)), L, max(1, L + int(rng.randint(-2, 3))) if rng.randint(0, 2) else int(rng.randint(1, 600)))
    elif fam == "longgap":
        ints = (int(rng.randint(2, 120)), int(rng.randint(0, 3)), int(rng.randint(0, 2)))
    elif fam == "twogaps":
        ints = (int(rng.randint(1, 130)), int(rng.randint(0, 2)))
    elif fam == "seam":
        nrow = int(rng.randint(513, MAX_ROWS + 1))
        which = int(rng.randint(1, (nrow - 18) // (KLANES * rows_per_lane(nrow)) + 1))
        ints = (nrow, which, int(rng.randint(0, 4)), int(rng.randint(40, 200)))
    elif fam == "tier":
        nrow = int(rng.randint(1, 514))
        ints = (nrow, max(1, lanes_used(nrow) + int(rng.randint(-2, 3))))
    elif fam == "floor":
        ints = (int(rng.randint(0, 3)), int(rng.randint(100, 301)), int(rng.randint(100, 301)))
        params, strategy = FLOOR_PARAMS, (INDEL, LEADING_INDEL)[rng.randint(0, 2)]
    elif fam == "params":
        L = int(rng.randint(1, 300))
        ints = (int(rng.randint(0, 5)), L, max(1, L + int(rng.randint(-3, 4))))
    else:
        ints = (int(rng.randint(0, 3)), int(rng.randint(4, 300)))
    ref, alt = FAMILIES[fam](seed, *ints)
    return ref, alt, params, strategy


# ------------------------------------------------------------------ one-comparison mutants of oracle/sw_oracle.c
# name -> (text in oracle/sw_oracle.c, its replacement); each text must occur exactly once
MUTANTS = collections.OrderedDict([
    ("insert_extension", ("int ext = (open_h > ext_h) ? 0 : SW_INSERT_EXT;", "int ext = (open_h >= ext_h) ? 0 : SW_INSERT_EXT;")),
    ("delete_extension", ("if (!(open_v > ext_v)) ext |= SW_DELETE_EXT;", "if (!(open_v >= ext_v)) ext |= SW_DELETE_EXT;")),
    ("insert_beats_diagonal", ("if (e11 > h11) b = SW_INSERT;", "if (e11 >= h11) b = SW_INSERT;")),
    ("delete_beats_both", ("if (f11 > h11) b = SW_DELETE;", "if (f11 >= h11) b = SW_DELETE;")),
    ("last_row_tie", ("iabs(nrow - j) < iabs(max_i - max_j)", "iabs(nrow - j) <= iabs(max_i - max_j)")),
    ("last_column_tie", ("iabs(i - ncol) <= iabs(max_i - max_j)", "iabs(i - ncol) < iabs(max_i - max_j)")),
    ("last_column_clause", ("(max_j == ncol || iabs(i - ncol) <= iabs(max_i - max_j))", "(iabs(i - ncol) <= iabs(max_i - max_j))")),
    ("floor", ("int32_t h11 = imax(SW_MIN_CUTOFF, m11);", "int32_t h11 = m11;")),
])
MAXIMUM_MUTANTS = ("last_row_tie", "last_column_tie", "last_column_clause")


class MutantOracle:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.sw_oracle_align.restype = C.c_int

    def align(self, ref, alt, params, strategy, cigar_len=None):
        return _call(self.lib.sw_oracle_align, (), ref, alt, params, strategy, cigar_len)


def build_mutants(directory):
    """Compiles every mutant into `directory` with the compiler and flags of oracle/Makefile's liboracle_sw.so rule.
    Raises (never skips) if a substitution no longer matches or there is no compiler."""
    with open(os.path.join(ROOT, "oracle", "sw_oracle.c")) as f:
        text = f.read()
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("gcc") or shutil.which("cc")
    if not cc:
        raise RuntimeError("no C compiler for the oracle mutants")
    out = collections.OrderedDict()
    for name, (old, new) in MUTANTS.items():
        if text.count(old) != 1:
            raise RuntimeError(f"mutant {name}: {old!r} occurs {text.count(old)} times in oracle/sw_oracle.c")
        src = os.path.join(str(directory), f"sw_mutant_{name}.c")
        lib = os.path.join(str(directory), f"libsw_mutant_{name}.so")
        with open(src, "w") as f:
            f.write(text.replace(old, new))
        subprocess.run([cc, "-std=gnu11", "-O2", "-fPIC", "-shared", "-fwrapv", "-o", lib, src], check=True)
        out[name] = MutantOracle(lib)
    return out


def mutant_counts(cases, answers, mutants):
    """name -> (cases whose answer the mutant changes, those among them with nrow + ncol > 128, their indices)."""
    res = collections.OrderedDict()
    for name, m in mutants.items():
        hit = []
        for k, c in enumerate(cases):
            ref, alt, p, s = expand(c)
            if m.align(ref, alt, p, s, cigar_len=c.cigar_len) != answers[k]:
                hit.append(k)
        big = [k for k in hit if sum(len(x) for x in expand(cases[k])[:2]) > 128]
        res[name] = (len(hit), len(big), hit, big)
    return res


def fixture_subset(cases, counts, per_mutant=40, every=12):
    """Indices for tests/golden/sw_edge_vectors.json: for every mutant the first cases it changes (for the three
    maximum rules: of those with nrow + ncol > 128), the first case of every (family, strategy), every `every`-th case
    of the rest."""
    keep = set(range(0, len(cases), every))
    for name, (_, _, hit, big) in counts.items():
        keep.update((big if name in MAXIMUM_MUTANTS else hit)[:per_mutant])
        keep.update(hit[:per_mutant // 4])
    seen = set()
    for k, c in enumerate(cases):
        if (c.family, c.strategy, c.cigar_len) not in seen:
            seen.add((c.family, c.strategy, c.cigar_len))
            keep.add(k)
    return sorted(keep)

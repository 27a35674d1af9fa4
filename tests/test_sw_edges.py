"""Smith-Waterman at its edges: ties, long gaps, stripe seams, the score floor (case families: tests/sw_cases.py).

CPU: the oracle is pinned on these inputs by a fixture of the reference's answers and, where oracle/_ref is built, by
the reference's objects on the whole set; guards on the oracle's own CIGARs and eight one-comparison mutants of the
oracle keep the set from drifting into triviality.  GPU: the HIP kernel against the oracle, bit for bit (CIGAR bytes,
count, offset), through the batch, single-pair and JNI entry points."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle.sw import INDEL, STRATEGIES
from tests import sw_cases
from tests.test_sw import PARAM_SETS, sw_ctx, sw_oracle, sw_reference  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNLIMITED = 1 << 14    # a CIGAR buffer nothing here fills: 2 * (1025 + 1403) bytes at the most


@pytest.fixture(scope="module")
def edge(sw_oracle):  # noqa: F811
    """The set and the oracle's answers, computed once: (cases, answers at each case's own cigar_len, expect(k, cl))."""
    cases = sw_cases.all_cases()
    full = {}
    limited = {}

    def expect(k, cigar_len):
        """(cigar, count, offset) of case k in a buffer of cigar_len bytes.  Text that fits is the unlimited text (the
        skip rule of PairWiseSW.h:442-447 only ever drops what does not fit), anything else is computed."""
        if k not in full:
            full[k] = sw_oracle.align(*sw_cases.expand(cases[k]), cigar_len=UNLIMITED)
        st, cig, cnt, off = full[k]
        assert st == 0
        if len(cig) <= cigar_len:
            return cig, cnt, off
        if (k, cigar_len) not in limited:
            limited[(k, cigar_len)] = sw_oracle.align(*sw_cases.expand(cases[k]), cigar_len=cigar_len)
        st, cig, cnt, off = limited[(k, cigar_len)]
        assert st == 0
        return cig, cnt, off

    own = []
    for k, c in enumerate(cases):
        ref, alt = sw_cases.expand(c)[:2]
        own.append((0,) + expect(k, c.cigar_len if c.cigar_len is not None else 2 * max(len(ref), len(alt))))
    return cases, own, expect


def fixture_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "sw_edge_vectors.json")) as f:
        return json.load(f)["vectors"]


def ops_of(cigar):
    return [(int(n), op) for n, op in re.findall(rb"(\d+)([MIDSR])", cigar)]


# ------------------------------------------------------------------ CPU
def test_sw_edge_oracle_matches_reference_generated_vectors(sw_oracle):  # noqa: F811
    # tests/golden/sw_edge_vectors.json: answers of GKL's AVX2 and AVX-512 objects (generator beside it)
    vs = fixture_vectors()
    assert len(vs) >= 500 and {v["family"] for v in vs} == set(sw_cases.FAMILIES)
    for v in vs:
        c = sw_cases.case_from_json(v)
        st, cig, cnt, off = sw_oracle.align(*sw_cases.expand(c), cigar_len=c.cigar_len)
        assert st == 0 and (cig.decode("ascii"), cnt, off) == (v["cigar"], v["count"], v["offset"]), v


def test_sw_edge_oracle_bit_identical_to_reference_objects(edge, sw_reference):  # noqa: F811
    cases, own, _ = edge
    engines = (1, 2) if sw_reference.has_avx512() else (1,)
    for k, c in enumerate(cases):
        for eng in engines:
            assert own[k] == sw_reference.align(*sw_cases.expand(c), cigar_len=c.cigar_len, engine=eng), (eng, c)


def test_sw_edge_set_keeps_its_shape(edge):
    """The guards, on the oracle's own CIGARs: gap runs of every length around the walker's 16-cell window, match runs
    between two gaps at the edges of its 32-cell window, a CIGAR cut short by a small buffer under every strategy, and
    the lengths, bytes and parameter bound the families promise."""
    cases, own, expect = edge
    runs = {b"I": set(), b"D": set()}
    between = set()
    for st, cig, _, _ in own:
        assert st == 0
        ops = ops_of(cig)
        for n, op in ops:
            if op in runs:
                runs[op].add(n)
        for q in range(1, len(ops) - 1):
            if ops[q][1] == b"M" and ops[q - 1][1] in (b"I", b"D") and ops[q + 1][1] in (b"I", b"D"):
                between.add(ops[q][0])
    for g in sw_cases.GAP_RUNS:
        assert g in runs[b"I"] and g in runs[b"D"], g
    for k in sw_cases.SPACINGS:
        assert k in between, k
    cut = set()
    for k, c in enumerate(cases):
        if c.cigar_len is not None and own[k][1] != expect(k, UNLIMITED)[0] and len(ops_of(expect(k, UNLIMITED)[0])) >= 2:
            cut.add(c.strategy)
    assert cut == set(STRATEGIES)
    seen = set()
    square = 0
    for c in cases:
        ref, alt, p, _ = sw_cases.expand(c)
        assert 1 <= len(ref) <= sw_cases.MAX_ROWS and 1 <= len(alt) <= sw_cases.MAX_COLS
        assert (len(ref) + len(alt)) * abs(p[3]) + abs(p[2]) < 2 ** 30
        seen.update(ref)
        seen.update(alt)
        square += len(ref) == len(alt)
    assert seen == set(range(256)) and square >= 100
    assert {tuple(c.params) for c in cases} >= set(sw_cases.ALL_PARAMS) | {sw_cases.FLOOR_PARAMS}
    # the rows-per-lane rule restated in sw_cases: every tier 1..8 has both its ends in the set, and the seams lie
    # where the rule puts them (513 -> 5 rows per lane, 641 -> 6, 1024 -> 8, 1025 -> three stripes of 6)
    assert [sw_cases.rows_per_lane(n) for n in (1, 64, 65, 128, 129, 512, 513, 640, 641, 1024, 1025)] == \
        [1, 1, 2, 2, 3, 8, 5, 5, 6, 8, 6]
    tiers = {sw_cases.rows_per_lane(c.ints[0]) for c in cases if c.family == "tier" and c.ints[0] <= 512}
    assert tiers == set(range(1, 9))


def test_sw_edge_set_changes_every_mutant_of_the_oracle(edge, tmp_path):
    """Eight one-comparison mutants of oracle/sw_oracle.c (the four tie breaks of the cell rule, the two tie rules of
    the maximum, its `max_j == ncol` clause, the floor): the set tells each from the oracle, the three maximum rules
    also among pairs with nrow + ncol > 128, where tied candidates lie in different 64-wide blocks of the kernel's
    in-order pass.  So does the subset the fixture holds.  No compiler or a substitution that no longer matches: an
    error, not a skip."""
    cases, own, _ = edge
    mutants = sw_cases.build_mutants(tmp_path)
    assert list(mutants) == list(sw_cases.MUTANTS) and len(mutants) == 8
    counts = sw_cases.mutant_counts(cases, own, mutants)
    for name, (n, nbig, _, _) in counts.items():
        print(f"{name}: {n} of {len(cases)} answers change, {nbig} with nrow + ncol > 128")
    for name, (n, nbig, _, _) in counts.items():
        assert n >= 1, name
        if name in sw_cases.MAXIMUM_MUTANTS:
            assert nbig >= 1, name
    index = {c: k for k, c in enumerate(cases)}
    held = [index[sw_cases.case_from_json(v)] for v in fixture_vectors()]   # KeyError: the fixture is stale
    for name, (_, _, hit, big) in counts.items():
        assert set(big if name in sw_cases.MAXIMUM_MUTANTS else hit) & set(held), name


# ------------------------------------------------------------------ GPU
def by_call(cases, picked):
    """Indices grouped by (params, strategy), in the set's order: one align_batch call each."""
    groups = {}
    for k in picked:
        groups.setdefault((tuple(cases[k].params), cases[k].strategy), []).append(k)
    return groups


def check_batch(ctx, cases, expect, ks, params, strategy, cigar_stride=None):
    refs, alts = zip(*(sw_cases.expand(cases[k])[:2] for k in ks))
    stride = cigar_stride or 2 * max(max(len(r), len(a)) for r, a in zip(refs, alts))
    cig, cnt, off = ctx.align_batch(list(refs), list(alts), params, strategy, cigar_stride=cigar_stride)
    for q, k in enumerate(ks):
        assert (cig[q], int(cnt[q]), int(off[q])) == expect(k, stride), (cases[k], stride)


@pytest.mark.gpu
def test_sw_edge_gpu_batch_parity(sw_ctx, edge):  # noqa: F811
    # every family, one call per (params, strategy): pairs of different rows-per-lane tiers share a launch
    cases, _, expect = edge
    groups = by_call(cases, range(len(cases)))
    assert len(groups) >= 4 * len(sw_cases.ALL_PARAMS)
    for (params, strategy), ks in groups.items():
        check_batch(sw_ctx, cases, expect, ks, params, strategy)


@pytest.mark.gpu
def test_sw_edge_gpu_single_pair_parity(sw_ctx, edge):  # noqa: F811
    # the seam, gap, floor and last-row-tie families one pair per call: each with its own default cigar_len
    cases, own, _ = edge
    n = 0
    for k, c in enumerate(cases):
        if c.family in ("seam", "longgap", "twogaps", "floor", "rowtie", "smallbuf"):
            ref, alt, p, s = sw_cases.expand(c)
            assert sw_ctx.align(ref, alt, p, s, cigar_len=c.cigar_len) == own[k][1:], c
            n += 1
    assert n >= 1000


@pytest.mark.gpu
def test_sw_edge_gpu_small_cigar_buffer_in_a_batch(sw_ctx, edge):  # noqa: F811
    # elements that do not fit are skipped, later shorter ones still written (PairWiseSW.h:442-447), on the batch path
    cases, _, expect = edge
    picked = [k for k, c in enumerate(cases) if c.cigar_len is None and len(ops_of(expect(k, UNLIMITED)[0])) >= 6]
    groups = by_call(cases, picked)
    print(len(picked), "cases in", len(groups), "calls per stride")
    assert len(picked) >= 300 and {s for _, s in groups} == set(STRATEGIES)
    assert {cases[k].family for k in picked} >= {"low", "longgap", "seam", "rowtie", "bytes"}
    for (params, strategy), ks in groups.items():
        for stride in sw_cases.SMALL_BUFFERS:
            check_batch(sw_ctx, cases, expect, ks, params, strategy, cigar_stride=stride)


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401
from gkl_amd import native
from oracle.sw import SwOracle
from tests import sw_cases
cases = sw_cases.all_cases()
params, strategy = tuple(json.loads(sys.argv[2])), int(sys.argv[3])
ks = [k for k, c in enumerate(cases) if tuple(c.params) == params and c.strategy == strategy and c.cigar_len is None]
rng = np.random.RandomState(7)
order = rng.permutation(np.repeat(ks, 2))
pairs = [sw_cases.expand(cases[k])[:2] for k in order]
stride = 2 * max(max(len(r), len(a)) for r, a in pairs)
oracle = SwOracle()
exp = {k: oracle.align(*sw_cases.expand(cases[k]), cigar_len=stride) for k in ks}
with native.SwContext() as ctx:
    cig, cnt, off = ctx.align_batch([r for r, _ in pairs], [a for _, a in pairs], params, strategy)
bad = [int(k) for q, k in enumerate(order) if (0, cig[q], int(cnt[q]), int(off[q])) != exp[k]]
print(json.dumps({"pairs": len(order), "families": sorted({cases[k].family for k in ks}), "bad": bad[:20]}))
"""


@pytest.mark.gpu
def test_sw_edge_gpu_more_pairs_than_wavefronts():
    """GKLHIP_SW_WAVES_PER_CU=1: 256 persistent wavefronts.  One batch of more than 256 pairs, long-gap and
    low-complexity pairs shuffled together: every wavefront goes round its loop again on a slab that still holds
    another pair's back-track words, maxima and operations.  The variable is read once per process: a fresh child."""
    env = dict(os.environ, GKLHIP_SW_WAVES_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(list(PARAM_SETS[0])), str(STRATEGIES[0])],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["pairs"] > 2 * 256 and {"low", "longgap", "twogaps", "seam", "tier"} <= set(res["families"]), res
    assert res["bad"] == [], res


@pytest.mark.gpu
def test_sw_edge_jni_batch_entry_point(edge):
    # one alignBatchNative call (include/gkl_sw_jni.h) with the sequences of one case of every family
    from tests import mockjni
    cases, _, _ = edge
    index = {c: k for k, c in enumerate(cases)}
    ks = [index[c] for c in sw_cases.one_per_family()]
    assert len(ks) == len(set(sw_cases.FAMILIES.values())) + 1   # smallbuf shares longgap's sequences
    refs, alts = zip(*(sw_cases.expand(cases[k])[:2] for k in ks))
    from oracle.sw import SwOracle
    oracle = SwOracle()
    rc, ret, cigs, offs, cls, msg = mockjni.run_sw_batch(list(refs), list(alts), PARAM_SETS[0], INDEL)
    assert rc == 0 and ret == len(ks) and msg == "", (cls, msg)
    stride = 2 * max(max(len(r), len(a)) for r, a in zip(refs, alts))
    for q, k in enumerate(ks):
        _, ecig, _, eoff = oracle.align(refs[q], alts[q], PARAM_SETS[0], INDEL, cigar_len=stride)
        assert (cigs[q], int(offs[q])) == (ecig, eoff), cases[k]

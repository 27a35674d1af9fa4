"""The inputs of tests/test_pdhmm_edges.py, checked with the oracle alone (no GPU): they must be able to tell a right
kernel from a wrong one.  An expected value of -inf proves nothing about a carry row, and a stripe seam the result does
not depend on is no test of the seam."""
import os
import re

import numpy as np
import pytest

from gkl_amd.pdhmm_batch import PdhmmBatch
from tests import pdhmm_edge_inputs as E
from tests.test_pdhmm import pd_oracle, pd_reference  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {"A": E.stripe_batch, "B": E.carry_batch, "C": E.packed_batch, "D": E.quality_batch}


def test_rows_per_lane_is_the_kernels():
    text = open(os.path.join(ROOT, "gkl_amd", "csrc", "pdhmm_job_layout.h")).read()
    m = re.search(r"^#define GKL_PD_RPL (\d+)$", text, re.M)
    assert m, "pdhmm_job_layout.h no longer defines GKL_PD_RPL"
    assert int(m.group(1)) == E.RPL, "the seams moved: set RPL of tests/pdhmm_edge_inputs.py to the kernels' rows per lane"
    assert (E.PACKED_MAX, E.n_stripes(E.PACKED_MAX), E.n_stripes(E.PACKED_MAX + 1)) == (64 * E.RPL - 1, 1, 2)


def test_stripe_counts_and_first_stripes():
    assert [E.n_stripes(R) for R in E.STRIPE_R] == E.STRIPE_COUNTS == [1, 1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4]
    assert E.STRIPE_R == [382, 383, 384, 385, 389, 390, 391, 766, 767, 768, 769, 1151, 1152, 1153]
    by_r = dict(zip(E.STRIPE_R, map(E.first_cnt, E.STRIPE_R)))
    assert [by_r[R] for R in (384, 768, 1152)] == [1, 1, 1]         # one lane ...
    assert [E.seam_rows(R)[0] for R in (384, 768, 1152)] == [(None, 0)] * 3   # ... that holds only row 0
    assert [by_r[R] for R in (767, 1151)] == [64, 64]               # 64 full lanes
    assert by_r[389] == 1 and by_r[390] == 2
    assert max(E.STRIPE_COUNTS) >= 4                                # the first carry buffer is written a second time and read
    assert [E.n_stripes(R) for R in E.CARRY_R] == [2, 3, 4] and [E.n_stripes(R) for R in E.QUAL_R] == [1, 2]
    assert all(E.n_stripes(R) == 1 for R in E.PACKED_R) and max(E.PACKED_R) == E.PACKED_MAX
    assert {R for R in E.PACKED_R if R % E.RPL == 0} == {6, 12, 378}   # first block: the pads and row 0, no read base


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_expected_values_are_finite(pd_oracle, group):  # noqa: F811
    b = GROUPS[group]()
    for sem in (0, 1, 2):   # the vector arithmetics and the scalar engine's (reference-tail mode)
        st, v = pd_oracle.compute(b, semantics=sem)
        assert st == 0
        assert int((~np.isfinite(v)).sum()) == 0, (group, sem, np.flatnonzero(~np.isfinite(v)))
        if group == "A":
            assert v.min() > -300.0
    if group == "C":
        assert b.batch == len(E.PACKED_R) * len(E.PACKED_H)
    if group == "D":
        q, i, d, g = (a.reshape(b.batch, b.max_read_len) for a in (b.read_qual, b.read_ins_qual, b.read_del_qual, b.gcp))
        rows = lambda a: np.concatenate([a[k, :b.read_lengths[k]] for k in range(b.batch)])  # noqa: E731
        assert set(rows(q).tolist()) == set(range(-128, 128))
        assert set(rows(g).tolist()) == set(range(128))
        corners = set(zip(rows(i).tolist(), rows(d).tolist()))
        assert {(0, 0), (0, 127), (127, 0), (127, 127), (64, 64)} <= corners and min(rows(i).min(), rows(d).min()) == 0


@pytest.mark.parametrize("group", ["A", "B"])
def test_every_stripe_seam_moves_the_result(pd_oracle, group):  # noqa: F811
    """The read base of the last row above a seam, and of the first row below it, replaced: the oracle's bits change.
    (Where the first stripe holds only row 0 of the matrices there is no base above the seam.)

    Group A (haplotype at least as long as the read): ANY other base in the row changes the bits, all three are tried.
    Group B has haplotypes of 1..5 columns under reads of hundreds of bases, where a replacement can turn one mismatch
    into another (the row can only be matched to the few columns to the right of column 1): there the result must change
    for at least one of the three other bases.  Against ONE column no row but the first can be a match row at all -- column
    0 of rows >= 1 is zero, so M(r, 1) = 0 for r > 1 -- and no base of a later row can matter: for H = 1 the row's
    insertion bytes (gap continuation 1 <-> 2, insertion quality + 1: every path through that row pays one of the two)
    stand in for its base."""
    pairs = E.stripe_pairs() if group == "A" else E.carry_pairs()
    mutants, of = [], []
    for k, p in enumerate(pairs):
        for seam in E.seam_rows(p[2].size):
            for row in seam:
                if row is None:
                    continue
                if p[0].size == 1 and row > 0:
                    ins, gcp = p[4].copy(), p[6].copy()
                    assert gcp[row] in (1, 2)
                    ins[row] += 1                                   # (the first inserted row pays the gap-open factor instead)
                    gcp[row] = 3 - gcp[row]
                    mutants.append((*p[:4], ins, p[5], gcp))
                    of.append((k, row, "gcp"))
                    continue
                for other in range(1, 4):
                    read = p[2].copy()
                    read[row] = E.ACGT[(int(np.flatnonzero(E.ACGT == read[row])[0]) + other) % 4]
                    mutants.append((p[0], p[1], read, *p[3:]))
                    of.append((k, row, "base"))
    n_seams = sum(E.n_stripes(p[2].size) - 1 for p in pairs)
    assert n_seams == (57 if group == "A" else 14 * (1 + 2 + 3))
    assert len(set(of)) == 2 * n_seams - (9 if group == "A" else 28)     # (the seams below a first stripe of row 0 alone have one row)
    for sem in (0, 2):
        _, base = pd_oracle.compute(PdhmmBatch.from_pairs(pairs), semantics=sem)
        _, got = pd_oracle.compute(PdhmmBatch.from_pairs(mutants), semantics=sem)
        moved = {}
        for m, key in enumerate(of):
            moved.setdefault(key, []).append(got[m].tobytes() != base[key[0]].tobytes())
        need = all if group == "A" else any
        dead = [key for key, ch in moved.items() if not need(ch)]
        assert not dead, (sem, dead)


@pytest.mark.parametrize("which", sorted(E.LADDERS))
def test_underflow_ladders_walk_through_the_subnormals(pd_oracle, which):  # noqa: F811
    b = E.ladder_batch(which)
    vs = [pd_oracle.compute(b, semantics=sem)[1] for sem in (0, 1, 2)]
    assert vs[0].tobytes() == vs[1].tobytes() == vs[2].tobytes()    # the tail mode does not matter on the ladders
    v = vs[0]
    lo, hi = E.SUBNORMAL_WINDOW
    assert -630.37 < lo < -630.36 and -614.71 < hi < -614.70
    assert not np.isnan(v).any()
    subnormal = int(((v > lo) & (v < hi)).sum())                    # (the process running this is not flushing them to zero)
    assert subnormal >= 4 and int(np.isneginf(v).sum()) >= 2 and int((v >= hi).sum()) >= 2
    assert np.all(np.diff(v[np.isfinite(v)]) < 0) and np.isneginf(v[int(np.isfinite(v).sum()):]).all()   # one walk down
    assert E.n_stripes(max(E.LADDERS["packed"]["R"])) == 1 and E.n_stripes(min(E.LADDERS["striped"]["R"])) == 2


@pytest.mark.parametrize("what", ["D", "packed", "striped"])
def test_oracle_is_the_reference_at_the_new_bytes(pd_oracle, pd_reference, what):  # noqa: F811
    """The oracle was pinned to the reference's objects with base qualities 2..60, insertion / deletion 5..70 and gap
    continuation 3..40 (test_pdhmm_oracle_bit_identical_to_reference_kernels); here at every byte, and at subnormal sums.

    Every byte but one: for base quality -1 all three engines of the reference index their 255-entry error table with 255,
    one entry past its end (pdhmm-serial.cc:33, pdhmm.h:58), and return whatever lies behind it; the oracle and the
    kernels read entry 0 there.  The comparison runs with that byte replaced by -2."""
    b = E.quality_batch() if what == "D" else E.ladder_batch(what)
    if what == "D":
        assert int(E.holds_byte_255(b).sum()) == 6                  # "qual -128..-1" and "qual all 256", three haplotypes each
        b = E.without_byte_255(b)
        assert not E.holds_byte_255(b).any() and int((b.read_qual == -2).sum()) >= 12
    _, vec = pd_oracle.compute(b, semantics=0)
    _, ser = pd_oracle.compute(b, semantics=1)
    st, ref0 = pd_reference.compute(b, engine=0)                    # the scalar engine everywhere
    assert st == 0 and ref0.tobytes() == ser.tobytes()
    st, ref1 = pd_reference.compute(b, engine=1)
    nv = b.batch - b.batch % pd_reference.simd_width(1)
    assert st == 0 and ref1[:nv].tobytes() == vec[:nv].tobytes() and ref1[nv:].tobytes() == ser[nv:].tobytes()
    if pd_reference.has_avx512():
        _, fused = pd_oracle.compute(b, semantics=2)
        st, ref2 = pd_reference.compute(b, engine=2)
        nv = b.batch - b.batch % pd_reference.simd_width(2)
        assert st == 0 and ref2[:nv].tobytes() == fused[:nv].tobytes() and ref2[nv:].tobytes() == ser[nv:].tobytes()
    if what == "D":
        # every D pair at a vector position too (the batch rotated by four pairs: the tail above becomes full groups)
        rot = b.subset(np.roll(np.arange(b.batch), 4))
        st, ref1 = pd_reference.compute(rot, engine=1)
        nv = rot.batch - rot.batch % 4
        assert st == 0 and ref1[:nv].tobytes() == np.roll(vec, 4)[:nv].tobytes()

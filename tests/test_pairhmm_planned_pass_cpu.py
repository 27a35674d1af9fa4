"""The inputs of tests/test_pairhmm_planned_pass.py, proved without a GPU: every batch of tests/planned_shapes.py takes
the planned fp64 pass by the routing rule and has, on the ORACLE's fallback flags, the property that sends the planner
down the branch the batch is named for; and the long-double reference of the device finalisation agrees with the host
formulas of the oracle."""
import ctypes as C

import numpy as np
import pytest

from gkl_amd.synth import make_batch
from tests import planned_shapes as ps


def flags(oracle, name, fma=1):
    b = ps.batch(name)
    u = ps.reference(oracle, name, fma)[3]
    return b, u.reshape(b.n_reads, b.n_haps)


def lanes64(lens):
    """Lanes a read takes in a chunk of the packed fp64 pass (10 rows per lane, at least one pad row)."""
    return (np.asarray(lens) + 10) // 10


@pytest.mark.parametrize("name", sorted(set(ps.CASES) | set(ps.SEQUENCE_G) | set(ps.SMALLEST_GRIDS_H)))
def test_every_case_takes_the_planned_pass_and_is_deterministic(name):
    b = ps.batch(name)
    assert ps.takes_planned_pass(b), (name, b.n_pairs, int(b.read_lens.max()))
    if name in ("A1", "D", "B:4095"):
        ps.batch.cache_clear()
        again = ps.batch(name)
        for f in ("read_off", "hap_off", "read_bases", "read_quals", "ins_gop", "del_gop", "gcp", "hap_bases"):
            assert np.array_equal(getattr(b, f), getattr(again, f)), f


def test_a1_has_more_packing_windows_than_the_grid_has_wavefronts(oracle):
    b, u = flags(oracle, "A1")
    assert b.n_haps == 1 and b.read_lens.min() >= 20 and b.read_lens.max() <= 30
    n_flagged = int(u.any(axis=1).sum())
    assert n_flagged > ps.PACK_WINDOW * ps.PACK_GRID_WAVES == 98304
    assert n_flagged < b.n_reads   # kept and flagged reads share the policy's wavefronts


@pytest.mark.parametrize("name,n_haps", [("A2:3", 3), ("A2:5", 5)])
@pytest.mark.parametrize("fma", [1, 0])
def test_a2_every_fail_count_in_a_thousand_reads(oracle, name, n_haps, fma):
    b, u = flags(oracle, name, fma)
    assert b.n_haps == n_haps and b.n_pairs > ps.DIRECT_PAIRS
    counts = np.bincount(u.sum(axis=1), minlength=n_haps + 1)
    assert counts.size == n_haps + 1 and counts.min() >= 1000, counts
    # within a read some pairs fail and some do not
    mixed = (u.sum(axis=1) > 0) & (u.sum(axis=1) < n_haps)
    assert mixed.sum() >= 1000 * (n_haps - 1)


@pytest.mark.parametrize("name,fma", [("B:1025", 1), ("B:4094", 1), ("B:4095", 1), ("B:4095", 0), ("B:4095/1", 1)])
def test_b_fail_counts_spread_over_the_histogram(oracle, name, fma):
    b, u = flags(oracle, name, fma)
    n = b.n_haps
    assert b.hap_lens.min() >= 20 and b.hap_lens.max() <= 45 and b.read_lens.min() >= 10 and b.read_lens.max() <= 40
    counts = u.sum(axis=1)
    assert len(set(counts.tolist())) >= 8, sorted(set(counts.tolist()))
    assert (counts == 0).any() and (counts == n).any()
    if n > 4000:
        assert (counts > 1024).any()
        for q in range(4):
            assert ((counts > q * n / 4) & (counts <= (q + 1) * n / 4)).any(), (q, sorted(counts.tolist()))
    # 1025: two counts per scan thread; 4094: the last size with the histogram in LDS; 4095: the first in global memory
    assert n in (1025, 4094, 4095)


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("n_haps", ps.C_N_HAPS)
def test_c_every_chunk_needs_the_mask_the_case_is_built_for(oracle, n_haps, fma):
    met = set()
    for fam in ps.C_READ_FAMILIES:
        b, u = flags(oracle, f"C:{n_haps}/{fam}", fma)
        assert b.hap_lens.min() >= 30 and b.hap_lens.max() <= 60
        need = ps.c_needed_mask(b)
        rows = u[: b.meta["n_short"]][:, ps.stream_order(b)]
        assert np.array_equal(rows, np.broadcast_to(need, rows.shape).astype(np.uint8)), (n_haps, fam)
        if b.n_reads > b.meta["n_short"]:
            assert 520 <= b.read_lens[-1] <= ps.CHUNK_READ_LEN_MAX
        at = lambda p: p < n_haps and bool(need[p])  # noqa: E731
        if n_haps > 64:
            if at(62) and at(63) and at(64):
                met.add("run carried over the segment boundary")
            if at(63) and not need[64]:
                met.add("run ends at the boundary")
            if need[64] and not need[63]:
                met.add("run starts at the boundary")
        if n_haps > 128 and not need[64:128].any() and need[:64].any() and need[128:].any():
            met.add("a whole segment skipped")
        if need.all():
            met.add("every haplotype needed")
    want = {"every haplotype needed"}
    if n_haps > 64:
        want |= {"run carried over the segment boundary", "run ends at the boundary", "run starts at the boundary"}
    if n_haps > 128:
        want |= {"a whole segment skipped"}
    assert met == want, (n_haps, want - met)


@pytest.mark.parametrize("fma", [1, 0])
def test_d_flagged_reads_of_every_lane_count(oracle, fma):
    b, u = flags(oracle, "D", fma)
    o64 = ps.reference(oracle, "D", fma)[2].reshape(u.shape)
    assert b.n_haps == 8 and b.hap_lens.min() >= 300 and b.hap_lens.max() <= 700
    flagged = u.any(axis=1)
    lens = b.read_lens[flagged]
    assert flagged.sum() >= 200
    assert ((lens >= 320) & (lens <= 329)).sum() >= 100 and set(lanes64(lens[(lens >= 320) & (lens <= 329)])) == {33}
    assert ((lens >= 630) & (lens <= 639)).sum() >= 30 and set(lanes64(lens[(lens >= 630) & (lens <= 639)])) == {64}
    assert (lens == 639).any() and (lens == 640).any() and lanes64(640) == 65
    assert ((lens >= 6) & (lens <= 9)).sum() >= 30 and set(lanes64(lens[lens <= 9])) == {1}
    rest = lens[(lens >= 10) & (lens <= 300)]
    assert rest.size >= 20 and rest.min() < 60 and rest.max() > 250
    # The planner orders the flagged reads by descending fail count, in no fixed order within a count.  Its first window
    # of 96 lies within the reads that fail against all eight, and fewer than 32 of those take less than 33 lanes: more
    # than 64 of the window's reads open a bin of their own, whatever the order.
    counts = u.sum(axis=1)
    top = (counts == 8) & (b.read_lens <= ps.CHUNK_READ_LEN_MAX)
    assert top.sum() >= ps.PACK_WINDOW and (lanes64(b.read_lens[top]) < 33).sum() < ps.PACK_WINDOW - 64
    assert ((counts > 0) & (counts < 8)).sum() >= 30
    fl = u == 1
    finite = np.isfinite(o64[fl]) & (o64[fl] > 0)
    assert finite.mean() >= 0.9, finite.mean()


def test_e_degenerate_fallback_counts(oracle):
    _, u = flags(oracle, "E:none")
    assert u.sum() == 0
    b, u = flags(oracle, "E:one")
    assert u.sum() == 1 and u[b.n_reads - 1, 3] == 1
    b, u = flags(oracle, "E:all")
    assert u.all() and (b.n_reads, b.n_haps) == (300, 220)


@pytest.mark.parametrize("fma", [1, 0])
def test_f_long_reads_need_scattered_haplotypes_of_several_stream_groups(oracle, fma):
    from gkl_amd import native
    b, u = flags(oracle, "F", fma)
    assert b.n_haps == 130
    lib = native.load_library()
    lib.gklhip_plan_describe.restype = C.c_int
    ng, nl = C.c_int32(), C.c_int32()
    n_chunks = lib.gklhip_plan_describe(b.n_reads, b.n_haps, np.ascontiguousarray(b.read_off).ctypes.data_as(C.c_void_p),
                                        np.ascontiguousarray(b.hap_off).ctypes.data_as(C.c_void_p), 8, None, C.c_int64(0),
                                        C.byref(ng), C.byref(nl))
    assert n_chunks > 0 and ng.value >= 3 and nl.value == 6
    long_reads = b.meta["long_reads"]
    assert long_reads.size == 6 and np.all((b.read_lens[long_reads] >= 640) & (b.read_lens[long_reads] <= 700))
    assert np.delete(b.read_lens, long_reads).max() <= 30
    order = ps.stream_order(b)
    for r in long_reads:
        row = u[r][order]
        runs = int(row[0]) + int(((row[1:] == 1) & (row[:-1] == 0)).sum())
        assert 0 < row.sum() < b.n_haps and runs >= 2, (r, row.sum(), runs)
        assert row[:64].any() and row[64:128].any()   # needed haplotypes in more than one 64-haplotype segment


# ---- the finalisation helper against the host formulas of the oracle ----
def test_finalisation_constants_are_the_correctly_rounded_ones():
    assert np.finfo(np.longdouble).nmant >= 63
    two = np.longdouble(2)
    assert ps.LOG10_INIT32 == float(np.log10(two ** 120)) and ps.LOG10_INIT64 == float(np.log10(two ** 1020))


def test_finalisation_reference_agrees_with_the_host_formulas(oracle):
    b = make_batch("hc", 300, 24, seed=11)
    _, o32, o64, ou = oracle.batch(b, want_raw=True, n_threads=8)
    fin = ps.Finalised(oracle, o32, o64, ou)
    kept, fl = fin.valid & ~fin.flagged, fin.valid & fin.flagged
    assert kept.sum() > 1000 and fl.sum() > 1000
    host32 = np.array([oracle.finalize_f32(x) for x in o32[kept]])
    same = host32 == fin.E32[kept]
    assert same.mean() >= 0.99, same.mean()
    near = same | (host32 == fin.E32_lo[kept]) | (host32 == fin.E32_hi[kept])
    assert near.all()
    host64 = np.array([oracle.finalize_f64(x) for x in o64[fl]])
    assert np.all(np.abs(host64 - fin.E[fl]) <= ps._ulp(fin.E[fl]))
    # the reference passes its own check, and a float log10 or a wrong constant does not
    out1 = fin.E.copy()
    assert fin.check(out1, 1)["max_ulp"] == 0.0
    out2 = np.where(fin.flagged, fin.E, fin.E32)
    fin.check(out2, 2)
    with np.errstate(divide="ignore"):
        float_log = np.log10(o32.astype(np.float32)).astype(np.float64) - ps.LOG10_INIT32   # what log10f would give
    with pytest.raises(AssertionError):
        fin.check(np.where(fin.flagged, fin.E, float_log), 1)
    with pytest.raises(AssertionError):
        fin.check(out1 + 4 * ps._ulp(out1), 1)
    with pytest.raises(AssertionError):
        fin.check(np.where(fin.flagged, fin.E, np.nextafter(fin.E32.astype(np.float32), np.float32(0)).astype(np.float64)), 2)


def test_exempt_pairs_stay_under_the_cap_for_the_fixed_seeds(oracle):
    worst = 0.0
    for name, fmas in ps.CASES.items():
        for fma in fmas:
            _, o32, o64, ou = ps.reference(oracle, name, fma)
            fin = ps.Finalised(oracle, o32, o64, ou)
            assert fin.n_exempt() <= ps.MAX_EXEMPT_SHARE * ou.size, (name, fma, fin.n_exempt())
            worst = max(worst, fin.n_exempt() / ou.size)
    for b in (make_batch("hc", 100, 10, seed=5), make_batch("hc", 300, 24, seed=11)):
        _, o32, o64, ou = oracle.batch(b, want_raw=True, n_threads=8)
        assert ps.Finalised(oracle, o32, o64, ou).n_exempt() <= ps.MAX_EXEMPT_SHARE * ou.size
    print("largest share of exempt pairs:", worst)

"""Several PDHMM region calls in one set of launches (gklhip_pdhmm_compute_cross_multi, PdhmmContext.compute_cross_multi)
on the MI355X: every region's bytes are the oracle's and the single call's, whichever regions ride along and in whatever
order; a bad region fails alone; the launches really are shared (gklhip_pdhmm_combine_counts); a call over the limits
falls back to single calls with the same bytes; the all-C++ cross-check build agrees."""
import os

import numpy as np
import pytest

from gkl_amd.pdhmm_batch import PdhmmBatch
from tests.test_pdhmm import expand_cross, random_pd_batch

SEMANTICS_OF_FMA_MODE = {1: 2, 0: 0}   # oracle semantics: 2 = GKL's AVX-512 object, 0 = its AVX2 object
INPUT_ERROR_TEXT = "Error while calculating pdhmm. Input arrays aren't valid."
REF_BATCHES = (0, 13, 8)               # per-region reference batch sizes in tail mode: the tails fall inside the regions


def three_route_region(rng, kw):
    """6 reads (one of 400 bases: striped) x 4 haplotypes that take all three routes, as in
    tests/test_pdhmm_server_gpu.py::test_all_three_kernel_routes_through_the_server."""
    acgt = np.frombuffer(b"ACGT", dtype=np.int8)
    one = np.zeros(1, np.int8)

    def hap(n_snp_kinds, odd=False):
        H = int(rng.randint(150, 260))
        b = acgt[rng.randint(0, 4, H)].copy()
        pd = np.zeros(H, np.int8)
        for k in range(n_snp_kinds):                      # distinct (base, allele set) kinds: a class each
            for j in (10 + 7 * k, 80 + 7 * k):
                b[j] = acgt[k % 4]
                pd[j] = 1 | (k + 1) << 3
        if odd:
            b[40] = ord("a")
        return b, pd

    haps = PdhmmBatch.from_pairs([(b, pd, one, one, one, one, one) for b, pd in (hap(0), hap(1), hap(5), hap(1, odd=True))])
    short = random_pd_batch(rng, 5, read_len=(30, 151), hap_len=(1, 2), **kw)
    long_ = random_pd_batch(rng, 1, read_len=(400, 400), hap_len=(1, 2), **kw)
    return PdhmmBatch.from_pairs(short.pairs() + long_.pairs()), haps


def make_regions(acgt_reads):
    """The region mix, most demanding first so that every K takes a prefix.  acgt_reads: read bases A, C, G, T only (in
    reference-tail mode any other read base under a SNP column is an input error when its pair falls into a scalar tail,
    as in GKL; tests/test_pdhmm_server_gpu.py)."""
    rng = np.random.RandomState(71)
    kw = dict(with_n=False, lower=False) if acgt_reads else {}

    def cross(n_reads, n_haps, read_len, hap_len, **more):
        return (random_pd_batch(rng, n_reads, read_len=read_len, hap_len=(1, 2), **kw),
                random_pd_batch(rng, n_haps, read_len=(1, 2), hap_len=hap_len, **kw, **more))

    striped = cross(4, 3, (20, 90), (60, 200), flag_rate=0.05)   # one read of 400 bases next to short ones
    striped = (PdhmmBatch.from_pairs(striped[0].pairs()[:2] + random_pd_batch(rng, 1, read_len=(400, 400), hap_len=(1, 2), **kw).pairs() +
                                     striped[0].pairs()[2:]), striped[1])
    return [cross(90, 3, (100, 151), (150, 260)),                # more than one chunk of reads
            cross(1, 1, (1, 60), (1, 90)),
            three_route_region(rng, kw),
            cross(40, 6, (1, 60), (1, 90)),
            striped,
            cross(8, 3, (1, 30), (1, 30)),                       # max_read_len / max_hap_len of 30 ...
            cross(6, 2, (200, 300), (500, 600), flag_rate=0.03), # ... next to 600
            cross(17, 5, (30, 120), (40, 160), flag_rate=0.3)]


class Mode:
    """One (fma_mode, tail mode): its context, its regions, and -- computed once, shared by the tests -- every region's
    oracle bytes and single-call bytes."""

    def __init__(self, fma_mode, tail):
        from gkl_amd import native
        from oracle.pdhmm import PdhmmOracle
        self.fma_mode, self.tail = fma_mode, tail
        self.ctx = native.PdhmmContext(fma_mode=fma_mode, reference_tail=bool(tail))
        self.regions = make_regions(acgt_reads=bool(tail))
        self.ref_batch = [REF_BATCHES[k % 3] if tail else 0 for k in range(len(self.regions))]
        oracle = PdhmmOracle()
        self.oracle, self.single, self.routing = [], [], []
        for (reads, haps), rb in zip(self.regions, self.ref_batch):
            expanded = expand_cross(reads, haps)
            if tail:
                st, exp = oracle.compute_reference(expanded, fma_mode=fma_mode, ref_batch=rb)
            else:
                st, exp = oracle.compute(expanded, semantics=SEMANTICS_OF_FMA_MODE[fma_mode])
            assert st == 0
            self.oracle.append(exp.tobytes())
            self.single.append(self.ctx.compute_cross(reads, haps, rb).tobytes())
            self.routing.append(self.ctx.last_routing())


@pytest.fixture(scope="module")
def modes():
    made = {}

    def get(fma_mode, tail):
        if (fma_mode, tail) not in made:
            made[(fma_mode, tail)] = Mode(fma_mode, tail)
        return made[(fma_mode, tail)]

    yield get
    for m in made.values():
        m.ctx.close()


def test_region_mix_is_what_the_cases_need():
    regions = make_regions(acgt_reads=True)
    shapes = [(r.batch, h.batch) for r, h in regions]
    assert shapes[:5] == [(90, 3), (1, 1), (6, 4), (40, 6), (5, 3)]
    assert int(regions[2][0].read_lengths.max()) == 400 and int(regions[4][0].read_lengths.max()) == 400
    assert sorted(int(x) for x in regions[4][0].read_lengths)[-2] <= 90
    assert regions[5][0].max_read_len <= 30 and regions[5][1].max_hap_len <= 30 and regions[6][1].max_hap_len >= 500
    # tail mode: with reference batches of 0, 13 and 8 pairs every region but the 1 x 1 has tails strictly inside it or at its end
    assert [REF_BATCHES[k % 3] for k in range(8)] == [0, 13, 8, 0, 13, 8, 0, 13]


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
@pytest.mark.parametrize("fma_mode", [1, 0], ids=["avx512-arith", "avx2-arith"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_multi_call_is_the_oracle_and_the_single_call(modes, K, fma_mode, tail):
    m = modes(fma_mode, tail)
    assert m.single == m.oracle                      # (the single call: what tests/test_pdhmm.py pins)
    got = m.ctx.compute_cross_multi(m.regions[:K], m.ref_batch[:K] if tail else None)
    assert len(got) == K
    for k in range(K):
        assert got[k].tobytes() == m.oracle[k], (K, k)
        assert got[k].tobytes() == m.single[k], (K, k)
    if K >= 3:   # the region whose haplotypes take all three routes
        tab, pred, odd = m.routing[2]
        assert tab >= 1 and pred >= 1 and odd == 1


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
def test_order_of_the_regions_does_not_matter(modes, tail):
    m = modes(1, tail)
    for seed in (1, 2):
        perm = [int(k) for k in np.random.RandomState(seed).permutation(len(m.regions))]
        got = m.ctx.compute_cross_multi([m.regions[k] for k in perm], [m.ref_batch[k] for k in perm])
        for at, k in enumerate(perm):
            assert got[at].tobytes() == m.single[k], (perm, at)
    # ... nor which others ride along: a sub-set, reversed
    pick = [6, 3, 0]
    got = m.ctx.compute_cross_multi([m.regions[k] for k in pick], [m.ref_batch[k] for k in pick])
    for at, k in enumerate(pick):
        assert got[at].tobytes() == m.single[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
def test_a_bad_region_fails_alone(modes, tail):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    m = modes(1, tail)
    reads, haps = m.regions[3]
    bad = PdhmmBatch.from_pairs(reads.pairs())
    bad.read_ins_qual = bad.read_ins_qual.copy()
    bad.read_ins_qual[11 * bad.max_read_len] = -1
    with pytest.raises(IllegalArgumentException) as single:
        m.ctx.compute_cross(bad, haps, m.ref_batch[3])
    assert str(single.value) == INPUT_ERROR_TEXT
    with pytest.raises(native.PdhmmMultiError) as e:
        m.ctx.compute_cross_multi([m.regions[0], (bad, haps), m.regions[4]], [m.ref_batch[0], m.ref_batch[3], m.ref_batch[4]])
    assert e.value.statuses == [native.OK, native.ERR_INVALID_ARG, native.OK]
    assert isinstance(e.value.errors[1], IllegalArgumentException) and str(e.value.errors[1]) == INPUT_ERROR_TEXT
    assert e.value.errors[0] is None and e.value.errors[2] is None and e.value.results[1] is None
    assert e.value.results[0].tobytes() == m.single[0] and e.value.results[2].tobytes() == m.single[4]
    # a region that fails the argument checks is left out before anything touches the device; the rest still run
    worse = PdhmmBatch.from_pairs(reads.pairs())
    worse.read_lengths = worse.read_lengths.copy()
    worse.read_lengths[0] = worse.max_read_len + 1
    with pytest.raises(native.PdhmmMultiError) as e:
        m.ctx.compute_cross_multi([(worse, haps), m.regions[1]], [0, m.ref_batch[1]])
    assert e.value.statuses == [native.ERR_INVALID_ARG, native.OK] and "read_lengths[0]" in str(e.value.errors[0])
    assert e.value.results[1].tobytes() == m.single[1]
    # the context computes clean calls afterwards
    got = m.ctx.compute_cross_multi(m.regions[:3], m.ref_batch[:3])
    assert [g.tobytes() for g in got] == m.single[:3]
    assert m.ctx.compute_cross(*m.regions[3], m.ref_batch[3]).tobytes() == m.single[3]


@pytest.mark.gpu
def test_one_call_of_eight_regions_is_one_launch_set(modes):
    from gkl_amd import native
    m = modes(1, 1)
    before = native.pdhmm_combine_counts()
    got = m.ctx.compute_cross_multi(m.regions, m.ref_batch)
    after = native.pdhmm_combine_counts()
    assert tuple(a - b for a, b in zip(after, before)) == (8, 8, 1)
    assert [g.tobytes() for g in got] == m.single
    assert m.ctx.last_routing() == tuple(sum(r[i] for r in m.routing) for i in range(3))
    assert m.ctx.last_kernel_ms() > 0.0
    # a single region through the multi entry point shares nothing; single calls count as launch sets of their own
    before = after
    m.ctx.compute_cross_multi(m.regions[:1], m.ref_batch[:1])
    m.ctx.compute_cross(*m.regions[1], m.ref_batch[1])
    assert tuple(a - b for a, b in zip(native.pdhmm_combine_counts(), before)) == (2, 0, 2)


@pytest.mark.gpu
def test_a_call_over_the_pair_limit_is_computed_region_by_region(modes):
    from gkl_amd import native
    m = modes(1, 1)
    rng = np.random.RandomState(73)
    kw = dict(with_n=False, lower=False)
    big = (random_pd_batch(rng, 1024, read_len=(1, 12), hap_len=(1, 2), **kw),
           random_pd_batch(rng, 128, read_len=(1, 2), hap_len=(1, 12), **kw))          # 131 072 pairs: the limit itself
    want_big = m.ctx.compute_cross(*big, 0)
    routing_big = m.ctx.last_routing()
    before = native.pdhmm_combine_counts()
    got = m.ctx.compute_cross_multi([big], [0])                                          # at the limit: one shared launch set
    assert got[0].tobytes() == want_big.tobytes()
    mid = native.pdhmm_combine_counts()
    assert tuple(a - b for a, b in zip(mid, before)) == (1, 0, 1)
    got = m.ctx.compute_cross_multi([big, m.regions[1]], [0, m.ref_batch[1]])            # one pair over it
    assert got[0].tobytes() == want_big.tobytes() and got[1].tobytes() == m.single[1]
    assert tuple(a - b for a, b in zip(native.pdhmm_combine_counts(), mid)) == (2, 0, 2)
    assert m.ctx.last_routing() == tuple(a + b for a, b in zip(routing_big, m.routing[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("fma_mode", [1, 0], ids=["avx512-arith", "avx2-arith"])
def test_full_haplotype_groups_across_many_regions(fma_mode):
    """Eight regions of 66 long reads (a chunk each) x 48 haplotypes are 25 344 (haplotype, chunk) jobs in the table launch:
    enough for groups of two haplotypes per unit, which no single one of them (3168 jobs) gets -- rows set up once per
    group, matrices restarted per haplotype.  Every region must still give the single call's bytes."""
    from gkl_amd import native
    rng = np.random.RandomState(79)
    acgt = np.frombuffer(b"ACGT", dtype=np.int8)
    one = np.zeros(1, np.int8)
    haps = []
    for k in range(48):
        H = int(rng.randint(20, 41))
        b = acgt[rng.randint(0, 4, H)].copy()
        pd = np.zeros(H, np.int8)
        j = int(rng.randint(2, H - 8))
        b[j], pd[j] = acgt[1], 1 | 5 << 3                # one SNP kind for all: a common class list
        if k % 3 == 0:
            pd[j + 2], pd[j + 5] = 2, 4                  # a deletion
        haps.append((b, pd, one, one, one, one, one))
    haps = PdhmmBatch.from_pairs(haps)
    regions = [(random_pd_batch(rng, 66, read_len=(330, 380), hap_len=(1, 2)), haps) for _ in range(2)]
    with native.PdhmmContext(fma_mode=fma_mode, reference_tail=False) as c:
        want = [c.compute_cross(*r).tobytes() for r in regions]
        assert c.last_routing() == (48, 0, 0)
        got = c.compute_cross_multi([regions[k % 2] for k in range(8)])
        assert c.last_routing() == (8 * 48, 0, 0)
        for k in range(8):
            assert got[k].tobytes() == want[k % 2], k


@pytest.mark.gpu
def test_cross_check_build_agrees(modes):
    from gkl_amd import native
    m = modes(1, 0)
    cxx = os.path.join(os.path.dirname(native.PDHMM_LIB_PATH), "libgklhip_pdhmm_cxx.so")
    assert os.path.exists(cxx), "make -C gkl_amd/csrc builds it"
    with native.PdhmmContext(fma_mode=1, reference_tail=False, lib_path=cxx) as c:
        got = c.compute_cross_multi(m.regions)
        assert [g.tobytes() for g in got] == m.oracle
    # the counts are the library's own: the cross-check build counted its call, the product library did not
    assert native.pdhmm_combine_counts(lib_path=cxx)[2] >= 1

"""PDHMM on the MI355X at its edges: stripe seams (up to four stripes: both carry buffers reused), carry columns flushed in
chunks of 64, the packed geometry's corners, every quality byte, gradual underflow.  The oracle is the expected value
everywhere, bit for bit; tests/test_pdhmm_edge_inputs_cpu.py shows that the inputs (tests/pdhmm_edge_inputs.py) can tell a
right kernel from a wrong one: no expected value of groups A to D is -inf, and every stripe seam moves the result."""
import os

import numpy as np
import pytest

from gkl_amd.pdhmm_batch import PdhmmBatch
from tests import pdhmm_edge_inputs as E
from tests.test_gpu_parity import REL_TOL
from tests.test_pdhmm import SEMANTICS_OF_FMA_MODE, expected_per_position, pd_ctx, pd_oracle  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
FMA_MODES = pytest.mark.parametrize("fma_mode", [1, 0], ids=["avx512-arith", "avx2-arith"])


@pytest.fixture(scope="module")
def native():
    from gkl_amd import native as n
    return n


@pytest.fixture(scope="module")
def want(pd_oracle):  # noqa: F811
    """want(name, batch, sem): the oracle's values, computed once per (name, semantics) and handed out read-only."""
    made = {}

    def get(name, batch, sem):
        if (name, sem) not in made:
            st, v = pd_oracle.compute(batch() if callable(batch) else batch, semantics=sem)
            assert st == 0, name
            v.setflags(write=False)
            made[(name, sem)] = v
        return made[(name, sem)]

    return get


@pytest.fixture(scope="module")
def inputs():
    """The groups' batches, built once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = {"A": E.stripe_batch, "B": E.carry_batch, "C": E.packed_batch, "D": E.quality_batch,
                          "packed": lambda: E.ladder_batch("packed"), "striped": lambda: E.ladder_batch("striped")}[name]()
        return made[name]

    return get


def cxx_path(native):
    cxx = os.path.join(os.path.dirname(native.PDHMM_LIB_PATH), "libgklhip_pdhmm_cxx.so")
    assert os.path.exists(cxx), "make -C gkl_amd/csrc builds it"
    return cxx


def same_bits(got, exp, what=""):
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())


# ------------------------------------------------------------------ 1. stripes, paired entry point
def test_stripes_paired(pd_ctx, want, inputs):  # noqa: F811
    b = inputs("A")
    exp = want("A", b, pd_ctx.sem)
    assert np.isfinite(exp).all()
    same_bits(pd_ctx.compute(b), exp, "batch")
    perm = np.random.RandomState(1).permutation(b.batch)
    same_bits(pd_ctx.compute(b.subset(perm)), exp[perm], "permuted")
    alone = [k for k in range(b.batch) if b.read_lengths[k] in (1152, 1153)]   # four stripes, in a call of one pair
    assert len(alone) == 2 * E.PAIRS_PER_R
    for k in alone:
        same_bits(pd_ctx.compute(b.subset([k])), exp[[k]], f"pair {k} alone")


# ------------------------------------------------------------------ 2. carry columns
def test_carry_columns(pd_ctx, want, inputs):  # noqa: F811
    b = inputs("B")
    exp = want("B", b, pd_ctx.sem)
    assert np.isfinite(exp).all()
    same_bits(pd_ctx.compute(b), exp)


@FMA_MODES
def test_carry_columns_stale_behind_a_short_haplotype(native, want, inputs, fma_mode):
    # one context: its carry rows first hold 193 columns of a long haplotype's jobs, then jobs of 1..5 columns run over them
    b = inputs("B")
    exp = want("B", b, SEMANTICS_OF_FMA_MODE[fma_mode])
    long_ = np.flatnonzero(b.hap_lengths == 193)
    short = np.flatnonzero(b.hap_lengths <= 5)
    assert long_.size == 3 and short.size == 15
    with native.PdhmmContext(fma_mode=fma_mode, reference_tail=False) as c:
        same_bits(c.compute(b.subset(long_)), exp[long_], "H = 193")
        same_bits(c.compute(b.subset(short)), exp[short], "H <= 5 after H = 193")
        same_bits(c.compute(b), exp, "mixed")
        back = np.arange(b.batch)[::-1]
        same_bits(c.compute(b.subset(back)), exp[back], "mixed, reversed")


# ------------------------------------------------------------------ 3. stripes through the other routes
CROSS_H = 1180   # the three kinds of haplotype, long enough for a related read of 1153 bases


@pytest.fixture(scope="module")
def stripe_cross():
    """(reads, haplotypes, expanded pairs): reads of 384, 768 and 1153 bases and ten short ones x the three kinds."""
    base, haps = E.kind_haps(seed=6005, H=CROSS_H)
    rng = np.random.RandomState(6006)
    reads = []
    for R in E.CARRY_R + [1, 5, 6, 7, 30, 64, 100, 151, 200, 383]:
        q = lambda lo, hi: rng.randint(lo, hi + 1, R).astype(np.int8)  # noqa: E731
        reads.append((E.related_read(rng, base, R), q(20, 40), q(30, 45), q(30, 45), q(8, 12)))
    return (*E.sides_as_batches(reads, haps), E.cross_pairs(reads, haps))


def test_stripes_cross_route(pd_ctx, want, stripe_cross):  # noqa: F811
    reads, haps, pairs = stripe_cross
    exp = want("stripe cross", pairs, pd_ctx.sem)
    assert np.isfinite(exp).all()
    same_bits(pd_ctx.compute_cross(reads, haps), exp)
    tab, pred, odd = pd_ctx.last_routing()
    assert tab > 0 and pred > 0 and odd > 0, (tab, pred, odd)      # striped reads x haplotypes: listed jobs of the full kernel


def test_stripes_multi_region_route(pd_ctx, want, stripe_cross):  # noqa: F811
    reads, haps, pairs = stripe_cross
    exp = want("stripe cross", pairs, pd_ctx.sem)
    got = pd_ctx.compute_cross_multi([(reads, haps), (reads, haps)])
    assert len(got) == 2
    for k in range(2):
        same_bits(got[k], exp, f"region {k}")


def test_stripes_device_resident_route(native, pd_ctx, want, inputs):  # noqa: F811
    import torch
    b = inputs("A")
    exp = want("A", b, pd_ctx.sem)
    sums = torch.empty(b.batch, dtype=torch.float64, device="cuda:0")
    out = pd_ctx.compute_device(native.PdhmmDeviceBatch.upload(b, "cuda:0"), sums=sums)
    torch.cuda.synchronize()
    same_bits(native.pdhmm_finalise_host(sums.cpu()), exp, "sums, finalised on the host")
    assert np.all(np.abs(out.cpu().numpy() - exp) <= REL_TOL * np.abs(exp))      # the device's own log10


def test_stripes_cxx_build(native, pd_ctx, want, inputs):  # noqa: F811
    b = inputs("A")
    with native.PdhmmContext(fma_mode=pd_ctx.fma_mode, reference_tail=False, lib_path=cxx_path(native)) as c:
        same_bits(c.compute(b), want("A", b, pd_ctx.sem))


@FMA_MODES
def test_stripes_in_the_reference_tail(native, pd_oracle, inputs, fma_mode):  # noqa: F811
    # 13 pairs: the last five (AVX-512 arithmetic: 13 mod 8) / the last one (AVX2: 13 mod 4) take the scalar engine's
    # arithmetic as tail jobs -- striped ones, of two, three and four stripes
    b = inputs("A")
    idx = [0, 3, 4, 7, 10, 13, 16, 19, 22, 27, 30, 36, 39]
    sub = b.subset(idx)
    assert [E.n_stripes(int(r)) for r in sub.read_lengths[-5:]] == [2, 3, 3, 4, 4]
    st, exp = expected_per_position(pd_oracle, sub, SEMANTICS_OF_FMA_MODE[fma_mode], 8 if fma_mode else 4)
    assert st == 0 and np.isfinite(exp).all()
    with native.PdhmmContext(fma_mode=fma_mode) as c:              # the default mode
        same_bits(c.compute(sub), exp)


# ------------------------------------------------------------------ 4. packed geometry
def test_packed_geometry(pd_ctx, want, inputs):  # noqa: F811
    b = inputs("C")
    exp = want("C", b, pd_ctx.sem)
    assert np.isfinite(exp).all()
    same_bits(pd_ctx.compute(b), exp, "paired")
    reads, haps = E.packed_sides()
    exp_x = want("C cross", E.cross_pairs(reads, haps), pd_ctx.sem)
    same_bits(pd_ctx.compute_cross(*E.sides_as_batches(reads, haps)), exp_x, "cross")


# ------------------------------------------------------------------ 5. quality bytes
def test_quality_bytes_paired(native, pd_ctx, want, inputs, monkeypatch):  # noqa: F811
    b = inputs("D")
    exp = want("D", b, pd_ctx.sem)
    assert np.isfinite(exp).all() and sorted({E.n_stripes(int(r)) for r in b.read_lengths}) == [1, 2]   # packed and striped reads
    same_bits(pd_ctx.compute(b), exp, "all kinds")
    table = np.arange(0, b.batch, len(E.HAP_KINDS))                 # the pairs over the haplotype of at most six classes
    same_bits(pd_ctx.compute(b.subset(table)), exp[table], "table kind")
    tab, pred, full = pd_ctx.last_routing()
    assert tab > 0 and pred == 0 and full == 0, (tab, pred, full)
    with native.PdhmmContext(fma_mode=pd_ctx.fma_mode, reference_tail=False, lib_path=cxx_path(native)) as c:
        same_bits(c.compute(b), exp, "C++ build")
    monkeypatch.setenv("GKL_HIP_PDHMM_TABLE", "0")
    with native.PdhmmContext(fma_mode=pd_ctx.fma_mode, reference_tail=False) as c:
        same_bits(c.compute(b), exp, "table route off")
        assert c.last_routing()[0] == 0 and c.last_routing()[1] > 0


def test_quality_bytes_cross(pd_ctx, want, inputs):  # noqa: F811
    b = inputs("D")
    _, reads, haps = E.quality_sides()
    same_bits(pd_ctx.compute_cross(*E.sides_as_batches(reads, haps)), want("D", b, pd_ctx.sem))
    assert pd_ctx.last_routing() == (1, 1, 1)


@FMA_MODES
def test_quality_bytes_in_the_reference_tail(native, pd_oracle, inputs, fma_mode):  # noqa: F811
    # 27 pairs: the last three take the scalar engine's arithmetic in either mode.  Base-quality byte -1 has no reference
    # value (E.holds_byte_255): its pairs go to the front; the tail holds base qualities 0..127 (packed), the insertion /
    # deletion corners and the gap-continuation bytes (both striped), one on each kind of haplotype
    b = inputs("D")
    names, _, _ = E.quality_sides()
    n_kinds = len(E.HAP_KINDS)
    tail = [names.index("qual 0..127, 128 bases") * n_kinds + 0, names.index("ins up, del down, 400 bases") * n_kinds + 1,
            names.index("gcp 0..127, 400 bases") * n_kinds + 2]
    order = [k for k in range(b.batch) if k not in tail] + tail
    sub = b.subset(order)
    assert not E.holds_byte_255(sub)[-3:].any() and sub.batch % 8 == sub.batch % 4 == 3
    st, exp = expected_per_position(pd_oracle, sub, SEMANTICS_OF_FMA_MODE[fma_mode], 8 if fma_mode else 4)
    assert st == 0 and np.isfinite(exp).all()
    with native.PdhmmContext(fma_mode=fma_mode) as c:              # the default mode
        same_bits(c.compute(sub), exp)


def test_negative_gap_bytes_are_input_errors(native, pd_ctx, want, inputs):  # noqa: F811
    a = inputs("A")
    pick = [int(np.flatnonzero(a.read_lengths == R)[0]) for R in (383, 1153)]
    good = a.subset(pick)
    exp = want("A", a, pd_ctx.sem)[pick]
    for k, row in ((1, 1152), (1, 0), (0, 382)):                    # last row of four stripes, its first row, row 383 of a packed read
        for name in ("read_ins_qual", "read_del_qual", "gcp"):
            bad = good.subset([0, 1])
            arr = getattr(bad, name).reshape(2, bad.max_read_len).copy()
            arr[k, row] = -1 if name == "gcp" else -128
            setattr(bad, name, arr.reshape(-1))
            with pytest.raises(native.IllegalArgumentException):
                pd_ctx.compute(bad)
            same_bits(pd_ctx.compute(good), exp, f"after {name}[{row}] < 0")


# ------------------------------------------------------------------ 6. gradual underflow
def ladder_sides(b):
    one = np.zeros(1, np.int8)
    p = b.pairs()
    return (PdhmmBatch.from_pairs([(one, one, *x[2:]) for x in p]), PdhmmBatch.from_pairs([(*p[0][:2], one, one, one, one, one)]))


def check_ladder(got, exp, what):
    assert not np.isnan(got).any(), what
    assert not np.isneginf(got[np.isfinite(exp)]).any(), (what, "flushed to zero")
    same_bits(got, exp, what)


@pytest.mark.parametrize("which", ["packed", "striped"])
def test_gradual_underflow(native, pd_ctx, want, inputs, monkeypatch, which):  # noqa: F811
    b = inputs(which)
    exp = want(which, b, pd_ctx.sem)
    lo, hi = E.SUBNORMAL_WINDOW
    assert int(((exp > lo) & (exp < hi)).sum()) >= 4 and int(np.isneginf(exp).sum()) >= 2   # subnormal sums, and sums of 0
    check_ladder(pd_ctx.compute(b), exp, "paired")
    if which == "packed":
        assert pd_ctx.last_routing()[0] > 0                         # the table kernel (the whole-job program)
    check_ladder(pd_ctx.compute_cross(*ladder_sides(b)), exp, "cross")
    if which == "packed":
        with native.PdhmmContext(fma_mode=pd_ctx.fma_mode, reference_tail=False, lib_path=cxx_path(native)) as c:
            check_ladder(c.compute(b), exp, "C++ build")
        monkeypatch.setenv("GKL_HIP_PDHMM_TABLE", "0")
        with native.PdhmmContext(fma_mode=pd_ctx.fma_mode, reference_tail=False) as c:
            check_ladder(c.compute(b), exp, "table route off")
            assert c.last_routing()[0] == 0

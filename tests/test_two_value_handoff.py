"""The two-value hand-off of the whole-job asm programs f32r8 and f64r10 (tools/gen_fwd_asm.py: `handoff`).

A lane used to fetch the bottom row M, X, Y of the lane above and compute row 0's X and M-inner from it; now the lane
above computes those two values with the lower lane's coefficients and sends them: one DPP less per fp32 step, two less
per fp64 step, the same operations in the same order on the same values -- so every bit must stay what it was.
The same two programs keep no running sum of M: the bottom row's Y of a read's last lane carries it (pMY = pYY = 1).

The static tests count the instructions of the generated programs.  The GPU tests compare the asm programs with the
oracle and with the all-C++ build of the library (libgklhip_pairhmm_cxxfast.so) bit for bit -- raw fp32 sums, raw fp64
sums, fallback flags, final doubles -- on batches built for the seams the change moves: the lane below a read's last
lane (masked: it must receive +0 whatever its neighbour holds), first lanes, separators in flight, the Y0 insertion.
Which reads share a chunk, and in which order, is the planner's decision (best fit, longest first): the batches hold
many reads of every lane count, in several compositions, so that reads of all sizes end up abutting."""
import importlib.util
import os

import numpy as np
import pytest

from gkl_amd.batch import FlatBatch
from gkl_amd.synth import make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_fwd_asm", os.path.join(ROOT, "tools", "gen_fwd_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def _fast_steps(g, c):
    """the instructions of each fast step of the unrolled block of program(c, False): a step starts at the v_and_or_b32
    that forms the lane's stream entry"""
    prog = g.program(c, False)
    lo = prog.index("80:")
    hi = prog.index("81:")
    starts = [i for i in range(lo, hi) if prog[i].startswith("v_and_or_b32")]
    assert len(starts) == g.U
    ends = starts[1:] + [hi]
    return [prog[a:b] for a, b in zip(starts, ends)]


@pytest.mark.parametrize("name,f64,R,n_dpp", [("f32r8", False, 8, 3), ("f64r10", True, 10, 5)])
def test_fast_steps_carry_two_values(name, f64, R, n_dpp):
    g = _gen()
    c = g.Cfg(name, f64, R, True)
    steps = _fast_steps(g, c)
    for u, st in enumerate(steps):
        dpp = [i for i in st if "_dpp" in i]
        # (the last step of a block shifts no stream entry: the next block's prologue does it -- one DPP either way)
        assert len(dpp) + (1 if u == g.U - 1 else 0) == n_dpp, (name, u, dpp)
        # the DPPs stay grouped behind one s_nop 1
        first = st.index(dpp[0])
        assert st[first - 1] == "s_nop 1" and st[first:first + len(dpp)] == dpp, (name, u)
    # arithmetic instructions per step: 8 per cell (five of them moved one lane up) + the running sum of X; the sum of M
    # rides in the bottom row's Y of a read's last lane, so nothing adds into the register that held it
    sm = c.v(c.SM) + ","
    for st in steps:
        arith = [i for i in st if i.split()[0] in (f"v_mul_f{64 if f64 else 32}", f"v_fmac_f{64 if f64 else 32}",
                                                   f"v_fma_f{64 if f64 else 32}", f"v_add_f{64 if f64 else 32}")]
        assert len(arith) == 8 * R + 1, (name, len(arith))
    prog = g.program(c, False)
    assert not [i for i in prog if i.startswith("v_") and i.split()[1] == sm], name
    assert [i for i in g.program(c, True) if i.startswith("v_add_f") and i.split()[1] == sm], "the wide variant keeps its sum"


@pytest.mark.parametrize("name,f64,R,n_dpp,n_mov", [("f32r8", False, 8, 3, 2), ("f64r10", True, 10, 5, 4)])
def test_general_step_carries_two_values(name, f64, R, n_dpp, n_mov):
    g = _gen()
    c = g.Cfg(name, f64, R, True)
    gs = g.general_step(c, "s72", 100, two=c.two)
    assert sum(1 for i in gs if "_dpp" in i) == n_dpp
    state = set(c.NX + c.NI + [r + 1 for r in c.NX + c.NI])
    movs = [i for i in gs if i.startswith("v_mov_b32") and int(i.split()[1].strip("v,")) in state]
    assert len(movs) == n_mov, movs


def test_the_other_programs_keep_three_values():
    """wide, narrow and unfused programs and the fast blocks of the round-3 arrangement: the hand-off they had"""
    g = _gen()
    for name, f64, R, fma, wide in (("f32r8", False, 8, True, True), ("f64r10", True, 10, True, True), ("f64r8", True, 8, True, False),
                                    ("f32r4", False, 4, True, False), ("f64r6", True, 6, True, False), ("f32r8", False, 8, False, False),
                                    ("f64r10", True, 10, False, False)):
        c = g.Cfg(name, f64, R, fma)
        gs = g.general_step(c, "s72", 100, wide, c.two and not wide)
        assert sum(1 for i in gs if "_dpp" in i) == 1 + 3 * c.w, (c.name, wide)
    o = []
    g.legacy_fast(o)
    assert sum(1 for i in o if "_dpp" in i) == 1 + (g.U - 1) + 3 * g.U   # the entry shifts (prologue, seven steps) + 3 values x 8 steps


# ---- GPU: bit for bit --------------------------------------------------------------------------------------------

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def batch_of(rng, read_lens, hap_lens, alphabet=b"ACGT", qual_range=(10, 45)):
    """reads of exactly these lengths, 70 % of them cut from a haplotype that is long enough (3 % of bases flipped)"""
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    haps = [alpha[rng.randint(0, alpha.size, size=int(n))] for n in hap_lens]
    rb, q = [], [[], [], [], []]
    for R in read_lens:
        R = int(R)
        h = haps[int(rng.randint(0, len(haps)))]
        if h.size >= R and rng.random_sample() < 0.7:
            off = int(rng.randint(0, h.size - R + 1))
            b = h[off:off + R].copy()
            flip = rng.random_sample(R) < 0.03
            b[flip] = alpha[rng.randint(0, alpha.size, size=int(flip.sum()))]
        else:
            b = alpha[rng.randint(0, alpha.size, size=R)]
        rb.append(b)
        for dst in q:
            dst.append(rng.randint(qual_range[0], qual_range[1] + 1, size=R).astype(np.uint8))
    read_off = np.zeros(len(read_lens) + 1, np.int64)
    read_off[1:] = np.cumsum([int(x) for x in read_lens])
    hap_off = np.zeros(len(haps) + 1, np.int64)
    hap_off[1:] = np.cumsum([h.size for h in haps])
    cat = lambda xs: np.concatenate(xs).astype(np.uint8)  # noqa: E731
    return FlatBatch(len(read_lens), len(haps), read_off, hap_off, cat(rb), cat(q[0]), cat(q[1]), cat(q[2]), cat(q[3]),
                     cat(haps), {"kind": "handoff"})


def lens_for_lanes(rng, lanes, rpl):
    """read lengths that take exactly `lanes` lanes at `rpl` rows per lane: ceil((R + 1) / rpl) lanes, the pad row included"""
    out = []
    for n in lanes:
        lo, hi = max(1, rpl * (int(n) - 1)), rpl * int(n) - 1
        out.append(int(rng.randint(lo, hi + 1)))
    return out


def seam_batches(rpl):
    """(name, batch, reads whose own result is not compared) for `rpl` rows per lane (8: the fp32 kernel, 10: fp64)"""
    rng = np.random.RandomState(1700 + rpl)
    out = []
    # reads of 1 .. 32 lanes, every count several times, in three compositions (shuffled; a heavy tail of small reads that
    # fill the gaps behind the long ones; pairs n + (64 - n) that fill a chunk exactly)
    every = np.repeat(np.arange(1, 33), 3)
    rng.shuffle(every)
    out.append(("lanes 1..32 shuffled", batch_of(rng, lens_for_lanes(rng, every, rpl), rng.randint(330, 600, size=7)), []))
    tail = np.concatenate([np.arange(1, 33), rng.randint(1, 5, size=90)])
    rng.shuffle(tail)
    out.append(("lanes 1..32 + small", batch_of(rng, lens_for_lanes(rng, tail, rpl), rng.randint(330, 600, size=6)), []))
    pairs = np.concatenate([[n, 64 - n] for n in range(1, 33)])
    out.append(("lanes n + (64 - n)", batch_of(rng, lens_for_lanes(rng, pairs, rpl), rng.randint(640, 900, size=5)), []))
    # single-lane reads: every lane is a first lane
    out.append(("single-lane reads", batch_of(rng, rng.randint(1, rpl, size=300), rng.randint(10, 300, size=8)), []))
    # overflowing reads (insertion and deletion quality 0) among healthy ones, of many lane counts: in some chunk a read's
    # first lane sits directly below an overflowing read's last lane
    lanes = rng.randint(1, 20, size=120)
    b = batch_of(rng, lens_for_lanes(rng, lanes, rpl), rng.randint(300, 520, size=4), qual_range=(20, 40))
    bad = [r for r in range(b.n_reads) if r % 4 == 1 and lanes[r] >= 12]
    for r in bad:
        lo, hi = int(b.read_off[r]), int(b.read_off[r + 1])
        b.ins_gop[lo:hi] = 0
        b.del_gop[lo:hi] = 0
        b.gcp[lo:hi] = 60
    assert len(bad) >= 5
    out.append(("below an overflowing read", b, bad))
    # haplotypes shorter than the array is deep: several separators in flight
    out.append(("short haplotypes", batch_of(rng, lens_for_lanes(rng, rng.randint(1, 33, size=100), rpl), rng.randint(3, 30, size=24)), []))
    # haplotypes of one and two bases
    out.append(("haplotypes of 1 and 2 bases", batch_of(rng, lens_for_lanes(rng, rng.randint(1, 33, size=80), rpl), [1, 2, 1, 2, 2, 1, 40]), []))
    # 'N' and odd bytes
    out.append(("N and odd bytes", batch_of(rng, lens_for_lanes(rng, rng.randint(1, 33, size=90), rpl), rng.randint(60, 600, size=9),
                                            alphabet=b"ACGTNacgtRY", qual_range=(0, 255)), []))
    return out


def compare(native, oracle, use_double, name, b, skip_reads):
    cxx = os.path.join(os.path.dirname(native.LIB_PATH), "libgklhip_pairhmm_cxxfast.so")
    assert os.path.exists(cxx), "make -C gkl_amd/csrc builds it"
    keep = np.ones(b.n_pairs, bool)
    for r in skip_reads:
        keep[r * b.n_haps:(r + 1) * b.n_haps] = False
    res = []
    for lib in (None, cxx):
        with native.PairHmmContext(use_double=use_double, rows_per_lane=8, lib_path=lib) as c:
            out = c.compute(b).copy()
            r32, r64, u = [x.copy() for x in c.raw(b.n_pairs)]
        res.append((out, r32, r64, u))
    oo, o32, o64, ou = oracle.batch(b, use_double=use_double, want_raw=True, n_threads=8)
    for which, (out, r32, r64, u) in zip(("asm", "cxx"), res):
        tag = (name, which, "fp64" if use_double else "fp32")
        assert np.array_equal(u[keep], ou[keep]), tag
        if not use_double:
            assert np.array_equal(bits(r32[keep]), bits(o32[keep])), tag
        fb = keep & (ou == 1)
        assert np.array_equal(bits(r64[fb]), bits(o64[fb])), tag
        assert np.array_equal(bits(out[keep]), bits(oo[keep])), tag


@pytest.mark.gpu
@pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
def test_seams_bit_for_bit(oracle, use_double):
    from gkl_amd import native
    # (fp32 contexts run their fallback pairs through the fp64 program too: both lane geometries in both modes)
    for rpl in (8, 10):
        for name, b, skip_reads in seam_batches(rpl):
            compare(native, oracle, use_double, name, b, skip_reads)


@pytest.mark.gpu
@pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
def test_planned_fp64_pass_bit_for_bit(oracle, use_double):
    """one `hc` batch above 65 536 pairs: the planned kernels, the packed fp64 pass in the f64r10 program"""
    from gkl_amd import native
    b = make_batch("hc", 1100, 64, seed=77)
    assert b.n_pairs > 65536
    compare(native, oracle, use_double, "hc 1100 x 64", b, [])
    if not use_double:
        with native.PairHmmContext() as c:
            c.compute(b)
            u = c.raw(b.n_pairs)[2]
        assert 0 < int(u.sum()) < u.size, "the batch should take both precisions"

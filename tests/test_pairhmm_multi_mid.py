"""Mid-size PairHMM regions (2049 - 65 536 pairs: the per-pair policy in two launches) in shared sets of one
gklhip_compute_multi call: prep_multi_kernel, fwd_stream_multi_kernel, pair_flag_multi_kernel and
pair_recompute_multi_kernel<fma, MAXR>.  Region k's output is, byte for byte, what the oracle computes and what the single
call writes for it on the same context, whichever other regions share its set, in both fma modes; the combiner's counters
say which sets formed.  Mid-size regions share sets among themselves only, and one alone is no set.

Shapes: the smallest at which these kernels can go wrong -- reads of 10-20 bases against haplotypes of 20-30 wherever a
case does not need longer ones; every region is just above 2048 pairs except the two at the upper limit."""
import dataclasses
import os

import numpy as np
import pytest

from gkl_amd.synth import make_batch, random_batch

pytestmark = pytest.mark.gpu

# the mid-size regions that qualify for a shared set, without the biggest one
QUALIFYING = ["m2049", "m2304", "m_allfb", "m_nofb", "m_r4", "m_r6", "m_odd"]
ROWS2 = ["m2049", "m2304", "m_nofb", "m_odd", "m_allfb"]
SHORT = dict(read_len=(10, 20), hap_len=(20, 30))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def six_arrays_bytes(b):
    up = lambda x: (int(x) + 255) // 256 * 256  # noqa: E731
    return 5 * up(b.read_off[-1]) + up(b.hap_off[-1])


def build_pool():
    rng = np.random.RandomState(68)
    return {
        "m2049": random_batch(rng, 683, 3, **SHORT),                        # the first mid-size count; the last flag block holds one pair
        "m2304": random_batch(rng, 64, 36, **SHORT),                        # exactly nine full flag blocks
        # every pair fails the policy: the list is the whole region, 1050 recomputing blocks take two pairs each
        "m_allfb": random_batch(rng, 50, 42, read_len=(100, 120), hap_len=(120, 160), qual_range=(20, 40), related=False),
        "m_nofb": make_batch("region", 70, 30, seed=4, **SHORT),            # no pair falls back: count 0
        # MAXR 4 and MAXR kRplF64 (a read that was cut from one haplotype underflows against most of the others: both kinds of pair)
        "m_r4": random_batch(rng, 70, 30, read_len=(130, 250), hap_len=(250, 270), qual_range=(10, 45)),
        "m_r6": random_batch(rng, 70, 30, read_len=(260, 383), hap_len=(383, 400), qual_range=(10, 45)),
        "m_odd": random_batch(rng, 69, 30, alphabet=b"ACGTNacgtRY", qual_range=(0, 255)),     # N, odd bytes, every quality byte
        "m_top": random_batch(rng, 256, 256, **SHORT),                      # 65 536 pairs: the last size that qualifies
        "m_over": random_batch(rng, 257, 256, **SHORT),                     # runs alone
        "m_big_in": random_batch(rng, 2200, 1, read_len=(100, 110), hap_len=(20, 30)),        # inputs above 1 MB: runs alone
        # small regions (tests/test_pairhmm_multi.py's shapes)
        "s_r2": make_batch("hc", 12, 3, seed=4, read_len=(20, 90), hap_len=(60, 120)),
        "s_nofb": make_batch("region", 10, 4, seed=4),
        "s_odd": random_batch(rng, 8, 3, alphabet=b"ACGTNacgtRY", qual_range=(0, 255)),
    }


class Pool:
    def __init__(self, oracle):
        self.batch = build_pool()
        # (out, raw32, raw64, used64) per fma mode, computed once
        self.want = {fma: {name: oracle.batch(b, fma_mode=fma, want_raw=True, n_threads=4) for name, b in self.batch.items()}
                     for fma in (0, 1)}
        self.ctx = {}
        self.singles = {}

    def context(self, fma, rows_per_lane=0):
        from gkl_amd import native
        key = (fma, rows_per_lane)
        if key not in self.ctx:
            self.ctx[key] = native.PairHmmContext(fma_mode=fma, rows_per_lane=rows_per_lane)
            self.singles[id(self.ctx[key])] = {}
        return self.ctx[key]

    def single(self, ctx, name):
        """The single call's output on this context (computed once per context and region)."""
        cache = self.singles.setdefault(id(ctx), {})
        if name not in cache:
            cache[name] = ctx.compute(self.batch[name])
        return cache[name]

    def check(self, ctx, fma, names, got):
        """Every region: the oracle's bytes and the bytes of the single call on the same context."""
        assert len(got) == len(names)
        for k, (name, out) in enumerate(zip(names, got)):
            assert np.array_equal(bits(out), bits(self.want[fma][name][0])), (k, name, "oracle")
            assert out.tobytes() == self.single(ctx, name).tobytes(), (k, name, "single call")

    def run(self, ctx, names):
        """One multi call and the combiner's counts for it (the single calls it is compared with are made before)."""
        from gkl_amd import native
        for n in set(names):
            self.single(ctx, n)
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([self.batch[n] for n in names])
        return got, native.small_call_counts(0)

    def n_fallback(self, fma, names):
        return int(sum(int(self.want[fma][n][3].sum()) for n in names))

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def pool(oracle):
    p = Pool(oracle)
    yield p
    p.close()


def test_the_pool_holds_what_it_says(pool):
    b = pool.batch
    pairs = {n: b[n].n_pairs for n in b}
    assert (pairs["m2049"], pairs["m2304"], pairs["m_allfb"], pairs["m_top"], pairs["m_over"]) == (2049, 2304, 2100, 65536, 65792)
    for n in QUALIFYING + ["m_big_in"]:
        assert 2048 < pairs[n] <= 65536, n
    for n in ("s_r2", "s_nofb", "s_odd"):
        assert pairs[n] <= 2048, n
    for n in QUALIFYING + ["m_top", "m_over"]:
        assert six_arrays_bytes(b[n]) <= 1 << 20, n
    assert six_arrays_bytes(b["m_big_in"]) > 1 << 20
    for n in ROWS2 + ["m_top", "m_over", "m_big_in"]:
        assert int(b[n].read_lens.max()) <= 127, n
    assert 128 <= int(b["m_r4"].read_lens.max()) <= 255
    assert 256 <= int(b["m_r6"].read_lens.max()) <= 383
    assert int(b["m_r4"].read_lens.min()) >= 128 and int(b["m_r6"].read_lens.min()) >= 256
    for fma in (0, 1):
        w = pool.want[fma]
        assert w["m_allfb"][3].all(), "every pair of `m_allfb` must fall back to fp64: change the seed"
        assert not w["m_nofb"][3].any(), "no pair of `m_nofb` may fall back: change the seed"
        # both kinds of pair in the regions whose lists are neither empty nor everything
        for n in ("m2049", "m2304", "m_odd", "m_top", "m_r4", "m_r6"):
            assert 0 < int(w[n][3].sum()) < pairs[n], n


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [2, 3, 64, 65])
def test_set_sizes_and_counters(pool, K, fma):
    """(At the parent of this change the counts are (0, 0, 0): every mid-size region ran alone.)"""
    ctx = pool.context(fma)
    names = [QUALIFYING[k % len(QUALIFYING)] for k in range(K)]
    got, counts = pool.run(ctx, names)
    stats = ctx.stats()
    print("K", K, "fma", fma, "counts", counts, "n_fallback", stats["n_fallback"])
    assert counts == ((65, 65, 2) if K == 65 else (K, K, 1))
    assert stats["n_fallback"] == pool.n_fallback(fma, names)
    assert stats["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_maxr_variants(pool, fma):
    """pair_recompute_multi_kernel<fma, 2> for a set of short reads, <fma, 4> with `m_r4` in it, <fma, kRplF64> with
    `m_r6`: the regions common to all give the same bytes in every composition."""
    ctx = pool.context(fma)
    first = None
    for names in (ROWS2, ROWS2 + ["m_r4"], ["m_r6"] + ROWS2, ROWS2 + ["m_r6"]):
        got, counts = pool.run(ctx, names)
        assert counts == (len(names), len(names), 1), names
        pool.check(ctx, fma, names, got)
        common = {n: got[names.index(n)].tobytes() for n in ROWS2}
        first = first or common
        assert common == first, names


@pytest.mark.parametrize("fma", [1, 0])
def test_mixed_call(pool, fma):
    ctx = pool.context(fma)
    for names in (["s_r2", "m2049", "s_nofb", "m2304", "s_odd"], ["m2049", "s_r2", "m2304", "s_nofb", "m_odd"]):
        got, counts = pool.run(ctx, names)
        assert counts == (5, 5, 2), names     # one set of small regions, one of mid-size ones
        assert ctx.stats()["n_fallback"] == pool.n_fallback(fma, names)
        pool.check(ctx, fma, names, got)
    names = ["m2049", "s_r2", "s_nofb"]
    got, counts = pool.run(ctx, names)
    assert counts == (2, 2, 1)                # the lone mid-size region runs alone
    pool.check(ctx, fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_limits(pool, fma):
    ctx = pool.context(fma)
    for names, want in ((["m_top", "m2049"], (2, 2, 1)), (["m_over", "m2049"], (0, 0, 0)), (["m_big_in", "m2049"], (0, 0, 0)),
                        (["m2049"], (0, 0, 0))):
        got, counts = pool.run(ctx, names)
        assert counts == want, names
        assert ctx.stats()["n_fallback"] == pool.n_fallback(fma, names)
        pool.check(ctx, fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_a_region_does_not_depend_on_its_company(pool, fma):
    ctx = pool.context(fma)
    rng = np.random.RandomState(5)
    seen = {}
    for names in [list(rng.permutation(QUALIFYING)) for _ in range(3)]:
        got, counts = pool.run(ctx, names)
        assert counts == (7, 7, 1)
        pool.check(ctx, fma, names, got)
        for n, out in zip(names, got):
            assert seen.setdefault(n, out.tobytes()) == out.tobytes(), (n, names)


@pytest.mark.parametrize("fma", [1, 0])
def test_raw_sums_per_region(pool, fma):
    """used64, the kept fp32 sums and the recomputed fp64 sums of every member of a mid-size set, pair by pair: the order
    in which the flagged pairs entered the region's list shows nowhere."""
    ctx = pool.context(fma)
    names = ["m2049", "m_allfb", "m_nofb", "m_odd", "m_r4"]
    got, counts = pool.run(ctx, names)
    assert counts == (5, 5, 1)
    pool.check(ctx, fma, names, got)      # (its single calls were made before the multi call)
    for k, n in enumerate(names):
        _, e32, e64, eu = pool.want[fma][n]
        r32, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert np.array_equal(u, eu), n
        assert np.array_equal(r32[u == 0].view(np.uint32), e32[eu == 0].view(np.uint32)), n
        assert np.array_equal(bits(r64[u == 1]), bits(e64[eu == 1])), n


@pytest.mark.parametrize("fma", [1, 0])
def test_one_bad_region_of_three(pool, fma):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(fma)
    bad = dataclasses.replace(pool.batch["m2049"], read_off=pool.batch["m2049"].read_off.copy())
    bad.read_off[4] = bad.read_off[3]          # a read offset that does not increase
    singles = [pool.single(ctx, n) for n in ("m2304", "m_odd")]
    native.small_call_counts(0, reset=True)
    with pytest.raises(native.PairHmmMultiError) as e:
        ctx.compute_multi([pool.batch["m2304"], bad, pool.batch["m_odd"]])
    assert native.small_call_counts(0) == (2, 2, 1)    # the two good ones share a set
    assert e.value.statuses == [0, 1, 0] and e.value.status == 1
    assert isinstance(e.value.errors[1], IllegalArgumentException) and "read 3 is empty or offsets are not increasing" in str(e.value.errors[1])
    assert e.value.results[1] is None
    pool.check(ctx, fma, ["m2304", "m_odd"], [e.value.results[0], e.value.results[2]])   # the oracle and the single calls
    assert e.value.results[0].tobytes() == singles[0].tobytes() and e.value.results[2].tobytes() == singles[1].tobytes()
    # and the context goes on
    assert np.array_equal(bits(ctx.compute(pool.batch["m2304"])), bits(pool.want[fma]["m2304"][0]))
    names = ["m2049", "m_odd"]
    got, counts = pool.run(ctx, names)
    assert counts == (2, 2, 1)
    pool.check(ctx, fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_rows_per_lane_4_context(pool, fma):
    """`m_r6`: its reads of 256 bases and more are long reads at four rows per lane, so it runs alone."""
    ctx = pool.context(fma, rows_per_lane=4)
    names = ["m2049", "m2304", "m_r4"]
    got, counts = pool.run(ctx, names)
    assert counts == (3, 3, 1)
    pool.check(ctx, fma, names, got)
    names = ["m2049", "m_r6", "m2304", "m_r4"]
    got, counts = pool.run(ctx, names)
    assert counts == (3, 3, 1)
    assert ctx.stats()["n_fallback"] == pool.n_fallback(fma, names)
    pool.check(ctx, fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_all_cxx_build(pool, fma):
    """One set of three regions through libgklhip_pairhmm_cxxfast.so (the combiner's counters are that library's own)."""
    import ctypes as C
    from gkl_amd import native
    names = ["m2049", "m_allfb", "m_r4"]

    def counts(lib, reset=False):
        out = (C.c_int64 * 3)()
        assert lib.gklhip_small_call_counts(0, out, 1 if reset else 0) == native.OK
        return int(out[0]), int(out[1]), int(out[2])

    with native.PairHmmContext(lib_path=os.path.join(native.LIB_DIR, "libgklhip_pairhmm_cxxfast.so"), fma_mode=fma) as c:
        singles = [c.compute(pool.batch[n]) for n in names]
        counts(c.lib, reset=True)
        got = c.compute_multi([pool.batch[n] for n in names])
        assert counts(c.lib) == (3, 3, 1)
        for n, out, s in zip(names, got, singles):
            assert np.array_equal(bits(out), bits(pool.want[fma][n][0])), n
            assert out.tobytes() == s.tobytes(), n

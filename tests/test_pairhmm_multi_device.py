"""Several device-resident PairHMM regions in one call (gklhip_compute_multi_device, PairHmmContext.compute_multi_device):
the regions' six byte arrays and their outputs lie in HBM, the regions that qualify share the set launches of
gklhip_compute_multi, and finalize_words_multi_kernel turns each region's packed words into doubles in place.  Region k's
output is, byte for byte, what gklhip_compute_device writes for it alone on the same context -- whichever regions ride
along, in whatever order, in both fma modes, in both device finalisation modes and on use_double contexts; the combiner's
counters say which sets formed, and the raw sums are the oracle's bits.

The shapes are the pools of tests/test_pairhmm_multi.py, test_pairhmm_multi_mid.py, test_pairhmm_double_small.py and
test_pairhmm_double_mid.py: the smallest at which each set variant can go wrong.  Per context every region is computed
once with compute_device alone and its bytes kept.  (At the parent of this change the library has no such symbol: every
test here fails.)"""
import dataclasses

import numpy as np
import pytest

from tests.test_gpu_parity import REL_TOL
from tests.test_pairhmm_double_mid import build_pool as build_double_mid_pool
from tests.test_pairhmm_double_small import QUALIFYING as DOUBLE_QUALIFYING
from tests.test_pairhmm_double_small import build_pool as build_double_pool
from tests.test_pairhmm_multi import QUALIFYING, bits, build_pool, mixed_list_of_70
from tests.test_pairhmm_multi_mid import QUALIFYING as MID_QUALIFYING
from tests.test_pairhmm_multi_mid import build_pool as build_mid_pool

pytestmark = pytest.mark.gpu


class DevPool:
    """Named regions, uploaded once; per context the single device call's bytes, computed once; the oracle's results,
    computed once per (region, fma, precision) and only for the regions a test asks about."""

    def __init__(self, oracle):
        from gkl_amd import native
        self.oracle = oracle
        self.batch = {}
        self.batch.update(build_pool())
        self.batch.update(build_mid_pool())
        self.batch.update({"d_" + n: b for n, b in build_double_pool().items()})
        self.batch.update({"d_" + n: b for n, b in build_double_mid_pool().items() if n in ("m2049", "m2304")})
        self.dev = {n: native.DeviceBatch.upload(b) for n, b in self.batch.items()}
        self.ctx, self.singles, self.wants = {}, {}, {}

    def context(self, **kw):
        from gkl_amd import native
        key = tuple(sorted(kw.items()))
        if key not in self.ctx:
            if "devices" in kw:
                kw = dict(kw, devices=list(kw["devices"]))
            self.ctx[key] = native.PairHmmContext(**kw)
        return self.ctx[key]

    def single(self, ctx, name):
        import torch
        cache = self.singles.setdefault(id(ctx), {})
        if name not in cache:
            out = ctx.compute_device(self.dev[name])
            torch.cuda.synchronize()
            cache[name] = out.cpu().numpy().tobytes()
        return cache[name]

    def want(self, name, fma, use_double=False):
        """(out, raw32, raw64, used64) of the oracle."""
        key = (name, fma, use_double)
        if key not in self.wants:
            self.wants[key] = self.oracle.batch(self.batch[name], use_double=use_double, fma_mode=fma, want_raw=True, n_threads=4)
        return self.wants[key]

    def run(self, ctx, names, **kw):
        """One multi call and the combiner's counts for it (the single calls it is compared with are made before)."""
        from gkl_amd import native
        for n in set(names):
            self.single(ctx, n)
        native.small_call_counts(0, reset=True)
        outs = ctx.compute_multi_device([self.dev[n] for n in names], **kw)
        return outs, native.small_call_counts(0)

    def check(self, ctx, names, outs):
        assert len(outs) == len(names)
        for k, (n, out) in enumerate(zip(names, outs)):
            assert out.numel() == self.batch[n].n_pairs
            assert out.cpu().numpy().tobytes() == self.single(ctx, n), (k, n, "single device call")

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def pool(oracle):
    p = DevPool(oracle)
    yield p
    p.close()


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [1, 2, 3, 17, 64, 65])
def test_set_sizes_and_counters(pool, K, fma):
    ctx = pool.context(fma_mode=fma)
    names = [QUALIFYING[k % len(QUALIFYING)] for k in range(K)]
    outs, counts = pool.run(ctx, names)
    stats = ctx.stats()
    print("K", K, "fma", fma, "counts", counts, "n_fallback", stats["n_fallback"])
    assert counts == ((65, 65, 2) if K == 65 else (K, K if K > 1 else 0, 1))
    assert stats["n_fallback"] == sum(int(pool.want(n, fma)[3].sum()) for n in names)
    assert stats["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, names, outs)


@pytest.mark.parametrize("finalize", [1, 2])
def test_finalisation_modes(pool, finalize):
    """cfg.finalize 1 (log10 in double) and 2 (the reference's float formula): the bytes of the single device call in that
    mode, for small sets and a mid-size one.  Mode 1 is the double formula: within REL_TOL of the host call wherever the
    outputs are finite."""
    from gkl_amd import native
    assert (native.FINALIZE_DEVICE_F64, native.FINALIZE_DEVICE_REF32) == (1, 2)
    ctx = pool.context(finalize=finalize)
    for names, want in ((QUALIFYING + ["edge", "r6"], (10, 10, 1)), (["m2049", "m_allfb", "m_r4"], (3, 3, 1))):
        outs, counts = pool.run(ctx, names)
        assert counts == want
        pool.check(ctx, names, outs)
        if finalize == 1:
            host = pool.context(fma_mode=1)
            for n, out in zip(names, outs):
                ref = host.compute(pool.batch[n])
                if np.isfinite(ref).all():
                    got = out.cpu().numpy()
                    assert np.max(np.abs(got - ref) / np.abs(ref)) < REL_TOL, n
    other = pool.context(finalize=3 - finalize)
    assert pool.single(ctx, "nofb") != pool.single(other, "nofb"), "the two modes must differ somewhere, or this test checks one"


def test_raw_sums_per_region(pool):
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(fma_mode=1)
    names = ["r2", "allfb", "nofb", "odd", "r4"]
    outs, _ = pool.run(ctx, names)
    pool.check(ctx, names, outs)          # (its single calls were made before the multi call)
    outs, _ = pool.run(ctx, names)
    for k, n in enumerate(names):
        _, e32, e64, eu = pool.want(n, 1)
        r32, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert np.array_equal(u, eu), n
        assert np.array_equal(r32[u == 0].view(np.uint32), e32[eu == 0].view(np.uint32)), n
        assert np.array_equal(bits(r64[u == 1]), bits(e64[eu == 1])), n
    with pytest.raises(IllegalArgumentException, match="no completed call to read back"):
        ctx.raw(pool.batch[names[-1]].n_pairs)
    with pytest.raises(IllegalArgumentException, match="region 5 of 5"):
        ctx.raw_region(5, 1)
    # the lanes go back with gklhip_release_idle, and the next call makes them again
    ctx.release_idle()
    outs, counts = pool.run(ctx, names)
    assert counts == (5, 5, 1)
    pool.check(ctx, names, outs)


@pytest.mark.parametrize("fma", [1, 0])
def test_narrow_and_wide_variants(pool, fma):
    ctx = pool.context(fma_mode=fma)
    narrow = ["r4", "one", "r2", "nofb", "odd", "allfb"]
    got_n, counts = pool.run(ctx, narrow)
    assert counts == (6, 6, 1)
    pool.check(ctx, narrow, got_n)
    for wide in (narrow + ["r6"], ["r6"] + narrow):
        got_w, counts = pool.run(ctx, wide)
        assert counts == (7, 7, 1)
        pool.check(ctx, wide, got_w)
    for names in (["r4", "r2", "r4", "r2"], ["edge", "r2", "one"], ["one", "edge"]):
        outs, _ = pool.run(ctx, names)
        pool.check(ctx, names, outs)


@pytest.mark.parametrize("fma", [1, 0])
def test_unfused_kernels(pool, fma):
    """A rows_per_lane=4 context: deferred but not fused, so the set leaves through fwd_stream_multi_kernel +
    pair_policy_multi_kernel (`r6`: long reads at four rows per lane, it runs alone)."""
    ctx = pool.context(fma_mode=fma, rows_per_lane=4)
    names = QUALIFYING + ["edge", "r6"]
    outs, counts = pool.run(ctx, names)
    assert counts == (9, 9, 1)
    pool.check(ctx, names, outs)


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [2, 3, 7])
def test_mid_size_sets(pool, K, fma):
    ctx = pool.context(fma_mode=fma)
    names = MID_QUALIFYING[:K]
    outs, counts = pool.run(ctx, names)
    assert counts == (K, K, 1)
    assert ctx.stats()["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, names, outs)


def test_mid_size_limits_and_mixed_calls(pool):
    ctx = pool.context(fma_mode=1)
    for names, want in ((["m_top", "m2049"], (2, 2, 1)), (["m_over", "m2049"], (0, 0, 0)), (["m_big_in", "m2049"], (0, 0, 0)),
                        (["m2049", "s_r2", "s_nofb"], (2, 2, 1)),                   # the lone mid-size region runs alone
                        (["s_r2", "m2049", "s_nofb", "m2304", "s_odd"], (5, 5, 2))):   # one set of small regions, one of mid-size ones
        outs, counts = pool.run(ctx, names)
        assert counts == want, names
        pool.check(ctx, names, outs)
    # ... as the host multi call counts the same list
    from gkl_amd import native
    names = ["m2049", "s_r2", "s_nofb"]
    native.small_call_counts(0, reset=True)
    ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (2, 2, 1)


@pytest.mark.parametrize("fma", [1, 0])
def test_double_precision_contexts(pool, fma):
    ctx = pool.context(use_double=True, fma_mode=fma)
    small = ["d_" + n for n in DOUBLE_QUALIFYING]
    mid = ["d_m2049", "d_m2304"]
    for names, want in ((small, (8, 8, 1)), (small[:1], (1, 0, 1)), (mid, (2, 2, 1)), (small[:3] + mid[:1], (3, 3, 1)), (mid[:1] + small + mid[1:], (10, 10, 2))):
        outs, counts = pool.run(ctx, names)
        assert counts == want, names
        stats = ctx.stats()
        assert stats["n_pairs"] == sum(pool.batch[n].n_pairs for n in names) == stats["n_fallback"]
        pool.check(ctx, names, outs)
    names = mid[:1] + small + mid[1:]
    for k, n in enumerate(names):
        want = pool.want(n, fma, use_double=True)
        _, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert u.all(), n
        assert np.array_equal(bits(r64), bits(want[2])), n
        assert np.array_equal(bits(outs[k].cpu().numpy()), bits(np.frombuffer(pool.single(ctx, n), np.float64)))


@pytest.mark.parametrize("rows_per_lane", [0, 4])
def test_a_mixed_list_longer_than_a_set(pool, rows_per_lane):
    """tests/test_pairhmm_multi.py's list of 70 regions -- planned twice, 66 small regions in two sets of 33, three mid-size
    ones in a set of their own, `long` alone: (69, 69, 3) as derived there -- with the regions in HBM."""
    ctx = pool.context(fma_mode=1, rows_per_lane=rows_per_lane)
    names = mixed_list_of_70()
    outs, counts = pool.run(ctx, names)
    print("rows_per_lane", rows_per_lane, "counts", counts)
    assert counts == (69, 69, 3)
    assert ctx.stats()["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, names, outs)


def test_regions_that_do_not_qualify_run_alone_inside_the_call(pool):
    ctx = pool.context(fma_mode=1)
    names = ["r2", "over", "one", "long", "r4"]
    outs, counts = pool.run(ctx, names)
    assert counts == (3, 3, 1)
    assert ctx.stats()["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, names, outs)


def test_a_region_does_not_depend_on_its_company(pool):
    ctx = pool.context(fma_mode=1)
    rng = np.random.RandomState(3)
    orders = [list(rng.permutation(QUALIFYING)) for _ in range(3)] + [QUALIFYING[1:6], QUALIFYING[::3]]
    for names in orders:
        outs, _ = pool.run(ctx, names)
        pool.check(ctx, names, outs)


def test_one_bad_region_of_three(pool):
    import torch
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(fma_mode=1)
    good = pool.dev["r2"]
    off = good.read_off.copy()
    off[4] = off[3]                       # an empty read
    bad = dataclasses.replace(good, read_off=off)
    sentinel = torch.full((pool.batch["r2"].n_pairs,), 7.0, dtype=torch.float64, device="cuda:0")
    for n in ("r4", "odd"):
        pool.single(ctx, n)

    def fresh(name):
        return torch.empty(pool.batch[name].n_pairs, dtype=torch.float64, device="cuda:0")

    # an empty read (its output tensor holds a sentinel), then a region without an output array
    for regions, outs, message in (([pool.dev["r4"], bad, pool.dev["odd"]], [fresh("r4"), sentinel, fresh("odd")], "read 3 is empty or offsets are not increasing"),
                                   ([pool.dev["r4"], good, pool.dev["odd"]], [fresh("r4"), None, fresh("odd")], "output array is NULL")):
        native.small_call_counts(0, reset=True)
        with pytest.raises(native.PairHmmMultiError) as e:
            ctx.compute_multi_device(regions, outs=outs)
        assert native.small_call_counts(0) == (2, 2, 1)       # the two good ones share a set
        assert e.value.statuses == [0, native.ERR_INVALID_ARG, 0] and e.value.status == native.ERR_INVALID_ARG
        assert isinstance(e.value.errors[1], IllegalArgumentException) and message in str(e.value.errors[1])
        assert e.value.results[1] is None
        pool.check(ctx, ["r4", "odd"], [e.value.results[0], e.value.results[2]])
        assert bool((sentinel == 7.0).all())
    # and the context goes on
    outs, counts = pool.run(ctx, ["one"])
    pool.check(ctx, ["one"], outs)


def test_unaligned_arrays(pool):
    """Every region's six arrays are views at odd byte offsets into one uint8 tensor, every output a view at an offset of
    8 bytes (and no more) from the alignment of a double's neighbours."""
    import torch
    from gkl_amd import native
    ctx = pool.context(fma_mode=1)
    names = QUALIFYING + ["m2049", "m2304"]
    total = sum(t.numel() + 2 for n in names for t in pool.dev[n].tensors) + 1
    arena = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    out_arena = torch.empty(sum(pool.batch[n].n_pairs + 2 for n in names) + 2, dtype=torch.float64, device="cuda:0")
    regions, outs, at, oat = [], [], 1, 1
    for n in names:
        views = []
        for t in pool.dev[n].tensors:
            v = arena[at:at + t.numel()]
            v.copy_(t)
            assert t.numel() == 0 or v.data_ptr() % 2 == 1
            views.append(v)
            at += t.numel() + (2 if t.numel() % 2 == 0 else 1)      # the next one starts at an odd offset again
        regions.append(native.DeviceBatch(pool.batch[n], tuple(views), pool.dev[n].read_off, pool.dev[n].hap_off))
        outs.append(out_arena[oat:oat + pool.batch[n].n_pairs])
        oat += pool.batch[n].n_pairs + (2 if pool.batch[n].n_pairs % 2 == 0 else 1)   # 8 mod 16 every time
        assert outs[-1].data_ptr() % 16 == 8
    for n in set(names):
        pool.single(ctx, n)
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi_device(regions, outs=outs)
    assert native.small_call_counts(0) == (10, 10, 2)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    pool.check(ctx, names, got)


def test_stream_ordering(pool):
    """The regions' arrays are overwritten with zeros on a side stream, and the copies of the real bytes from pinned
    memory are enqueued behind them on the same stream; the call gets that stream.  Its sets run on streams of their
    own, behind an event recorded on the caller's stream.  This does not prove the wait: it fails if the wait is missing
    AND the race is lost."""
    import torch
    from gkl_amd import native
    ctx = pool.context(fma_mode=1)
    names = QUALIFYING + ["m2049", "m2304"]
    for n in set(names):
        pool.single(ctx, n)
    pinned = {n: [t.cpu().pin_memory() for t in pool.dev[n].tensors] for n in names}
    fresh = {n: native.DeviceBatch(pool.batch[n], tuple(torch.empty_like(t) for t in pool.dev[n].tensors), pool.dev[n].read_off, pool.dev[n].hap_off)
             for n in names}
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for n in names:
            for t, src in zip(fresh[n].tensors, pinned[n]):
                t.zero_()
                t.copy_(src, non_blocking=True)
    outs = ctx.compute_multi_device([fresh[n] for n in names], stream=side)
    pool.check(ctx, names, outs)


def test_multi_device_context_runs_region_by_region(pool):
    from gkl_amd import native
    ctx = pool.context(fma_mode=1, devices=(0, 0))
    assert ctx.n_devices == 2
    names = ["r2", "nofb", "allfb", "m2049", "m2304"]
    outs, counts = pool.run(ctx, names)
    assert counts == (0, 0, 0)
    pool.check(ctx, names, outs)
    assert isinstance(outs, list) and native.small_call_counts(0) == (0, 0, 0)

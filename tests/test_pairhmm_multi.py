"""Several PairHMM region calls in one set of launches (gklhip_compute_multi, PairHmmContext.compute_multi): region k's
output is, byte for byte, what the single call writes for it on the same context -- and what the oracle computes --
whichever other regions ride along, in whatever order, in both fma modes.  With the explicit entry point the composition
of a set is an input, so every variant of the combined-launch kernels (prep_multi_kernel, pair_fused_multi_kernel narrow
and wide, fwd_stream_multi_kernel + pair_policy_multi_kernel) is reached deterministically, and the combiner's counters
can be asserted exactly."""
import dataclasses
import os
import threading

import numpy as np
import pytest

from gkl_amd.synth import make_batch, random_batch

pytestmark = pytest.mark.gpu

QUALIFYING = ["one", "row", "col", "r2", "r4", "allfb", "nofb", "odd"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def build_pool():
    """The smallest shapes at which a variant of the combined launches can go wrong (reads x haplotypes)."""
    rng = np.random.RandomState(67)
    pool = {
        "one": random_batch(rng, 1, 1, read_len=(1, 1), hap_len=(1, 1)),                        # begin[] steps of 1
        "row": make_batch("hc", 1, 9, seed=9),                                                    # one read
        "col": make_batch("hc", 33, 1, seed=10),                                                  # one haplotype
        "r2": make_batch("hc", 12, 3, seed=4, read_len=(20, 90), hap_len=(60, 120)),              # rows == 2
        "r4": make_batch("hc", 6, 2, seed=5, read_len=(130, 250), hap_len=(200, 300)),            # rows == 4: the narrow variant's limit
        "r6": make_batch("hc", 4, 2, seed=6, read_len=(260, 383), hap_len=(300, 400)),            # rows == kRplF64: the wide variant for the whole set
        "allfb": random_batch(rng, 5, 4, read_len=(100, 120), hap_len=(120, 160), qual_range=(20, 40), related=False),
        "nofb": make_batch("region", 10, 4, seed=4),
        "odd": random_batch(rng, 8, 3, alphabet=b"ACGTNacgtRY", qual_range=(0, 255)),             # N, odd bytes, every quality byte
        "edge": random_batch(rng, 64, 32, read_len=(10, 20), hap_len=(20, 30)),                   # 2048 pairs: the last size that qualifies
        "over": random_batch(rng, 683, 3, read_len=(10, 20), hap_len=(20, 30)),                   # 2049 pairs: runs alone inside the multi call
    }
    b = random_batch(rng, 2, 2, read_len=(400, 400), hap_len=(420, 450), qual_range=(10, 45))     # one read of 400 bases: runs alone
    keep = 400 + 25
    pool["long"] = dataclasses.replace(b, read_off=np.array([0, 400, keep], np.int64),
                                       **{f: getattr(b, f)[:keep] for f in ("read_bases", "read_quals", "ins_gop", "del_gop", "gcp")})
    return pool


class Pool:
    def __init__(self, oracle):
        self.batch = build_pool()
        # (out, raw32, raw64, used64) per fma mode, computed once
        self.want = {fma: {name: oracle.batch(b, fma_mode=fma, want_raw=True, n_threads=4) for name, b in self.batch.items()}
                     for fma in (0, 1)}
        self.ctx = {}

    def context(self, fma, rows_per_lane=0):
        from gkl_amd import native
        key = (fma, rows_per_lane)
        if key not in self.ctx:
            self.ctx[key] = native.PairHmmContext(fma_mode=fma, rows_per_lane=rows_per_lane)
        return self.ctx[key]

    def check(self, ctx, fma, names, got, singles=None):
        """Every region: the oracle's bytes and the bytes of the single call on the same context."""
        assert len(got) == len(names)
        singles = {} if singles is None else singles
        for k, (name, out) in enumerate(zip(names, got)):
            assert np.array_equal(bits(out), bits(self.want[fma][name][0])), (k, name, "oracle")
            if name not in singles:
                singles[name] = ctx.compute(self.batch[name])
            assert out.tobytes() == singles[name].tobytes(), (k, name, "single call")
        return singles

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
    for fma in (0, 1):
        w = pool.want[fma]
        assert w["allfb"][3].all(), "every pair of `allfb` must fall back to fp64: change the seed"
        assert not w["nofb"][3].any(), "no pair of `nofb` may fall back: change the seed"
    b = pool.batch
    assert (b["one"].n_pairs, b["row"].n_pairs, b["col"].n_pairs, b["edge"].n_pairs, b["over"].n_pairs) == (1, 9, 33, 2048, 2049)
    assert int(b["r2"].read_lens.max()) <= 127 and 128 <= int(b["r4"].read_lens.max()) <= 255 and 256 <= int(b["r6"].read_lens.max()) <= 383
    assert sorted(b["long"].read_lens.tolist()) == [25, 400]


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 64, 65])
def test_set_sizes_and_counters(pool, K, fma):
    from gkl_amd import native
    ctx = pool.context(fma)
    names = [QUALIFYING[k % len(QUALIFYING)] for k in range(K)]
    singles = {n: ctx.compute(pool.batch[n]) for n in set(names)}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    counts = native.small_call_counts(0)
    stats = ctx.stats()
    print("K", K, "fma", fma, "counts", counts, "n_fallback", stats["n_fallback"])
    assert counts == ((65, 65, 2) if K == 65 else (K, K if K > 1 else 0, 1))
    assert stats["n_fallback"] == pool.n_fallback(fma, names)
    assert stats["n_pairs"] == sum(pool.batch[n].n_pairs for n in names)
    pool.check(ctx, fma, names, got, singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_narrow_and_wide_variants(pool, fma):
    """A set whose reads all have at most 255 bases takes pair_fused_multi_kernel<., 4>; one region with longer reads
    (`r6`) moves the whole set to <., kRplF64>: the same regions give the same bytes in both."""
    from gkl_amd import native
    ctx = pool.context(fma)
    narrow = ["r4", "one", "r2", "nofb", "odd", "allfb"]
    got_n = ctx.compute_multi([pool.batch[n] for n in narrow])
    singles = pool.check(ctx, fma, narrow, got_n)
    for wide in (narrow + ["r6"], ["r6"] + narrow):
        native.small_call_counts(0, reset=True)
        got_w = ctx.compute_multi([pool.batch[n] for n in wide])
        assert native.small_call_counts(0) == (7, 7, 1)
        pool.check(ctx, fma, wide, got_w, singles)
        for n in narrow:
            assert got_w[wide.index(n)].tobytes() == got_n[narrow.index(n)].tobytes(), n
    for names in (["r4", "r2", "r4", "r2"], ["edge", "r2", "one"], ["one", "edge"]):
        pool.check(ctx, fma, names, ctx.compute_multi([pool.batch[n] for n in names]), singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_unfused_kernels(pool, fma):
    """A context created with rows_per_lane=4: run_device fuses a small call only when cfg.rows_per_lane == 0 (fused_call),
    while whether the call is deferred (small_call_defers) does not look at rows_per_lane -- so these calls are deferred
    but not fused, and a set of them leaves through fwd_stream_multi_kernel + pair_policy_multi_kernel.  (`r6`: its reads
    of 256 bases and more are long reads at four rows per lane, so it runs alone.)"""
    from gkl_amd import native
    ctx = pool.context(fma, rows_per_lane=4)
    names = QUALIFYING + ["edge", "r6"]
    singles = {n: ctx.compute(pool.batch[n]) for n in names}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (9, 9, 1)
    assert ctx.stats()["n_fallback"] == pool.n_fallback(fma, names)
    pool.check(ctx, fma, names, got, singles)


# A list longer than one set's lanes, so it is planned twice (once to classify, once when a region's set is staged), with every
# class in it: 66 small regions (QUALIFYING in turn), three mid-size ones from tests/test_pairhmm_multi_mid.py's pool at 5, 30
# and 60, and `long`, which does not qualify, at 17.  The counters, from the cutting rule (pairhmm_multi_sets.h):
#   * a context has ONE kind of small fp32 region (fused with rows_per_lane 0, unfused with 4), so the 66 small ones are one
#     run -- the mid-size regions and `long` do not interrupt it -- that multi_cut_sets cuts into ceil(66 / 64) = 2 sets of
#     33 + 33: 66 calls, 66 combined, 2 sets of launches;
#   * multi_cut_mid_sets puts the three mid-size regions into one set: 3 calls, 3 combined, 1 set;
#   * `long` takes the single call's general pass, which counts nothing;
# (calls, combined, sets) = (69, 69, 3), in both kinds of context.
MIXED_MID = {5: "m2049", 30: "m2304", 60: "m_nofb"}


def mixed_list_of_70():
    names, k = [], 0
    for at in range(70):
        if at in MIXED_MID or at == 17:
            names.append(MIXED_MID.get(at, "long"))
        else:
            names.append(QUALIFYING[k % len(QUALIFYING)])
            k += 1
    assert len(names) == 70 and k == 66
    return names


@pytest.mark.parametrize("rows_per_lane", [0, 4])
def test_a_mixed_list_longer_than_a_set(pool, rows_per_lane):
    from gkl_amd import native
    from tests.test_pairhmm_multi_mid import build_pool as build_mid_pool
    mid = build_mid_pool()
    ctx = pool.context(1, rows_per_lane=rows_per_lane)
    names = mixed_list_of_70()
    batch = {n: mid[n] if n in mid else pool.batch[n] for n in set(names)}
    singles = {n: ctx.compute(b) for n, b in batch.items()}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([batch[n] for n in names])
    counts = native.small_call_counts(0)
    print("rows_per_lane", rows_per_lane, "counts", counts)
    assert counts == (69, 69, 3)
    assert ctx.stats()["n_pairs"] == sum(batch[n].n_pairs for n in names)
    for k, (n, out) in enumerate(zip(names, got)):
        assert out.tobytes() == singles[n].tobytes(), (k, n, "single call")
        if n not in mid:
            assert np.array_equal(bits(out), bits(pool.want[1][n][0])), (k, n, "oracle")


def test_regions_that_do_not_qualify_run_alone_inside_the_call(pool):
    from gkl_amd import native
    ctx = pool.context(1)
    names = ["r2", "over", "one", "long", "r4"]
    singles = {n: ctx.compute(pool.batch[n]) for n in names}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    # three regions in one set; the other two take the single call's path for their size, which counts nothing here
    assert native.small_call_counts(0) == (3, 3, 1)
    assert ctx.stats()["n_fallback"] == pool.n_fallback(1, names)
    pool.check(ctx, 1, names, got, singles)


def test_a_region_does_not_depend_on_its_company(pool):
    ctx = pool.context(1)
    rng = np.random.RandomState(3)
    seen = {}
    orders = [list(rng.permutation(QUALIFYING)) for _ in range(3)] + [QUALIFYING[1:6], QUALIFYING[::3]]
    for names in orders:
        got = ctx.compute_multi([pool.batch[n] for n in names])
        pool.check(ctx, 1, names, got, {})
        for n, out in zip(names, got):
            assert seen.setdefault(n, out.tobytes()) == out.tobytes(), (n, names)


def test_raw_sums_per_region(pool):
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(1)
    names = ["r2", "allfb", "nofb", "odd", "r4"]
    pool.check(ctx, 1, names, ctx.compute_multi([pool.batch[n] for n in names]))   # (its single calls come before the multi call below)
    ctx.compute_multi([pool.batch[n] for n in names])
    for k, n in enumerate(names):
        _, e32, e64, eu = pool.want[1][n]
        r32, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert np.array_equal(u, eu), n
        assert np.array_equal(r32[u == 0].view(np.uint32), e32[eu == 0].view(np.uint32)), n
        assert np.array_equal(bits(r64[u == 1]), bits(e64[eu == 1])), n
    with pytest.raises(IllegalArgumentException, match="no completed call to read back"):
        ctx.raw(pool.batch[names[-1]].n_pairs)
    with pytest.raises(IllegalArgumentException, match="region 5 of 5"):
        ctx.raw_region(5, 1)
    # a single call makes gklhip_get_raw readable again, and the regions of the multi call unreadable
    ctx.compute(pool.batch["r2"])
    assert np.array_equal(ctx.raw(pool.batch["r2"].n_pairs)[2], pool.want[1]["r2"][3])
    with pytest.raises(IllegalArgumentException, match="no completed multi call"):
        ctx.raw_region(0, pool.batch["r2"].n_pairs)


def test_one_bad_region_of_three(pool):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(1)
    bad = dataclasses.replace(pool.batch["r2"], read_off=pool.batch["r2"].read_off.copy())
    bad.read_off[4] = bad.read_off[3]          # a read offset that does not increase
    with pytest.raises(native.PairHmmMultiError) as e:
        ctx.compute_multi([pool.batch["r4"], bad, pool.batch["odd"]])
    assert e.value.statuses == [0, 1, 0] and e.value.status == 1
    assert isinstance(e.value.errors[1], IllegalArgumentException) and "read 3 is empty or offsets are not increasing" in str(e.value.errors[1])
    assert e.value.results[1] is None
    assert np.array_equal(bits(e.value.results[0]), bits(pool.want[1]["r4"][0]))
    assert np.array_equal(bits(e.value.results[2]), bits(pool.want[1]["odd"][0]))
    # and the context goes on
    assert np.array_equal(bits(ctx.compute(pool.batch["r4"])), bits(pool.want[1]["r4"][0]))
    assert np.array_equal(bits(ctx.compute_multi([pool.batch["one"]])[0]), bits(pool.want[1]["one"][0]))


def test_a_multi_call_beside_other_callers(pool, oracle):
    """One multi call of 8 regions, 20 times, while four threads make single 100 x 10 calls on contexts of their own: the
    set waits for a flight slot like their sets do, and every answer is exact."""
    from gkl_amd import native
    hc = make_batch("hc", 100, 10, seed=3)
    want_hc = oracle.batch(hc, n_threads=4)
    ctx = pool.context(1)
    regions = [pool.batch[n] for n in QUALIFYING]
    errors, done = [], threading.Event()
    start = threading.Barrier(5)

    def caller(i):
        try:
            with native.PairHmmContext() as c:
                c.compute(hc)
                start.wait()
                calls = 0
                while not done.is_set() or calls < 5:
                    if not np.array_equal(bits(c.compute(hc)), bits(want_hc)):
                        errors.append((i, calls))
                        return
                    calls += 1
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))
            start.abort()

    th = [threading.Thread(target=caller, args=(i,)) for i in range(4)]
    [t.start() for t in th]
    try:
        start.wait()
        for _ in range(20):
            got = ctx.compute_multi(regions)
            for n, out in zip(QUALIFYING, got):
                assert np.array_equal(bits(out), bits(pool.want[1][n][0])), n
    finally:
        done.set()
        [t.join() for t in th]
    assert not errors, errors[:4]


def test_all_cxx_build(pool):
    from gkl_amd import native
    names = ["r2", "allfb", "nofb", "odd", "r4"]
    with native.PairHmmContext(lib_path=os.path.join(native.LIB_DIR, "libgklhip_pairhmm_cxxfast.so")) as c:
        got = c.compute_multi([pool.batch[n] for n in names])
        for n, out in zip(names, got):
            assert np.array_equal(bits(out), bits(pool.want[1][n][0])), n
        assert got[0].tobytes() == c.compute(pool.batch["r2"]).tobytes()

"""Small calls of a double-precision context (gklhip_config.use_double, GATK's --native-pair-hmm-use-double-precision): a
region of up to 2048 pairs with no read of 384 bases or more is a small call of its own kind (kSmallDouble) -- one pair per
wavefront in pairhmm_pair_f64_kernel, deferred to the combiner like the fp32 small calls, and the regions of one
gklhip_compute_multi call share sets of up to 64 (prep_multi_kernel + pair_f64_multi_kernel, narrow and wide).  Every
output is compared bit for bit with the oracle's `use_double` result, computed live; the combiner's counters are asserted
exactly."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd.synth import make_batch, random_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALIFYING = ["one", "row", "col", "bounds", "r2", "r4", "r6", "odd"]
BOUNDS = [1, 127, 128, 255, 256, 383]   # the three rows-per-lane variants at both ends


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def exact_reads(b, lens):
    """`b` (whose reads are at least as long) with its reads cut to exactly `lens` bases."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cut = {f: np.concatenate([getattr(b, f)[int(b.read_off[r]):int(b.read_off[r]) + n] for r, n in enumerate(lens)])
           for f in ("read_bases", "read_quals", "ins_gop", "del_gop", "gcp")}
    return dataclasses.replace(b, read_off=off, **cut)


def build_pool():
    """The smallest shapes at which a variant of the fp64 per-pair launches can go wrong (reads x haplotypes)."""
    rng = np.random.RandomState(70)
    pool = {
        "one": random_batch(rng, 1, 1, read_len=(1, 1), hap_len=(1, 1)),                        # begin[] steps of 1
        "row": make_batch("hc", 1, 9, seed=9),                                                    # one read
        "col": make_batch("hc", 33, 1, seed=10),                                                  # one haplotype
        "bounds": exact_reads(random_batch(rng, 6, 2, read_len=(383, 383), hap_len=(290, 310), qual_range=(6, 14)), BOUNDS),   # (low qualities: unrelated reads of 383 bases stay inside fp64's range)
        "r2": make_batch("hc", 12, 3, seed=4, read_len=(20, 90), hap_len=(60, 120)),              # rows == 2
        "r4": make_batch("hc", 6, 2, seed=5, read_len=(130, 250), hap_len=(200, 300)),            # rows == 4: the narrow form's limit
        "r6": make_batch("hc", 4, 2, seed=6, read_len=(260, 383), hap_len=(300, 400)),            # rows == kRplF64: the wide form for the whole set
        "odd": random_batch(rng, 8, 3, alphabet=b"ACGTNacgtRY", qual_range=(0, 255)),             # N, odd bytes, every quality byte
        "edge": random_batch(rng, 64, 32, read_len=(10, 20), hap_len=(20, 30), qual_range=(5, 50)),                   # 2048 pairs: the last size that qualifies
        "over": random_batch(rng, 683, 3, read_len=(10, 20), hap_len=(20, 30), qual_range=(5, 50)),                   # 2049 pairs: runs alone inside the multi call
        "small": make_batch("region", 10, 4, seed=4),                                             # a plain 10 x 4 region
    }
    b = random_batch(rng, 2, 2, read_len=(400, 400), hap_len=(420, 450), qual_range=(10, 45))     # one read of 400 bases: runs alone
    pool["long"] = exact_reads(b, [400, 25])
    return pool


class Pool:
    def __init__(self, oracle):
        self.batch = build_pool()
        # (out, raw32, raw64, used64) of the use_double oracle per fma mode, computed once
        self.want = {fma: {name: oracle.batch(b, use_double=True, fma_mode=fma, want_raw=True, n_threads=4) for name, b in self.batch.items()}
                     for fma in (0, 1)}
        self.ctx = {}

    def context(self, fma):
        from gkl_amd import native
        if fma not in self.ctx:
            self.ctx[fma] = native.PairHmmContext(use_double=True, fma_mode=fma)
        return self.ctx[fma]

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

    def n_pairs(self, names):
        return int(sum(self.batch[n].n_pairs for n in names))

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
    assert (b["one"].n_pairs, b["row"].n_pairs, b["col"].n_pairs, b["edge"].n_pairs, b["over"].n_pairs) == (1, 9, 33, 2048, 2049)
    assert (b["one"].read_lens.tolist(), np.diff(b["one"].hap_off).tolist()) == ([1], [1])
    assert (b["row"].n_reads, b["row"].n_haps, b["col"].n_reads, b["col"].n_haps) == (1, 9, 33, 1)
    assert b["bounds"].read_lens.tolist() == BOUNDS and b["bounds"].n_haps == 2
    assert (b["r2"].n_pairs, b["r4"].n_pairs, b["r6"].n_pairs, b["odd"].n_pairs, b["small"].n_pairs) == (36, 12, 8, 24, 40)
    assert int(b["r2"].read_lens.max()) <= 90
    assert 130 <= int(b["r4"].read_lens.min()) and int(b["r4"].read_lens.max()) <= 250
    assert 260 <= int(b["r6"].read_lens.min()) and int(b["r6"].read_lens.max()) <= 383
    assert (b["edge"].n_reads, b["edge"].n_haps, b["over"].n_reads, b["over"].n_haps) == (64, 32, 683, 3)
    assert b["long"].read_lens.tolist() == [400, 25]
    for name in ("row", "col", "r2", "r4", "odd", "edge", "over", "small"):
        assert int(b[name].read_lens.max()) <= 383, name
    for fma in (0, 1):
        for name, w in pool.want[fma].items():
            assert w[3].all(), (name, "the use_double oracle takes every pair in fp64")
            assert np.isfinite(w[0]).all(), (name, "a likelihood that underflowed fp64 checks nothing: change the seed")


@pytest.mark.parametrize("fma", [1, 0])
def test_every_region_singly(pool, fma):
    ctx = pool.context(fma)
    for name, b in pool.batch.items():
        out = ctx.compute(b)
        assert np.array_equal(bits(out), bits(pool.want[fma][name][0])), name
        st = ctx.stats()
        assert st["n_pairs"] == b.n_pairs and st["n_fallback"] == b.n_pairs, (name, st)


def test_a_lone_double_caller_is_counted_as_a_small_call(pool):
    from gkl_amd import native
    b = pool.batch["small"]
    native.small_call_counts(0, reset=True)
    with native.PairHmmContext(use_double=True) as c:
        for _ in range(5):
            assert np.array_equal(bits(c.compute(b)), bits(pool.want[1]["small"][0]))
    assert native.small_call_counts(0) == (5, 0, 5)


@pytest.mark.parametrize("fma", [1, 0])
def test_a_multi_device_context_keeps_the_general_pass(pool, fma):
    """devices=[0, 0]: every call is sharded over two engines of device 0.  Their shards are small enough to qualify, and
    must not: a multi-device double-precision context behaves as it always did -- the oracle's bits, nothing counted."""
    from gkl_amd import native
    with native.PairHmmContext(use_double=True, fma_mode=fma, devices=[0, 0]) as c:
        assert c.n_devices == 2
        native.small_call_counts(0, reset=True)
        for name in ("small", "r2", "bounds", "edge", "one"):
            out = c.compute(pool.batch[name])
            assert np.array_equal(bits(out), bits(pool.want[fma][name][0])), name
        got = c.compute_multi([pool.batch[n] for n in ("r2", "small", "r4")])
        for n, out in zip(("r2", "small", "r4"), got):
            assert np.array_equal(bits(out), bits(pool.want[fma][n][0])), n
        assert native.small_call_counts(0) == (0, 0, 0)


def test_raw_sums_of_a_single_call(pool):
    """gklhip_get_raw after a single small call: the fp64 sums of every pair, every flag set, as the general pass leaves them."""
    ctx = pool.context(1)
    for name in ("bounds", "odd", "over"):
        out = ctx.compute(pool.batch[name])
        _, r64, u = ctx.raw(pool.batch[name].n_pairs)
        assert np.array_equal(bits(out), bits(pool.want[1][name][0])), name
        assert u.all() and np.array_equal(bits(r64), bits(pool.want[1][name][2])), name
        assert ctx.stats()["n_fallback"] == pool.batch[name].n_pairs


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [1, 2, 3, 17, 64, 65])
def test_set_sizes_and_counters(pool, K, fma):
    from gkl_amd import native
    ctx = pool.context(fma)
    names = [QUALIFYING[k % len(QUALIFYING)] for k in range(K)]
    singles = {n: ctx.compute(pool.batch[n]) for n in set(names)}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    counts = native.small_call_counts(0)
    stats = ctx.stats()
    print("K", K, "fma", fma, "counts", counts, "n_fallback", stats["n_fallback"], "n_pairs", stats["n_pairs"])
    assert counts == ((65, 65, 2) if K == 65 else (K, K if K > 1 else 0, 1))
    assert stats["n_pairs"] == pool.n_pairs(names)
    assert stats["n_fallback"] == stats["n_pairs"]
    pool.check(ctx, fma, names, got, singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_narrow_and_wide_forms(pool, fma):
    """A set whose reads all have at most 255 bases takes pair_f64_multi_kernel<., 4>; one region with longer reads (`r6`)
    moves the whole set to <., kRplF64>: the same regions give the same bytes in both."""
    from gkl_amd import native
    ctx = pool.context(fma)
    narrow = ["r2", "one", "row", "r2", "one"]
    native.small_call_counts(0, reset=True)
    got_n = ctx.compute_multi([pool.batch[n] for n in narrow])
    assert native.small_call_counts(0) == (5, 5, 1)
    singles = pool.check(ctx, fma, narrow, got_n)
    for wide in (narrow + ["r6"], ["r6"] + narrow):
        native.small_call_counts(0, reset=True)
        got_w = ctx.compute_multi([pool.batch[n] for n in wide])
        assert native.small_call_counts(0) == (6, 6, 1)
        pool.check(ctx, fma, wide, got_w, singles)
        off = wide.index("r2")
        for k, n in enumerate(narrow):
            assert got_w[off + k].tobytes() == got_n[k].tobytes(), n


def test_regions_that_do_not_qualify_run_alone_inside_the_call(pool):
    from gkl_amd import native
    ctx = pool.context(1)
    names = ["edge", "over", "long", "r2", "r2"]
    singles = {n: ctx.compute(pool.batch[n]) for n in set(names)}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    # three regions in one set; `over` and `long` take the single call's path for their size, which counts nothing here
    assert native.small_call_counts(0) == (3, 3, 1)
    assert ctx.stats()["n_fallback"] == ctx.stats()["n_pairs"] == pool.n_pairs(names)
    pool.check(ctx, 1, names, got, singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_raw_sums_per_region(pool, fma):
    ctx = pool.context(fma)
    names = ["bounds", "r2", "odd", "r6", "one"]
    pool.check(ctx, fma, names, ctx.compute_multi([pool.batch[n] for n in names]))   # (its single calls come before the multi call below)
    ctx.compute_multi([pool.batch[n] for n in names])
    for k, n in enumerate(names):
        _, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert u.all(), n
        assert np.array_equal(bits(r64), bits(pool.want[fma][n][2])), n


def test_combining_switched_off_in_a_child_process(pool, tmp_path):
    """GKL_HIP_COMBINE=0 is read once per process: the same multi call there takes the general pass region by region."""
    names = ["bounds", "r2", "odd", "r6", "one", "edge"]
    env = dict(os.environ, GKL_HIP_COMBINE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "child"
    p = subprocess.run([sys.executable, "-m", "tests.pairhmm_double_child", "--out", str(out), "--names", ",".join(names)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(str(out) + ".json") as f:
        rec = json.load(f)
    assert rec["counts"] == [0, 0, 0], rec
    assert rec["n_fallback"] == rec["n_pairs"] == pool.n_pairs(names)
    got = np.load(str(out) + ".npz")
    for k, n in enumerate(names):
        assert np.array_equal(bits(got[f"out{k}"]), bits(pool.want[1][n][0])), n


def test_one_bad_region_of_three(pool):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(1)
    bad = dataclasses.replace(pool.batch["r2"], read_off=pool.batch["r2"].read_off + 1)   # offsets that do not start at 0
    with pytest.raises(native.PairHmmMultiError) as e:
        ctx.compute_multi([pool.batch["r4"], bad, pool.batch["odd"]])
    assert e.value.statuses == [0, native.ERR_INVALID_ARG, 0] and e.value.status == native.ERR_INVALID_ARG
    assert isinstance(e.value.errors[1], IllegalArgumentException) and "offset arrays must start at 0" in str(e.value.errors[1])
    assert e.value.results[1] is None
    assert np.array_equal(bits(e.value.results[0]), bits(pool.want[1]["r4"][0]))
    assert np.array_equal(bits(e.value.results[2]), bits(pool.want[1]["odd"][0]))
    # and the context goes on
    assert np.array_equal(bits(ctx.compute_multi([pool.batch["one"]])[0]), bits(pool.want[1]["one"][0]))

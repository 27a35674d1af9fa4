"""The small-read limit at 511 bases (gklhip_set_small_read_limit / GKL_HIP_SMALL_READ_LIMIT=511): a region whose longest
read has 384 to 511 bases takes the small-call path -- the 8-row forms of the fused per-pair kernel, of the one-launch
policy kernel, of the two-launch policy of mid-size regions and of the all-fp64 per-pair kernel, alone and in the shared
sets of gklhip_compute_multi.  Without the switch such a region keeps the general pass and runs alone, as before.  Every
output is compared bit for bit with the oracle's, computed live once per arithmetic mode; the combiner's counters are
asserted exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd import server
from gkl_amd.synth import make_batch, random_batch
from tests.test_pairhmm_double_small import bits, exact_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS8 = [1, 127, 128, 255, 256, 383, 384, 511]   # both ends of all four rows-per-lane tiers
MID8_LONG = [384, 450, 511]
DOUBLE_NAMES = ["bounds8", "hc8", "region8", "r2", "r512"]   # what the double-precision oracle is computed for


def mid8(seed):
    """70 x 30 = 2100 pairs, a mid-size region: three reads of exactly 384, 450 and 511 bases, the rest short (low
    qualities: unrelated reads of this length stay inside fp64's range)."""
    rng = np.random.RandomState(seed)
    b = random_batch(rng, 70, 30, read_len=(511, 511), hap_len=(520, 600), qual_range=(6, 14))
    return exact_reads(b, MID8_LONG + [int(x) for x in rng.randint(20, 91, size=67)])


def build_pool():
    """The smallest shapes at which an 8-row form can go wrong (reads x haplotypes)."""
    pool = {
        "bounds8": exact_reads(random_batch(np.random.RandomState(72), 8, 2, read_len=(511, 511), hap_len=(500, 530), qual_range=(6, 14)), BOUNDS8),
        "hc8": make_batch("hc", 6, 3, seed=6, read_len=(384, 511), hap_len=(520, 600)),       # the fused kernel's two exits at 8 rows
        "region8": make_batch("region", 6, 3, seed=7, read_len=(384, 511), hap_len=(520, 600)),   # no pair recomputed
        "r2": make_batch("hc", 12, 3, seed=4, read_len=(20, 90), hap_len=(60, 120)),          # a narrow companion
        "mid8": mid8(73),
        "mid8b": mid8(74),
    }
    b = random_batch(np.random.RandomState(75), 2, 2, read_len=(512, 512), hap_len=(520, 550), qual_range=(6, 14))   # one read of 512 bases: outside the limit
    pool["r512"] = exact_reads(b, [512, 25])
    return pool


class Pool:
    def __init__(self, oracle):
        self.batch = build_pool()
        # (out, raw32, raw64, used64) of the oracle per fma mode, computed once: the fp32 policy for every region, the
        # use_double arithmetic for the small ones
        self.want = {fma: {name: oracle.batch(b, fma_mode=fma, want_raw=True, n_threads=4) for name, b in self.batch.items()} for fma in (0, 1)}
        self.want64 = {fma: {name: oracle.batch(self.batch[name], use_double=True, fma_mode=fma, want_raw=True, n_threads=4) for name in DOUBLE_NAMES}
                       for fma in (0, 1)}
        self.ctx = {}

    def context(self, fma, use_double=False, rows_per_lane=0):
        """A context with the limit at 511, set through the setter."""
        from gkl_amd import native
        key = (fma, use_double, rows_per_lane)
        if key not in self.ctx:
            self.ctx[key] = native.PairHmmContext(use_double=use_double, fma_mode=fma, rows_per_lane=rows_per_lane)
            self.ctx[key].set_small_read_limit(511)
        return self.ctx[key]

    def check(self, ctx, want, names, got, singles=None):
        """Every region: the oracle's bytes and the bytes of the single call on the same context."""
        assert len(got) == len(names)
        singles = {} if singles is None else singles
        for k, (name, out) in enumerate(zip(names, got)):
            assert np.array_equal(bits(out), bits(want[name][0])), (k, name, "oracle")
            if name not in singles:
                singles[name] = ctx.compute(self.batch[name])
            assert out.tobytes() == singles[name].tobytes(), (k, name, "single call")
        return singles

    def check_raw(self, name, want, raw):
        r32, r64, u = raw
        e32, e64, eu = want[name][1:4]
        assert np.array_equal(u, eu), (name, "used64")
        assert r32.tobytes() == e32.tobytes(), (name, "raw32")
        assert r64[eu == 1].tobytes() == e64[eu == 1].tobytes(), (name, "raw64")

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
    assert b["bounds8"].read_lens.tolist() == BOUNDS8 and np.diff(b["bounds8"].hap_off).tolist() == [524, 501]
    assert b["hc8"].read_lens.tolist() == [426, 414, 503, 428, 408, 504] and np.diff(b["hc8"].hap_off).tolist() == [523, 564, 573]
    assert b["region8"].n_reads == 6 and b["region8"].n_haps == 3
    assert 395 <= int(b["region8"].read_lens.min()) and int(b["region8"].read_lens.max()) <= 401
    assert int(b["r2"].read_lens.max()) <= 90 and b["r2"].n_pairs == 36
    assert b["r512"].read_lens.tolist() == [512, 25] and b["r512"].n_haps == 2
    for n in ("mid8", "mid8b"):
        assert (b[n].n_reads, b[n].n_haps, b[n].n_pairs) == (70, 30, 2100)
        assert b[n].read_lens.tolist()[:3] == MID8_LONG
        assert 20 <= int(b[n].read_lens[3:].min()) and int(b[n].read_lens[3:].max()) <= 90
    assert (b["bounds8"].n_pairs, b["hc8"].n_pairs, b["region8"].n_pairs) == (16, 18, 18)
    for fma in (0, 1):
        for name, w in pool.want[fma].items():
            assert np.isfinite(w[0]).all(), (name, fma, "a likelihood that underflowed fp64 checks nothing: change the seed")
        for name, w in pool.want64[fma].items():
            assert w[3].all(), (name, "the use_double oracle takes every pair in fp64")
            assert np.isfinite(w[0]).all(), (name, fma, "double", "a likelihood that underflowed fp64 checks nothing: change the seed")
    w = pool.want[1]
    # what the fp32 policy decides (fma_mode 1)
    u = w["bounds8"][3].reshape(8, 2)
    assert int(u.sum()) == 11 and u[6:].all() and float(w["bounds8"][0].min()) == pytest.approx(-266.0, abs=0.5)
    u = w["hc8"][3]
    assert (int((u == 0).sum()), int(u.sum())) == (16, 2) and float(w["hc8"][0].min()) == pytest.approx(-93.04, abs=0.01)
    assert int(w["region8"][3].sum()) == 0 and float(w["region8"][0].min()) == pytest.approx(-48.5, abs=0.1)
    # reads above 383 bases on both sides of the policy, in both regions together and in hc8 alone (bounds8: all four
    # pairs of its two long reads are recomputed, its short reads stay fp32)
    long_hc8 = np.repeat(b["hc8"].read_lens > 383, 3)
    assert (w["hc8"][3][long_hc8] == 1).any() and (w["hc8"][3][long_hc8] == 0).any()
    long_b8 = np.repeat(b["bounds8"].read_lens > 383, 2)
    assert (w["bounds8"][3][long_b8] == 1).all() and (w["bounds8"][3][~long_b8] == 0).any()


@pytest.mark.parametrize("fma", [1, 0])
def test_single_calls_fp32_context(pool, fma):
    ctx = pool.context(fma)
    for name, b in pool.batch.items():
        out = ctx.compute(b)
        assert np.array_equal(bits(out), bits(pool.want[fma][name][0])), name
        pool.check_raw(name, pool.want[fma], ctx.raw(b.n_pairs))
        st = ctx.stats()
        assert st["n_pairs"] == b.n_pairs and st["n_fallback"] == int(pool.want[fma][name][3].sum()), (name, st)


def test_a_lone_caller_of_long_read_regions_is_counted_as_a_small_call(pool):
    from gkl_amd import native
    ctx = pool.context(1)
    native.small_call_counts(0, reset=True)
    for _ in range(5):
        assert np.array_equal(bits(ctx.compute(pool.batch["hc8"])), bits(pool.want[1]["hc8"][0]))
    assert native.small_call_counts(0) == (5, 0, 5)


@pytest.mark.parametrize("fma", [1, 0])
def test_shared_sets_of_the_fused_kind(pool, fma):
    """A set with a read of 384 bases or more moves from the 4- or 6-row form to the 8-row form as a whole: the narrow
    companion gives the same bytes in either company."""
    from gkl_amd import native
    ctx = pool.context(fma)
    native.small_call_counts(0, reset=True)
    r2_alone = ctx.compute_multi([pool.batch["r2"], pool.batch["r2"]])   # the 4-row form
    assert native.small_call_counts(0) == (2, 2, 1)
    singles = None
    for names in (["r2", "hc8", "bounds8", "region8"], ["hc8", "r2"], ["r2", "r2", "hc8"]):
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([pool.batch[n] for n in names])
        n = len(names)
        assert native.small_call_counts(0) == (n, n, 1), names
        st = ctx.stats()
        assert st["n_pairs"] == pool.n_pairs(names)
        assert st["n_fallback"] == sum(int(pool.want[fma][x][3].sum()) for x in names)
        for k, x in enumerate(names):
            pool.check_raw(x, pool.want[fma], ctx.raw_region(k, pool.batch[x].n_pairs))
            if x == "r2":
                assert got[k].tobytes() == r2_alone[0].tobytes(), (names, k)
        singles = pool.check(ctx, pool.want[fma], names, got, singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_one_launch_policy_kind(pool, fma):
    """rows_per_lane=8: the packed fp32 pass, then pairhmm_pair_policy_kernel / pair_policy_multi_kernel at 8 rows."""
    from gkl_amd import native
    ctx = pool.context(fma, rows_per_lane=8)
    native.small_call_counts(0, reset=True)
    out = ctx.compute(pool.batch["hc8"])
    assert native.small_call_counts(0) == (1, 0, 1)
    assert np.array_equal(bits(out), bits(pool.want[fma]["hc8"][0]))
    pool.check_raw("hc8", pool.want[fma], ctx.raw(pool.batch["hc8"].n_pairs))
    names = ["hc8", "bounds8"]
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (2, 2, 1)
    for k, x in enumerate(names):
        pool.check_raw(x, pool.want[fma], ctx.raw_region(k, pool.batch[x].n_pairs))
    pool.check(ctx, pool.want[fma], names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_mid_size_kind(pool, fma):
    from gkl_amd import native
    ctx = pool.context(fma)
    names = ["mid8", "mid8b"]
    singles = {n: ctx.compute(pool.batch[n]) for n in names}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (2, 2, 1)
    for k, x in enumerate(names):
        pool.check_raw(x, pool.want[fma], ctx.raw_region(k, pool.batch[x].n_pairs))
    pool.check(ctx, pool.want[fma], names, got, singles)
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch["mid8"]])
    assert native.small_call_counts(0) == (0, 0, 0)   # one mid-size region is no set: the single call's path, which counts nothing
    pool.check(ctx, pool.want[fma], ["mid8"], got, singles)


@pytest.mark.parametrize("fma", [1, 0])
def test_double_precision_context(pool, fma):
    from gkl_amd import native
    ctx = pool.context(fma, use_double=True)
    want = pool.want64[fma]
    for name in ("bounds8", "hc8"):
        b = pool.batch[name]
        native.small_call_counts(0, reset=True)
        out = ctx.compute(b)
        assert native.small_call_counts(0) == (1, 0, 1), name
        assert np.array_equal(bits(out), bits(want[name][0])), name
        _, r64, u = ctx.raw(b.n_pairs)
        assert u.all() and np.array_equal(bits(r64), bits(want[name][2])), name
        st = ctx.stats()
        assert st["n_fallback"] == st["n_pairs"] == b.n_pairs, (name, st)
    names = ["r2", "bounds8", "hc8"]
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (3, 3, 1)
    assert ctx.stats()["n_fallback"] == ctx.stats()["n_pairs"] == pool.n_pairs(names)
    for k, x in enumerate(names):
        _, r64, u = ctx.raw_region(k, pool.batch[x].n_pairs)
        assert u.all() and np.array_equal(bits(r64), bits(want[x][2])), x
    pool.check(ctx, want, names, got)


@pytest.mark.parametrize("use_double", [False, True])
def test_a_read_of_512_bases_stays_outside(pool, use_double):
    from gkl_amd import native
    ctx = pool.context(1, use_double=use_double)
    want = pool.want64[1] if use_double else pool.want[1]
    names = ["r2", "r512", "hc8"]
    singles = {n: ctx.compute(pool.batch[n]) for n in names}
    native.small_call_counts(0, reset=True)
    got = ctx.compute_multi([pool.batch[n] for n in names])
    assert native.small_call_counts(0) == (2, 2, 1)   # `r512` takes the general pass, which counts nothing
    pool.check(ctx, want, names, got, singles)


def test_the_default_is_383_and_the_setter_goes_both_ways(pool):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    names = ["r2", "hc8", "r2"]
    with native.PairHmmContext() as ctx:
        def multi():
            native.small_call_counts(0, reset=True)
            got = ctx.compute_multi([pool.batch[n] for n in names])
            counts = native.small_call_counts(0)
            for n, out in zip(names, got):
                assert np.array_equal(bits(out), bits(pool.want[1][n][0])), n
            return counts
        assert multi() == (2, 2, 1)   # `hc8` runs alone, as it always did
        native.small_call_counts(0, reset=True)
        ctx.compute(pool.batch["hc8"])
        assert native.small_call_counts(0) == (0, 0, 0)
        ctx.set_small_read_limit(511)
        assert multi() == (3, 3, 1)
        ctx.set_small_read_limit(383)
        assert multi() == (2, 2, 1)
        for bad in (400, 0, 512, 639, -1):
            with pytest.raises(IllegalArgumentException):
                ctx.set_small_read_limit(bad)
        assert multi() == (2, 2, 1)   # a refused value changes nothing
    with native.PairHmmContext(small_read_limit=511) as ctx:
        native.small_call_counts(0, reset=True)
        assert np.array_equal(bits(ctx.compute(pool.batch["hc8"])), bits(pool.want[1]["hc8"][0]))
        assert native.small_call_counts(0) == (1, 0, 1)
    with pytest.raises(IllegalArgumentException):
        native.PairHmmContext(small_read_limit=400)


def run_child(tmp_path, tag, names, **env_extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
    out = tmp_path / tag
    p = subprocess.run([sys.executable, "-m", "tests.pairhmm_small_long_reads_child", "--out", str(out), "--names", ",".join(names)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(str(out) + ".json") as f:
        return json.load(f), np.load(str(out) + ".npz")


def test_the_environment_sets_the_default_of_a_child_process(pool, tmp_path):
    """GKL_HIP_SMALL_READ_LIMIT and GKL_HIP_COMBINE are read once per process: a plain context there, no setter."""
    names = ["hc8", "r2"]
    for tag, extra, counts in (("on", {}, [2, 2, 1]), ("nocombine", {"GKL_HIP_COMBINE": "0"}, [0, 0, 0])):
        rec, got = run_child(tmp_path, tag, names, GKL_HIP_SMALL_READ_LIMIT="511", **extra)
        assert rec["counts"] == counts, (tag, rec)
        assert rec["n_pairs"] == pool.n_pairs(names)
        for k, n in enumerate(names):
            assert np.array_equal(bits(got[f"out{k}"]), bits(pool.want[1][n][0])), (tag, n)


def test_a_server_follows_its_environment_and_a_client_cannot_set_the_limit(pool, tmp_path):
    from gkl_amd import native
    from gkl_amd.errors import RuntimeException
    env = dict(os.environ, GKL_HIP_SMALL_READ_LIMIT="511")
    h = server.start(str(tmp_path / "s.sock"), env=env, timeout=120)
    try:
        with native.PairHmmContext(server=h.socket_path) as c:
            assert c.is_remote
            for name in ("hc8", "bounds8"):
                assert np.array_equal(bits(c.compute(pool.batch[name])), bits(pool.want[1][name][0])), name
            with pytest.raises(RuntimeException, match="unsupported"):
                c.set_small_read_limit(511)
            # ... and the server's combiner saw both calls as small calls
            assert tuple(h.stats()["small_call_counts"][0]) == (2, 0, 2)
    finally:
        assert h.stop() == 0

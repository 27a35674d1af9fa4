"""Mid-size regions of a double-precision context (gklhip_config.use_double; 2049 - 65 536 pairs, no read too long for a
chunk of the packed fp64 pass) in shared sets of one gklhip_compute_multi call (kSmallDoubleStream): prep_multi_kernel,
fwd_stream_f64_multi_kernel<fma, kRplF64Jobs> and finalize64_multi_kernel -- three launches and one synchronise for up to
64 regions.  Region k's output is, byte for byte, what the live `use_double` oracle computes and what the single call
writes for it on the same context, whichever other regions share its set, in both fma modes; the combiner's counters say
which sets formed.  (At the parent of this change every counter assertion below reads (0, 0, 0) and fails, except where
small regions of the same call share a set of their own: every mid-size region ran alone.)

Shapes: the smallest at which these launches can go wrong -- reads of 10-20 bases against haplotypes of 20-30 wherever
a case does not need longer ones."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd.synth import random_batch
from tests.test_pairhmm_double_small import bits, exact_reads
from tests.test_pairhmm_double_small import build_pool as build_small_pool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the mid-size regions that qualify for a shared set, without the biggest one
QUALIFYING = ["m2049", "m2304", "m_n", "m_long", "m_groups", "m_chunks"]
VARIANTS = ["m_n", "m_long", "m_groups", "m_chunks"]
SHORT = dict(read_len=(10, 20), hap_len=(20, 30), qual_range=(5, 50))
LONG_READS = [384, 500, 639]   # beyond the per-pair kernel's 383 bases, up to the chunk's limit (64 lanes x 10 rows - 1)


def six_arrays_bytes(b):
    up = lambda x: (int(x) + 255) // 256 * 256  # noqa: E731
    return 5 * up(b.read_off[-1]) + up(b.hap_off[-1])


def build_pool():
    rng = np.random.RandomState(71)
    small = build_small_pool()
    pool = {
        "m2049": random_batch(rng, 683, 3, **SHORT),                        # the first size that qualifies; the last finalising block holds one pair
        "m2304": random_batch(rng, 64, 36, **SHORT),                        # a second plain region: exactly nine full finalising blocks
        # haplotypes with an 'N' leave the asm whole-job program (WaveJob::run), the one without keeps it; odd bytes, every
        # quality byte.  (A seed of its own: a read whose first gap-continuation byte is 0 has likelihood 0 against every
        # haplotype -- not an underflow, but log10 gives -inf -- and most seeds deal one such read among 700.)
        "m_n": random_batch(np.random.RandomState(163), 700, 3, read_len=(10, 20), hap_len=(20, 30), alphabet=b"ACGTNacgtRY", qual_range=(0, 255)),
        # more than one haplotype stream group
        "m_groups": random_batch(rng, 17, 128, read_len=(10, 20), hap_len=(20, 500), qual_range=(5, 50)),
        # at least 64 chunks, not a multiple of 8: the launch holds padded blocks
        "m_chunks": random_batch(rng, 2100, 3, **SHORT),
        "m_top": random_batch(rng, 2048, 32, **SHORT),                      # 65 536 pairs: the largest size that shares
        "m_over": random_batch(rng, 2056, 32, **SHORT),                     # 65 792 pairs: runs alone
        "m_big_in": random_batch(rng, 2200, 1, read_len=(100, 110), hap_len=(20, 30), qual_range=(5, 50)),   # inputs above 1 MB: runs alone
        # small company for the mixed calls (tests/test_pairhmm_double_small.py's shapes)
        "r2": small["r2"],
        "long": small["long"],                                              # one read of 400 bases and 4 pairs: runs alone
    }
    # three reads cut to exactly 384, 500 and 639 bases, the rest short (low qualities: reads of this length stay inside fp64's range)
    b = random_batch(rng, 70, 30, read_len=(639, 639), hap_len=(640, 700), qual_range=(6, 14))
    pool["m_long"] = exact_reads(b, LONG_READS + [int(x) for x in rng.randint(10, 21, size=67)])
    return pool


class Pool:
    def __init__(self, oracle):
        self.batch = build_pool()
        # (out, raw32, raw64, used64) of the use_double oracle per fma mode, computed once
        self.want = {fma: {name: oracle.batch(b, use_double=True, fma_mode=fma, want_raw=True, n_threads=4) for name, b in self.batch.items()}
                     for fma in (0, 1)}
        self.ctx = {}
        self.singles = {}

    def context(self, fma):
        from gkl_amd import native
        if fma not in self.ctx:
            self.ctx[fma] = native.PairHmmContext(use_double=True, fma_mode=fma)
        return self.ctx[fma]

    def single(self, fma, name):
        """The single call's output on the context of this fma mode (computed once per context and region)."""
        key = (fma, name)
        if key not in self.singles:
            self.singles[key] = self.context(fma).compute(self.batch[name])
        return self.singles[key]

    def check(self, fma, names, got):
        """Every region: the oracle's bytes and the bytes of the single call on the same context."""
        assert len(got) == len(names)
        for k, (name, out) in enumerate(zip(names, got)):
            assert np.array_equal(bits(out), bits(self.want[fma][name][0])), (k, name, "oracle")
            assert out.tobytes() == self.single(fma, name).tobytes(), (k, name, "single call")

    def run(self, fma, names):
        """One multi call and the combiner's counts for it (the single calls it is compared with are made before)."""
        from gkl_amd import native
        ctx = self.context(fma)
        for n in set(names):
            self.single(fma, n)
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([self.batch[n] for n in names])
        return got, native.small_call_counts(0)

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
    pairs = {n: b[n].n_pairs for n in b}
    assert (pairs["m2049"], pairs["m2304"], pairs["m_top"], pairs["m_over"]) == (2049, 2304, 65536, 65792)
    assert (b["m2049"].n_reads, b["m2049"].n_haps) == (683, 3)
    assert (b["m_top"].n_reads, b["m_top"].n_haps, b["m_over"].n_reads, b["m_over"].n_haps) == (2048, 32, 2056, 32)
    assert (b["m_groups"].n_reads, b["m_groups"].n_haps) == (17, 128)
    for n in QUALIFYING + ["m_top", "m_big_in"]:
        assert 2048 < pairs[n] <= 65536, n
    assert pairs["r2"] <= 2048 and pairs["long"] <= 2048
    for n in QUALIFYING + ["m_top", "m_over"]:
        assert six_arrays_bytes(b[n]) <= 1 << 20, n
    assert six_arrays_bytes(b["m_big_in"]) > 1 << 20
    for n in ("m2049", "m2304", "m_n", "m_groups", "m_chunks", "m_top", "m_over"):
        assert 10 <= int(b[n].read_lens.min()) and int(b[n].read_lens.max()) <= 20, n
    assert b["m_long"].read_lens.tolist()[:3] == LONG_READS and int(b["m_long"].read_lens[3:].max()) <= 20
    assert (b["m_long"].n_reads, b["m_long"].n_haps) == (70, 30)
    assert b["long"].read_lens.tolist() == [400, 25]
    hap_lens = np.diff(b["m_groups"].hap_off)
    assert 20 <= int(hap_lens.min()) and int(hap_lens.max()) <= 500
    has_n = [b"N" in bytes(b["m_n"].hap_bases[int(b["m_n"].hap_off[h]):int(b["m_n"].hap_off[h + 1])]) for h in range(3)]
    assert any(has_n) and not all(has_n), "haplotypes with and without an N"
    assert set(np.unique(b["m_n"].read_quals).tolist()) == set(range(256)), "every quality byte"
    for fma in (0, 1):
        for name, w in pool.want[fma].items():
            assert w[3].all(), (name, "the use_double oracle takes every pair in fp64")
            assert np.isfinite(w[0]).all(), (name, "a likelihood that underflowed fp64 checks nothing: change the seed")


def test_the_plans_are_what_the_variants_need(pool):
    """Checked on the plan itself: the statistics of the single call (gklhip_get_stats: n_chunks, n_hap_groups,
    rows_per_lane -- plan_call fills them from the plan the launches use).  `m_groups`: more than one haplotype stream
    group.  `m_chunks`: at least 64 chunks (from there on the streaming grid is padded to a multiple of 8 chunks per
    group) and not a multiple of 8, so the launch holds padded blocks."""
    ctx = pool.context(1)
    seen = {}
    for n in QUALIFYING + ["m_top"]:
        ctx.compute(pool.batch[n])
        st = ctx.stats()
        seen[n] = (st["n_chunks"], st["n_hap_groups"], st["rows_per_lane"])
    print("(n_chunks, n_hap_groups, rows_per_lane):", seen)
    assert all(v[2] == 10 for v in seen.values())
    assert seen["m_groups"][1] > 1
    assert seen["m_chunks"][0] >= 64 and seen["m_chunks"][0] % 8 != 0
    assert seen["m2049"][0] < 64 and seen["m2049"][0] % 8 != 0    # no padding below 64 chunks


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("K", [2, 3, 64, 65])
def test_set_sizes_and_counters(pool, K, fma):
    names = [QUALIFYING[k % len(QUALIFYING)] for k in range(K)]
    got, counts = pool.run(fma, names)
    stats = pool.context(fma).stats()
    print("K", K, "fma", fma, "counts", counts, "n_fallback", stats["n_fallback"], "n_pairs", stats["n_pairs"])
    assert counts == ((65, 65, 2) if K == 65 else (K, K, 1))
    assert stats["n_pairs"] == pool.n_pairs(names)
    assert stats["n_fallback"] == stats["n_pairs"]
    pool.check(fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_mixed_call(pool, fma):
    names = ["r2", "m2049", "r2", "m_n", "long", "r2"]
    got, counts = pool.run(fma, names)
    assert counts == (5, 5, 2)                # one set of the three small regions, one of the two mid-size ones; `long` runs alone
    st = pool.context(fma).stats()
    assert st["n_fallback"] == st["n_pairs"] == pool.n_pairs(names)
    pool.check(fma, names, got)
    names = ["r2", "m2049", "r2"]
    got, counts = pool.run(fma, names)
    assert counts == (2, 2, 1)                # the lone mid-size region is no set and runs alone
    pool.check(fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_limits(pool, fma):
    for names, want in ((["m_top", "m2049"], (2, 2, 1)), (["m_over", "m2049"], (0, 0, 0)), (["m_big_in", "m2049"], (0, 0, 0))):
        got, counts = pool.run(fma, names)
        assert counts == want, names
        st = pool.context(fma).stats()
        assert st["n_fallback"] == st["n_pairs"] == pool.n_pairs(names)
        pool.check(fma, names, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_every_variant_in_one_set(pool, fma):
    got, counts = pool.run(fma, VARIANTS)
    assert counts == (4, 4, 1)
    pool.check(fma, VARIANTS, got)


@pytest.mark.parametrize("fma", [1, 0])
def test_a_region_does_not_depend_on_its_company(pool, fma):
    rng = np.random.RandomState(5)
    seen = {}
    for names in [list(rng.permutation(QUALIFYING)) for _ in range(3)]:
        got, counts = pool.run(fma, names)
        assert counts == (6, 6, 1)
        pool.check(fma, names, got)
        for n, out in zip(names, got):
            assert seen.setdefault(n, out.tobytes()) == out.tobytes(), (n, names)


@pytest.mark.parametrize("fma", [1, 0])
def test_raw_sums_per_region(pool, fma):
    names = ["m2049", "m_n", "m_long", "m_groups", "m_chunks"]
    got, counts = pool.run(fma, names)
    assert counts == (5, 5, 1)
    pool.check(fma, names, got)      # (its single calls were made before the multi call)
    ctx = pool.context(fma)
    for k, n in enumerate(names):
        _, r64, u = ctx.raw_region(k, pool.batch[n].n_pairs)
        assert u.all(), n
        assert np.array_equal(bits(r64), bits(pool.want[fma][n][2])), n


@pytest.mark.parametrize("fma", [1, 0])
def test_one_bad_region_of_three(pool, fma):
    from gkl_amd import native
    from gkl_amd.errors import IllegalArgumentException
    ctx = pool.context(fma)
    bad = dataclasses.replace(pool.batch["m2049"], read_off=pool.batch["m2049"].read_off.copy())
    bad.read_off[4] = bad.read_off[3]          # a read offset that does not increase
    singles = [pool.single(fma, n) for n in ("m2304", "m_n")]
    native.small_call_counts(0, reset=True)
    with pytest.raises(native.PairHmmMultiError) as e:
        ctx.compute_multi([pool.batch["m2304"], bad, pool.batch["m_n"]])
    assert native.small_call_counts(0) == (2, 2, 1)    # the two good ones share a set
    assert e.value.statuses == [0, native.ERR_INVALID_ARG, 0] and e.value.status == native.ERR_INVALID_ARG
    assert isinstance(e.value.errors[1], IllegalArgumentException) and "read 3 is empty or offsets are not increasing" in str(e.value.errors[1])
    assert e.value.results[1] is None
    pool.check(fma, ["m2304", "m_n"], [e.value.results[0], e.value.results[2]])   # the oracle and the single calls
    assert e.value.results[0].tobytes() == singles[0].tobytes() and e.value.results[2].tobytes() == singles[1].tobytes()
    # and the context goes on
    assert np.array_equal(bits(ctx.compute(pool.batch["m2304"])), bits(pool.want[fma]["m2304"][0]))
    names = ["m2049", "m_n"]
    got, counts = pool.run(fma, names)
    assert counts == (2, 2, 1)
    pool.check(fma, names, got)


def run_child(tmp_path, names, fma, **env_add):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_add)
    out = tmp_path / "child"
    p = subprocess.run([sys.executable, "-m", "tests.pairhmm_double_mid_child", "--out", str(out), "--names", ",".join(names), "--fma", str(fma)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(str(out) + ".json") as f:
        rec = json.load(f)
    return rec, np.load(str(out) + ".npz")


def test_combining_switched_off_in_a_child_process(pool, tmp_path):
    """GKL_HIP_COMBINE=0 is read once per process: the same multi call there takes the general pass region by region."""
    names = VARIANTS + ["m2049"]
    rec, got = run_child(tmp_path, names, 1, GKL_HIP_COMBINE="0")
    assert rec["counts"] == [0, 0, 0], rec
    assert rec["n_fallback"] == rec["n_pairs"] == pool.n_pairs(names)
    for k, n in enumerate(names):
        assert np.array_equal(bits(got[f"out{k}"]), bits(pool.want[1][n][0])), n


@pytest.mark.parametrize("fma", [1, 0])
def test_cxx_steps_in_a_child_process(pool, tmp_path, fma):
    """GKLHIP_ASM_GENERAL=0: the same set through the C++ steps instead of the whole-job asm programs."""
    names = VARIANTS + ["m2049"]
    rec, got = run_child(tmp_path, names, fma, GKLHIP_ASM_GENERAL="0")
    assert rec["counts"] == [5, 5, 1], rec
    assert rec["n_fallback"] == rec["n_pairs"] == pool.n_pairs(names)
    for k, n in enumerate(names):
        assert np.array_equal(bits(got[f"out{k}"]), bits(pool.want[fma][n][0])), n

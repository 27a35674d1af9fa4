"""Concurrent callers' mid-size regions in shared sets (gklhip_set_mid_combine / GKL_HIP_COMBINE_MID; off by default): a
single gklhip_compute of a region of 2049 - 65 536 pairs enters the small-call combiner and leaves with the like regions
of the threads that meet it on the device, through the set kernels of the multi call (prep_multi_kernel,
fwd_stream_multi_kernel, pair_flag_multi_kernel, pair_recompute_multi_kernel; use_double: fwd_stream_f64_multi_kernel,
finalize64_multi_kernel) -- alone, as a set of one.  Every output is, byte for byte, the oracle's, whoever rides along;
the combiner's counters say what entered.  (At the parent of this change the setter does not exist and every count
asserted as (1, 0, 1) for a mid-size region reads (0, 0, 0).)

Shapes: the pools of tests/test_pairhmm_multi_mid.py and tests/test_pairhmm_double_mid.py, the smallest at which the set
kernels can go wrong (reads of 10-20 bases against haplotypes of 20-30, regions just above 2048 pairs, the variants of
each kernel family, the limits).  What each region is supposed to be is asserted again below.

One check is less than its issue asked for.  A device-finalising context (which never enters) cannot give "the oracle's
bytes" for its log10 values, with the switch on or off, at this commit or its parent: the device's log10 is not the host
libm's (tests/test_gpu_parity.py bounds it: 3.9e-6 absolute for GKLHIP_FINALIZE_DEVICE_REF32).  Asserted for it instead:
the raw sums and fallback flags are the oracle's bit for bit, the output is byte for byte what the same context writes
with the switch off, and it lies within that bound of the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd.synth import make_batch
from tests.test_pairhmm_double_mid import QUALIFYING as QUALIFYING_F64
from tests.test_pairhmm_double_mid import build_pool as build_pool_f64
from tests.test_pairhmm_multi_mid import QUALIFYING as QUALIFYING_F32
from tests.test_pairhmm_multi_mid import build_pool as build_pool_f32
from tests.test_pairhmm_multi_mid import six_arrays_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "hc:100:10:3"   # a GATK-sized region
MEET = dict(GKL_HIP_COMBINE_MID=1, GKL_HIP_COMBINE_MIN=4, GKL_HIP_COMBINE_WAIT_US=2000000)
OFF, LONE = (0, 0, 0), (1, 0, 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Pools:
    """Both pools and the oracle's (out, raw32, raw64, used64) for them, computed once."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.batch = {"f32": build_pool_f32(), "f64": build_pool_f64()}
        self.batch["f32"][SMALL] = self.batch["f64"][SMALL] = make_batch("hc", 100, 10, seed=3)
        self.entering = {"f32": QUALIFYING_F32 + ["m_top"], "f64": QUALIFYING_F64 + ["m_top"]}
        self.cache = {}

    def want(self, pool, name, fma, use_double=None):
        use_double = (pool == "f64") if use_double is None else use_double
        key = (pool, name, fma, use_double)
        if key not in self.cache:
            self.cache[key] = self.oracle.batch(self.batch[pool][name], use_double=use_double, fma_mode=fma, want_raw=True, n_threads=4)
        return self.cache[key]

    def check_raw(self, pool, name, fma, raw, use_double=None):
        _, e32, e64, eu = self.want(pool, name, fma, use_double)
        r32, r64, u = raw
        assert np.array_equal(u, eu), name
        assert np.array_equal(bits(r64[u == 1]), bits(e64[eu == 1])), name
        if not ((pool == "f64") if use_double is None else use_double):
            assert np.array_equal(r32[u == 0].view(np.uint32), e32[eu == 0].view(np.uint32)), name


@pytest.fixture(scope="module")
def pools(oracle):
    return Pools(oracle)


def counted(ctx, batch):
    from gkl_amd import native
    native.small_call_counts(0, reset=True)
    out = ctx.compute(batch)
    return out, native.small_call_counts(0)


def test_the_regions_are_what_they_are_supposed_to_be(pools):
    for p in ("f32", "f64"):
        b = pools.batch[p]
        pairs = {n: b[n].n_pairs for n in b}
        assert (pairs["m2049"], pairs["m2304"], pairs["m_top"], pairs["m_over"], pairs[SMALL]) == (2049, 2304, 65536, 65792, 1000)
        for n in pools.entering[p] + ["m_big_in"]:
            assert 2048 < pairs[n] <= 65536, (p, n)
        for n in pools.entering[p] + ["m_over", SMALL]:
            assert six_arrays_bytes(b[n]) <= 1 << 20, (p, n)
        assert six_arrays_bytes(b["m_big_in"]) > 1 << 20
    b = pools.batch["f32"]
    assert int(b["m_r6"].read_lens.max()) <= 383 and max(int(b[n].read_lens.max()) for n in pools.entering["f32"] + ["m_over", "m_big_in"] if n != "m_r6") <= 255
    assert b["m_allfb"].n_pairs == 2100
    for fma in (0, 1):
        assert pools.want("f32", "m_allfb", fma)[3].all() and not pools.want("f32", "m_nofb", fma)[3].any()
        for n in ("m2049", "m2304", "m_odd", "m_top", "m_r4", "m_r6"):      # both kinds of pair
            assert 0 < int(pools.want("f32", n, fma)[3].sum()) < b[n].n_pairs, n
        for n in pools.entering["f64"]:
            w = pools.want("f64", n, fma)
            assert w[3].all() and np.isfinite(w[0]).all(), n
    d = pools.batch["f64"]
    assert d["m_long"].read_lens.tolist()[:3] == [384, 500, 639] and int(d["m_long"].read_lens.max()) == 639
    assert max(int(d[n].read_lens.max()) for n in pools.entering["f64"] + ["m_over"] if n != "m_long") <= 20


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_lone_calls(pools, pool, fma):
    """Each entering region on a fresh context: once with the switch off, once with it on."""
    from gkl_amd import native
    for name in pools.entering[pool]:
        b = pools.batch[pool][name]
        want = pools.want(pool, name, fma)
        with native.PairHmmContext(use_double=pool == "f64", fma_mode=fma) as ctx:
            off, counts = counted(ctx, b)
            assert counts == OFF, (name, counts)
            ctx.set_mid_combine(True)
            on, counts = counted(ctx, b)
            assert counts == LONE, (name, counts)
            st = ctx.stats()              # n_fallback as the finaliser counted it
            raw = ctx.raw(b.n_pairs)
            assert ctx.stats()["n_fallback"] == st["n_fallback"], name   # ... and as gklhip_get_raw read it back
            assert np.array_equal(bits(off), bits(want[0])), name
            assert np.array_equal(bits(on), bits(want[0])), name
            assert on.tobytes() == off.tobytes(), name
            pools.check_raw(pool, name, fma, raw)
            assert st["n_pairs"] == b.n_pairs and st["n_fallback"] == int(want[3].sum()), (name, st)
            ctx.set_mid_combine(False)
            _, counts = counted(ctx, b)
            assert counts == OFF, (name, counts)


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_a_context_that_starts_switched_on(pools, pool, fma):
    """No switched-off call came before to reserve anything: the biggest region first, then every other one, and
    get_stats after each as the finaliser counted."""
    from gkl_amd import native
    with native.PairHmmContext(use_double=pool == "f64", fma_mode=fma) as ctx:
        ctx.set_mid_combine(True)
        for name in ["m_top"] + pools.entering[pool]:
            b = pools.batch[pool][name]
            want = pools.want(pool, name, fma)
            out, counts = counted(ctx, b)
            assert counts == LONE, (name, counts)
            assert np.array_equal(bits(out), bits(want[0])), name
            st = ctx.stats()
            assert st["n_pairs"] == b.n_pairs and st["n_fallback"] == int(want[3].sum()), (name, st)
        pools.check_raw(pool, name, fma, ctx.raw(b.n_pairs))


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_what_never_enters(pools, pool, fma):
    from gkl_amd import native
    dbl = pool == "f64"
    mid = pools.batch[pool]["m2049"]
    want_mid = pools.want(pool, "m2049", fma)[0]
    with native.PairHmmContext(use_double=dbl, fma_mode=fma) as ctx:
        ctx.set_mid_combine(True)
        for name in ("m_over", "m_big_in"):
            out, counts = counted(ctx, pools.batch[pool][name])
            assert counts == OFF, (name, counts)
            assert np.array_equal(bits(out), bits(pools.want(pool, name, fma)[0])), name
        # a small region counts as it always did, and a mid-size one behind it enters
        out, counts = counted(ctx, pools.batch[pool][SMALL])
        assert counts == LONE
        assert np.array_equal(bits(out), bits(pools.want(pool, SMALL, fma)[0]))
        out, counts = counted(ctx, mid)
        assert counts == LONE and np.array_equal(bits(out), bits(want_mid))
    # (two devices: `m_top`, whose half on each device is still a mid-size call)
    for kw, name in ((dict(record_events=True), "m2049"), (dict(devices=[0, 0]), "m_top")):
        with native.PairHmmContext(use_double=dbl, fma_mode=fma, **kw) as ctx:
            ctx.set_mid_combine(True)
            out, counts = counted(ctx, pools.batch[pool][name])
            assert counts == OFF, (kw, counts)
            assert np.array_equal(bits(out), bits(pools.want(pool, name, fma)[0])), kw


@pytest.mark.parametrize("fma", [1, 0])
def test_a_device_finalising_context_never_enters(pools, fma):
    """(See the module's docstring: raw sums and flags bit for bit, the output byte for byte that of the switched-off
    context and within the bound of tests/test_gpu_parity.py of the oracle.)"""
    from gkl_amd import native
    b = pools.batch["f32"]["m2049"]
    want = pools.want("f32", "m2049", fma)
    with native.PairHmmContext(fma_mode=fma, finalize=native.FINALIZE_DEVICE_REF32) as ctx:
        off, counts = counted(ctx, b)
        assert counts == OFF
        ctx.set_mid_combine(True)
        on, counts = counted(ctx, b)
        assert counts == OFF
        pools.check_raw("f32", "m2049", fma, ctx.raw(b.n_pairs))
        assert on.tobytes() == off.tobytes()
        finite = np.isfinite(want[0])    # (a read of likelihood 0 gives -inf on both sides)
        assert np.array_equal(bits(on[~finite]), bits(want[0][~finite]))
        worst = float(np.max(np.abs(on[finite] - want[0][finite])))
        print("device finalisation: max |out - oracle| =", worst, "equal bytes:", float(np.mean(bits(on) == bits(want[0]))))
        assert worst <= 3.9e-6


def test_a_lone_region_of_a_multi_call_enters_like_a_single_call(pools):
    """One mid-size region alone in a multi call, and one beside small company, run through the single-call path."""
    from gkl_amd import native
    with native.PairHmmContext() as ctx:
        ctx.set_mid_combine(True)
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([pools.batch["f32"]["m2049"]])
        assert native.small_call_counts(0) == LONE
        assert np.array_equal(bits(got[0]), bits(pools.want("f32", "m2049", 1)[0]))
        native.small_call_counts(0, reset=True)
        got = ctx.compute_multi([pools.batch["f32"][n] for n in ("m2049", "m2304")])   # the multi call's own set: unchanged
        assert native.small_call_counts(0) == (2, 2, 1)
        for n, out in zip(("m2049", "m2304"), got):
            assert np.array_equal(bits(out), bits(pools.want("f32", n, 1)[0])), n


# ---- callers that meet: a child process with the switch and the trigger in its environment ----
def run_child(tmp_path, *args, **env_add):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.update({k: str(v) for k, v in env_add.items()})
    out = tmp_path / "child"
    p = subprocess.run([sys.executable, "-m", "tests.pairhmm_mid_combine_child", *map(str, args), "--out", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(str(out) + ".json") as f:
        rec = json.load(f)
    return rec, np.load(str(out) + ".npz")


def meet(pools, tmp_path, plan, rounds=20):
    """Runs the plan's threads and checks every thread's every region against the oracle of the thread's own mode."""
    rec, got = run_child(tmp_path, "threads", "--plan", json.dumps(plan), "--rounds", rounds, **MEET)
    print("counts", rec["counts"], "calls", rec["calls"])
    assert not rec["errors"] and not rec["changed"], rec
    for i, t in enumerate(plan):
        for k, n in enumerate(t["names"]):
            want = pools.want(t["pool"], n, t["fma"], use_double=bool(t["double"]))[0]
            assert np.array_equal(bits(got[f"t{i}_{k}"]), bits(want)), (i, n)
    calls, combined, sets = rec["counts"]
    assert rec["calls"] == sum(rounds * len(t["names"]) for t in plan)
    assert calls == rec["calls"], rec
    assert combined > 0 and sets < calls, rec
    return rec


@pytest.mark.parametrize("fma", [1, 0])
@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_four_callers_meet(pools, tmp_path, pool, fma):
    """Each thread walks the entering regions in another rotation: the members of a set and their block offsets differ
    from set to set.  The trigger (at least four waiting, or none in the air) guarantees that a call arriving while a set
    is in flight waits for company; nothing about timing is asserted."""
    names = pools.entering[pool]
    plan = [dict(pool=pool, double=int(pool == "f64"), fma=fma, names=names, rot=2 * i + 1) for i in range(4)]
    rec = meet(pools, tmp_path, plan)
    assert rec["calls"] == 4 * 20 * len(names)


@pytest.mark.parametrize("fma", [1, 0])
def test_the_two_precisions_never_share(pools, tmp_path, fma):
    names = ["m2049", "m2304", "m_nofb", "m_r4", "m_odd"]    # (not `m_allfb`: all of its pairs are fp64 in both modes)
    for n in names:
        assert pools.want("f32", n, fma, use_double=False)[0].tobytes() != pools.want("f32", n, fma, use_double=True)[0].tobytes(), n
    plan = [dict(pool="f32", double=i % 2, fma=fma, names=names, rot=i) for i in range(4)]
    meet(pools, tmp_path, plan)


@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_small_callers_beside_mid_size_ones(pools, tmp_path, pool):
    dbl = int(pool == "f64")
    mid = ["m2049", "m2304", pools.entering[pool][2]]
    plan = [dict(pool=pool, double=dbl, fma=1, names=[SMALL, SMALL, SMALL], rot=0) for _ in range(2)] + \
           [dict(pool=pool, double=dbl, fma=1, names=mid, rot=i) for i in range(2)]
    meet(pools, tmp_path, plan)


@pytest.mark.parametrize("pool", ["f32", "f64"])
def test_the_pair_cap(pools, tmp_path, pool):
    """`m_top` beside `m2049`: the largest region and the smallest in sets of unequal members -- this test checks BYTES (in
    `meet`), not the cap.  No set holds more than kCombineMidPairs = 131 072 pairs, so the sets cannot be fewer than the pairs
    computed / 131 072; but which callers meet is a matter of timing, a round's first caller always leads alone, and real
    runs count far more sets than that bound with or without the cap.  The cap itself is checked where it is deterministic:
    `combine_pick`, the function `SmallCombiner::run` calls, in tests/native/pairhmm_mid_combine_check.cpp."""
    names = ["m_top", "m2049"]
    plan = [dict(pool=pool, double=int(pool == "f64"), fma=1, names=names, rot=i % 2) for i in range(4)]
    rec = meet(pools, tmp_path, plan)
    total = 4 * 20 * (65536 + 2049)
    assert rec["counts"][2] * 131072 >= total, rec


# ---- through the server: its sessions call gklhip_compute on their own contexts ----
@pytest.mark.parametrize("switch", [True, False])
def test_clients_of_the_server(oracle, tmp_path, switch):
    from gkl_amd import server
    from tests.test_server_gpu import child_env, no_gpu_files, run_clients
    e = child_env(**MEET)
    if not switch:
        del e["GKL_HIP_COMBINE_MID"]
    sock = tmp_path / "mid.sock"
    h = server.start(str(sock), env=e, timeout=120)
    try:
        specs = [(f"hc:70:30:{41 + i}", 0, 1) for i in range(4)]
        res = run_clients(sock, tmp_path, specs, repeat=20)
        for (sp, _, _), (rec, outs) in zip(specs, res):
            assert rec["remote"] and no_gpu_files(rec) and "unstable" not in rec, rec
            b = make_batch("hc", 70, 30, seed=int(sp.split(":")[3]))
            assert b.n_pairs == 2100
            assert np.array_equal(bits(outs["out0"]), bits(oracle.batch(b, n_threads=4))), sp
        st = h.stats()
        calls, combined, sets = st["small_call_counts"][0]
        print("switch", switch, "small_call_counts", (calls, combined, sets))
        assert st["calls_served"] == 4 * 21
        if switch:
            assert calls == 4 * 21 and combined > 0 and sets < calls, st
        else:
            assert (calls, combined, sets) == OFF, st
    finally:
        assert h.stop() == 0


# ---- through the JNI symbols ----
@pytest.mark.parametrize("use_double", [False, True])
def test_jni_callers(oracle, tmp_path, use_double):
    b = make_batch("hc", 8 * 70, 30, seed=7)
    assert b.n_reads // 8 * b.n_haps == 2100
    rec, got = run_child(tmp_path, "jni", "--spec", "hc:560:30:7", "--threads", 8, "--iters", 10, "--double", int(use_double),
                         GKL_HIP_COMBINE_MID=1)
    print("jni", rec)
    assert rec["rc"] == 0, rec
    assert np.array_equal(bits(got["out0"]), bits(oracle.batch(b, use_double=use_double, n_threads=4)))
    assert rec["counts"][0] > 0, rec    # the slices are mid-size calls, and they entered

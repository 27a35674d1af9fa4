"""The planned fp64 pass at the planner's edge shapes (tests/planned_shapes.py; their properties are proved on the
oracle's flags in tests/test_pairhmm_planned_pass_cpu.py), and the device finalisation against a long-double reference.

Every call is checked three ways (check_planned):
* the routing rule that sends it to the planned pass;
* a host call: `out`, the raw fp32 sums, the raw fp64 sums of the flagged pairs and the flags, bit for bit against the
  oracle (tests.test_gpu_parity.check_against_oracle), and the fallback count of the statistics;
* device-resident calls in both device finalisation modes: raw sums and flags again bit for bit, and the output under
  the finalisation rule of planned_shapes.Finalised -- within 2 ulp of log10 taken in long double where the device takes
  a double log10 (one ulp is the vendor's documented bound for it, one the subtraction's rounding), exactly
  double(float(L) - log10f(2^120)) for the kept pairs of the float-formula mode.

Measured on an MI355X (docs/NOTES.md 79): the largest distance is 1.0 ulp in every case and both modes, no pair is exempt,
and the file takes 11 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd.synth import make_batch
from tests import planned_shapes as ps
from tests.test_gpu_parity import bits, check_against_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from gkl_amd import native as n
    return n


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    """Neither small-read limit nor the mid-size combiner: contexts as a caller without settings gets them."""
    monkeypatch.delenv("GKL_HIP_SMALL_READ_LIMIT", raising=False)
    monkeypatch.delenv("GKL_HIP_COMBINE_MID", raising=False)


class CachedOracle:
    """What check_against_oracle asks of an oracle, answered from the reference computed once per process."""

    def __init__(self, oracle, name):
        self.oracle, self.name = oracle, name

    def batch(self, b, use_double=False, fma_mode=1, want_raw=False, n_threads=1):
        assert b is ps.batch(self.name) and not use_double and want_raw
        return ps.reference(self.oracle, self.name, fma_mode)


_FINALISED = {}


def finalised(oracle, name, fma):
    if (name, fma) not in _FINALISED:
        _, o32, o64, ou = ps.reference(oracle, name, fma)
        _FINALISED[name, fma] = ps.Finalised(oracle, o32, o64, ou)
    return _FINALISED[name, fma]


def check_raw(ctx, ref, what):
    _, o32, o64, ou = ref
    r32, r64, u = ctx.raw(ou.size)
    assert np.array_equal(u, ou), f"{what}: fallback flags differ"
    assert np.array_equal(bits(r32), bits(o32)), f"{what}: raw fp32 sums are not bit-identical"
    assert np.array_equal(bits(r64[ou == 1]), bits(o64[ou == 1])), f"{what}: raw fp64 sums are not bit-identical"


def check_device(native, oracle, ctx, mode, name, fma, db=None):
    """One device-resident call of batch `name` on `ctx` (finalisation `mode`): raw sums, flags, finalisation rule."""
    import torch
    b = ps.batch(name) if isinstance(name, str) else name
    db = db or native.DeviceBatch.upload(b)
    dev = ctx.compute_device(db)
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    if isinstance(name, str):
        ref, fin = ps.reference(oracle, name, fma), finalised(oracle, name, fma)
    else:
        ref = oracle.batch(b, fma_mode=fma, want_raw=True, n_threads=8)
        fin = ps.Finalised(oracle, *ref[1:])
    check_raw(ctx, ref, f"device call, mode {mode}")
    print(f"[{name if isinstance(name, str) else 'per-pair'} fma {fma}] ", end="")
    return fin.check(out, mode)


def check_planned(native, oracle, name, fma, host, dev):
    """host: a host context; dev: {finalisation mode: device context}."""
    b = ps.batch(name)
    assert b.n_pairs > ps.DIRECT_PAIRS or int(b.read_lens.max()) >= ps.FORCING_READ_LEN, "the call would not take the planned pass"
    assert b.n_pairs < ps.HOST_SHARD_PAIRS, "the host call would run as two passes"
    assert ps.takes_planned_pass(b)
    ou = ps.reference(oracle, name, fma)[3]
    check_against_oracle(host, CachedOracle(oracle, name), b, fma_mode=fma)
    assert host.stats()["n_fallback"] == int(ou.sum())
    db = native.DeviceBatch.upload(b)
    for mode, ctx in dev.items():
        check_device(native, oracle, ctx, mode, name, fma, db)


class Contexts:
    def __init__(self, native, fma, modes=None):
        self.native, self.fma = native, fma
        self.modes = modes or (native.FINALIZE_DEVICE_F64, native.FINALIZE_DEVICE_REF32)

    def __enter__(self):
        n = self.native
        self.host = n.PairHmmContext(use_double=False, fma_mode=self.fma)
        self.dev = {m: n.PairHmmContext(use_double=False, fma_mode=self.fma, finalize=m) for m in self.modes}
        return self

    def __exit__(self, *a):
        self.host.close()
        for c in self.dev.values():
            c.close()


# the cases of a group share their contexts (the four read families of a case C)
GROUPS = {}
for _name in ps.CASES:
    GROUPS.setdefault(_name.split("/")[0] if _name.startswith("C:") else _name, []).append(_name)
GROUP_RUNS = [(g, fma) for g, names in GROUPS.items() for fma in ps.CASES[names[0]]]


@pytest.mark.parametrize("group,fma", GROUP_RUNS, ids=[f"{g}-fma{f}" for g, f in GROUP_RUNS])
def test_planned_pass_at_the_planners_edge_shapes(native, oracle, group, fma):
    with Contexts(native, fma) as c:
        for name in GROUPS[group]:
            check_planned(native, oracle, name, fma, c.host, c.dev)


def test_one_context_many_shapes(native, oracle):
    """G: calls of different shapes one after another on ONE host context and ONE device context -- the arrival
    counters, the per-read fail counts, the chunk counter and the global histogram are the context's and must start
    every call clean, whatever the call before left (a histogram in global memory, no failure at all, 120 000 reads)."""
    with Contexts(native, 1, modes=(native.FINALIZE_DEVICE_F64,)) as c:
        for name in ps.SEQUENCE_G:
            check_planned(native, oracle, name, 1, c.host, c.dev)


@pytest.mark.parametrize("shape,seed", [((100, 10), 5), ((300, 24), 11)], ids=["fused", "mid-size"])
def test_per_pair_paths_follow_the_finalisation_rule(native, oracle, shape, seed):
    """The fused call and the mid-size call write their device finalisation from the per-pair kernels: the same rule."""
    b = make_batch("hc", *shape, seed=seed)
    assert not ps.takes_planned_pass(b)
    db = native.DeviceBatch.upload(b)
    with Contexts(native, 1) as c:
        for mode, ctx in c.dev.items():
            check_device(native, oracle, ctx, mode, b, 1, db)


def test_smallest_grids(oracle):
    """H: GKLHIP_PLAN_BLOCKS=1 (read once per process: a child) -- one block runs the policy and the run detection, so the
    block that sorts the affected reads and the one that orders the jobs are the only ones."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), GKLHIP_PLAN_BLOCKS="1")
    env.pop("GKL_HIP_SMALL_READ_LIMIT", None)
    env.pop("GKL_HIP_COMBINE_MID", None)
    p = subprocess.run([sys.executable, "-m", "tests.pairhmm_plan_blocks_child", "--names", ",".join(ps.SMALLEST_GRIDS_H)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["plan_blocks"] == "1"
    for name in ps.SMALLEST_GRIDS_H:
        want = ps.digests(*ps.reference(oracle, name, 1))
        assert got[name]["host"] == want, name
        assert {k: v for k, v in got[name]["device"].items() if k != "out"} == {k: v for k, v in want.items() if k != "out"}, name

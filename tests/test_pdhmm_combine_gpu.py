"""Concurrent PDHMM cross calls share launches (GKL_HIP_PDHMM_COMBINE=1, off by default) on the MI355X: the threads of one
process and the session threads of the server.  Whatever is combined with whatever, every caller gets the bytes of the
direct single call; the counts (gklhip_pdhmm_combine_counts) are asserted only where the leader's hold guarantees them.
Every child process runs under a time limit."""
import subprocess
import sys

import numpy as np
import pytest

from gkl_amd import native, server
from tests.pd_server_client import region
from tests.test_pdhmm_server_cpu import pd_client
from tests.test_server_gpu import ROOT, child_env, no_gpu_files, read_json, wait_until

SHAPES = [(61, 41), (20, 7), (33, 12), (90, 5)]     # four differently shaped region calls
# the leader holds until four calls have met or ten seconds have passed: four callers released together always meet
COMBINE_ENV = dict(GKL_HIP_PDHMM_COMBINE=1, GKL_HIP_PDHMM_COMBINE_MIN=4, GKL_HIP_PDHMM_COMBINE_WAIT_US=10_000_000)


def plain_env():
    e = child_env()
    for k in list(e):
        if k.startswith("GKL_HIP_PDHMM_COMBINE"):
            del e[k]
    return e


@pytest.fixture(scope="module")
def direct():
    """The direct single-call bytes and routing of the four regions, per seed (a context of this process, combiner off)."""
    made = {}
    ctx = native.PdhmmContext(device=0)

    def get(seed):
        if seed not in made:
            made[seed] = []
            for i, shape in enumerate(SHAPES):
                out = ctx.compute_cross(*region(seed + i, *shape))
                made[seed].append((out.tobytes(), list(ctx.last_routing())))
        return made[seed]

    yield get
    ctx.close()


def run_threads(tmp_path, name, env, seed):
    out = tmp_path / name
    p = subprocess.Popen([sys.executable, "-m", "tests.pd_combine_child", "--out", str(out), "--seed", str(seed),
                          "--shapes", ",".join(f"{r}:{h}" for r, h in SHAPES)], cwd=ROOT, env=env)
    try:
        assert p.wait(300) == 0
    finally:
        if p.poll() is None:
            p.kill()
    rec = read_json(out)
    assert rec["errors"] == [None] * len(SHAPES), rec
    return rec, np.load(str(out) + ".npz")


@pytest.mark.gpu
def test_four_threads_leave_in_one_launch_set(tmp_path, direct):
    rec, got = run_threads(tmp_path, "combined", child_env(**COMBINE_ENV), seed=300)
    for i, (want, routing) in enumerate(direct(300)):
        assert got[f"out{i}"].tobytes() == want, i
        assert rec["routing"][i] == routing, i        # every caller gets its OWN routing back
    assert rec["counts"] == [4, 4, 1]


@pytest.mark.gpu
def test_default_is_the_uncombined_path(tmp_path, direct):
    rec, got = run_threads(tmp_path, "plain", plain_env(), seed=300)
    for i, (want, routing) in enumerate(direct(300)):
        assert got[f"out{i}"].tobytes() == want, i
        assert rec["routing"][i] == routing, i
    assert rec["counts"] == [4, 0, 4]


@pytest.mark.gpu
def test_server_sessions_share_launches(tmp_path, direct):
    h = server.start(str(tmp_path / "s.sock"), timeout=120, env=child_env(**COMBINE_ENV))
    try:
        go = tmp_path / "go"
        calls = 3
        procs = [pd_client("region", h.socket_path, tmp_path / f"c{i}", "--calls", calls, "--seed", 300 + i, "--shape", f"{r}:{hp}",
                           "--go", go) for i, (r, hp) in enumerate(SHAPES)]
        try:
            wait_until(lambda: h.pdhmm_stats()["live_connections"] >= 4 or any(p.poll() is not None for p in procs), 300)
            go.touch()
            for p in procs:
                assert p.wait(300) == 0
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        for i, (want, _) in enumerate(direct(300)):
            rec = read_json(tmp_path / f"c{i}")
            assert rec["remote"] and "unstable" not in rec and no_gpu_files(rec), rec
            assert np.load(str(tmp_path / f"c{i}") + ".npz")["out"].tobytes() == want, i
        st = h.pdhmm_stats()
        assert st["calls_failed"] == 0 and st["calls_served"] == 4 * (calls + 1)
        n_calls, n_shared, n_sets = st["combine_counts"]
        # every client makes the same number of calls and every call waits for three others (or ten seconds): the four
        # sessions move in step, so calls did share launch sets; how many exactly is up to the clients' timing
        assert n_calls == 4 * (calls + 1) and n_shared >= 2 and n_sets < n_calls, st
        print("PDHMM server combine counts:", st["combine_counts"])
    finally:
        assert h.stop() == 0

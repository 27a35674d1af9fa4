"""The PairHMM server on the MI355X: client processes (which never open the device) get the oracle's bits for their
own batches in every arithmetic mode, their small calls meet in the server's combiner, the JNI library computes
through the server, a client killed in the middle of a call costs nothing but its own connection, and --devices
spreads connections.  One server per module (started under a time limit, stopped in teardown); at most 8 clients."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from gkl_amd import server
from gkl_amd.synth import make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(0, 1), (1, 1), (0, 0), (1, 0)]   # (use_double, fma_mode)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    h = server.start(str(tmp_path_factory.mktemp("gsrv") / "s.sock"), timeout=120)
    yield h
    assert h.stop() == 0


def child_env(**extra):
    e = dict(os.environ)
    e.pop("GKL_HIP_SERVER", None)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    e.update({k: str(v) for k, v in extra.items()})
    return e


def client(mode, sock, out, *args, env=None):
    return subprocess.Popen([sys.executable, "-m", "tests.server_client", mode, "--socket", str(sock), "--out", str(out),
                             *map(str, args)], cwd=ROOT, env=env or child_env())


def read_json(prefix):
    with open(str(prefix) + ".json") as f:
        return json.load(f)


def wait_until(cond, timeout=60.0):
    t_end = time.monotonic() + timeout
    while not cond():
        assert time.monotonic() < t_end, "timed out"
        time.sleep(0.01)


def no_gpu_files(rec):
    return not [f for f in rec["open_files"] if f == "/dev/kfd" or f.startswith("/dev/dri/")]


def run_clients(sock, tmp_path, specs, repeat=1):
    """specs: (spec string, use_double, fma) per client; all start their timed calls together."""
    go = tmp_path / "go"
    procs = [client("batches", sock, tmp_path / f"c{i}", "--spec", sp, "--double", d, "--fma", f, "--repeat", repeat, "--go", go)
             for i, (sp, d, f) in enumerate(specs)]
    try:
        wait_until(lambda: server_live(sock) >= len(specs) or any(p.poll() is not None for p in procs), 300)
        go.touch()
        for p in procs:
            assert p.wait(600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [(read_json(tmp_path / f"c{i}"), np.load(str(tmp_path / f"c{i}") + ".npz")) for i in range(len(specs))]


def server_live(sock):
    from gkl_amd import native
    return native.server_stats(str(sock))["live_connections"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_clients", [4, 8])
def test_clients_are_bit_exact_in_every_mode_and_never_open_the_gpu(gpu_server, oracle, tmp_path, n_clients):
    specs = []
    for i in range(n_clients):
        d, f = MODES[i % 4]
        specs.append((f"hc:100:10:{11 + i},region:80:12:{31 + i}", d, f))
    res = run_clients(gpu_server.socket_path, tmp_path, specs, repeat=2)
    for (sp, d, f), (rec, outs) in zip(specs, res):
        assert rec["remote"] and "unstable" not in rec, rec
        assert no_gpu_files(rec), [x for x in rec["open_files"] if x.startswith("/dev")]
        for i, item in enumerate(sp.split(",")):
            kind, r, h, seed = item.split(":")
            want = oracle.batch(make_batch(kind, int(r), int(h), seed=int(seed)), use_double=bool(d), fma_mode=f, n_threads=4)
            assert np.array_equal(bits(outs[f"out{i}"]), bits(want)), (item, d, f)
    st = gpu_server.stats()
    assert st["arenas_registered"] + st["arenas_copied"] >= n_clients
    print("server stats:", st)


@pytest.mark.gpu
def test_concurrent_clients_meet_in_the_servers_combiner(oracle, tmp_path):
    """GKL_HIP_COMBINE_MIN=4 with a long wait in the server's environment: four clients calling at once.  What the
    trigger guarantees is that a call arriving while a set is in flight waits for the others -- so calls get combined;
    no timing is asserted."""
    sock = tmp_path / "comb.sock"
    h = server.start(str(sock), env=child_env(GKL_HIP_COMBINE_MIN=4, GKL_HIP_COMBINE_WAIT_US=2000000), timeout=120)
    try:
        specs = [("hc:100:10:3", 0, 1)] * 4
        res = run_clients(sock, tmp_path, specs, repeat=30)
        want = oracle.batch(make_batch("hc", 100, 10, seed=3), n_threads=4)
        for rec, outs in res:
            assert no_gpu_files(rec) and "unstable" not in rec
            assert np.array_equal(bits(outs["out0"]), bits(want))
        st = h.stats()
        calls, combined, sets = st["small_call_counts"][0]
        assert st["calls_served"] == 4 * 31
        assert 0 < calls <= 4 * 31 and combined > 0 and sets < calls, st
    finally:
        assert h.stop() == 0


@pytest.mark.gpu
def test_jni_library_in_client_mode_is_bit_exact(gpu_server, oracle, tmp_path):
    env = child_env(GKL_HIP_SERVER=gpu_server.socket_path)
    p = client("jni", gpu_server.socket_path, tmp_path / "jni", "--spec", "hc:300:24:21", env=env)
    assert p.wait(300) == 0
    rec = read_json(tmp_path / "jni")
    assert rec["rc"] == 0, rec
    assert no_gpu_files(rec)
    want = oracle.batch(make_batch("hc", 300, 24, seed=21), n_threads=4)
    assert np.array_equal(bits(np.load(str(tmp_path / "jni") + ".npz")["out0"]), bits(want))


@pytest.mark.gpu
def test_a_client_killed_mid_call_leaves_the_server_bit_exact(gpu_server, oracle, tmp_path):
    before = gpu_server.stats()["live_connections"]
    victim = client("loop", gpu_server.socket_path, tmp_path / "victim", "--spec", "hc:2000:64:5")
    try:
        wait_until(lambda: os.path.exists(str(tmp_path / "victim") + ".json"), 300)
        wait_until(lambda: gpu_server.stats()["calls_active"] >= 1, 60)
    finally:
        victim.kill()
        victim.wait()
    assert no_gpu_files(read_json(tmp_path / "victim"))
    res = run_clients(gpu_server.socket_path, tmp_path, [("hc:100:10:9,region:80:12:9", 0, 1), ("hc:2000:64:5", 1, 1)])
    for (rec, outs), (item, d) in zip(res, [("hc:100:10:9", 0), ("hc:2000:64:5", 1)]):
        kind, r, hh, seed = item.split(":")
        want = oracle.batch(make_batch(kind, int(r), int(hh), seed=int(seed)), use_double=bool(d), n_threads=8)
        assert np.array_equal(bits(outs["out0"]), bits(want))
    wait_until(lambda: gpu_server.stats()["live_connections"] == before, 60)


@pytest.mark.gpu
def test_devices_list_spreads_connections_and_the_copy_path_is_bit_exact(oracle, tmp_path):
    """--devices 0,0: two connections land on the two entries.  GKL_HIP_SERVER_REGISTER=0: the arenas are copied into
    the server's pinned staging instead of page-locked in place -- same bits."""
    from gkl_amd import native
    sock = tmp_path / "dev.sock"
    h = server.start(str(sock), devices=[0, 0], env=child_env(GKL_HIP_SERVER_REGISTER=0), timeout=120)
    try:
        b = make_batch("region", 120, 16, seed=5)
        want = oracle.batch(b, n_threads=4)
        with native.PairHmmContext(server=str(sock)) as c1, native.PairHmmContext(server=str(sock)) as c2:
            st = h.stats()
            assert st["devices"] == [0, 0] and st["connections_per_device"] == [1, 1], st
            for c in (c1, c2):
                assert np.array_equal(bits(c.compute(b)), bits(want))
        st = h.stats()
        assert st["arenas_copied"] >= 2 and st["arenas_registered"] == 0, st
    finally:
        assert h.stop() == 0

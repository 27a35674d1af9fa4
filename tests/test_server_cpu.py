"""The PairHMM server (gkl_amd/csrc/pairhmm_server.cpp) and its client (pairhmm_remote.cpp) without a GPU: the server
is linked against the stub C ABI (tests/native/stub_gklhip.cpp: a checksum per pair instead of PairHMM), the clients
are the real product libraries, whose client path makes no HIP call.  Concurrency, arena growth, malformed and
refused requests, clients and servers that die in the middle of a call."""
import ctypes as C
import os
import re
import signal
import socket
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from gkl_amd import native, server
from gkl_amd.errors import RuntimeException
from gkl_amd.synth import random_batch
from tests import mockjni

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "gkl_amd", "csrc")


def build_stub_server(dest):
    """gklhip_server from the product's pairhmm_server.cpp, linked against the stub C ABI (as mockjni.build_stub links
    the JNI layer)."""
    srcs = [os.path.join(CSRC, "pairhmm_server.cpp"), os.path.join(NATIVE, "stub_gklhip.cpp"),
            os.path.join(NATIVE, "stub_server_extras.cpp")]
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-Wno-unused-parameter", *srcs, "-o", dest,
                    "-lpthread"], check=True)
    return dest


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    return build_stub_server(str(tmp_path_factory.mktemp("stubsrv") / "gklhip_server_stub"))


@pytest.fixture(scope="module")
def sockdir(tmp_path_factory):
    return tmp_path_factory.mktemp("sock")


def start_stub(exe, path, **env):
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    return server.start(str(path), env=e, timeout=30, server_path=exe)


@pytest.fixture(scope="module")
def srv(stub_exe, sockdir):
    h = start_stub(stub_exe, sockdir / "main.sock")
    yield h
    assert h.stop() == 0


def child_env():
    e = dict(os.environ)
    e.pop("GKL_HIP_SERVER", None)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    return e


def client(mode, sock, out, *args, env=None):
    return subprocess.Popen([sys.executable, "-m", "tests.server_client", mode, "--socket", str(sock), "--out", str(out),
                             *map(str, args)], cwd=ROOT, env=env or child_env())


def read_json(prefix):
    import json
    with open(str(prefix) + ".json") as f:
        return json.load(f)


def wait_until(cond, timeout=30.0):
    t_end = time.monotonic() + timeout
    while not cond():
        assert time.monotonic() < t_end, "timed out"
        time.sleep(0.01)


# ---- the wire protocol by hand (gkl_amd/csrc/pairhmm_remote.h) ----
MAGIC, HELLO, ARENA, COMPUTE, STATS = 0x534C4B47, 1, 2, 3, 4


def request(type_, body=b""):
    return struct.pack("<II", MAGIC, type_) + body.ljust(112, b"\0")


def hello_body(protocol=1, abi=native.ABI_VERSION, control=0):
    return struct.pack("<iiii", abi, protocol, control, 0) + bytes(native.Config(native.ABI_VERSION, -1, 0, 1, 1, -1, 0, 0))


def read_reply(s):
    head = b""
    while len(head) < 16:
        k = s.recv(16 - len(head))
        if not k:
            return None
        head += k
    status, tlen, plen, _ = struct.unpack("<iIII", head)
    rest = b""
    while len(rest) < tlen + plen:
        k = s.recv(tlen + plen - len(rest))
        if not k:
            break
        rest += k
    return status, rest[:tlen].decode(), rest[tlen:]


def raw_connect(path, protocol=1, abi=native.ABI_VERSION):
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(20)
    s.connect(str(path))
    s.sendall(request(HELLO, hello_body(protocol, abi)))
    return s, read_reply(s)


def closed(s):
    try:
        return s.recv(1) == b""
    except ConnectionResetError:
        return True


def test_the_client_path_loads_no_device_and_the_socket_is_private(srv):
    st = os.stat(srv.socket_path)
    assert (st.st_mode & 0o777) == 0o600
    info = srv.stats()
    assert info["protocol"] == 1 and info["pid"] == srv.pid
    with native.PairHmmContext(server=srv.socket_path) as c:
        assert c.is_remote and c.n_devices == 1
        b = random_batch(np.random.RandomState(3), 20, 4)
        assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
        for call in (lambda: c.raw(b.n_pairs), lambda: c.step_times(0), lambda: c.issue_ceiling()):
            with pytest.raises(RuntimeException, match="unsupported"):
                call()
        assert c.release_idle() == 0


def test_eight_client_processes_of_random_shapes(srv, tmp_path):
    go = tmp_path / "go"
    procs = [client("random", srv.socket_path, tmp_path / f"c{i}", "--calls", 50, "--seed", 100 + i, "--go", go)
             for i in range(8)]
    wait_until(lambda: srv.stats()["live_connections"] >= 8 or any(p.poll() is not None for p in procs), 120)
    go.touch()
    for p in procs:
        assert p.wait(300) == 0
    for i in range(8):
        r = read_json(tmp_path / f"c{i}")
        assert r["remote"] and (r["good"], r["bad"]) == (50, 0), r
    wait_until(lambda: srv.stats()["live_connections"] == 0)


def test_arena_grows_across_calls(srv):
    before = srv.stats()
    rng = np.random.RandomState(9)
    with native.PairHmmContext(server=srv.socket_path) as c:
        for n_reads, n_haps, rl in ((2, 2, 20), (50, 10, 200), (400, 30, 900), (1500, 60, 1500), (30, 3, 50)):
            b = random_batch(rng, n_reads, n_haps, read_len=(rl // 2, rl), hap_len=(rl // 2, rl))
            assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
    after = srv.stats()
    grown = after["arenas_registered"] + after["arenas_copied"] - before["arenas_registered"] - before["arenas_copied"]
    assert grown >= 2   # the first arena and at least one bigger one


def test_copy_path_gives_the_same_results(stub_exe, sockdir):
    h = start_stub(stub_exe, sockdir / "copy.sock", STUB_REGISTER=0)
    try:
        rng = np.random.RandomState(5)
        with native.PairHmmContext(server=h.socket_path) as c:
            for _ in range(5):
                b = random_batch(rng, int(rng.randint(1, 200)), int(rng.randint(1, 20)), read_len=(1, 400))
                assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
        st = h.stats()
        assert st["arenas_copied"] >= 1 and st["arenas_registered"] == 0
    finally:
        assert h.stop() == 0


def test_malformed_requests_are_refused_and_others_keep_working(srv, tmp_path):
    other = client("random", srv.socket_path, tmp_path / "other", "--calls", 200, "--seed", 7)
    refused0 = srv.stats()["requests_refused"]
    rng = np.random.RandomState(1)

    def with_arena(size=1 << 16, seal=True):
        s, (st, _, _) = raw_connect(srv.socket_path)
        assert st == 0
        fd = os.memfd_create("t", os.MFD_ALLOW_SEALING)
        os.ftruncate(fd, size)
        if seal:
            import fcntl
            fcntl.fcntl(fd, fcntl.F_ADD_SEALS, fcntl.F_SEAL_SHRINK | fcntl.F_SEAL_GROW)
        socket.send_fds(s, [request(ARENA, struct.pack("<Q", size))], [fd])
        os.close(fd)
        return s, read_reply(s)

    def compute_req(n_reads, n_haps, offs):
        return request(COMPUTE, struct.pack("<ii9Q", n_reads, n_haps, *offs))

    cases = []
    # a call before any arena
    s, _ = raw_connect(srv.socket_path)
    s.sendall(compute_req(1, 1, [0] * 9))
    cases.append(s)
    # an arena that is not sealed against shrinking
    s, r = with_arena(seal=False)
    assert r[0] == native.ERR_INVALID_ARG and "seal" in r[1]
    assert closed(s)
    # offsets outside the arena, negative counts, read_off not monotone, an unknown message, a bad magic
    bad = [compute_req(1, 1, [1 << 20] + [0] * 8), compute_req(-1, 3, [0] * 9), compute_req(1, 1, [0, 64, 128, 128, 128, 128, 128, 128, 1 << 17])]
    for req in bad:
        s, r = with_arena()
        assert r[0] == 0
        s.sendall(req)
        cases.append(s)
    s, _ = raw_connect(srv.socket_path)
    s.sendall(request(99))
    cases.append(s)
    s, _ = raw_connect(srv.socket_path)
    s.sendall(struct.pack("<II", 0x12345678, COMPUTE) + bytes(112))
    cases.append(s)
    for s in cases:
        r = read_reply(s)
        assert r is not None and r[0] == native.ERR_INVALID_ARG, r
        assert closed(s)
        s.close()
    assert srv.stats()["requests_refused"] - refused0 >= len(cases) + 1
    # the well-behaved client, and a new one, are unaffected
    with native.PairHmmContext(server=srv.socket_path) as c:
        b = random_batch(rng, 30, 5)
        assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
    assert other.wait(300) == 0
    r = read_json(tmp_path / "other")
    assert (r["good"], r["bad"]) == (200, 0)


def test_not_monotone_read_offsets_are_refused(srv):
    import fcntl
    s, (st, _, _) = raw_connect(srv.socket_path)
    assert st == 0
    size = 1 << 16
    fd = os.memfd_create("t", os.MFD_ALLOW_SEALING)
    os.ftruncate(fd, size)
    fcntl.fcntl(fd, fcntl.F_ADD_SEALS, fcntl.F_SEAL_SHRINK | fcntl.F_SEAL_GROW)
    os.pwrite(fd, struct.pack("<3q", 0, 5, 3), 0)       # read_off
    os.pwrite(fd, struct.pack("<2q", 0, 4), 64)         # hap_off
    socket.send_fds(s, [request(ARENA, struct.pack("<Q", size))], [fd])
    os.close(fd)
    assert read_reply(s)[0] == 0
    s.sendall(request(COMPUTE, struct.pack("<ii9Q", 2, 1, 0, 64, 128, 192, 256, 320, 384, 448, 512)))
    st, text, _ = read_reply(s)
    assert st == native.ERR_INVALID_ARG and "monotone" in text
    assert closed(s)


def test_protocol_or_abi_mismatch_is_refused(srv):
    for proto, abi in ((99, native.ABI_VERSION), (1, native.ABI_VERSION + 7)):
        s, r = raw_connect(srv.socket_path, protocol=proto, abi=abi)
        assert r[0] == native.ERR_UNSUPPORTED and "protocol" in r[1], r
        assert closed(s)
    # and the server is fine
    assert srv.stats()["protocol"] == 1


def test_a_client_killed_in_the_middle_of_a_call(stub_exe, sockdir, tmp_path):
    h = start_stub(stub_exe, sockdir / "slow.sock", STUB_DELAY_US=200000)
    try:
        victim = client("loop", h.socket_path, tmp_path / "victim", "--spec", "hc:20:4:1")
        wait_until(lambda: os.path.exists(str(tmp_path / "victim") + ".json"), 120)
        with native.PairHmmContext(server=h.socket_path) as c:
            assert h.stats()["live_connections"] == 2
            wait_until(lambda: h.stats()["calls_active"] >= 1)
            victim.kill()
            victim.wait()
            rng = np.random.RandomState(2)
            for _ in range(3):
                b = random_batch(rng, 10, 3)
                assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
            wait_until(lambda: h.stats()["live_connections"] == 1)
        wait_until(lambda: h.stats()["live_connections"] == 0)
    finally:
        assert h.stop() == 0


def test_server_gone_fails_the_call_in_c_python_and_java(stub_exe, sockdir, tmp_path):
    h = start_stub(stub_exe, sockdir / "gone.sock")
    rng = np.random.RandomState(4)
    b = random_batch(rng, 10, 3)
    c = native.PairHmmContext(server=h.socket_path)
    assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
    assert h.stop() == 0
    assert not os.path.exists(h.socket_path)   # SIGTERM removes the socket
    lib = native.load_library()
    cb = native.CBatch(b.n_reads, b.n_haps, np.ascontiguousarray(b.read_off).ctypes.data_as(native._i64p),
                       np.ascontiguousarray(b.hap_off).ctypes.data_as(native._i64p),
                       *[np.ascontiguousarray(x).ctypes.data for x in (b.read_bases, b.read_quals, b.ins_gop, b.del_gop, b.gcp, b.hap_bases)])
    out = np.zeros(b.n_pairs)
    keep = (b,)
    assert lib.gklhip_compute(c.handle, C.byref(cb), out.ctypes.data) == native.ERR_HIP
    assert h.socket_path in lib.gklhip_last_error().decode()
    del keep
    with pytest.raises(RuntimeException, match="went away"):
        c.compute(b)
    c.close()
    with pytest.raises(RuntimeException, match=re.escape(str(h.socket_path))):
        native.PairHmmContext(server=h.socket_path)
    # the JNI layer in client mode: the server dies during computeLikelihoodsNative, the one retry cannot reconnect
    h2 = start_stub(stub_exe, sockdir / "gone2.sock", STUB_DELAY_US=1000000)
    env = child_env()
    env["GKL_HIP_SERVER"] = h2.socket_path
    p = client("jni", h2.socket_path, tmp_path / "jni", "--spec", "hc:12:3:5", env=env)
    try:
        wait_until(lambda: h2.stats()["calls_active"] >= 1, 120)
    finally:
        h2.proc.kill()
        h2.proc.wait()
    assert p.wait(120) == 0
    r = read_json(tmp_path / "jni")
    assert r["rc"] != 0 and r["exception"] == "java/lang/RuntimeException" and h2.socket_path in r["message"], r


def test_jni_layer_in_client_mode_computes_through_the_server(srv, tmp_path):
    env = child_env()
    env["GKL_HIP_SERVER"] = srv.socket_path
    env["GKL_HIP_JNI_PIPELINE_PAIRS"] = "100"   # a pipelined-size call still goes as ONE request in client mode
    p = client("jni", srv.socket_path, tmp_path / "jni", "--spec", "hc:300:6:8", env=env)
    assert p.wait(120) == 0
    r = read_json(tmp_path / "jni")
    assert r["rc"] == 0, r
    from gkl_amd.synth import make_batch
    got = np.load(str(tmp_path / "jni") + ".npz")["out0"]
    assert np.array_equal(got, mockjni.stub_expected(make_batch("hc", 300, 6, seed=8)))


def test_sigterm_lets_the_call_in_flight_finish(stub_exe, sockdir):
    h = start_stub(stub_exe, sockdir / "term.sock", STUB_DELAY_US=500000)
    b = random_batch(np.random.RandomState(8), 6, 2)
    import threading
    res = {}
    with native.PairHmmContext(server=h.socket_path) as c:
        t = threading.Thread(target=lambda: res.setdefault("out", c.compute(b)))
        t.start()
        wait_until(lambda: h.stats()["calls_active"] >= 1)
        h.proc.send_signal(signal.SIGTERM)
        t.join(60)
        assert h.proc.wait(30) == 0
    assert np.array_equal(res["out"], mockjni.stub_expected(b))
    assert not os.path.exists(h.socket_path)

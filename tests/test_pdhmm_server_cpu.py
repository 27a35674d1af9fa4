"""PDHMM through the server (gkl_amd/csrc/pairhmm_server.cpp, pdhmm_remote.cpp) without a GPU.  The server is built
exactly as tests/test_server_cpu.py builds it -- pairhmm_server.cpp + the two PairHMM stubs + -lpthread, so it links no
PDHMM symbol -- and finds its PDHMM library at run time through GKL_HIP_PDHMM_LIB: tests/native/stub_gklhip_pdhmm.cpp, a
checksum per pair instead of PDHMM.  The clients are the real product libraries, whose client path makes no HIP call."""
import ctypes as C
import fcntl
import os
import signal
import socket
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

from gkl_amd import native, server
from gkl_amd.errors import IllegalArgumentException, RuntimeException
from gkl_amd.pdhmm_batch import PdhmmBatch
from gkl_amd.synth import random_batch
from tests import mockjni
from tests.pd_server_client import JNI_VERSION_1_8
from tests.test_pdhmm import random_pd_batch
from tests.test_server_cpu import (ARENA, COMPUTE, NATIVE, ROOT, build_stub_server, child_env, client, closed,
                                   raw_connect, read_json, read_reply, request, wait_until)

PD_HELLO, PD_COMPUTE, PD_STATS = 5, 6, 7
INVALID_TEXT = "Error while calculating pdhmm. Input arrays aren't valid."


# ---- the Python twin of tests/native/stub_gklhip_pdhmm.cpp ----
def stub_pd_expected(reads, haps, cross, fma_mode, tail_mode, ref_batch_pairs=0):
    """What the stub PDHMM library writes: paired (cross False; reads and haps are the same batch) or reads x haps."""
    def u(a, n, stride):
        return np.asarray(a, np.int8).view(np.uint8).reshape(n, stride).astype(np.uint64)

    nr, nh = reads.batch, haps.batch
    rl, hl = np.asarray(reads.read_lengths, np.int64), np.asarray(haps.hap_lengths, np.int64)
    w = sum(k * u(a, nr, reads.max_read_len) for k, a in zip((1, 3, 5, 7, 11), (reads.read_bases, reads.read_qual,
                                                                              reads.read_ins_qual, reads.read_del_qual, reads.gcp)))
    pos = np.arange(1, reads.max_read_len + 1, dtype=np.uint64)[None, :]
    hr = (w * pos * (np.arange(reads.max_read_len)[None, :] < rl[:, None])).sum(axis=1)
    hw = u(haps.hap_bases, nh, haps.max_hap_len) + 13 * u(haps.hap_pdbases, nh, haps.max_hap_len)
    hpos = np.arange(1, haps.max_hap_len + 1, dtype=np.uint64)[None, :]
    hh = (hw * hpos * (np.arange(haps.max_hap_len)[None, :] < hl[:, None])).sum(axis=1)
    if cross:
        p = np.arange(nr * nh)
        r, h = p // nh, p % nh
    else:
        r = h = p = np.arange(nr)
    k = hh[h] + 1000003 * hl[h].astype(np.uint64) + 999983 * rl[r].astype(np.uint64) + np.uint64(17 * fma_mode + 31 * tail_mode)
    if cross:
        k = k + np.uint64(7919 * (ref_batch_pairs % 1000) + 5) + 104729 * (p % 1000).astype(np.uint64)
    return hr[r].astype(np.float64) * (1.0 / 1048576.0) + k.astype(np.float64)


def padded(b, max_hap_len, max_read_len, fill=0x55):
    """The same batch with wider rows (the padding is not zero: a stride taken for a length would show)."""
    def wide(a, old, new):
        out = np.full((b.batch, new), fill, np.int8)
        out[:, :old] = np.asarray(a, np.int8).reshape(b.batch, old)
        return out.reshape(-1)
    h = [wide(a, b.max_hap_len, max_hap_len) for a in (b.hap_bases, b.hap_pdbases)]
    r = [wide(a, b.max_read_len, max_read_len) for a in (b.read_bases, b.read_qual, b.read_ins_qual, b.read_del_qual, b.gcp)]
    return PdhmmBatch(b.batch, max_hap_len, max_read_len, *h, *r, b.hap_lengths, b.read_lengths)


def call(ctx, reads, haps, cross, fma, tail, ref_batch_pairs=0):
    assert ctx.lib.gklhip_pdhmm_set_fma_mode(ctx.handle, fma) == 0 and ctx.lib.gklhip_pdhmm_set_tail_mode(ctx.handle, tail) == 0
    return ctx.compute_cross(reads, haps, ref_batch_pairs) if cross else ctx.compute(reads)


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    return build_stub_server(str(tmp_path_factory.mktemp("pdstubsrv") / "gklhip_server_stub"))


@pytest.fixture(scope="module")
def stub_pd_lib(tmp_path_factory):
    dest = str(tmp_path_factory.mktemp("pdstublib") / "libstub_gklhip_pdhmm.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall",
                    "-Wno-unused-parameter", os.path.join(NATIVE, "stub_gklhip_pdhmm.cpp"), "-o", dest, "-lpthread"], check=True)
    return dest


@pytest.fixture(scope="module")
def sockdir(tmp_path_factory):
    return tmp_path_factory.mktemp("pdsock")


def start_stub(exe, path, pd_lib, **env):
    e = dict(os.environ)
    e["GKL_HIP_PDHMM_LIB"] = pd_lib
    e.update({k: str(v) for k, v in env.items()})
    return server.start(str(path), env=e, timeout=30, server_path=exe)


@pytest.fixture(scope="module")
def srv(stub_exe, stub_pd_lib, sockdir):
    h = start_stub(stub_exe, sockdir / "main.sock", stub_pd_lib)
    yield h
    assert h.stop() == 0


def pd_client(mode, sock, out, *args, env=None):
    return subprocess.Popen([sys.executable, "-m", "tests.pd_server_client", mode, "--socket", str(sock), "--out", str(out),
                             *map(str, args)], cwd=ROOT, env=env or child_env())


def test_both_layouts_and_both_modes(srv):
    rng = np.random.RandomState(11)
    pairs = padded(random_pd_batch(rng, 37, read_len=(1, 55), hap_len=(1, 70)), 83, 61)
    reads = random_pd_batch(rng, 13, read_len=(1, 90), hap_len=(1, 2))
    haps = random_pd_batch(rng, 5, read_len=(1, 2), hap_len=(1, 130))
    assert srv.pdhmm_stats()["protocol"] == 1 and srv.pdhmm_stats()["pid"] == srv.pid
    with native.PdhmmContext(server=srv.socket_path) as c:
        assert c.is_remote and srv.pdhmm_stats()["library_state"] == 1
        for fma in (0, 1):
            for tail in (0, 1):
                assert np.array_equal(call(c, pairs, pairs, False, fma, tail), stub_pd_expected(pairs, pairs, False, fma, tail))
                assert c.last_routing() == (37, 37, 0) and c.last_kernel_ms() == 1.25 + 37
                assert np.array_equal(call(c, reads, haps, True, fma, tail, 27), stub_pd_expected(reads, haps, True, fma, tail, 27))
                assert c.last_routing() == (13, 5, 1) and c.last_kernel_ms() == 1.25 + 65
        # (the twin tells the modes, the layouts and ref_batch_pairs apart)
        assert not np.array_equal(stub_pd_expected(reads, haps, True, 1, 1, 27), stub_pd_expected(reads, haps, True, 1, 0, 27))
        assert not np.array_equal(stub_pd_expected(reads, haps, True, 1, 1, 27), stub_pd_expected(reads, haps, True, 1, 1, 26))
        assert c.buffer_bytes() >= 1 << 20
        # the argument checks run in the client, with the local path's statuses and messages
        bad = padded(pairs, 83, 61)
        bad.hap_lengths = bad.hap_lengths.copy()
        bad.hap_lengths[0] = 0
        with pytest.raises(IllegalArgumentException, match="hap_lengths\\[0\\] = 0 outside 1..83"):
            c.compute(bad)
        assert np.array_equal(call(c, pairs, pairs, False, 1, 1), stub_pd_expected(pairs, pairs, False, 1, 1))


def test_arena_grows_across_calls(srv):
    before = srv.stats()
    rng = np.random.RandomState(12)
    small = random_pd_batch(rng, 8)
    big = random_pd_batch(rng, 300, read_len=(200, 700), hap_len=(300, 900))   # 2.6 MB of arrays: more than the first arena
    with native.PdhmmContext(server=srv.socket_path) as c:
        assert np.array_equal(c.compute(small), stub_pd_expected(small, small, False, 1, 1))
        first = c.buffer_bytes()
        assert np.array_equal(c.compute(big), stub_pd_expected(big, big, False, 1, 1))
        assert c.buffer_bytes() > first
        assert np.array_equal(c.compute(small), stub_pd_expected(small, small, False, 1, 1))
    after = srv.stats()
    assert after["arenas_registered"] + after["arenas_copied"] - before["arenas_registered"] - before["arenas_copied"] == 2


def test_copy_path_gives_the_same_results(stub_exe, stub_pd_lib, sockdir):
    h = start_stub(stub_exe, sockdir / "copy.sock", stub_pd_lib, STUB_REGISTER=0)
    try:
        rng = np.random.RandomState(13)
        reads = random_pd_batch(rng, 13, read_len=(1, 90), hap_len=(1, 2))
        haps = random_pd_batch(rng, 5, read_len=(1, 2), hap_len=(1, 130))
        with native.PdhmmContext(server=h.socket_path) as c:
            assert np.array_equal(call(c, reads, haps, True, 0, 1, 27), stub_pd_expected(reads, haps, True, 0, 1, 27))
            assert np.array_equal(call(c, reads, reads, False, 1, 0), stub_pd_expected(reads, reads, False, 1, 0))
        st = h.stats()
        assert st["arenas_copied"] == 1 and st["arenas_registered"] == 0
    finally:
        assert h.stop() == 0


def test_eight_pdhmm_and_four_pairhmm_client_processes_at_once(stub_exe, stub_pd_lib, sockdir, tmp_path):
    h = start_stub(stub_exe, sockdir / "mixed.sock", stub_pd_lib)
    try:
        go = tmp_path / "go"
        pd = [pd_client("random", h.socket_path, tmp_path / f"pd{i}", "--calls", 50, "--seed", 200 + i, "--go", go) for i in range(8)]
        ph = [client("random", h.socket_path, tmp_path / f"ph{i}", "--calls", 50, "--seed", 300 + i, "--go", go) for i in range(4)]
        wait_until(lambda: (h.pdhmm_stats()["live_connections"] >= 8 and h.stats()["live_connections"] >= 4)
                   or any(p.poll() is not None for p in pd + ph), 120)
        go.touch()
        for p in pd + ph:
            assert p.wait(300) == 0
        for name in [f"pd{i}" for i in range(8)] + [f"ph{i}" for i in range(4)]:
            r = read_json(tmp_path / name)
            assert r["remote"] and (r["good"], r["bad"]) == (50, 0), (name, r)
        wait_until(lambda: h.pdhmm_stats()["live_connections"] == 0 and h.stats()["live_connections"] == 0)
        st, pst = h.stats(), h.pdhmm_stats()
        # each kind of counter counts its own kind of connection and call only
        assert (st["calls_served"], st["calls_failed"], st["connections_total"]) == (200, 0, 4)
        assert (pst["calls_served"], pst["calls_failed"], pst["calls_active"], pst["connections_total"]) == (400, 0, 0, 8)
        assert pst["pairs_served"] > 400
    finally:
        assert h.stop() == 0


def test_missing_pdhmm_library_is_refused_and_pairhmm_goes_on(stub_exe, sockdir, tmp_path):
    nowhere = str(tmp_path / "nowhere" / "libgklhip_pdhmm.so")
    h = start_stub(stub_exe, sockdir / "nolib.sock", nowhere)
    try:
        assert h.pdhmm_stats()["library_state"] == 0
        lib = native.load_pdhmm_library()
        ctx = C.c_void_p()
        assert lib.gklhip_pdhmm_connect(os.fsencode(h.socket_path), -1, C.byref(ctx)) == native.ERR_UNSUPPORTED
        msg = lib.gklhip_pdhmm_last_error().decode()
        assert nowhere in msg and h.socket_path in msg and not ctx.value
        with pytest.raises(RuntimeException, match="cannot serve PDHMM"):
            native.PdhmmContext(server=h.socket_path)
        assert h.pdhmm_stats()["library_state"] == -1 and h.pdhmm_stats()["live_connections"] == 0
        with native.PairHmmContext(server=h.socket_path) as c:
            b = random_batch(np.random.RandomState(3), 20, 4)
            assert np.array_equal(c.compute(b), mockjni.stub_expected(b))
    finally:
        assert h.stop() == 0


# ---- the wire protocol by hand (gkl_amd/csrc/pairhmm_remote.h) ----
def pd_connect(path):
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(20)
    s.connect(str(path))
    s.sendall(request(PD_HELLO, struct.pack("<iiii", native.ABI_VERSION, 1, -1, 0)))
    return s, read_reply(s)


def pd_compute_req(layout, n_reads, n_haps, max_hap, max_read, flags, ref, offs):
    body = struct.pack("<6iq10Q", layout, n_reads, n_haps, max_hap, max_read, flags, ref, *offs)
    assert len(body) == 112
    return request(PD_COMPUTE, body)


def send_arena(s, size=1 << 16, hap_len=2, read_len=2):
    """An arena for one pair with rows of 4 bytes: hap_lengths at 0, read_lengths at 64, the seven arrays from 128 on
    (64 apart), out at 1024."""
    fd = os.memfd_create("t", os.MFD_ALLOW_SEALING)
    os.ftruncate(fd, size)
    fcntl.fcntl(fd, fcntl.F_ADD_SEALS, fcntl.F_SEAL_SHRINK | fcntl.F_SEAL_GROW)
    os.pwrite(fd, struct.pack("<q", hap_len), 0)
    os.pwrite(fd, struct.pack("<q", read_len), 64)
    for k in range(7):
        os.pwrite(fd, bytes([65 + k, 67 + k, 1, 1]), 128 + 64 * k)
    socket.send_fds(s, [request(ARENA, struct.pack("<Q", size))], [fd])
    os.close(fd)
    return read_reply(s)


GOOD_OFFS = [128, 192, 256, 320, 384, 448, 512, 0, 64, 1024]   # (hap_bases ... gcp, hap_lengths, read_lengths, out)


def test_malformed_pdhmm_requests_are_refused_and_others_keep_working(srv, tmp_path):
    other = pd_client("random", srv.socket_path, tmp_path / "other", "--calls", 100, "--seed", 7)
    refused0 = srv.stats()["requests_refused"]
    # the hand-made request is right when nothing is wrong with it: status 0 and a PdComputeReply
    s, r = pd_connect(srv.socket_path)
    assert r[0] == 0 and struct.unpack("<i", r[2]) == (0,)
    assert send_arena(s)[0] == 0
    s.sendall(pd_compute_req(0, 1, 1, 4, 4, 3, 0, GOOD_OFFS))
    st, text, payload = read_reply(s)
    assert st == 0 and struct.unpack("<f3i", payload) == (2.25, 1, 1, 0), (st, text)
    # kPdStats works on a PDHMM connection too
    s.sendall(request(PD_STATS))
    st, _, payload = read_reply(s)
    assert st == 0 and len(payload) == C.sizeof(native.PdhmmServerInfo)
    s.close()

    cases = []   # (socket, text the refusal must hold)
    s, _ = pd_connect(srv.socket_path)                                       # a call before any arena
    s.sendall(pd_compute_req(0, 1, 1, 4, 4, 3, 0, GOOD_OFFS))
    cases.append((s, "arena"))
    outside = list(GOOD_OFFS)
    outside[4] = 1 << 20                                                     # read_ins_qual beyond the arena
    big = (1 << 31) - 1
    wrap = list(GOOD_OFFS)
    wrap[0] = (1 << 64) - 8                                                  # offset + items * stride passes 2^64
    for req, lens, why in ((pd_compute_req(0, 1, 1, 4, 4, 3, 0, outside), (2, 2), "outside"),
                           # (items and strides are 32-bit, so their product always fits 64 bits; with this offset the
                           #  end of the range, offset + items * stride, does not)
                           (pd_compute_req(0, 1, 1, big, big, 3, 0, wrap), (2, 2), "outside"),
                           (pd_compute_req(0, 1, 1, 4, 4, 3, 0, GOOD_OFFS), (0, 2), "length"),
                           (pd_compute_req(0, 1, 1, 4, 4, 3, 0, GOOD_OFFS), (2, 5), "length"),
                           (pd_compute_req(1, 1 << 16, 1 << 16, 4, 4, 3, 0, GOOD_OFFS), (2, 2), "2^31"),
                           (request(COMPUTE, struct.pack("<ii9Q", 1, 1, *([0] * 9))), (2, 2), "unknown request type 3")):
        s, r = pd_connect(srv.socket_path)
        assert r[0] == 0 and send_arena(s, hap_len=lens[0], read_len=lens[1])[0] == 0
        s.sendall(req)
        cases.append((s, why))
    s, r = raw_connect(srv.socket_path)                                      # a PDHMM call on a PairHMM connection
    assert r[0] == 0 and send_arena(s)[0] == 0
    s.sendall(pd_compute_req(0, 1, 1, 4, 4, 3, 0, GOOD_OFFS))
    cases.append((s, "unknown request type 6"))
    for s, why in cases:
        r = read_reply(s)
        assert r is not None and r[0] == native.ERR_INVALID_ARG and why in r[1], (why, r)
        assert closed(s)
        s.close()
    # a first message that is neither hello
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.settimeout(20)
    s.connect(srv.socket_path)
    s.sendall(request(PD_COMPUTE))
    assert read_reply(s)[0] == native.ERR_INVALID_ARG and closed(s)
    s.close()
    assert srv.stats()["requests_refused"] - refused0 == len(cases) + 1
    rng = np.random.RandomState(1)
    with native.PdhmmContext(server=srv.socket_path) as c:
        b = random_pd_batch(rng, 30)
        assert np.array_equal(c.compute(b), stub_pd_expected(b, b, False, 1, 1))
    assert other.wait(300) == 0
    r = read_json(tmp_path / "other")
    assert (r["good"], r["bad"]) == (100, 0)


def test_a_library_error_passes_through_and_the_context_goes_on(srv, stub_pd_lib):
    rng = np.random.RandomState(21)
    good = random_pd_batch(rng, 20)
    bad = random_pd_batch(rng, 20)
    bad.gcp = bad.gcp.copy()
    bad.gcp[7 * bad.max_read_len] = -3
    # what the library itself answers, called directly
    stub = C.CDLL(stub_pd_lib)
    stub.gklhip_pdhmm_last_error.restype = C.c_char_p
    d = C.c_void_p()
    assert stub.gklhip_pdhmm_init(-1, C.byref(d)) == 0
    cb = native.CPdhmmBatch(bad.batch, bad.max_hap_len, bad.max_read_len,
                            *[a.ctypes.data for a in (bad.hap_bases, bad.hap_pdbases, bad.read_bases, bad.read_qual,
                                                      bad.read_ins_qual, bad.read_del_qual, bad.gcp, bad.hap_lengths, bad.read_lengths)])
    out = np.empty(bad.batch)
    assert stub.gklhip_pdhmm_compute(d, C.byref(cb), C.c_void_p(out.ctypes.data)) == native.ERR_INVALID_ARG
    direct = stub.gklhip_pdhmm_last_error().decode()
    stub.gklhip_pdhmm_done(d)
    assert direct == INVALID_TEXT
    failed0 = srv.pdhmm_stats()["calls_failed"]
    with native.PdhmmContext(server=srv.socket_path) as c:
        with pytest.raises(IllegalArgumentException) as via:
            c.compute(bad)
        assert str(via.value) == direct
        assert np.array_equal(c.compute(good), stub_pd_expected(good, good, False, 1, 1))
    assert srv.pdhmm_stats()["calls_failed"] == failed0 + 1


def test_a_client_killed_in_the_middle_of_a_call(stub_exe, stub_pd_lib, sockdir, tmp_path):
    h = start_stub(stub_exe, sockdir / "slow.sock", stub_pd_lib, STUB_DELAY_US=200000)
    try:
        victim = pd_client("loop", h.socket_path, tmp_path / "victim")
        wait_until(lambda: os.path.exists(str(tmp_path / "victim") + ".json") or victim.poll() is not None, 120)
        with native.PdhmmContext(server=h.socket_path) as c:
            assert h.pdhmm_stats()["live_connections"] == 2
            wait_until(lambda: h.pdhmm_stats()["calls_active"] >= 1)
            victim.kill()
            victim.wait()
            b = random_pd_batch(np.random.RandomState(2), 10)
            assert np.array_equal(c.compute(b), stub_pd_expected(b, b, False, 1, 1))
            wait_until(lambda: h.pdhmm_stats()["live_connections"] == 1)
        wait_until(lambda: h.pdhmm_stats()["live_connections"] == 0)
    finally:
        assert h.stop() == 0


def test_sigterm_lets_the_pdhmm_call_in_flight_finish(stub_exe, stub_pd_lib, sockdir):
    h = start_stub(stub_exe, sockdir / "term.sock", stub_pd_lib, STUB_DELAY_US=500000)
    b = random_pd_batch(np.random.RandomState(8), 6)
    res = {}
    with native.PdhmmContext(server=h.socket_path) as c:
        t = threading.Thread(target=lambda: res.setdefault("out", c.compute(b)))
        t.start()
        wait_until(lambda: h.pdhmm_stats()["calls_active"] >= 1)
        h.proc.send_signal(signal.SIGTERM)
        t.join(60)
        assert h.proc.wait(30) == 0
        # the server is gone: the next call fails with a message that names the socket, it neither hangs nor crashes
        with pytest.raises(RuntimeException, match="went away"):
            c.compute(b)
        lib = native.load_pdhmm_library()
        assert h.socket_path in lib.gklhip_pdhmm_last_error().decode()
    assert np.array_equal(res["out"], stub_pd_expected(b, b, False, 1, 1))
    assert not os.path.exists(h.socket_path)
    with pytest.raises(RuntimeException, match="cannot reach"):
        native.PdhmmContext(server=h.socket_path)


def test_client_mode_of_init_opens_no_device(srv, tmp_path):
    env = child_env()
    env["GKL_HIP_SERVER"] = srv.socket_path
    p = pd_client("once", srv.socket_path, tmp_path / "once", "--seed", 5, env=env)
    assert p.wait(120) == 0
    r = read_json(tmp_path / "once")
    assert r["remote"] and (r["good"], r["bad"]) == (1, 0), r
    assert not [f for f in r["open_files"] if f.startswith("/dev/kfd") or f.startswith("/dev/dri")], r["open_files"]


def test_jni_library_loads_with_the_server_up_and_not_without(srv, tmp_path):
    env = child_env()
    env["GKL_HIP_SERVER"] = srv.socket_path
    calls0 = srv.pdhmm_stats()["calls_served"]
    p = pd_client("jniload", srv.socket_path, tmp_path / "up", "--run", 1, "--shape", "9:4", env=env)
    assert p.wait(120) == 0
    r = read_json(tmp_path / "up")
    assert r["onload"] == JNI_VERSION_1_8 and r["rc"] == [0, 0], r
    assert not [f for f in r["open_files"] if f.startswith("/dev/kfd") or f.startswith("/dev/dri")], r["open_files"]
    assert srv.pdhmm_stats()["calls_served"] == calls0 + 2   # computePDHMMNative and computeLikelihoodsNative went to the server
    from tests.golden_io import load_pdhmm_file
    from tests.pd_server_client import region
    got = np.load(str(tmp_path / "up") + ".npz")
    flat, _ = load_pdhmm_file("pdhmm_syn_199_68_51.txt")
    assert np.array_equal(got["flat"], stub_pd_expected(flat, flat, False, 1, 1))
    reads, haps = region(1, 9, 4)
    assert np.array_equal(got["holders"], stub_pd_expected(reads, haps, True, 1, 1, 36))   # (36 pairs: one reference batch)
    env["GKL_HIP_SERVER"] = str(tmp_path / "absent.sock")
    p = pd_client("jniload", env["GKL_HIP_SERVER"], tmp_path / "down", env=env)
    assert p.wait(120) == 0
    assert read_json(tmp_path / "down")["onload"] == -1   # JNI_ERR: System.load throws, GATK falls back to Java

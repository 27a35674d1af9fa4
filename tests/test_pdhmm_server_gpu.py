"""PDHMM through the server on the MI355X: what a client context gets is, byte for byte, what a direct call of the same
library gives in this (server-less) process -- the path tests/test_pdhmm.py pins to the oracle -- in both layouts, both
arithmetic modes and both tail modes, whichever kernel a haplotype is routed to; the JNI library computes through the
server; client processes never open the device.  One server for the module, started under a time limit."""
import numpy as np
import pytest

from gkl_amd import native, server
from gkl_amd.errors import IllegalArgumentException
from gkl_amd.pdhmm_batch import PdhmmBatch
from tests import mockjni
from tests.golden_io import load_pdhmm_file
from tests.pd_server_client import JNI_VERSION_1_8, region
from tests.test_pdhmm import random_pd_batch
from tests.test_pdhmm_server_cpu import pd_client
from tests.test_server_gpu import child_env, no_gpu_files, read_json, wait_until


@pytest.fixture(scope="module")
def gpu_server(tmp_path_factory):
    h = server.start(str(tmp_path_factory.mktemp("pdgsrv") / "s.sock"), timeout=120)
    yield h
    assert h.stop() == 0


@pytest.mark.gpu
def test_client_contexts_are_byte_identical_to_direct_calls(gpu_server):
    rng = np.random.RandomState(41)
    fixture, _ = load_pdhmm_file("pdhmm_syn_199_68_51.txt")
    # (read bases A, C, G, T only: in reference-tail mode the scalar engine, like GKL's, rejects any other read base under
    #  a SNP column when such a pair sits in a batch's tail -- tests/test_pdhmm.py covers that -- and these are valid inputs)
    acgt = dict(with_n=False, lower=False)
    pairs = random_pd_batch(rng, 37, read_len=(1, 61), hap_len=(1, 83), **acgt)
    reads = random_pd_batch(rng, 13, read_len=(1, 151), hap_len=(1, 2), **acgt)
    haps = random_pd_batch(rng, 5, read_len=(1, 2), hap_len=(1, 260), **acgt)
    for fma in (0, 1):
        for tail in (False, True):
            with native.PdhmmContext(device=0, fma_mode=fma, reference_tail=tail) as d, \
                    native.PdhmmContext(fma_mode=fma, reference_tail=tail, server=gpu_server.socket_path) as c:
                assert c.is_remote and not d.is_remote
                for b in (fixture, pairs):
                    want = d.compute(b)
                    assert c.compute(b).tobytes() == want.tobytes(), (fma, tail, b.batch)
                    assert c.last_routing() == d.last_routing()
                    if b is fixture and fma == 1 and tail:
                        from oracle.pdhmm import PdhmmOracle
                        assert want.tobytes() == PdhmmOracle().compute_reference(b, fma_mode=1)[1].tobytes()
                want = d.compute_cross(reads, haps, 27)
                assert c.compute_cross(reads, haps, 27).tobytes() == want.tobytes(), (fma, tail)
    st = gpu_server.pdhmm_stats()
    assert st["library_state"] == 1 and st["calls_failed"] == 0 and st["calls_served"] >= 12
    wait_until(lambda: gpu_server.pdhmm_stats()["live_connections"] == 0)   # (the server notices a closed connection on its own thread)


@pytest.mark.gpu
def test_all_three_kernel_routes_through_the_server(gpu_server):
    """A 6 x 4 cross call: a read of 400 bases (striped), a plain haplotype (table kernel), one with seven or more column
    classes (predicate kernel), one with a base outside ACGTN (byte-comparing kernel)."""
    rng = np.random.RandomState(43)
    acgt = np.frombuffer(b"ACGT", dtype=np.int8)
    one = np.zeros(1, np.int8)

    def hap(n_snp_kinds, odd=False):
        H = int(rng.randint(150, 260))
        b = acgt[rng.randint(0, 4, H)].copy()
        pd = np.zeros(H, np.int8)
        for k in range(n_snp_kinds):                      # distinct (base, allele set) kinds: a class each
            for j in (10 + 7 * k, 80 + 7 * k):
                b[j] = acgt[k % 4]
                pd[j] = 1 | (k + 1) << 3
        if odd:
            b[40] = ord("a")
        return b, pd

    haps = PdhmmBatch.from_pairs([(b, pd, one, one, one, one, one) for b, pd in (hap(0), hap(1), hap(5), hap(1, odd=True))])
    short = random_pd_batch(rng, 5, read_len=(30, 151), hap_len=(1, 2), with_n=False, lower=False)
    long_ = random_pd_batch(rng, 1, read_len=(400, 400), hap_len=(1, 2), with_n=False, lower=False)
    reads = PdhmmBatch.from_pairs(short.pairs() + long_.pairs())
    assert reads.batch == 6 and int(reads.read_lengths.max()) >= 385
    with native.PdhmmContext(device=0) as d, native.PdhmmContext(server=gpu_server.socket_path) as c:
        want = d.compute_cross(reads, haps)
        tab, pred, odd = d.last_routing()
        assert tab >= 1 and pred >= 1 and odd == 1 and tab + pred + odd == 4, (tab, pred, odd)
        assert c.compute_cross(reads, haps).tobytes() == want.tobytes()
        assert c.last_routing() == (tab, pred, odd)


@pytest.mark.gpu
def test_jni_library_in_client_mode_is_byte_identical(gpu_server, tmp_path):
    env = child_env(GKL_HIP_SERVER=gpu_server.socket_path)
    p = pd_client("jniload", gpu_server.socket_path, tmp_path / "jni", "--run", 1, "--seed", 9, "--shape", "20:7", env=env)
    assert p.wait(300) == 0
    rec = read_json(tmp_path / "jni")
    assert rec["onload"] == JNI_VERSION_1_8 and rec["rc"] == [0, 0], rec
    assert no_gpu_files(rec), [x for x in rec["open_files"] if x.startswith("/dev")]
    got = np.load(str(tmp_path / "jni") + ".npz")
    flat, _ = load_pdhmm_file("pdhmm_syn_199_68_51.txt")
    rc, want, cls, msg = mockjni.run_pdhmm(flat)                       # the mock JVM in this process: the direct path
    assert rc == 0 and got["flat"].tobytes() == want.tobytes(), (cls, msg)
    rc, want, cls, msg = mockjni.run_pdhmm(None, holders=region(9, 20, 7))
    assert rc == 0 and got["holders"].tobytes() == want.tobytes(), (cls, msg)


@pytest.mark.gpu
def test_eight_concurrent_client_processes(gpu_server, tmp_path):
    go = tmp_path / "go"
    live0 = gpu_server.pdhmm_stats()["live_connections"]
    procs = [pd_client("region", gpu_server.socket_path, tmp_path / f"c{i}", "--calls", 20, "--seed", 60 + i, "--shape", "61:41",
                       "--go", go) for i in range(8)]
    try:
        wait_until(lambda: gpu_server.pdhmm_stats()["live_connections"] >= live0 + 8 or any(p.poll() is not None for p in procs), 300)
        go.touch()
        for p in procs:
            assert p.wait(300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    with native.PdhmmContext(device=0) as d:
        for i in range(8):
            rec = read_json(tmp_path / f"c{i}")
            assert rec["remote"] and "unstable" not in rec and no_gpu_files(rec), rec
            assert np.load(str(tmp_path / f"c{i}") + ".npz")["out"].tobytes() == d.compute_cross(*region(60 + i, 61, 41)).tobytes(), i
    st = gpu_server.pdhmm_stats()
    assert st["calls_failed"] == 0 and st["calls_active"] == 0
    print("PDHMM server stats:", st)


@pytest.mark.gpu
def test_invalid_input_fails_like_the_direct_path_and_the_context_goes_on(gpu_server):
    rng = np.random.RandomState(47)
    good = random_pd_batch(rng, 30, with_n=False, lower=False)
    bad = random_pd_batch(rng, 30, with_n=False, lower=False)
    bad.read_ins_qual = bad.read_ins_qual.copy()
    bad.read_ins_qual[11 * bad.max_read_len] = -1
    failed0 = gpu_server.pdhmm_stats()["calls_failed"]
    with native.PdhmmContext(device=0) as d, native.PdhmmContext(server=gpu_server.socket_path) as c:
        with pytest.raises(IllegalArgumentException) as direct:
            d.compute(bad)
        with pytest.raises(IllegalArgumentException) as via:
            c.compute(bad)
        assert str(via.value) == str(direct.value) == "Error while calculating pdhmm. Input arrays aren't valid."
        assert c.compute(good).tobytes() == d.compute(good).tobytes()
    assert gpu_server.pdhmm_stats()["calls_failed"] == failed0 + 1

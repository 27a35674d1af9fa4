"""Double-precision callers (useDoublePrecision = true / gklhip_config.use_double) that meet: client processes of one
PairHMM server in the server's combiner, among themselves and beside fp32 clients (a set never mixes precisions), and the
threads of one process through the JNI symbols.  Every output has the bits of its own mode's oracle."""
import numpy as np
import pytest

from gkl_amd import server
from gkl_amd.synth import make_batch
from tests import mockjni
from tests.test_server_gpu import bits, child_env, no_gpu_files, run_clients

pytestmark = pytest.mark.gpu


def test_double_clients_meet_in_the_servers_combiner(oracle, tmp_path):
    """GKL_HIP_COMBINE_MIN=4 with a long wait in the server's environment: four double-precision clients calling at once.
    What the trigger guarantees is that a call arriving while a set is in flight waits for the others -- so calls get
    combined; no timing is asserted."""
    sock = tmp_path / "dcomb.sock"
    h = server.start(str(sock), env=child_env(GKL_HIP_COMBINE_MIN=4, GKL_HIP_COMBINE_WAIT_US=2000000), timeout=120)
    try:
        specs = [("hc:100:10:3", 1, 1)] * 4
        res = run_clients(sock, tmp_path, specs, repeat=30)
        want = oracle.batch(make_batch("hc", 100, 10, seed=3), use_double=True, n_threads=4)
        for rec, outs in res:
            assert no_gpu_files(rec) and "unstable" not in rec
            assert np.array_equal(bits(outs["out0"]), bits(want))
        st = h.stats()
        calls, combined, sets = st["small_call_counts"][0]
        print("small_call_counts", (calls, combined, sets), "calls_served", st["calls_served"])
        assert st["calls_served"] == 4 * 31
        assert 0 < calls <= 4 * 31 and combined > 0 and sets < calls, st
    finally:
        assert h.stop() == 0


def test_double_and_fp32_clients_of_one_server_get_their_own_bits(oracle, tmp_path):
    """Two double-precision and two fp32 clients call one server at once for 20 rounds: calls of both precisions wait in
    the combiner's queue together (a call that arrives while a set is in flight waits up to 20 ms for company), sets get
    combined, and every client still gets the bits of its own mode -- a set that mixed the two would show."""
    b = make_batch("hc", 100, 10, seed=3)
    want = {0: oracle.batch(b, n_threads=4), 1: oracle.batch(b, use_double=True, n_threads=4)}
    assert not np.array_equal(bits(want[0]), bits(want[1])), "the two modes must differ on this batch: a mixed set would show"
    sock = tmp_path / "mixed.sock"
    h = server.start(str(sock), env=child_env(GKL_HIP_COMBINE_MIN=2, GKL_HIP_COMBINE_WAIT_US=20000), timeout=120)
    try:
        specs = [("hc:100:10:3", 1, 1), ("hc:100:10:3", 0, 1), ("hc:100:10:3", 1, 1), ("hc:100:10:3", 0, 1)]
        res = run_clients(sock, tmp_path, specs, repeat=20)
        for (_, d, _), (rec, outs) in zip(specs, res):
            assert no_gpu_files(rec) and "unstable" not in rec
            assert np.array_equal(bits(outs["out0"]), bits(want[d])), d
        calls, combined, sets = h.stats()["small_call_counts"][0]
        print("small_call_counts", (calls, combined, sets))
        assert 0 < calls <= 4 * 21 and combined > 0 and sets < calls, (calls, combined, sets)
    finally:
        assert h.stop() == 0


def test_double_precision_threads_through_the_jni_symbols(oracle):
    b = make_batch("hc", 8 * 40, 10, seed=77)
    rc, out, cls, msg, _ = mockjni.run_concurrent(b, n_threads=8, iters=10, use_double=True)
    assert rc == 0, (cls, msg)
    assert np.array_equal(bits(out), bits(oracle.batch(b, use_double=True, n_threads=8)))

"""gklhip_compute_multi on a CLIENT context (no GPU): the wire protocol has no multi request, so the client library
computes the regions as consecutive single calls through the server -- here the stub server of tests/test_server_cpu.py
(a checksum per pair instead of PairHMM).  One region of three fails the argument checks: it never reaches the server,
and the other two are computed."""
import numpy as np
import pytest

from gkl_amd import native
from gkl_amd.errors import IllegalArgumentException, RuntimeException
from gkl_amd.synth import random_batch
from tests import mockjni
from tests.test_server_cpu import sockdir, srv, stub_exe  # noqa: F401  (fixtures)


def test_client_context_computes_a_multi_call_region_by_region(srv):  # noqa: F811
    rng = np.random.RandomState(11)
    good = [random_batch(rng, 20, 4), random_batch(rng, 7, 3), random_batch(rng, 1, 9)]
    bad = random_batch(rng, 6, 2)
    bad.read_off = bad.read_off.copy()
    bad.read_off[3] = bad.read_off[2]          # a read offset that does not increase
    served0 = srv.stats()["calls_served"]
    with native.PairHmmContext(server=srv.socket_path) as c:
        singles = [c.compute(b) for b in good]
        for b, out in zip(good, singles):
            assert np.array_equal(out, mockjni.stub_expected(b))
        assert srv.stats()["calls_served"] == served0 + 3
        with pytest.raises(native.PairHmmMultiError) as e:
            c.compute_multi([good[0], bad, good[1]])
        assert e.value.statuses == [0, 1, 0] and e.value.status == 1
        assert isinstance(e.value.errors[1], IllegalArgumentException) and "read 2 is empty or offsets are not increasing" in str(e.value.errors[1])
        assert e.value.errors[0] is None and e.value.errors[2] is None and e.value.results[1] is None
        assert e.value.results[0].tobytes() == singles[0].tobytes() and e.value.results[2].tobytes() == singles[1].tobytes()
        assert srv.stats()["calls_served"] == served0 + 5      # the two good regions; the bad one never left the client
        # all good: the list of arrays, same bytes as the single calls
        got = c.compute_multi(good)
        assert [g.tobytes() for g in got] == [s.tobytes() for s in singles]
        assert srv.stats()["calls_served"] == served0 + 8
        # the raw sums stay on the server
        with pytest.raises(RuntimeException, match="unsupported"):
            c.raw_region(0, good[0].n_pairs)
        with pytest.raises(IllegalArgumentException, match="no regions to process"):
            c.compute_multi([])

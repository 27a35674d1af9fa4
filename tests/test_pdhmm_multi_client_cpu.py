"""gklhip_pdhmm_compute_cross_multi on a CLIENT context (no GPU): the wire protocol has no multi request, so the client
library computes the regions as consecutive single calls through the server -- here the stub server and stub PDHMM library
of tests/test_pdhmm_server_cpu.py.  Checks the per-region argument checks, statuses and messages, that a failing region
leaves the others computed, and what last_routing / last_kernel_ms hold afterwards."""
import numpy as np
import pytest

from gkl_amd import native
from gkl_amd.errors import IllegalArgumentException
from tests.test_pdhmm import random_pd_batch
from tests.test_pdhmm_server_cpu import INVALID_TEXT, sockdir, srv, stub_exe, stub_pd_expected, stub_pd_lib  # noqa: F401  (fixtures)


def regions_of(rng, n):
    return [(random_pd_batch(rng, int(rng.randint(1, 20)), read_len=(1, 90), hap_len=(1, 2)),
             random_pd_batch(rng, int(rng.randint(1, 7)), read_len=(1, 2), hap_len=(1, 130))) for _ in range(n)]


def test_client_context_computes_a_multi_call_region_by_region(srv):  # noqa: F811
    rng = np.random.RandomState(5)
    regions = regions_of(rng, 5)
    ref = [0, 13, 8, 0, 27]
    served0 = srv.pdhmm_stats()["calls_served"]
    with native.PdhmmContext(server=srv.socket_path) as c:
        got = c.compute_cross_multi(regions, ref)
        assert len(got) == 5
        for (reads, haps), rb, out in zip(regions, ref, got):
            assert np.array_equal(out, stub_pd_expected(reads, haps, True, 1, 1, rb))
        # the stub reports (n_reads, n_haps, 1) as routing and 1.25 + pairs as kernel time per call: the sums
        assert c.last_routing() == (sum(r.batch for r, _ in regions), sum(h.batch for _, h in regions), 5)
        assert c.last_kernel_ms() == pytest.approx(sum(1.25 + r.batch * h.batch for r, h in regions))
        assert srv.pdhmm_stats()["calls_served"] == served0 + 5
        got = c.compute_cross_multi(regions[:2])          # ref_batch_pairs None = all 0
        for (reads, haps), out in zip(regions, got):
            assert np.array_equal(out, stub_pd_expected(reads, haps, True, 1, 1, 0))
    assert native.pdhmm_combine_counts() == (0, 0, 0)     # a client computes nothing itself


def test_failing_regions_fail_alone_on_a_client_context(srv):  # noqa: F811
    rng = np.random.RandomState(6)
    regions = regions_of(rng, 4)
    bad_reads = random_pd_batch(rng, 9, read_len=(1, 90), hap_len=(1, 2))
    bad_reads.gcp = bad_reads.gcp.copy()
    bad_reads.gcp[3 * bad_reads.max_read_len] = -3                       # the library's input error, found by the server
    short = random_pd_batch(rng, 4, read_len=(1, 90), hap_len=(1, 2))
    short.read_lengths = short.read_lengths.copy()
    short.read_lengths[2] = short.max_read_len + 5                       # fails the argument checks in the client
    mix = [regions[0], (bad_reads, regions[1][1]), regions[2], (short, regions[3][1]), regions[3]]
    failed0 = srv.pdhmm_stats()["calls_failed"]
    with native.PdhmmContext(server=srv.socket_path) as c:
        with pytest.raises(native.PdhmmMultiError) as e:
            c.compute_cross_multi(mix, [0, 0, 13, 0, 8])
        assert e.value.statuses == [native.OK, native.ERR_INVALID_ARG, native.OK, native.ERR_INVALID_ARG, native.OK]
        assert isinstance(e.value.errors[1], IllegalArgumentException) and str(e.value.errors[1]) == INVALID_TEXT   # the FIRST failing region's text
        assert isinstance(e.value.errors[3], IllegalArgumentException)
        for k, rb in ((0, 0), (2, 13), (4, 8)):
            assert e.value.errors[k] is None
            assert np.array_equal(e.value.results[k], stub_pd_expected(*mix[k], True, 1, 1, rb)), k
        assert e.value.results[1] is None and e.value.results[3] is None
        # the argument-check failure never reached the server; the input error did
        assert srv.pdhmm_stats()["calls_failed"] == failed0 + 1
        # when the region that fails the checks comes first, its message is the one kept
        with pytest.raises(native.PdhmmMultiError) as e:
            c.compute_cross_multi([(short, regions[3][1]), regions[0]])
        assert "read_lengths[2]" in str(e.value.errors[0]) and e.value.statuses == [native.ERR_INVALID_ARG, native.OK]
        # the call itself refused
        with pytest.raises(IllegalArgumentException, match="no regions to process"):
            c.compute_cross_multi([])
        with pytest.raises(native.PdhmmMultiError) as e:
            c.compute_cross_multi([regions[0]], [-1])
        assert "ref_batch_pairs must not be negative" in str(e.value.errors[0])
        # and the context goes on
        out = c.compute_cross_multi([regions[1]])[0]
        assert np.array_equal(out, stub_pd_expected(*regions[1], True, 1, 1, 0))

"""Several PDHMM region calls whose inputs lie in HBM, in one set of launches, results left in HBM
(gklhip_pdhmm_compute_cross_multi_device, PdhmmContext.compute_cross_multi_device) on the MI355X.

The regions are those of tests/test_pdhmm_multi.py (make_regions): the smallest shapes that reach every kernel route and
a change of row stride -- what the gather kernel can get wrong.  Every region's raw sums, finalised on the host, are the
oracle's bytes and the host single call's; its sums and its device log10 values are byte for byte those of a
compute_cross_device call of the region alone on the same context; the device log10 values are within REL_TOL of the
host's (tests/test_gpu_parity.py), checked as assert_parity of tests/test_pdhmm_device.py does.

A client context of the server needs no GPU: tests/test_pdhmm_multi_device_cpu.py has that case, with the stub server."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from gkl_amd.pdhmm_batch import PdhmmBatch
from tests.test_pdhmm_device import assert_parity
from tests.test_pdhmm_multi import INPUT_ERROR_TEXT, Mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def native():
    from gkl_amd import native as n
    return n


class DeviceMode:
    """A Mode of tests/test_pdhmm_multi.py (context, regions, oracle and host single-call bytes) plus, computed once and
    shared by the tests, every region's arrays in HBM and the bytes a compute_cross_device call of it alone leaves."""

    def __init__(self, native, fma_mode, tail):
        import torch
        self.host = Mode(fma_mode, tail)
        self.ctx, self.ref_batch = self.host.ctx, self.host.ref_batch
        self.dbs = [native.PdhmmDeviceBatch.upload_cross(r, h, DEV) for r, h in self.host.regions]
        self.pairs = [r.batch * h.batch for r, h in self.host.regions]
        self.out, self.sums = [], []
        for (rdb, hdb), rb, n in zip(self.dbs, self.ref_batch, self.pairs):
            s = torch.empty(n, dtype=torch.float64, device=DEV)
            o = self.ctx.compute_cross_device(rdb, hdb, rb, sums=s)
            self.out.append(to_bytes(o))
            self.sums.append(to_bytes(s))

    def new_sums(self, ks):
        import torch
        return [torch.empty(self.pairs[k], dtype=torch.float64, device=DEV) for k in ks]

    def run(self, ks, **kw):
        """The multi device call over the regions ks, with sums; returns (outs, sums)."""
        sums = self.new_sums(ks)
        outs = self.ctx.compute_cross_multi_device([self.dbs[k] for k in ks], [self.ref_batch[k] for k in ks], sums=sums, **kw)
        return outs, sums

    def assert_single_bytes(self, ks, outs, sums=None):
        for at, k in enumerate(ks):
            assert to_bytes(outs[at]) == self.out[k], (ks, at)
            if sums is not None and sums[at] is not None:
                assert to_bytes(sums[at]) == self.sums[k], (ks, at)


def to_bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def modes(native):
    made = {}

    def get(fma_mode, tail):
        if (fma_mode, tail) not in made:
            made[(fma_mode, tail)] = DeviceMode(native, fma_mode, tail)
        return made[(fma_mode, tail)]

    yield get
    for m in made.values():
        m.ctx.close()


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
@pytest.mark.parametrize("fma_mode", [1, 0], ids=["avx512-arith", "avx2-arith"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_multi_device_call_is_the_oracle_the_host_call_and_the_single_device_call(native, modes, K, fma_mode, tail):
    m = modes(fma_mode, tail)
    h = m.host
    assert h.single == h.oracle
    sums = m.new_sums(range(K))
    outs = m.ctx.compute_cross_multi_device(m.dbs[:K], m.ref_batch[:K] if tail else None, sums=sums)
    assert len(outs) == K
    assert m.ctx.last_routing() == tuple(sum(r[i] for r in h.routing[:K]) for i in range(3))
    assert m.ctx.last_kernel_ms() > 0.0
    for k in range(K):
        finalised = native.pdhmm_finalise_host(sums[k].cpu()).tobytes()
        assert finalised == h.oracle[k], (K, k)
        assert finalised == h.single[k], (K, k)
        assert_parity(native, np.frombuffer(h.single[k], np.float64), outs[k], sums[k], f"multi device K={K} region {k}")
    m.assert_single_bytes(range(K), outs, sums)


@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
def test_order_of_the_regions_does_not_matter(modes, tail):
    m = modes(1, tail)
    ks = list(range(len(m.dbs)))[::-1]
    outs, sums = m.run(ks)
    m.assert_single_bytes(ks, outs, sums)
    ks = [6, 3, 0]   # ... nor which others ride along
    outs, sums = m.run(ks)
    m.assert_single_bytes(ks, outs, sums)


# ------------------------------------------------------------------ the launches are shared; the limits
def test_one_call_of_eight_regions_is_one_launch_set(native, modes):
    m = modes(1, 1)
    ks = list(range(8))
    native.pdhmm_combine_counts(reset=True)
    outs, sums = m.run(ks)
    assert native.pdhmm_combine_counts() == (8, 8, 1)
    m.assert_single_bytes(ks, outs, sums)
    native.pdhmm_combine_counts(reset=True)
    outs, sums = m.run([0])
    assert native.pdhmm_combine_counts() == (1, 0, 1)
    m.assert_single_bytes([0], outs, sums)
    # the single device calls count nothing
    m.ctx.compute_cross_device(*m.dbs[1], m.ref_batch[1])
    assert native.pdhmm_combine_counts() == (1, 0, 1)


@pytest.mark.parametrize("n,counts", [(64, (64, 64, 1)), (65, (65, 0, 65))], ids=["64-regions", "65-regions"])
def test_the_region_limit(native, modes, n, counts):
    m = modes(1, 1)
    assert m.pairs[1] == 1   # the 1 x 1 region
    ks = [1] * n
    native.pdhmm_combine_counts(reset=True)
    outs, sums = m.run(ks)
    assert native.pdhmm_combine_counts() == counts
    m.assert_single_bytes(ks, outs, sums)
    assert m.ctx.last_routing() == tuple(n * v for v in m.host.routing[1])


# ------------------------------------------------------------------ alignment of the inputs, guards around the results
def guarded(a, off):
    """The bytes of `a` as a view that starts `off` bytes into a larger 0xAB-filled tensor: (the whole tensor, the view)."""
    import torch
    a = np.ascontiguousarray(a, np.int8).reshape(-1)
    whole = torch.full((off + a.size + 9,), 0xAB - 256, dtype=torch.int8, device=DEV)
    whole[off:off + a.size] = torch.from_numpy(a).to(DEV)
    return whole, whole[off:off + a.size]


def with_stride(a, n, old, new):
    out = np.zeros((n, new), np.int8)
    out[:, :old] = np.asarray(a, np.int8).reshape(n, old)
    return out.reshape(-1)


def test_inputs_at_odd_addresses_and_odd_strides(native, modes):
    m = modes(1, 1)
    ks = [0, 2, 5, 6]   # more than one chunk; all three routes and a striped read; strides of 30 next to 600
    offs = (1, 3, 7)
    wholes, regions, at = [], [], 0
    for k in ks:
        reads, haps = m.host.regions[k]
        mr, mh = reads.max_read_len | 1, haps.max_hap_len | 1
        views = []
        for name, b, old, new in ([(n, haps, haps.max_hap_len, mh) for n in ("hap_bases", "hap_pdbases")] +
                                  [(n, reads, reads.max_read_len, mr) for n in ("read_bases", "read_qual", "read_ins_qual", "read_del_qual", "gcp")]):
            off = offs[at % 3]
            at += 1
            whole, view = guarded(with_stride(getattr(b, name), b.batch, old, new), off)
            assert view.data_ptr() % 16 != 0 and view.numel() == b.batch * new and new % 2 == 1
            wholes.append((whole, off, view.numel()))
            views.append(view)
        regions.append((native.PdhmmDeviceBatch(reads.batch, 0, mr, None, tuple(views[2:]), None, np.ascontiguousarray(reads.read_lengths, np.int64)),
                        native.PdhmmDeviceBatch(haps.batch, mh, 0, tuple(views[:2]), None, np.ascontiguousarray(haps.hap_lengths, np.int64), None)))
    sums = m.new_sums(ks)
    outs = m.ctx.compute_cross_multi_device(regions, [m.ref_batch[k] for k in ks], sums=sums)
    m.assert_single_bytes(ks, outs, sums)
    for whole, off, n in wholes:   # the guards around every input array
        assert bool((whole[:off] == 0xAB - 256).all()) and bool((whole[off + n:] == 0xAB - 256).all())


def test_nothing_outside_the_result_arrays_changes(modes):
    import torch
    m = modes(1, 1)
    ks = list(range(8))
    wholes = []
    for k in ks:
        n = m.pairs[k]
        wholes.append(tuple(torch.full((3 + n + 5,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)))
    outs = m.ctx.compute_cross_multi_device([m.dbs[k] for k in ks], [m.ref_batch[k] for k in ks],
                                            outs=[w[0][3:3 + m.pairs[k]] for k, w in zip(ks, wholes)],
                                            sums=[w[1][3:3 + m.pairs[k]] for k, w in zip(ks, wholes)])
    m.assert_single_bytes(ks, outs, [w[1][3:3 + m.pairs[k]] for k, w in zip(ks, wholes)])
    for k, pair in zip(ks, wholes):
        for whole in pair:
            assert bool((whole[:3] == SENTINEL).all()) and bool((whole[3 + m.pairs[k]:] == SENTINEL).all()), k


# ------------------------------------------------------------------ bad regions
@pytest.mark.parametrize("tail", [0, 1], ids=["vector-tail", "reference-tail"])
def test_a_bad_region_fails_alone(native, modes, tail):
    import torch
    from gkl_amd.errors import IllegalArgumentException
    m = modes(1, tail)
    reads, haps = m.host.regions[3]
    bad = PdhmmBatch.from_pairs(reads.pairs())
    bad.read_ins_qual = bad.read_ins_qual.copy()
    bad.read_ins_qual[11 * bad.max_read_len] = -1
    bad_db = native.PdhmmDeviceBatch.upload_cross(bad, haps, DEV)
    ks = [0, 3, 4]
    outs = [torch.full((m.pairs[k],), SENTINEL, dtype=torch.float64, device=DEV) for k in ks]
    sums = [torch.full((m.pairs[k],), SENTINEL, dtype=torch.float64, device=DEV) for k in ks]
    with pytest.raises(native.PdhmmMultiError) as e:
        m.ctx.compute_cross_multi_device([m.dbs[0], bad_db, m.dbs[4]], [m.ref_batch[k] for k in ks], outs=outs, sums=sums)
    assert e.value.statuses == [native.OK, native.ERR_INVALID_ARG, native.OK]
    assert isinstance(e.value.errors[1], IllegalArgumentException) and str(e.value.errors[1]) == INPUT_ERROR_TEXT
    assert e.value.errors[0] is None and e.value.errors[2] is None and e.value.results[1] is None
    torch.cuda.synchronize()
    assert bool((outs[1] == SENTINEL).all()) and bool((sums[1] == SENTINEL).all())
    m.assert_single_bytes([0, 4], [e.value.results[0], e.value.results[2]], [sums[0], sums[2]])
    # a region that fails the argument checks is left out before anything touches the device; the rest still run
    rdb, hdb = m.dbs[3]
    lengths = rdb.read_lengths.copy()
    lengths[0] = rdb.max_read_len + 1
    worse = (dataclasses.replace(rdb, read_lengths=lengths), hdb)
    outs = [torch.full((m.pairs[k],), SENTINEL, dtype=torch.float64, device=DEV) for k in (3, 1)]
    sums = [torch.full((m.pairs[k],), SENTINEL, dtype=torch.float64, device=DEV) for k in (3, 1)]
    with pytest.raises(native.PdhmmMultiError) as e:
        m.ctx.compute_cross_multi_device([worse, m.dbs[1]], [0, m.ref_batch[1]], outs=outs, sums=sums)
    assert e.value.statuses == [native.ERR_INVALID_ARG, native.OK] and "read_lengths[0]" in str(e.value.errors[0])
    torch.cuda.synchronize()
    assert bool((outs[0] == SENTINEL).all()) and bool((sums[0] == SENTINEL).all())
    m.assert_single_bytes([1], [e.value.results[1]], [sums[1]])
    # the context computes clean calls afterwards
    outs, sums = m.run([0, 1, 2])
    m.assert_single_bytes([0, 1, 2], outs, sums)


# ------------------------------------------------------------------ the interface
def test_sums_are_optional(modes):
    m = modes(1, 1)
    ks = [0, 1, 2, 3]
    regions, rb = [m.dbs[k] for k in ks], [m.ref_batch[k] for k in ks]
    m.assert_single_bytes(ks, m.ctx.compute_cross_multi_device(regions, rb))
    some = m.new_sums(ks)
    some[1] = some[3] = None
    m.assert_single_bytes(ks, m.ctx.compute_cross_multi_device(regions, rb, sums=some), some)


def test_ordered_behind_the_callers_stream(native, modes):
    # the inputs are still on their way -- asynchronous copies from pinned memory on a side stream -- when the call is made
    # with that stream: the library's work (the gather kernel first) waits for them
    import torch
    m = modes(1, 0)
    ks = [0, 3, 6]
    side = torch.cuda.Stream(device=DEV)
    pinned = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int8).reshape(-1)).pin_memory()  # noqa: E731
    host = []
    for k in ks:
        reads, haps = m.host.regions[k]
        host.append(([pinned(getattr(haps, n)) for n in ("hap_bases", "hap_pdbases")],
                     [pinned(getattr(reads, n)) for n in ("read_bases", "read_qual", "read_ins_qual", "read_del_qual", "gcp")]))
    sums = m.new_sums(ks)
    with torch.cuda.stream(side):
        regions = []
        for k, (hp, rp) in zip(ks, host):
            reads, haps = m.host.regions[k]
            regions.append((native.PdhmmDeviceBatch(reads.batch, 0, reads.max_read_len, None, tuple(t.to(DEV, non_blocking=True) for t in rp), None,
                                                    np.ascontiguousarray(reads.read_lengths, np.int64)),
                            native.PdhmmDeviceBatch(haps.batch, haps.max_hap_len, 0, tuple(t.to(DEV, non_blocking=True) for t in hp), None,
                                                    np.ascontiguousarray(haps.hap_lengths, np.int64), None)))
        outs = m.ctx.compute_cross_multi_device(regions, sums=sums, stream=side)
    m.assert_single_bytes(ks, outs, sums)


def test_interleaved_with_the_other_calls_on_one_context(native, modes):
    # host multi, device multi, host single, device single, device multi: every result is the first of its kind
    # (the forms share the context's input block, its sums and its pinned blocks)
    import torch
    m = modes(1, 1)
    h = m.host
    ks = [0, 2, 4, 6]
    with native.PdhmmContext(fma_mode=1, reference_tail=True) as c:
        rb = [m.ref_batch[k] for k in ks]
        host_multi = c.compute_cross_multi([h.regions[k] for k in ks], rb)
        assert [g.tobytes() for g in host_multi] == [h.single[k] for k in ks]
        sums = m.new_sums(ks)
        outs = c.compute_cross_multi_device([m.dbs[k] for k in ks], rb, sums=sums)
        m.assert_single_bytes(ks, outs, sums)
        assert c.compute_cross(*h.regions[2], m.ref_batch[2]).tobytes() == h.single[2]
        s = torch.empty(m.pairs[0], dtype=torch.float64, device=DEV)
        o = c.compute_cross_device(*m.dbs[0], m.ref_batch[0], sums=s)
        m.assert_single_bytes([0], [o], [s])
        sums = m.new_sums(ks)
        outs = c.compute_cross_multi_device([m.dbs[k] for k in ks], rb, sums=sums)
        m.assert_single_bytes(ks, outs, sums)
        assert [g.tobytes() for g in c.compute_cross_multi([h.regions[k] for k in ks], rb)] == [h.single[k] for k in ks]


def test_cross_check_build_agrees(native, modes):
    m = modes(1, 0)
    cxx = os.path.join(os.path.dirname(native.PDHMM_LIB_PATH), "libgklhip_pdhmm_cxx.so")
    assert os.path.exists(cxx), "make -C gkl_amd/csrc builds it"
    ks = [0, 1, 2]
    with native.PdhmmContext(fma_mode=1, reference_tail=False, lib_path=cxx) as c:
        sums = m.new_sums(ks)
        outs = c.compute_cross_multi_device([m.dbs[k] for k in ks], sums=sums)
        m.assert_single_bytes(ks, outs, sums)
        for k in ks:
            assert native.pdhmm_finalise_host(sums[k].cpu()).tobytes() == m.host.oracle[k]
    assert native.pdhmm_combine_counts(lib_path=cxx)[2] >= 1   # the cross-check build counted its own call


def test_argument_errors_are_the_host_multi_calls(native, modes):
    import torch
    m = modes(1, 1)
    lib = m.ctx.lib
    reads, haps = m.host.regions[1]
    rdb, hdb = m.dbs[1]
    keep = [np.ascontiguousarray(a, np.int8) for a in (haps.hap_bases, haps.hap_pdbases, reads.read_bases, reads.read_qual,
                                                       reads.read_ins_qual, reads.read_del_qual, reads.gcp)]
    shape = (reads.batch, haps.batch, haps.max_hap_len, reads.max_read_len)
    host_x = (native.CPdhmmCross * 1)(native.CPdhmmCross(*shape, *[a.ctypes.data for a in keep], hdb.hap_lengths.ctypes.data,
                                                         rdb.read_lengths.ctypes.data))
    dev_x = (native.CPdhmmCross * 1)(native.CPdhmmCross(*shape, *hdb.hap_pointers(), *rdb.read_pointers(), hdb.hap_lengths.ctypes.data,
                                                        rdb.read_lengths.ctypes.data))
    host_out = np.full(1, SENTINEL)
    dev_out = torch.full((1,), SENTINEL, dtype=torch.float64, device=DEV)
    host_ptrs, dev_ptrs = (C.c_void_p * 1)(host_out.ctypes.data), (C.c_void_p * 1)(dev_out.data_ptr())
    status = (C.c_int32 * 1)()
    m.run([0])
    before = (m.ctx.last_kernel_ms(), m.ctx.last_routing(), m.ctx.buffer_bytes(), native.pdhmm_combine_counts())

    def both(ctx, n, null_regions=False, null_out=False):
        res = []
        for device in (False, True):
            x, ptrs = (dev_x, dev_ptrs) if device else (host_x, host_ptrs)
            args = (ctx, n, None if null_regions else x, None, None if null_out else ptrs)
            st = (lib.gklhip_pdhmm_compute_cross_multi_device(*args, None, status, None) if device else
                  lib.gklhip_pdhmm_compute_cross_multi(*args, status))
            res.append((st, lib.gklhip_pdhmm_last_error().decode()))
        return res

    cases = [both(None, 1), both(m.ctx.handle, 0), both(m.ctx.handle, -3), both(m.ctx.handle, 1, null_regions=True),
             both(m.ctx.handle, 1, null_out=True)]
    for host, device in cases:
        assert host[0] == native.ERR_INVALID_ARG and device == host
    assert "context is NULL" in cases[0][0][1] and cases[1][0][1] == "no regions to process" and "is NULL" in cases[3][0][1]
    # a NULL out_dev[k] counts like a NULL out_host[k]: the region's own argument error
    null_entry = (C.c_void_p * 1)(None)
    st_host = lib.gklhip_pdhmm_compute_cross_multi(m.ctx.handle, 1, host_x, None, null_entry, status)
    host = (st_host, status[0], lib.gklhip_pdhmm_last_error().decode())
    st_dev = lib.gklhip_pdhmm_compute_cross_multi_device(m.ctx.handle, 1, dev_x, None, null_entry, None, status, None)
    assert (st_dev, status[0], lib.gklhip_pdhmm_last_error().decode()) == host and host[0] == native.ERR_INVALID_ARG
    assert host[2] == "Input arrays aren't valid."
    # nothing was launched or counted, nothing written
    assert (m.ctx.last_kernel_ms(), m.ctx.last_routing(), m.ctx.buffer_bytes(), native.pdhmm_combine_counts()) == before
    torch.cuda.synchronize()
    assert bool((dev_out == SENTINEL).all()) and host_out[0] == SENTINEL
    # the binding refuses lists of the wrong length and result tensors of the wrong size before the library sees them
    with pytest.raises(native.IllegalArgumentException):
        m.ctx.compute_cross_multi_device([m.dbs[0], m.dbs[1]], outs=[None])
    with pytest.raises(native.IllegalArgumentException):
        m.ctx.compute_cross_multi_device([m.dbs[0]], sums=[torch.empty(7, dtype=torch.float64, device=DEV)])

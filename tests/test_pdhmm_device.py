"""Device-resident PDHMM calls (gklhip_pdhmm_compute_device / _cross_device): inputs and results in HBM.

The check of every parity case: the raw sums the call leaves in HBM, finalised on the host
(native.pdhmm_finalise_host), are BYTE-identical to the host call's output on the same context -- the sums are the host
path's bit for bit -- and the device's own log10 values are within REL_TOL of it (the bar of the PairHMM device path,
tests/test_gpu_parity.py).  The largest absolute difference between the two is printed per case."""
import ctypes as C

import numpy as np
import pytest

from gkl_amd.pdhmm_batch import PdhmmBatch
from tests.test_gpu_parity import REL_TOL
from tests.test_pdhmm import cross_product, expand_cross, holders_fixture_batch, random_pd_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID_TEXT = "Error while calculating pdhmm. Input arrays aren't valid."


@pytest.fixture(scope="module")
def native():
    from gkl_amd import native as n
    return n


@pytest.fixture(scope="module", params=[1, 0], ids=["avx512-arith", "avx2-arith"])
def ctx(request, native):
    # the position-independent mode, like pd_ctx of tests/test_pdhmm.py
    with native.PdhmmContext(fma_mode=request.param, reference_tail=False) as c:
        c.fma_mode = request.param
        yield c


def assert_parity(native, host, out, sums, what=""):
    """host: the host call's array; out / sums: the device call's tensors."""
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert native.pdhmm_finalise_host(sums.cpu()).tobytes() == host.tobytes(), "the sums are not the host path's"
    assert got.shape == host.shape
    finite = np.isfinite(host)
    assert np.array_equal(got[~finite], host[~finite])
    diff = np.abs(got[finite] - host[finite])
    print(f"[pdhmm device] {what}: {host.size} pairs, max abs difference of the device log10 {diff.max() if diff.size else 0.0:.3e}")
    assert np.all(diff <= REL_TOL * np.abs(host[finite]))


def paired_both_ways(native, c, b, what=""):
    import torch
    host = c.compute(b)
    routing, db = c.last_routing(), native.PdhmmDeviceBatch.upload(b, DEV)
    sums = torch.empty(b.batch, dtype=torch.float64, device=DEV)
    out = c.compute_device(db, sums=sums)
    assert c.last_routing() == routing
    assert_parity(native, host, out, sums, what)
    return host, out


def cross_both_ways(native, c, reads, haps, ref_batch_pairs=0, what=""):
    import torch
    host = c.compute_cross(reads, haps, ref_batch_pairs)
    routing = c.last_routing()
    rdb, hdb = native.PdhmmDeviceBatch.upload_cross(reads, haps, DEV)
    sums = torch.empty(reads.batch * haps.batch, dtype=torch.float64, device=DEV)
    out = c.compute_cross_device(rdb, hdb, ref_batch_pairs, sums=sums)
    assert c.last_routing() == routing
    assert_parity(native, host, out, sums, what)
    return host, out


def cross_sides(seed, n_reads, n_haps, read_len, hap_len):
    """The two sides of tests.test_pdhmm.cross_product(RandomState(seed), ...): the same draws in the same order."""
    rng = np.random.RandomState(seed)
    reads = random_pd_batch(rng, n_reads, read_len=read_len, hap_len=(1, 2))
    haps = random_pd_batch(rng, n_haps, read_len=(1, 2), hap_len=hap_len)
    return reads, haps


# ------------------------------------------------------------------ paired
@pytest.mark.parametrize("kw", [dict(), dict(read_len=(1, 8), hap_len=(1, 6), flag_rate=0.6),
                                dict(read_len=(380, 390), hap_len=(60, 70)),   # straddles 384 bases: packed and striped jobs
                                dict(odd_haps=0.3)], ids=["defaults", "tiny", "around-384", "odd-haps"])
def test_paired_parity(native, ctx, kw):
    b = random_pd_batch(np.random.RandomState(77), 96, **kw)
    if "read_len" in kw and kw["read_len"][0] == 380:
        assert b.read_lengths.min() < 384 <= b.read_lengths.max()
    paired_both_ways(native, ctx, b, f"paired {kw}")


@pytest.mark.parametrize("fma_mode,width", [(1, 8), (0, 4)])
def test_paired_default_tail_mode(native, fma_mode, width):
    # the library's default: the last 101 mod width pairs take the scalar engine's arithmetic (tail jobs).  with_n=False as
    # in the tail-mode tests of tests/test_pdhmm.py: GKL's scalar engine rejects a non-ACGT read base under a SNP column
    b = random_pd_batch(np.random.RandomState(77), 101, with_n=False)
    assert 101 % width == (5 if fma_mode else 1)
    with native.PdhmmContext(fma_mode=fma_mode) as c:
        paired_both_ways(native, c, b, f"paired, reference tail, fma {fma_mode}")


# ------------------------------------------------------------------ cross
def test_cross_parity_position_independent(native, ctx):
    reads, haps = cross_sides(40, 40, 6, (1, 60), (1, 90))
    pairs = cross_product(np.random.RandomState(40), 40, 6, (1, 60), (1, 90))
    host, _ = cross_both_ways(native, ctx, reads, haps, what="cross 40 x 6")
    assert ctx.compute(pairs).tobytes() == host.tobytes()   # (position-independent: the expanded pairs give the same)


@pytest.mark.parametrize("fma_mode", [1, 0])
def test_cross_default_tail_mode_with_reference_batches(native, fma_mode):
    # batches of 13 pairs: 13 mod 8 = 5 (13 mod 4 = 1) scalar-arithmetic tail pairs per batch.  Reads without 'N' (see
    # test_paired_default_tail_mode), else the same draws as cross_product(RandomState(40), 40, 6, (1, 60), (1, 90))
    rng = np.random.RandomState(40)
    reads = random_pd_batch(rng, 40, read_len=(1, 60), hap_len=(1, 2), with_n=False)
    haps = random_pd_batch(rng, 6, read_len=(1, 2), hap_len=(1, 90), with_n=False)
    with native.PdhmmContext(fma_mode=fma_mode) as c:
        cross_both_ways(native, c, reads, haps, ref_batch_pairs=13, what=f"cross 40 x 6, batches of 13, fma {fma_mode}")


@pytest.mark.parametrize("fma_mode", [1, 0])
def test_cross_default_tail_mode_input_error_of_the_scalar_engine(native, fma_mode):
    # cross_product(RandomState(40), 40, 6, (1, 60), (1, 90)) itself in default tail mode with batches of 13: its reads hold
    # 'N' under SNP columns at tail positions, which GKL's scalar engine answers with PDHMM_INPUT_DATA_ERROR (the oracle:
    # compute_reference(..., ref_batch=13) returns status 2) -- the host call raises, and the device-resident call
    # raises the same and writes nothing
    import torch
    reads, haps = cross_sides(40, 40, 6, (1, 60), (1, 90))
    rdb, hdb = native.PdhmmDeviceBatch.upload_cross(reads, haps, DEV)
    out = torch.full((240,), 12345.0, dtype=torch.float64, device=DEV)
    sums = torch.full((240,), 12345.0, dtype=torch.float64, device=DEV)
    with native.PdhmmContext(fma_mode=fma_mode) as c:
        with pytest.raises(native.IllegalArgumentException) as host_error:
            c.compute_cross(reads, haps, 13)
        with pytest.raises(native.IllegalArgumentException) as device_error:
            c.compute_cross_device(rdb, hdb, 13, out=out, sums=sums)
        assert str(device_error.value) == str(host_error.value) == INVALID_TEXT
        torch.cuda.synchronize()
        assert bool((out == 12345.0).all()) and bool((sums == 12345.0).all())
        # position-independent mode on the same context: the same inputs are fine, and so is the context
        assert c.lib.gklhip_pdhmm_set_tail_mode(c.handle, 0) == 0
        cross_both_ways(native, c, reads, haps, ref_batch_pairs=13, what=f"cross 40 x 6 after an input error, fma {fma_mode}")


def test_cross_holders_fixture(native, ctx):
    reads, haps, _, _ = holders_fixture_batch()
    one = b"\0"
    r1 = PdhmmBatch.from_pairs([(one, one, r[0], r[1], r[2], r[3], r[4]) for r in reads])
    hb = PdhmmBatch.from_pairs([(h[0], h[1], one, one, one, one, one) for h in haps])
    assert (r1.batch, hb.batch) == (276, 48)
    cross_both_ways(native, ctx, r1, hb, what="holders fixture 276 x 48")


def test_cross_mixed_routing(native, ctx):
    # table-routed, predicate-routed and odd-base haplotypes in one call (as
    # test_pdhmm_gpu_cross_entry_point_with_odd_haplotype_bases builds them): the routing, decided from the haplotype
    # bytes the call reads back, is the host call's
    rng = np.random.RandomState(5)
    reads = random_pd_batch(rng, 70, read_len=(30, 151), hap_len=(1, 2), odd_haps=0.5)
    haps = random_pd_batch(rng, 9, read_len=(1, 2), hap_len=(100, 260), flag_rate=0.08, odd_haps=0.5)
    cross_both_ways(native, ctx, reads, haps, what="cross 70 x 9, mixed routing")
    routing = ctx.last_routing()
    assert sum(routing) == 9 and routing[2] > 0 and routing[0] + routing[1] > 0
    assert ctx.compute_cross(reads, haps).tobytes() == ctx.compute(expand_cross(reads, haps)).tobytes()


# ------------------------------------------------------------------ sizes of the finalisation kernel's grid
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_paired_sizes(native, ctx, n):
    paired_both_ways(native, ctx, random_pd_batch(np.random.RandomState(n), n), f"paired {n}")


def test_cross_one_by_one(native, ctx):
    reads, haps = cross_sides(1, 1, 1, (1, 60), (1, 90))
    cross_both_ways(native, ctx, reads, haps, what="cross 1 x 1")


def test_cross_above_the_pinned_sums_limit(native, ctx):
    # 132 000 pairs: just above the 131 072 up to which the host call's kernels store the sums into pinned memory
    reads, haps = cross_sides(400, 400, 330, (1, 4), (1, 4))
    assert reads.batch * haps.batch == 132000 > 131072
    cross_both_ways(native, ctx, reads, haps, what="cross 400 x 330")


# ------------------------------------------------------------------ the interface
def test_sums_none_gives_the_same_output(native, ctx):
    import torch
    b = random_pd_batch(np.random.RandomState(77), 96)
    db = native.PdhmmDeviceBatch.upload(b, DEV)
    sums = torch.empty(b.batch, dtype=torch.float64, device=DEV)
    with_sums = ctx.compute_device(db, sums=sums).cpu().numpy()
    assert ctx.compute_device(db).cpu().numpy().tobytes() == with_sums.tobytes()
    reads, haps = cross_sides(40, 40, 6, (1, 60), (1, 90))
    rdb, hdb = native.PdhmmDeviceBatch.upload_cross(reads, haps, DEV)
    xs = torch.empty(240, dtype=torch.float64, device=DEV)
    assert ctx.compute_cross_device(rdb, hdb).cpu().numpy().tobytes() == ctx.compute_cross_device(rdb, hdb, sums=xs).cpu().numpy().tobytes()


def test_input_error_leaves_the_results_untouched(native, ctx):
    import torch
    good = random_pd_batch(np.random.RandomState(5), 8)
    bad = random_pd_batch(np.random.RandomState(5), 8)
    bad.gcp[3] = -1
    assert bad.read_lengths[0] > 3   # (the byte is inside a read)
    out = torch.full((8,), 12345.0, dtype=torch.float64, device=DEV)
    sums = torch.full((8,), 12345.0, dtype=torch.float64, device=DEV)
    with pytest.raises(native.IllegalArgumentException) as e:
        ctx.compute_device(native.PdhmmDeviceBatch.upload(bad, DEV), out=out, sums=sums)
    assert str(e.value) == INVALID_TEXT
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all()) and bool((sums == 12345.0).all())
    # the cross form
    rdb, hdb = native.PdhmmDeviceBatch.upload_cross(bad, bad, DEV)
    xout = torch.full((64,), 12345.0, dtype=torch.float64, device=DEV)
    xsums = torch.full((64,), 12345.0, dtype=torch.float64, device=DEV)
    with pytest.raises(native.IllegalArgumentException) as e:
        ctx.compute_cross_device(rdb, hdb, out=xout, sums=xsums)
    assert str(e.value) == INVALID_TEXT
    torch.cuda.synchronize()
    assert bool((xout == 12345.0).all()) and bool((xsums == 12345.0).all())
    # the next device call and the next host call on the context are correct
    with native.PdhmmContext(fma_mode=ctx.fma_mode, reference_tail=False) as fresh:
        expected = fresh.compute(good)
    host, _ = paired_both_ways(native, ctx, good, "after an input error")
    assert host.tobytes() == expected.tobytes()


def test_ordered_behind_the_callers_stream(native, ctx):
    # the inputs are still on their way -- asynchronous copies from pinned memory on a side stream -- when the call is made
    # with that stream: the library's work waits for them
    import torch
    b = random_pd_batch(np.random.RandomState(9), 257, read_len=(40, 151), hap_len=(60, 200))
    host = ctx.compute(b)
    side = torch.cuda.Stream(device=DEV)
    pinned = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int8)).pin_memory()  # noqa: E731
    hp = [pinned(a) for a in (b.hap_bases, b.hap_pdbases)]
    rp = [pinned(a) for a in (b.read_bases, b.read_qual, b.read_ins_qual, b.read_del_qual, b.gcp)]
    sums = torch.empty(b.batch, dtype=torch.float64, device=DEV)
    with torch.cuda.stream(side):
        ht = tuple(t.to(DEV, non_blocking=True) for t in hp)
        rt = tuple(t.to(DEV, non_blocking=True) for t in rp)
        db = native.PdhmmDeviceBatch(b.batch, b.max_hap_len, b.max_read_len, ht, rt, np.ascontiguousarray(b.hap_lengths, np.int64),
                                     np.ascontiguousarray(b.read_lengths, np.int64))
        out = ctx.compute_device(db, sums=sums, stream=side)
    assert_parity(native, host, out, sums, "paired 257 behind a side stream")
    # ... and the cross form
    with torch.cuda.stream(side):
        rdb = native.PdhmmDeviceBatch(b.batch, 0, b.max_read_len, None, tuple(t.to(DEV, non_blocking=True) for t in rp), None, db.read_lengths)
        hdb = native.PdhmmDeviceBatch(9, b.max_hap_len, 0, tuple(t[:9 * b.max_hap_len].to(DEV, non_blocking=True) for t in hp), None,
                                      db.hap_lengths[:9].copy(), None)
        xsums = torch.empty(b.batch * 9, dtype=torch.float64, device=DEV)
        xout = ctx.compute_cross_device(rdb, hdb, sums=xsums, stream=side)
    assert_parity(native, ctx.compute_cross(b, b.subset(np.arange(9))), xout, xsums, "cross 257 x 9 behind a side stream")


def test_host_and_device_calls_interleaved(native, ctx):
    import torch
    small = random_pd_batch(np.random.RandomState(21), 50)
    big = random_pd_batch(np.random.RandomState(22), 700, read_len=(20, 200), hap_len=(30, 260))
    with native.PdhmmContext(fma_mode=ctx.fma_mode, reference_tail=False) as fresh:
        exp_small = fresh.compute(small)
    with native.PdhmmContext(fma_mode=ctx.fma_mode, reference_tail=False) as fresh:
        exp_big = fresh.compute(big)
    with native.PdhmmContext(fma_mode=ctx.fma_mode, reference_tail=False) as c:
        assert c.compute(small).tobytes() == exp_small.tobytes()                       # host
        s1 = torch.empty(big.batch, dtype=torch.float64, device=DEV)
        o1 = c.compute_device(native.PdhmmDeviceBatch.upload(big, DEV), sums=s1)       # device, larger
        assert_parity(native, exp_big, o1, s1, "interleaved: device, big")
        assert c.compute(big).tobytes() == exp_big.tobytes()                           # host
        s2 = torch.empty(small.batch, dtype=torch.float64, device=DEV)
        o2 = c.compute_device(native.PdhmmDeviceBatch.upload(small, DEV), sums=s2)     # device
        assert_parity(native, exp_small, o2, s2, "interleaved: device, small")
        assert c.compute(small).tobytes() == exp_small.tobytes()


def test_argument_errors_are_the_host_calls(native, ctx):
    import torch
    lib, b = ctx.lib, random_pd_batch(np.random.RandomState(5), 8)
    host_arrays = [np.ascontiguousarray(a, np.int8) for a in (b.hap_bases, b.hap_pdbases, b.read_bases, b.read_qual, b.read_ins_qual,
                                                              b.read_del_qual, b.gcp)]
    db = native.PdhmmDeviceBatch.upload(b, DEV)
    out = torch.full((64,), 12345.0, dtype=torch.float64, device=DEV)
    host_out = np.empty(64)
    ctx.compute(b)
    before = (ctx.last_kernel_ms(), ctx.last_routing(), ctx.buffer_bytes())

    def both(hl, rl, ref_batch_pairs=None, null_out=False):
        """(status, text) of the host call and of the device call with the same arguments."""
        hl, rl = np.ascontiguousarray(hl, np.int64), np.ascontiguousarray(rl, np.int64)
        res = []
        for device in (False, True):
            ptrs = (db.hap_pointers() + db.read_pointers()) if device else [a.ctypes.data for a in host_arrays]
            o = None if null_out else (out.data_ptr() if device else host_out.ctypes.data)
            if ref_batch_pairs is None:
                cb = native.CPdhmmBatch(b.batch, b.max_hap_len, b.max_read_len, *ptrs, hl.ctypes.data, rl.ctypes.data)
                st = (lib.gklhip_pdhmm_compute_device(ctx.handle, C.byref(cb), o, None, None) if device else
                      lib.gklhip_pdhmm_compute(ctx.handle, C.byref(cb), o))
            else:
                cb = native.CPdhmmCross(b.batch, b.batch, b.max_hap_len, b.max_read_len, *ptrs, hl.ctypes.data, rl.ctypes.data)
                st = (lib.gklhip_pdhmm_compute_cross_device(ctx.handle, C.byref(cb), ref_batch_pairs, o, None, None) if device else
                      lib.gklhip_pdhmm_compute_cross_batched(ctx.handle, C.byref(cb), ref_batch_pairs, o))
            res.append((st, lib.gklhip_pdhmm_last_error().decode()))
        return res

    zero, long_ = b.hap_lengths.copy(), b.read_lengths.copy()
    zero[2], long_[5] = 0, b.max_read_len + 1
    cases = [both(b.hap_lengths, b.read_lengths, null_out=True), both(b.hap_lengths, b.read_lengths, 0, null_out=True),
             both(zero, b.read_lengths), both(b.hap_lengths, long_), both(zero, b.read_lengths, 0), both(b.hap_lengths, long_, 0),
             both(b.hap_lengths, b.read_lengths, -1)]
    for host, device in cases:
        assert host[0] == native.ERR_INVALID_ARG and device == host
    assert cases[0][1][1] == "Input arrays aren't valid." and "hap_lengths[2] = 0" in cases[2][1][1]
    assert "read_lengths[5]" in cases[3][1][1] and cases[6][1][1] == "ref_batch_pairs must not be negative"
    # nothing was launched: the context reports its last good call, and the output is untouched
    assert (ctx.last_kernel_ms(), ctx.last_routing(), ctx.buffer_bytes()) == before
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())
    # the binding refuses result tensors of the wrong size or kind before the library sees them
    with pytest.raises(native.IllegalArgumentException):
        ctx.compute_device(db, out=torch.empty(7, dtype=torch.float64, device=DEV))
    with pytest.raises(native.IllegalArgumentException):
        ctx.compute_device(db, sums=torch.empty(8, dtype=torch.float32, device=DEV))

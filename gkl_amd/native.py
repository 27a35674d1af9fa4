"""ctypes binding of the C ABI (include/gkl_hip_pairhmm.h) -- the only way Python reaches
the HIP kernels.  There is no fallback: if ``libgklhip_pairhmm.so`` is missing or no
gfx950 device is visible, everything here raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .batch import FlatBatch
from .errors import IllegalArgumentException, OutOfMemoryError, RuntimeException

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libgklhip_pairhmm.so")

ABI_VERSION = 2
OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_OOM, ERR_HIP, ERR_UNSUPPORTED = range(6)
FINALIZE_REFERENCE_HOST, FINALIZE_DEVICE_F64, FINALIZE_DEVICE_REF32 = 0, 1, 2

_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("use_double", C.c_int32),
                ("max_threads", C.c_int32), ("fma_mode", C.c_int32), ("finalize", C.c_int32),
                ("record_events", C.c_int32), ("rows_per_lane", C.c_int32)]


class CBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_haps", C.c_int32), ("read_off", _i64p), ("hap_off", _i64p),
                ("read_bases", C.c_void_p), ("read_quals", C.c_void_p), ("ins_gop", C.c_void_p),
                ("del_gop", C.c_void_p), ("gcp", C.c_void_p), ("hap_bases", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_fallback", C.c_int64), ("cells", C.c_int64),
                ("cells_fp64", C.c_int64), ("n_chunks", C.c_int32), ("n_hap_groups", C.c_int32),
                ("rows_per_lane", C.c_int32), ("n_long_pairs", C.c_int32), ("ms_fwd_main", C.c_float),
                ("ms_fwd_fallback", C.c_float), ("ms_total_device", C.c_float), ("lane_fill", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SERVER_MAX_DEVICES = 16


class ServerInfo(C.Structure):
    """gklhip_server_info: the PairHMM server's counters (gklhip_server_stats)."""
    _fields_ = [("protocol", C.c_int32), ("pid", C.c_int32), ("calls_served", C.c_int64), ("calls_failed", C.c_int64),
                ("calls_active", C.c_int32), ("live_connections", C.c_int32), ("connections_total", C.c_int64),
                ("arenas_registered", C.c_int64), ("arenas_copied", C.c_int64), ("requests_refused", C.c_int64),
                ("n_devices", C.c_int32), ("reserved", C.c_int32), ("device", C.c_int32 * SERVER_MAX_DEVICES),
                ("connections", C.c_int32 * SERVER_MAX_DEVICES), ("small_calls", (C.c_int64 * 3) * SERVER_MAX_DEVICES)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_[:10]}
        k = self.n_devices
        d["devices"] = list(self.device[:k])
        d["connections_per_device"] = list(self.connections[:k])
        d["small_call_counts"] = [tuple(int(x) for x in self.small_calls[i]) for i in range(k)]
        return d


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen the product library; raises (never falls back) when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    try:
        # PyTorch-ROCm wheels bundle their own libamdhip64; whichever HIP runtime is loaded
        # first owns the device, so let torch's load first and share it (torch is only used
        # for device memory / streams / torch.distributed, never for compute).
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeException(f"{p} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.gklhip_abi_version.restype = C.c_int
    lib.gklhip_device_count.restype = C.c_int
    lib.gklhip_strerror.restype = C.c_char_p
    lib.gklhip_strerror.argtypes = [C.c_int]
    lib.gklhip_last_error.restype = C.c_char_p
    lib.gklhip_init.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.gklhip_init.restype = C.c_int
    lib.gklhip_init_devices.argtypes = [C.POINTER(Config), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
    lib.gklhip_init_devices.restype = C.c_int
    lib.gklhip_num_devices.argtypes = [C.c_void_p]
    lib.gklhip_num_devices.restype = C.c_int
    lib.gklhip_gather_backend.argtypes = [C.c_void_p]
    lib.gklhip_gather_backend.restype = C.c_int
    lib.gklhip_measure_issue_ceiling.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.gklhip_measure_issue_ceiling.restype = C.c_int
    lib.gklhip_small_call_counts.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int]
    lib.gklhip_release_idle.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.gklhip_release_idle.restype = C.c_int
    lib.gklhip_fault_inject.argtypes = [C.c_char_p]
    lib.gklhip_fault_inject.restype = C.c_int
    lib.gklhip_small_call_counts.restype = C.c_int
    if hasattr(lib, "gklhip_set_small_read_limit"):   # (absent from an older build loaded by path for an A/B)
        lib.gklhip_set_small_read_limit.argtypes = [C.c_void_p, C.c_int32]
        lib.gklhip_set_small_read_limit.restype = C.c_int
    if hasattr(lib, "gklhip_set_mid_combine"):        # (likewise)
        lib.gklhip_set_mid_combine.argtypes = [C.c_void_p, C.c_int]
        lib.gklhip_set_mid_combine.restype = C.c_int
    lib.gklhip_gather_note.argtypes = [C.c_void_p]
    lib.gklhip_gather_note.restype = C.c_char_p
    lib.gklhip_partition_reads.argtypes = [C.c_int32, _i64p, C.c_int32, C.POINTER(C.c_int32)]
    lib.gklhip_partition_reads.restype = C.c_int
    lib.gklhip_rccl_selftest.argtypes = [C.c_int32]
    lib.gklhip_rccl_selftest.restype = C.c_int
    lib.gklhip_done.argtypes = [C.c_void_p]
    lib.gklhip_done.restype = C.c_int
    lib.gklhip_compute.argtypes = [C.c_void_p, C.POINTER(CBatch), C.c_void_p]
    lib.gklhip_compute.restype = C.c_int
    lib.gklhip_compute_device.argtypes = [C.c_void_p, C.POINTER(CBatch), C.c_void_p, C.c_void_p]
    lib.gklhip_compute_device.restype = C.c_int
    lib.gklhip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    lib.gklhip_get_step_times.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.POINTER(C.c_float)]
    lib.gklhip_get_step_times.restype = C.c_int
    lib.gklhip_get_stats.restype = C.c_int
    lib.gklhip_get_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gklhip_get_raw.restype = C.c_int
    lib.gklhip_compute_multi.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CBatch), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.gklhip_compute_multi.restype = C.c_int
    if hasattr(lib, "gklhip_compute_multi_device"):   # (absent from an older build loaded by path for an A/B)
        lib.gklhip_compute_multi_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CBatch), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_void_p]
        lib.gklhip_compute_multi_device.restype = C.c_int
    lib.gklhip_get_raw_region.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gklhip_get_raw_region.restype = C.c_int
    lib.gklhip_get_table_f32.argtypes = [C.c_int, C.c_void_p, C.c_int64]
    lib.gklhip_get_table_f32.restype = C.c_int64
    lib.gklhip_get_table_f64.argtypes = [C.c_int, C.c_void_p, C.c_int64]
    lib.gklhip_get_table_f64.restype = C.c_int64
    lib.gklhip_connect.argtypes = [C.c_char_p, C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.gklhip_connect.restype = C.c_int
    lib.gklhip_is_remote.argtypes = [C.c_void_p]
    lib.gklhip_is_remote.restype = C.c_int
    lib.gklhip_server_stats.argtypes = [C.c_char_p, C.POINTER(ServerInfo)]
    lib.gklhip_server_stats.restype = C.c_int
    if lib.gklhip_abi_version() != ABI_VERSION:
        raise RuntimeException("libgklhip_pairhmm.so ABI mismatch")
    if path is None:
        _lib = lib
    return lib


def _exception(lib, status: int, msg: str):
    if status == ERR_INVALID_ARG:
        return IllegalArgumentException(msg)
    if status == ERR_OOM:
        return OutOfMemoryError(msg)
    return RuntimeException(f"{lib.gklhip_strerror(status).decode()}: {msg}")


def _raise(lib, status: int):
    msg = (lib.gklhip_last_error() or b"").decode() or lib.gklhip_strerror(status).decode()
    raise _exception(lib, status, msg)


class PairHmmMultiError(Exception):
    """compute_multi: some regions failed.  results[k] is region k's array or None, statuses[k] its status code,
    errors[k] the exception a single call would have raised (None for a region that succeeded); status is what
    gklhip_compute_multi returned (the first failing region's status)."""

    def __init__(self, results, statuses, errors, status):
        first = next(e for e in errors if e is not None)
        super().__init__(f"{sum(e is not None for e in errors)} of {len(errors)} regions failed; the first: {first}")
        self.results, self.statuses, self.errors, self.status = results, statuses, errors, int(status)


def host_table(which: int, dtype) -> np.ndarray:
    """Lookup tables exactly as the library uploads them (0 ph2pr, 1 matchToMatch, 2 ph2pr/3)."""
    lib = load_library()
    if np.dtype(dtype) == np.float32:
        n = lib.gklhip_get_table_f32(which, None, 0)
        a = np.empty(n, np.float32)
        lib.gklhip_get_table_f32(which, a.ctypes.data, n)
    else:
        n = lib.gklhip_get_table_f64(which, None, 0)
        a = np.empty(n, np.float64)
        lib.gklhip_get_table_f64(which, a.ctypes.data, n)
    return a


@dataclass
class DeviceBatch:
    """A FlatBatch whose byte arrays live in HBM (torch uint8 tensors own the memory)."""
    host: FlatBatch
    tensors: tuple  # read_bases, read_quals, ins, del, gcp, hap_bases
    read_off: np.ndarray
    hap_off: np.ndarray

    @staticmethod
    def upload(batch: FlatBatch, device="cuda:0") -> "DeviceBatch":
        import torch
        ts = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in
                   (batch.read_bases, batch.read_quals, batch.ins_gop, batch.del_gop, batch.gcp,
                    batch.hap_bases))
        return DeviceBatch(batch, ts, np.ascontiguousarray(batch.read_off, np.int64),
                           np.ascontiguousarray(batch.hap_off, np.int64))

    def c_batch(self) -> CBatch:
        t = self.tensors
        return CBatch(self.host.n_reads, self.host.n_haps, self.read_off.ctypes.data_as(_i64p),
                      self.hap_off.ctypes.data_as(_i64p), *[x.data_ptr() for x in t])


class PinnedBatch:
    """A FlatBatch whose six byte arrays live in page-locked memory from gklhip_host_alloc -- what the JNI shim's
    marshalling arenas are (jni_shim.cpp), so that gklhip_compute's host-to-device copies are plain DMA."""

    def __init__(self, batch: FlatBatch):
        import dataclasses
        lib = load_library()
        lib.gklhip_host_alloc.restype = C.c_void_p
        lib.gklhip_host_alloc.argtypes = [C.c_size_t]
        lib.gklhip_host_free.argtypes = [C.c_void_p]
        self._lib, self._ptrs, arrays = lib, [], {}
        for name in ("read_bases", "read_quals", "ins_gop", "del_gop", "gcp", "hap_bases"):
            src = np.ascontiguousarray(getattr(batch, name), np.uint8)
            p = lib.gklhip_host_alloc(max(1, src.size))
            if not p:
                raise OutOfMemoryError("gklhip_host_alloc failed")
            self._ptrs.append(p)
            dst = np.ctypeslib.as_array((C.c_uint8 * max(1, src.size)).from_address(p))[:src.size]
            dst[:] = src
            arrays[name] = dst
        self.batch = dataclasses.replace(batch, **arrays)

    def close(self):
        for p in self._ptrs:
            self._lib.gklhip_host_free(p)
        self._ptrs = []

    def __enter__(self):
        return self.batch

    def __exit__(self, *a):
        self.close()


def partition_reads(read_off, n_parts: int):
    """The library's sharding rule (gklhip_partition_reads): boundaries of contiguous read ranges balanced by cells."""
    lib = load_library()
    ro = np.ascontiguousarray(read_off, np.int64)
    bounds = (C.c_int32 * (n_parts + 1))()
    st = lib.gklhip_partition_reads(ro.size - 1, ro.ctypes.data_as(_i64p), n_parts, bounds)
    if st != OK:
        _raise(lib, st)
    return list(bounds)


def small_call_counts(device: int = 0, reset: bool = False):
    """(small host-buffer calls, those launched together with other threads' calls, sets of launches) on `device`."""
    lib = load_library()
    out = (C.c_int64 * 3)()
    st = lib.gklhip_small_call_counts(int(device), out, 1 if reset else 0)
    if st != OK:
        _raise(lib, st)
    return int(out[0]), int(out[1]), int(out[2])


def server_stats(socket_path: str) -> dict:
    """Counters of the PairHMM server on `socket_path` (gklhip_server_stats): calls served, live connections,
    connections and small-call counts per device, arenas registered in place versus copied.  Makes no HIP call."""
    lib = load_library()
    info = ServerInfo()
    st = lib.gklhip_server_stats(os.fsencode(socket_path), C.byref(info))
    if st != OK:
        _raise(lib, st)
    return info.as_dict()


def rccl_selftest(device: int = 0) -> None:
    lib = load_library()
    st = lib.gklhip_rccl_selftest(device)
    if st != OK:
        _raise(lib, st)


class PairHmmContext:
    """One gklhip context (= one initNative).  `devices` = a list of device ordinals: every call is sharded over
    them inside the library (a device may appear twice).  `server` = the socket of a PairHMM server
    (gkl_amd.server): a client context whose calls that server computes (gklhip_connect; this process makes no HIP
    call for it).  GKL_HIP_SERVER in the environment makes every context without `devices` a client context."""

    def __init__(self, use_double: bool = False, max_threads: int = 0, device: int = -1,
                 fma_mode: int = 1, finalize: int = -1, record_events: bool = False,
                 rows_per_lane: int = 0, lib_path: Optional[str] = None, devices=None, server: Optional[str] = None,
                 small_read_limit: Optional[int] = None):
        self.lib = load_library(lib_path)
        cfg = Config(ABI_VERSION, device, int(use_double), int(max_threads), int(fma_mode),
                     int(finalize), int(record_events), int(rows_per_lane))
        h = C.c_void_p()
        if server is not None:
            if devices:
                raise IllegalArgumentException("a client context of a server takes no device list")
            st = self.lib.gklhip_connect(os.fsencode(server), C.byref(cfg), C.byref(h))
        elif devices:
            arr = (C.c_int32 * len(devices))(*devices)
            st = self.lib.gklhip_init_devices(C.byref(cfg), arr, len(devices), C.byref(h))
        else:
            st = self.lib.gklhip_init(C.byref(cfg), C.byref(h))
        if st != OK:
            _raise(self.lib, st)
        self.handle = h
        self.use_double = bool(use_double)
        if small_read_limit is not None:
            try:
                self.set_small_read_limit(small_read_limit)
            except Exception:
                self.close()
                raise

    @property
    def n_devices(self) -> int:
        return self.lib.gklhip_num_devices(self.handle)

    @property
    def is_remote(self) -> bool:
        """True for a client context of a PairHMM server."""
        return bool(self.lib.gklhip_is_remote(self.handle))

    @property
    def gather_backend(self) -> str:
        """none | peer | rccl (lazily created: before the first device-resident call, what it will try) |
        peer-after-rccl-failure (gather_note says why)"""
        return ("none", "peer", "rccl", "peer-after-rccl-failure")[self.lib.gklhip_gather_backend(self.handle)]

    def set_small_read_limit(self, max_read_len: int) -> None:
        """The longest read of a region that takes the small-call path (gklhip_set_small_read_limit): 383, the default,
        or 511.  New contexts start from GKL_HIP_SMALL_READ_LIMIT; a client context of a server cannot set it."""
        st = self.lib.gklhip_set_small_read_limit(self.handle, int(max_read_len))
        if st != OK:
            _raise(self.lib, st)

    def set_mid_combine(self, on: bool) -> None:
        """Whether this context's mid-size single calls (2049 - 65 536 pairs) enter the small-call combiner and share
        sets of launches with those of concurrent callers (gklhip_set_mid_combine): off by default.  New contexts start
        from GKL_HIP_COMBINE_MID; a client context of a server cannot set it."""
        st = self.lib.gklhip_set_mid_combine(self.handle, 1 if on else 0)
        if st != OK:
            _raise(self.lib, st)

    def release_idle(self) -> int:
        """Give back the streams / twin engines the context holds only for speed, if it is idle (gklhip_release_idle);
        returns how many streams went."""
        n = C.c_int32(0)
        st = self.lib.gklhip_release_idle(self.handle, C.byref(n))
        if st != OK:
            _raise(self.lib, st)
        return int(n.value)

    def issue_ceiling(self, use_double: bool = False, ms_budget: float = 50.0):
        """(cells per second of the recurrence's bare instruction mix, sustained clock in GHz) -- diagnostics."""
        cells, clk = C.c_double(0.0), C.c_double(0.0)
        st = self.lib.gklhip_measure_issue_ceiling(self.handle, 1 if use_double else 0, float(ms_budget), C.byref(cells), C.byref(clk))
        if st != OK:
            _raise(self.lib, st)
        return cells.value, clk.value

    @property
    def gather_note(self) -> str:
        return (self.lib.gklhip_gather_note(self.handle) or b"").decode()

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gklhip_done(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- host buffers in / out: what the JNI shim does --
    def compute(self, batch: FlatBatch, out: Optional[np.ndarray] = None) -> np.ndarray:
        n = batch.n_pairs
        if out is None:
            out = np.empty(n, np.float64)
        if out.dtype != np.float64 or out.size < n or not out.flags.c_contiguous:
            raise IllegalArgumentException("likelihood array must be contiguous float64 of n_reads*n_haps")
        keep = [np.ascontiguousarray(a, np.uint8) for a in
                (batch.read_bases, batch.read_quals, batch.ins_gop, batch.del_gop, batch.gcp,
                 batch.hap_bases)]
        ro = np.ascontiguousarray(batch.read_off, np.int64)
        ho = np.ascontiguousarray(batch.hap_off, np.int64)
        cb = CBatch(batch.n_reads, batch.n_haps, ro.ctypes.data_as(_i64p), ho.ctypes.data_as(_i64p),
                    *[a.ctypes.data for a in keep])
        st = self.lib.gklhip_compute(self.handle, C.byref(cb), out.ctypes.data)
        if st != OK:
            _raise(self.lib, st)
        return out

    def compute_multi(self, batches) -> list:
        """Several region calls in shared sets of launches (gklhip_compute_multi): the GATK-sized regions of up to 2048
        pairs among themselves, the mid-size ones of up to 65 536 pairs among themselves.  batches is a list of
        FlatBatch; returns the list of their likelihood arrays, each byte for byte what compute() returns for it alone.
        When regions fail, the others are still computed: PairHmmMultiError carries their arrays and every region's
        status and exception."""
        n = len(batches)
        keep, cbs, outs = [], (CBatch * max(n, 1))(), []
        for k, b in enumerate(batches):
            arrs = [np.ascontiguousarray(a, np.uint8) for a in (b.read_bases, b.read_quals, b.ins_gop, b.del_gop, b.gcp, b.hap_bases)]
            ro = np.ascontiguousarray(b.read_off, np.int64)
            ho = np.ascontiguousarray(b.hap_off, np.int64)
            keep.append((arrs, ro, ho))
            cbs[k] = CBatch(b.n_reads, b.n_haps, ro.ctypes.data_as(_i64p), ho.ctypes.data_as(_i64p), *[a.ctypes.data for a in arrs])
            outs.append(np.empty(max(b.n_reads * b.n_haps, 0), np.float64))
        out_ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        status = (C.c_int32 * max(n, 1))()
        st = self.lib.gklhip_compute_multi(self.handle, n, cbs, out_ptrs, status)
        if st == OK:
            return outs
        if n <= 0 or all(status[k] == OK for k in range(n)):
            _raise(self.lib, st)   # the call itself was refused
        # the library keeps the first failing region's message; the others get their status's text
        msg = (self.lib.gklhip_last_error() or b"").decode()
        first = next(k for k in range(n) if status[k] != OK)
        errors = [None if status[k] == OK else _exception(self.lib, status[k], msg if k == first else f"region {k} failed with status {status[k]}")
                  for k in range(n)]
        raise PairHmmMultiError([o if status[k] == OK else None for k, o in enumerate(outs)], [int(status[k]) for k in range(n)], errors, st)

    # -- everything resident in HBM; `out` is a torch float64 CUDA tensor --
    def compute_device(self, dbatch: DeviceBatch, out=None, stream=None):
        import torch
        n = dbatch.host.n_pairs
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=dbatch.tensors[0].device)
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        cb = dbatch.c_batch()
        st = self.lib.gklhip_compute_device(self.handle, C.byref(cb), out.data_ptr(), stream.cuda_stream)
        if st != OK:
            _raise(self.lib, st)
        return out

    def compute_multi_device(self, dbatches, outs=None, stream=None) -> list:
        """compute_multi for regions resident in HBM (gklhip_compute_multi_device; synchronous).  dbatches is a list of
        DeviceBatch; returns the list of their torch float64 tensors, each byte for byte what compute_device() writes
        for it alone.  outs, if given, is a list of float64 CUDA tensors of n_reads * n_haps elements on the context's
        device (an entry may be None: the region then fails as one without an output array does); stream defaults to the
        current torch stream.  When regions fail, the others are still computed: PairHmmMultiError carries their tensors
        (None for a failed region) and every region's status and exception."""
        import torch
        n = len(dbatches)
        if outs is None:
            outs = [torch.empty(d.host.n_pairs, dtype=torch.float64, device=d.tensors[0].device) for d in dbatches]
        outs = list(outs)
        if len(outs) != n:
            raise IllegalArgumentException("one output tensor per region")
        for d, o in zip(dbatches, outs):
            if o is not None and (o.dtype != torch.float64 or not o.is_cuda or o.numel() < d.host.n_pairs or not o.is_contiguous()):
                raise IllegalArgumentException("likelihood tensor must be a contiguous float64 CUDA tensor of n_reads*n_haps")
        if stream is None:
            dev = next((o.device for o in outs if o is not None), None)
            stream = torch.cuda.current_stream(dev)
        cbs = (CBatch * max(n, 1))()
        for k, d in enumerate(dbatches):
            cbs[k] = d.c_batch()
        out_ptrs = (C.c_void_p * max(n, 1))(*[None if o is None else o.data_ptr() for o in outs])
        status = (C.c_int32 * max(n, 1))()
        st = self.lib.gklhip_compute_multi_device(self.handle, n, cbs, out_ptrs, status, stream.cuda_stream)
        if st == OK:
            return outs
        if n <= 0 or all(status[k] == OK for k in range(n)):
            _raise(self.lib, st)   # the call itself was refused
        msg = (self.lib.gklhip_last_error() or b"").decode()
        first = next(k for k in range(n) if status[k] != OK)
        errors = [None if status[k] == OK else _exception(self.lib, status[k], msg if k == first else f"region {k} failed with status {status[k]}")
                  for k in range(n)]
        raise PairHmmMultiError([o if status[k] == OK else None for k, o in enumerate(outs)], [int(status[k]) for k in range(n)], errors, st)

    def step_times(self, steps_back: int = 0):
        """record_events=2 contexts: (ms_main, ms_fallback, ms_total_device) of the call `steps_back` calls ago."""
        a, b, t = C.c_float(0), C.c_float(0), C.c_float(0)
        st = self.lib.gklhip_get_step_times(self.handle, int(steps_back), C.byref(a), C.byref(b), C.byref(t))
        if st != OK:
            _raise(self.lib, st)
        return a.value, b.value, t.value

    def stats(self) -> dict:
        s = Stats()
        st = self.lib.gklhip_get_stats(self.handle, C.byref(s))
        if st != OK:
            _raise(self.lib, st)
        return s.as_dict()

    def raw(self, n_pairs: int):
        """Raw scaled sums of the last call: (raw32, raw64, used64)."""
        r32 = np.zeros(n_pairs, np.float32)
        r64 = np.zeros(n_pairs, np.float64)
        u = np.zeros(n_pairs, np.uint8)
        st = self.lib.gklhip_get_raw(self.handle, r32.ctypes.data, r64.ctypes.data, u.ctypes.data)
        if st != OK:
            _raise(self.lib, st)
        return r32, r64, u

    def raw_region(self, k: int, n_pairs: int):
        """Raw scaled sums of region k of the last compute_multi call: (raw32, raw64, used64)."""
        r32 = np.zeros(n_pairs, np.float32)
        r64 = np.zeros(n_pairs, np.float64)
        u = np.zeros(n_pairs, np.uint8)
        st = self.lib.gklhip_get_raw_region(self.handle, int(k), r32.ctypes.data, r64.ctypes.data, u.ctypes.data)
        if st != OK:
            _raise(self.lib, st)
        return r32, r64, u


# ---------------------------------------------------------------- PDHMM (include/gkl_hip_pdhmm.h)
PDHMM_LIB_PATH = os.environ.get("GKL_AMD_PDHMM_LIB") or os.path.join(LIB_DIR, "libgklhip_pdhmm.so")   # the variable: A/B of library builds (dev tool)


class CPdhmmBatch(C.Structure):
    _fields_ = [("batch", C.c_int32), ("max_hap_len", C.c_int32), ("max_read_len", C.c_int32),
                ("hap_bases", C.c_void_p), ("hap_pdbases", C.c_void_p), ("read_bases", C.c_void_p),
                ("read_qual", C.c_void_p), ("read_ins_qual", C.c_void_p), ("read_del_qual", C.c_void_p),
                ("gcp", C.c_void_p), ("hap_lengths", C.c_void_p), ("read_lengths", C.c_void_p)]


class CPdhmmCross(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_haps", C.c_int32), ("max_hap_len", C.c_int32), ("max_read_len", C.c_int32),
                ("hap_bases", C.c_void_p), ("hap_pdbases", C.c_void_p), ("read_bases", C.c_void_p),
                ("read_qual", C.c_void_p), ("read_ins_qual", C.c_void_p), ("read_del_qual", C.c_void_p),
                ("gcp", C.c_void_p), ("hap_lengths", C.c_void_p), ("read_lengths", C.c_void_p)]


class PdhmmServerInfo(C.Structure):
    """gklhip_pdhmm_server_info: the server's PDHMM counters (gklhip_pdhmm_server_stats)."""
    _fields_ = [("protocol", C.c_int32), ("pid", C.c_int32), ("library_state", C.c_int32), ("reserved0", C.c_int32),
                ("calls_served", C.c_int64), ("calls_failed", C.c_int64), ("calls_active", C.c_int32),
                ("live_connections", C.c_int32), ("connections_total", C.c_int64), ("pairs_served", C.c_int64),
                ("combine_counts", C.c_int64 * 3), ("reserved", C.c_int64 * 6)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}
        d["combine_counts"] = tuple(int(v) for v in self.combine_counts)
        return d


_pd_lib = None


def load_pdhmm_library(path: Optional[str] = None):
    global _pd_lib
    if _pd_lib is not None and path is None:
        return _pd_lib
    p = path or PDHMM_LIB_PATH
    try:
        import torch  # noqa: F401  (HIP runtime load order, see load_library)
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeException(f"{p} is not built (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.gklhip_pdhmm_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.gklhip_pdhmm_init.restype = C.c_int
    lib.gklhip_pdhmm_set_fma_mode.argtypes = [C.c_void_p, C.c_int]
    lib.gklhip_pdhmm_set_fma_mode.restype = C.c_int
    lib.gklhip_pdhmm_set_tail_mode.argtypes = [C.c_void_p, C.c_int]
    lib.gklhip_pdhmm_set_tail_mode.restype = C.c_int
    lib.gklhip_pdhmm_compute.argtypes = [C.c_void_p, C.POINTER(CPdhmmBatch), C.c_void_p]
    lib.gklhip_pdhmm_compute.restype = C.c_int
    lib.gklhip_pdhmm_compute_cross.argtypes = [C.c_void_p, C.POINTER(CPdhmmCross), C.c_void_p]
    lib.gklhip_pdhmm_compute_cross.restype = C.c_int
    lib.gklhip_pdhmm_compute_cross_batched.argtypes = [C.c_void_p, C.POINTER(CPdhmmCross), C.c_int64, C.c_void_p]
    lib.gklhip_pdhmm_compute_cross_batched.restype = C.c_int
    lib.gklhip_pdhmm_compute_cross_multi.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CPdhmmCross), C.POINTER(C.c_int64),
                                                     C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.gklhip_pdhmm_compute_cross_multi.restype = C.c_int
    lib.gklhip_pdhmm_combine_counts.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int]
    lib.gklhip_pdhmm_combine_counts.restype = C.c_int
    lib.gklhip_pdhmm_reference_batch_pairs.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    lib.gklhip_pdhmm_reference_batch_pairs.restype = C.c_int64
    lib.gklhip_pdhmm_available_memory_mb.argtypes = [C.c_int32]
    lib.gklhip_pdhmm_available_memory_mb.restype = C.c_int32
    lib.gklhip_pdhmm_done.argtypes = [C.c_void_p]
    lib.gklhip_pdhmm_done.restype = C.c_int
    lib.gklhip_pdhmm_last_kernel_ms.argtypes = [C.c_void_p]
    lib.gklhip_pdhmm_last_kernel_ms.restype = C.c_float
    lib.gklhip_pdhmm_buffer_bytes.argtypes = [C.c_void_p]
    lib.gklhip_pdhmm_buffer_bytes.restype = C.c_int64
    lib.gklhip_pdhmm_last_routing.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.gklhip_pdhmm_last_routing.restype = C.c_int
    lib.gklhip_pdhmm_get_table.argtypes = [C.c_int, C.c_void_p, C.c_int64]
    lib.gklhip_pdhmm_get_table.restype = C.c_int64
    lib.gklhip_pdhmm_last_error.restype = C.c_char_p
    lib.gklhip_pdhmm_connect.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.gklhip_pdhmm_connect.restype = C.c_int
    lib.gklhip_pdhmm_is_remote.argtypes = [C.c_void_p]
    lib.gklhip_pdhmm_is_remote.restype = C.c_int
    lib.gklhip_pdhmm_server_stats.argtypes = [C.c_char_p, C.POINTER(PdhmmServerInfo)]
    lib.gklhip_pdhmm_server_stats.restype = C.c_int
    # the device-resident calls: other builds and stubs of the library (an older build under GKL_AMD_PDHMM_LIB, the
    # tests' stub) may not have them and must still load -- calling one there raises AttributeError
    if hasattr(lib, "gklhip_pdhmm_compute_device"):
        lib.gklhip_pdhmm_compute_device.argtypes = [C.c_void_p, C.POINTER(CPdhmmBatch), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gklhip_pdhmm_compute_device.restype = C.c_int
    if hasattr(lib, "gklhip_pdhmm_compute_cross_device"):
        lib.gklhip_pdhmm_compute_cross_device.argtypes = [C.c_void_p, C.POINTER(CPdhmmCross), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.gklhip_pdhmm_compute_cross_device.restype = C.c_int
    if hasattr(lib, "gklhip_pdhmm_compute_cross_multi_device"):
        lib.gklhip_pdhmm_compute_cross_multi_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CPdhmmCross), C.POINTER(C.c_int64),
                                                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_void_p]
        lib.gklhip_pdhmm_compute_cross_multi_device.restype = C.c_int
    if hasattr(lib, "gklhip_pdhmm_finalise_host"):
        lib.gklhip_pdhmm_finalise_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.gklhip_pdhmm_finalise_host.restype = C.c_int
    if path is None:
        _pd_lib = lib
    return lib


def pdhmm_host_table(which: int) -> np.ndarray:
    lib = load_pdhmm_library()
    n = lib.gklhip_pdhmm_get_table(which, None, 0)
    a = np.empty(n, np.float64)
    lib.gklhip_pdhmm_get_table(which, a.ctypes.data, n)
    return a


def pdhmm_reference_batch_pairs(max_memory_mb: int, max_read_len: int, max_hap_len: int, total_pairs: int) -> int:
    """Pairs per batch of the reference's computeLikelihoodsNative (pdhmm/JavaData.h:83-101)."""
    return int(load_pdhmm_library().gklhip_pdhmm_reference_batch_pairs(max_memory_mb, max_read_len, max_hap_len, total_pairs))


def pdhmm_available_memory_mb(max_memory_mb: int) -> int:
    """min(maxMemoryInMB, free RAM of the host): what the reference's initNative keeps (pdhmm-implementation.h:204-235)."""
    return int(load_pdhmm_library().gklhip_pdhmm_available_memory_mb(max_memory_mb))


def pdhmm_combine_counts(device: int = -1, reset: bool = False, lib_path: Optional[str] = None):
    """(region calls computed, region calls that shared a launch set with another, launch sets) of the cross calls this
    process computed on `device` (-1: all devices) -- gklhip_pdhmm_combine_counts.  Client contexts count nothing here: the
    server's counts are pdhmm_server_stats()["combine_counts"]."""
    lib = load_pdhmm_library(lib_path)
    out = (C.c_int64 * 3)()
    st = lib.gklhip_pdhmm_combine_counts(device, out, 1 if reset else 0)
    if st != OK:
        _raise_pdhmm(lib, st)
    return int(out[0]), int(out[1]), int(out[2])


class PdhmmMultiError(Exception):
    """compute_cross_multi: some regions failed.  results[k] is region k's array or None, statuses[k] its status code,
    errors[k] the exception a single call would have raised (None for a region that succeeded)."""

    def __init__(self, results, statuses, errors):
        first = next(e for e in errors if e is not None)
        super().__init__(f"{sum(e is not None for e in errors)} of {len(errors)} regions failed; the first: {first}")
        self.results, self.statuses, self.errors = results, statuses, errors


def _pdhmm_exception(status: int, msg: str):
    if status == ERR_INVALID_ARG:
        return IllegalArgumentException(msg)
    if status == ERR_OOM:
        return OutOfMemoryError(msg)
    return RuntimeException(msg)


def _raise_pdhmm(lib, status: int):
    msg = (lib.gklhip_pdhmm_last_error() or b"").decode()
    if status == ERR_INVALID_ARG:
        raise IllegalArgumentException(msg)
    if status == ERR_OOM:
        raise OutOfMemoryError(msg)
    raise RuntimeException(msg)


def pdhmm_server_stats(socket_path: str) -> dict:
    """PDHMM counters of the server on `socket_path` (gklhip_pdhmm_server_stats): whether it has loaded its PDHMM
    library, calls served / failed / active, live PDHMM connections, pairs served.  Makes no HIP call."""
    lib = load_pdhmm_library()
    info = PdhmmServerInfo()
    st = lib.gklhip_pdhmm_server_stats(os.fsencode(socket_path), C.byref(info))
    if st != OK:
        _raise_pdhmm(lib, st)
    return info.as_dict()


def pdhmm_finalise_host(sums) -> np.ndarray:
    """The host calls' finalisation of raw sums (gklhip_pdhmm_finalise_host): log10(sum) - log10(2^1020) with the host
    libm, i.e. GKL's bits -- for the `sums` of PdhmmContext.compute_device / compute_cross_device, brought to the host
    (a numpy array or a CPU tensor).  Needs no GPU."""
    lib = load_pdhmm_library()
    s = np.ascontiguousarray(np.asarray(sums), np.float64).reshape(-1)
    out = np.empty(s.size, np.float64)
    st = lib.gklhip_pdhmm_finalise_host(s.ctypes.data, s.size, out.ctypes.data)
    if st != OK:
        _raise_pdhmm(lib, st)
    return out


_PD_HAP_ARRAYS = ("hap_bases", "hap_pdbases")
_PD_READ_ARRAYS = ("read_bases", "read_qual", "read_ins_qual", "read_del_qual", "gcp")


@dataclass
class PdhmmDeviceBatch:
    """A PdhmmBatch whose seven byte arrays live in HBM: torch int8 tensors own the memory, the two length arrays stay
    numpy on the host (the library's planner reads them).  One side of a cross product holds its own arrays only: the
    other side's tensors and lengths are None."""
    batch: int
    max_hap_len: int
    max_read_len: int
    hap_tensors: Optional[tuple]    # (hap_bases, hap_pdbases), each [batch * max_hap_len]
    read_tensors: Optional[tuple]   # (read_bases, read_qual, read_ins_qual, read_del_qual, gcp), each [batch * max_read_len]
    hap_lengths: Optional[np.ndarray]
    read_lengths: Optional[np.ndarray]

    @staticmethod
    def upload(b, device="cuda:0", side: str = "both") -> "PdhmmDeviceBatch":
        """b: a PdhmmBatch (or anything with its fields).  side: "both", or "reads" / "haps" for one side of a cross product."""
        import torch
        up = lambda names: tuple(torch.from_numpy(np.ascontiguousarray(getattr(b, n), np.int8).reshape(-1)).to(device)  # noqa: E731
                                 for n in names)
        haps, reads = side in ("both", "haps"), side in ("both", "reads")
        if not (haps or reads):
            raise IllegalArgumentException(f"side {side!r} (both, reads or haps)")
        return PdhmmDeviceBatch(b.batch, b.max_hap_len if haps else 0, b.max_read_len if reads else 0,
                                up(_PD_HAP_ARRAYS) if haps else None, up(_PD_READ_ARRAYS) if reads else None,
                                np.ascontiguousarray(b.hap_lengths, np.int64) if haps else None,
                                np.ascontiguousarray(b.read_lengths, np.int64) if reads else None)

    @staticmethod
    def upload_cross(reads, haps, device="cuda:0"):
        """The cross form: (reads_db, haps_db) for PdhmmContext.compute_cross_device, from what compute_cross takes."""
        return PdhmmDeviceBatch.upload(reads, device, "reads"), PdhmmDeviceBatch.upload(haps, device, "haps")

    def _checked(self, tensors, row: int, what: str):
        # the library trusts these addresses: a tensor of the wrong kind or size would be read out of bounds on the device
        if tensors is None or (self.hap_lengths if what == "haplotype" else self.read_lengths) is None:
            raise IllegalArgumentException(f"this device batch holds no {what} arrays")
        for t in tensors:
            if not t.is_cuda or t.element_size() != 1 or not t.is_contiguous() or t.numel() != self.batch * row:
                raise IllegalArgumentException(f"{what} arrays must be contiguous one-byte CUDA tensors of batch * max length = "
                                               f"{self.batch * row} elements")
        return [t.data_ptr() for t in tensors]

    def hap_pointers(self):
        return self._checked(self.hap_tensors, self.max_hap_len, "haplotype")

    def read_pointers(self):
        return self._checked(self.read_tensors, self.max_read_len, "read")


def _pd_result_tensor(t, n: int, device, name: str):
    """`out` / `sums` of a device-resident call: given, it must be a contiguous float64 tensor of n elements on `device`."""
    import torch
    if t is None:
        return torch.empty(n, dtype=torch.float64, device=device)
    if t.dtype != torch.float64 or not t.is_cuda or t.device != device or not t.is_contiguous() or t.numel() != n:
        raise IllegalArgumentException(f"{name} must be a contiguous float64 tensor of {n} elements on {device}")
    return t


class PdhmmContext:
    """One gklhip_pdhmm context (= IntelPDHMM.initNative)."""

    def __init__(self, device: int = -1, fma_mode: int = 1, reference_tail: Optional[bool] = None, lib_path: Optional[str] = None,
                 server: Optional[str] = None):
        """fma_mode 1: bit-identical to GKL's AVX-512 PDHMM object, 0: to its AVX2 object.  reference_tail: the last
        `batch mod SIMD width` pairs of every reference batch take the scalar engine's arithmetic, as in GKL -- None:
        the library's setting (default: on; GKL_HIP_PDHMM_TAIL=vector turns it off), True / False: set it.
        lib_path: another build of the library (the all-C++ cross-check build of the tests).
        server: socket path of a running server (gkl_amd.server): a client context, whose calls that server computes
        (no HIP call in this process).  GKL_HIP_SERVER in the environment makes every context a client context."""
        self.lib = load_pdhmm_library(lib_path)
        h = C.c_void_p()
        if server is not None:
            st = self.lib.gklhip_pdhmm_connect(os.fsencode(server), device, C.byref(h))
        else:
            st = self.lib.gklhip_pdhmm_init(device, C.byref(h))
        if st != OK:
            self._raise(st)
        self.handle = h
        st = self.lib.gklhip_pdhmm_set_fma_mode(self.handle, int(fma_mode))
        if st != OK:
            self._raise(st)
        if reference_tail is not None:
            st = self.lib.gklhip_pdhmm_set_tail_mode(self.handle, 1 if reference_tail else 0)
            if st != OK:
                self._raise(st)

    def _raise(self, status):
        _raise_pdhmm(self.lib, status)

    @property
    def is_remote(self) -> bool:
        """True for a client context of the server (server=PATH or GKL_HIP_SERVER)."""
        return bool(self.lib.gklhip_pdhmm_is_remote(self.handle))

    def compute(self, b) -> np.ndarray:
        keep = [np.ascontiguousarray(a, np.int8) for a in (b.hap_bases, b.hap_pdbases, b.read_bases, b.read_qual,
                                                           b.read_ins_qual, b.read_del_qual, b.gcp)]
        hl = np.ascontiguousarray(b.hap_lengths, np.int64)
        rl = np.ascontiguousarray(b.read_lengths, np.int64)
        cb = CPdhmmBatch(b.batch, b.max_hap_len, b.max_read_len, *[a.ctypes.data for a in keep],
                         hl.ctypes.data, rl.ctypes.data)
        out = np.empty(max(b.batch, 0), np.float64)
        st = self.lib.gklhip_pdhmm_compute(self.handle, C.byref(cb), out.ctypes.data)
        if st != OK:
            self._raise(st)
        return out

    def compute_cross(self, reads, haps, ref_batch_pairs: int = 0) -> np.ndarray:
        """Every read against every haplotype (IntelPDHMM.computeLikelihoods), out[r * n_haps + h].
        ref_batch_pairs: in reference-tail mode, the size of the batches the reference cuts the pair list into
        (reference_batch_pairs()); 0 = one batch.
        reads: PdhmmBatch-like with the five read arrays [n][max_read_len] + read_lengths (its haplotype side is
        ignored); haps: PdhmmBatch-like with hap_bases / hap_pdbases [n][max_hap_len] + hap_lengths."""
        keep = [np.ascontiguousarray(a, np.int8) for a in (haps.hap_bases, haps.hap_pdbases, reads.read_bases,
                                                           reads.read_qual, reads.read_ins_qual, reads.read_del_qual,
                                                           reads.gcp)]
        hl = np.ascontiguousarray(haps.hap_lengths, np.int64)
        rl = np.ascontiguousarray(reads.read_lengths, np.int64)
        cb = CPdhmmCross(reads.batch, haps.batch, haps.max_hap_len, reads.max_read_len, *[a.ctypes.data for a in keep],
                         hl.ctypes.data, rl.ctypes.data)
        out = np.empty(max(reads.batch * haps.batch, 0), np.float64)
        st = self.lib.gklhip_pdhmm_compute_cross_batched(self.handle, C.byref(cb), C.c_int64(ref_batch_pairs), out.ctypes.data)
        if st != OK:
            self._raise(st)
        return out

    def compute_cross_multi(self, regions, ref_batch_pairs=None):
        """Several region calls in one set of launches (gklhip_pdhmm_compute_cross_multi): regions is a list of
        (reads, haps) as compute_cross takes them, ref_batch_pairs None or one number per region; returns the list of
        their arrays, each byte for byte what compute_cross returns for it alone.  When regions fail, the others are still
        computed: PdhmmMultiError carries their arrays and every region's status and exception."""
        n = len(regions)
        keep, crosses, outs = [], (CPdhmmCross * max(n, 1))(), []
        for k, (reads, haps) in enumerate(regions):
            arrs = [np.ascontiguousarray(a, np.int8) for a in (haps.hap_bases, haps.hap_pdbases, reads.read_bases, reads.read_qual,
                                                               reads.read_ins_qual, reads.read_del_qual, reads.gcp)]
            hl = np.ascontiguousarray(haps.hap_lengths, np.int64)
            rl = np.ascontiguousarray(reads.read_lengths, np.int64)
            keep.append((arrs, hl, rl))
            crosses[k] = CPdhmmCross(reads.batch, haps.batch, haps.max_hap_len, reads.max_read_len, *[a.ctypes.data for a in arrs],
                                     hl.ctypes.data, rl.ctypes.data)
            outs.append(np.empty(max(reads.batch * haps.batch, 0), np.float64))
        out_ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        rb = None if ref_batch_pairs is None else (C.c_int64 * max(n, 1))(*[int(v) for v in ref_batch_pairs])
        status = (C.c_int32 * max(n, 1))()
        st = self.lib.gklhip_pdhmm_compute_cross_multi(self.handle, n, crosses, rb, out_ptrs, status)
        if st == OK:
            return outs
        self._raise_multi(st, n, status, outs)

    def _raise_multi(self, st, n, status, outs):
        """A multi-region call returned st != OK: the exception of the call itself, or PdhmmMultiError with the regions' own."""
        if n <= 0 or all(status[k] == OK for k in range(n)):
            self._raise(st)   # the call itself was refused
        # the library keeps the first failing region's message; the reference has one text per status for the others
        msg = (self.lib.gklhip_pdhmm_last_error() or b"").decode()
        first = next(k for k in range(n) if status[k] != OK)
        errors = [None if status[k] == OK else _pdhmm_exception(status[k], msg if k == first or status[k] == status[first] else
                                                                f"region {k} failed with status {status[k]}") for k in range(n)]
        raise PdhmmMultiError([o if status[k] == OK else None for k, o in enumerate(outs)], [int(status[k]) for k in range(n)], errors)

    # -- device-resident calls: byte arrays and results in HBM; `out` / `sums` are torch float64 CUDA tensors --
    def compute_device(self, db: PdhmmDeviceBatch, out=None, sums=None, stream=None):
        """gklhip_pdhmm_compute_device: compute() with the arrays of `db` in HBM.  Returns the float64 tensor of log10
        likelihoods (`out`, or a new one), evaluated with the device's log10: equal to compute() to the last bits, not
        bit for bit.  sums: a float64 tensor that receives the raw sums -- pdhmm_finalise_host(sums.cpu()) is compute()'s
        output byte for byte.  The call is ordered behind the work already on `stream` (default: torch's current stream)
        and synchronous: the results are in place when it returns."""
        import torch
        hp, rp = db.hap_pointers(), db.read_pointers()
        device = db.read_tensors[0].device
        out = _pd_result_tensor(out, max(db.batch, 0), device, "out")
        if sums is not None:
            sums = _pd_result_tensor(sums, max(db.batch, 0), device, "sums")
        if stream is None:
            stream = torch.cuda.current_stream(device)
        cb = CPdhmmBatch(db.batch, db.max_hap_len, db.max_read_len, *hp, *rp, db.hap_lengths.ctypes.data, db.read_lengths.ctypes.data)
        st = self.lib.gklhip_pdhmm_compute_device(self.handle, C.byref(cb), out.data_ptr(), None if sums is None else sums.data_ptr(),
                                                  stream.cuda_stream)
        if st != OK:
            self._raise(st)
        return out

    def compute_cross_device(self, reads_db: PdhmmDeviceBatch, haps_db: PdhmmDeviceBatch, ref_batch_pairs: int = 0, out=None, sums=None,
                             stream=None):
        """gklhip_pdhmm_compute_cross_device: compute_cross() with both sides in HBM (PdhmmDeviceBatch.upload_cross),
        out[r * n_haps + h].  As compute_device; the two haplotype arrays are read back to the host once, early, for
        the planner."""
        import torch
        hp, rp = haps_db.hap_pointers(), reads_db.read_pointers()
        device = reads_db.read_tensors[0].device
        if haps_db.hap_tensors[0].device != device:
            raise IllegalArgumentException("reads and haplotypes are on different devices")
        n = max(reads_db.batch * haps_db.batch, 0)
        out = _pd_result_tensor(out, n, device, "out")
        if sums is not None:
            sums = _pd_result_tensor(sums, n, device, "sums")
        if stream is None:
            stream = torch.cuda.current_stream(device)
        cb = CPdhmmCross(reads_db.batch, haps_db.batch, haps_db.max_hap_len, reads_db.max_read_len, *hp, *rp,
                         haps_db.hap_lengths.ctypes.data, reads_db.read_lengths.ctypes.data)
        st = self.lib.gklhip_pdhmm_compute_cross_device(self.handle, C.byref(cb), C.c_int64(ref_batch_pairs), out.data_ptr(),
                                                        None if sums is None else sums.data_ptr(), stream.cuda_stream)
        if st != OK:
            self._raise(st)
        return out

    def compute_cross_multi_device(self, regions, ref_batch_pairs=None, outs=None, sums=None, stream=None):
        """gklhip_pdhmm_compute_cross_multi_device: compute_cross_multi() with every region's two sides in HBM.  regions: a
        list of (reads_db, haps_db) as PdhmmDeviceBatch.upload_cross returns them; ref_batch_pairs: None or one number per
        region; outs: None, or one float64 tensor (or None: a new one) per region; sums: None, or a list whose entries are
        float64 tensors or None.  Returns the list of output tensors, each byte for byte what compute_cross_device leaves
        for its region alone.  Ordered behind `stream` and synchronous, as compute_cross_device.  When regions fail, the
        others are still computed: PdhmmMultiError carries their tensors and every region's status and exception."""
        import torch
        n = len(regions)
        crosses, out_list, sums_list, device = (CPdhmmCross * max(n, 1))(), [], [], None
        if (outs is not None and len(outs) != n) or (sums is not None and len(sums) != n) or \
                (ref_batch_pairs is not None and len(ref_batch_pairs) != n):
            raise IllegalArgumentException(f"outs, sums and ref_batch_pairs must be None or hold one entry per region ({n})")
        for k, (reads_db, haps_db) in enumerate(regions):
            hp, rp = haps_db.hap_pointers(), reads_db.read_pointers()
            if device is None:
                device = reads_db.read_tensors[0].device
            if haps_db.hap_tensors[0].device != device or reads_db.read_tensors[0].device != device:
                raise IllegalArgumentException("the regions' reads and haplotypes are on different devices")
            pairs = max(reads_db.batch * haps_db.batch, 0)
            out_list.append(_pd_result_tensor(None if outs is None else outs[k], pairs, device, f"outs[{k}]"))
            sums_list.append(None if sums is None or sums[k] is None else _pd_result_tensor(sums[k], pairs, device, f"sums[{k}]"))
            crosses[k] = CPdhmmCross(reads_db.batch, haps_db.batch, haps_db.max_hap_len, reads_db.max_read_len, *hp, *rp,
                                     haps_db.hap_lengths.ctypes.data, reads_db.read_lengths.ctypes.data)
        if stream is None and device is not None:
            stream = torch.cuda.current_stream(device)
        out_ptrs = (C.c_void_p * max(n, 1))(*[o.data_ptr() for o in out_list])
        sums_ptrs = None if sums is None else (C.c_void_p * max(n, 1))(*[None if s is None else s.data_ptr() for s in sums_list])
        rb = None if ref_batch_pairs is None else (C.c_int64 * max(n, 1))(*[int(v) for v in ref_batch_pairs])
        status = (C.c_int32 * max(n, 1))()
        st = self.lib.gklhip_pdhmm_compute_cross_multi_device(self.handle, n, crosses, rb, out_ptrs, sums_ptrs, status,
                                                              None if stream is None else stream.cuda_stream)
        if st == OK:
            return out_list
        self._raise_multi(st, n, status, out_list)

    def last_kernel_ms(self) -> float:
        return float(self.lib.gklhip_pdhmm_last_kernel_ms(self.handle))

    def buffer_bytes(self) -> int:
        """Device + pinned host bytes the context holds right now (they shrink again after 16 small calls)."""
        return int(self.lib.gklhip_pdhmm_buffer_bytes(self.handle))

    def last_routing(self):
        """Last cross call: its haplotypes by kernel (LDS prior table, predicate, byte-comparing); last paired call: its
        packed jobs (wavefront-loads of whole pairs) by kernel."""
        out = (C.c_int32 * 3)()
        st = self.lib.gklhip_pdhmm_last_routing(self.handle, out)
        if st != OK:
            self._raise(st)
        return int(out[0]), int(out[1]), int(out[2])

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gklhip_pdhmm_done(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- Smith-Waterman (include/gkl_hip_sw.h)
SW_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libgklhip_sw.so")
SW_SOFTCLIP, SW_INDEL, SW_LEADING_INDEL, SW_IGNORE = 9, 10, 11, 12
_sw_lib = None


class CSwParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("open", C.c_int32), ("extend", C.c_int32)]


def load_sw_library(path: Optional[str] = None):
    global _sw_lib
    if _sw_lib is not None and path is None:
        return _sw_lib
    p = path or SW_LIB_PATH
    try:
        import torch  # noqa: F401  (HIP runtime load order, see load_library)
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeException(f"{p} is not built (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.gklhip_sw_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.gklhip_sw_init.restype = C.c_int
    lib.gklhip_sw_done.argtypes = [C.c_void_p]
    lib.gklhip_sw_done.restype = C.c_int
    lib.gklhip_sw_align.argtypes = [C.c_void_p, C.POINTER(CSwParams), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p,
                                    C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    lib.gklhip_sw_align.restype = C.c_int
    lib.gklhip_sw_align_batch.argtypes = [C.c_void_p, C.POINTER(CSwParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.gklhip_sw_align_batch.restype = C.c_int
    lib.gklhip_sw_last_kernel_ms.argtypes = [C.c_void_p]
    lib.gklhip_sw_last_kernel_ms.restype = C.c_float
    lib.gklhip_sw_last_error.restype = C.c_char_p
    if path is None:
        _sw_lib = lib
    return lib


class SwContext:
    """One gklhip_sw context (= IntelSmithWaterman.initNative)."""

    def __init__(self, device: int = -1):
        self.lib = load_sw_library()
        h = C.c_void_p()
        st = self.lib.gklhip_sw_init(device, C.byref(h))
        if st != OK:
            self._raise(st)
        self.handle = h

    def _raise(self, status):
        msg = (self.lib.gklhip_sw_last_error() or b"").decode()
        if status == ERR_INVALID_ARG:
            raise IllegalArgumentException(msg)
        if status == ERR_OOM:
            raise OutOfMemoryError(msg)
        raise RuntimeException(msg)

    def align(self, ref: bytes, alt: bytes, params, strategy: int, cigar_len: Optional[int] = None):
        """(cigar bytes, cigar_count, offset) of one pair; cigar_len defaults to the Java side's 2*max(len)."""
        ref, alt = bytes(ref), bytes(alt)
        if cigar_len is None:
            cigar_len = 2 * max(len(ref), len(alt))
        buf = C.create_string_buffer(max(cigar_len, 1))
        cnt, off = C.c_uint32(0), C.c_int32(0)
        p = CSwParams(*[int(v) for v in params])
        st = self.lib.gklhip_sw_align(self.handle, C.byref(p), int(strategy), ref, len(ref), alt, len(alt), buf,
                                      int(cigar_len), C.byref(cnt), C.byref(off))
        if st != OK:
            self._raise(st)
        return buf.raw[:cigar_len].rstrip(b"\0"), cnt.value, off.value

    @staticmethod
    def pack(refs, alts, cigar_stride: Optional[int] = None):
        """Flat arrays of gklhip_sw_align_batch for lists of byte strings (reusable across calls)."""
        n = len(refs)
        if n != len(alts):
            raise IllegalArgumentException("refs and alts differ in length")
        refs, alts = [bytes(r) for r in refs], [bytes(a) for a in alts]
        if cigar_stride is None:
            cigar_stride = 2 * max([1] + [max(len(r), len(a)) for r, a in zip(refs, alts)])
        ro = np.zeros(n + 1, np.int64)
        ao = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in refs], out=ro[1:])
        np.cumsum([len(a) for a in alts], out=ao[1:])
        rb = np.frombuffer(b"".join(refs) or b"\0", dtype=np.uint8)
        ab = np.frombuffer(b"".join(alts) or b"\0", dtype=np.uint8)
        return {"n": n, "ref_off": ro, "alt_off": ao, "refs": rb, "alts": ab, "cigar_stride": int(cigar_stride),
                "cells": int(sum(len(r) * len(a) for r, a in zip(refs, alts)))}

    def align_packed(self, pk, params, strategy: int):
        """One gklhip_sw_align_batch call on pack()'s arrays: (cigar byte matrix [n][stride], counts, offsets)."""
        n, stride = pk["n"], pk["cigar_stride"]
        cig = np.zeros(max(n, 1) * stride, np.uint8)
        cnt = np.zeros(max(n, 1), np.uint32)
        off = np.zeros(max(n, 1), np.int32)
        p = CSwParams(*[int(v) for v in params])
        st = self.lib.gklhip_sw_align_batch(self.handle, C.byref(p), int(strategy), n, pk["refs"].ctypes.data,
                                            pk["ref_off"].ctypes.data, pk["alts"].ctypes.data, pk["alt_off"].ctypes.data,
                                            cig.ctypes.data, stride, cnt.ctypes.data, off.ctypes.data)
        if st != OK:
            self._raise(st)
        return cig.reshape(max(n, 1), stride)[:n], cnt[:n], off[:n]

    def align_batch(self, refs, alts, params, strategy: int, cigar_stride: Optional[int] = None):
        """Lists of byte strings in, (list of cigar bytes, counts, offsets) out -- one launch for all pairs."""
        rows, cnt, off = self.align_packed(self.pack(refs, alts, cigar_stride), params, strategy)
        return [rows[k].tobytes().rstrip(b"\0") for k in range(len(refs))], cnt.copy(), off.copy()

    def last_kernel_ms(self) -> float:
        return float(self.lib.gklhip_sw_last_kernel_ms(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gklhip_sw_done(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- batch inflate (include/inflate/gkl_hip_inflate.h)
INFLATE_LIB_PATH = os.path.join(LIB_DIR, "libgklhip_inflate.so")
INFLATE_OK, INFLATE_INVALID_BLOCK, INFLATE_INVALID_SYMBOL, INFLATE_INVALID_LOOKBACK, INFLATE_END_INPUT, INFLATE_OUT_OVERFLOW = range(6)
_inflate_lib = None


def load_inflate_library(path: Optional[str] = None):
    global _inflate_lib
    if _inflate_lib is not None and path is None:
        return _inflate_lib
    p = path or INFLATE_LIB_PATH
    try:
        import torch  # noqa: F401  (HIP runtime load order, see load_library)
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeException(f"{p} is not built (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.gklhip_inflate_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.gklhip_inflate_init.restype = C.c_int
    lib.gklhip_inflate_done.argtypes = [C.c_void_p]
    lib.gklhip_inflate_done.restype = C.c_int
    lib.gklhip_inflate_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    lib.gklhip_inflate_batch.restype = C.c_int
    lib.gklhip_inflate_batch_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
    lib.gklhip_inflate_batch_device.restype = C.c_int
    lib.gklhip_bgzf_scan.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.gklhip_bgzf_scan.restype = C.c_int
    lib.gklhip_bgzf_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gklhip_bgzf_inflate.restype = C.c_int
    lib.gklhip_inflate_last_kernel_ms.argtypes = [C.c_void_p]
    lib.gklhip_inflate_last_kernel_ms.restype = C.c_float
    lib.gklhip_inflate_last_error.restype = C.c_char_p
    if path is None:
        _inflate_lib = lib
    return lib


class BgzfError(IllegalArgumentException):
    """A BGZF file image that gklhip_bgzf_scan / gklhip_bgzf_inflate refuse; bad_member is the first member at fault."""

    def __init__(self, msg, bad_member):
        super().__init__(msg)
        self.bad_member = bad_member


def bgzf_scan(data, max_members: Optional[int] = None):
    """gklhip_bgzf_scan (host only, no device needed): (payload_off int64[n], payload_len int32[n], crc32 uint32[n],
    isize uint32[n], bytes_used) of the BGZF members of a file image; BgzfError at a malformed member."""
    lib = load_inflate_library()
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    length = len(data)
    n, used = C.c_int32(0), C.c_int64(0)
    if max_members is None:
        st = lib.gklhip_bgzf_scan(buf.ctypes.data, length, 0, None, None, None, None, C.byref(n), C.byref(used))
        if st != OK:
            raise BgzfError((lib.gklhip_inflate_last_error() or b"").decode(), n.value)
        max_members = n.value
    m = max(int(max_members), 1)
    off, plen = np.zeros(m, np.int64), np.zeros(m, np.int32)
    crc, isize = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    st = lib.gklhip_bgzf_scan(buf.ctypes.data, length, int(max_members), off.ctypes.data, plen.ctypes.data, crc.ctypes.data,
                              isize.ctypes.data, C.byref(n), C.byref(used))
    if st != OK:
        raise BgzfError((lib.gklhip_inflate_last_error() or b"").decode(), n.value)
    k = n.value
    return off[:k], plen[:k], crc[:k], isize[:k], used.value


class InflateContext:
    """One gklhip_inflate context: batches of independent raw-deflate streams, one wavefront per stream."""

    def __init__(self, device: int = -1):
        self.lib = load_inflate_library()
        h = C.c_void_p()
        st = self.lib.gklhip_inflate_init(device, C.byref(h))
        if st != OK:
            self._raise(st)
        self.handle = h

    def _raise(self, status):
        msg = (self.lib.gklhip_inflate_last_error() or b"").decode()
        if status == ERR_INVALID_ARG:
            raise IllegalArgumentException(msg)
        if status == ERR_OOM:
            raise OutOfMemoryError(msg)
        raise RuntimeException(msg)

    def inflate_batch_raw(self, src: np.ndarray, src_off: np.ndarray, dst: np.ndarray, dst_off: np.ndarray, want_crc: bool = True):
        """gklhip_inflate_batch on flat arrays: src / dst uint8, src_off / dst_off int64[n + 1]; dst is written in place
        (only the bytes the streams produce).  Returns (out_len int32[n], consumed int32[n], crc32 uint32[n] or None,
        status int32[n])."""
        n = len(src_off) - 1
        if n < 0 or len(dst_off) != n + 1:
            raise IllegalArgumentException("n + 1 offsets each")
        src_off, dst_off = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(dst_off, np.int64)
        if src.dtype != np.uint8 or dst.dtype != np.uint8 or not src.flags.c_contiguous or not dst.flags.c_contiguous:
            raise IllegalArgumentException("src and dst must be contiguous uint8 arrays")
        if n and (src_off[-1] > src.size or dst_off[-1] > dst.size):
            raise IllegalArgumentException("offsets exceed the arrays")
        m = max(n, 1)
        out_len, consumed, status = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        crc = np.zeros(m, np.uint32) if want_crc else None
        st = self.lib.gklhip_inflate_batch(self.handle, n, src.ctypes.data, src_off.ctypes.data, dst.ctypes.data, dst_off.ctypes.data,
                                           out_len.ctypes.data, consumed.ctypes.data, crc.ctypes.data if want_crc else None,
                                           status.ctypes.data)
        if st != OK:
            self._raise(st)
        return out_len[:n], consumed[:n], (crc[:n] if want_crc else None), status[:n]

    def inflate_batch(self, streams, capacities):
        """Lists in, lists out: (outputs, crcs, statuses, consumed).  outputs[k] is the valid prefix (all of the output
        when statuses[k] == INFLATE_OK), crcs[k] its CRC-32."""
        streams = [bytes(s) for s in streams]
        n = len(streams)
        if len(capacities) != n:
            raise IllegalArgumentException("one capacity per stream")
        so, do = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in streams], out=so[1:])
        np.cumsum([int(c) for c in capacities], out=do[1:])
        src = np.frombuffer(b"".join(streams) or b"\0", dtype=np.uint8)
        dst = np.zeros(max(int(do[-1]), 1), np.uint8)
        out_len, consumed, crc, status = self.inflate_batch_raw(src, so, dst, do)
        outs = [dst[do[k]:do[k] + out_len[k]].tobytes() for k in range(n)]
        return outs, [int(c) for c in crc], [int(s) for s in status], [int(c) for c in consumed]

    def inflate_batch_device(self, src, src_off, dst, dst_off, want_crc: bool = True, stream=None):
        """gklhip_inflate_batch_device (synchronous): src and dst are contiguous torch uint8 CUDA tensors on the
        context's device, src_off / dst_off int64[n + 1] on the host; dst is written in place.  Returns torch tensors
        (out_len int32, consumed int32, crc32 as int32 bit patterns or None, status int32) on that device."""
        import torch
        n = len(src_off) - 1
        if n < 0 or len(dst_off) != n + 1:
            raise IllegalArgumentException("n + 1 offsets each")
        for t in (src, dst):
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
                raise IllegalArgumentException("src and dst must be contiguous uint8 CUDA tensors")
        src_off, dst_off = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(dst_off, np.int64)
        if n and (src_off[-1] > src.numel() or dst_off[-1] > dst.numel()):
            raise IllegalArgumentException("offsets exceed the tensors")
        m = max(n, 1)
        out_len, consumed, status = (torch.zeros(m, dtype=torch.int32, device=dst.device) for _ in range(3))
        crc = torch.zeros(m, dtype=torch.int32, device=dst.device) if want_crc else None
        if stream is None:
            stream = torch.cuda.current_stream(dst.device)
        st = self.lib.gklhip_inflate_batch_device(self.handle, n, src.data_ptr(), src_off.ctypes.data, dst.data_ptr(),
                                                  dst_off.ctypes.data, out_len.data_ptr(), consumed.data_ptr(),
                                                  crc.data_ptr() if want_crc else None, status.data_ptr(), stream.cuda_stream)
        if st != OK:
            self._raise(st)
        return out_len[:n], consumed[:n], (crc[:n] if want_crc else None), status[:n]

    bgzf_scan = staticmethod(bgzf_scan)

    def bgzf_inflate(self, data, out_cap: Optional[int] = None) -> bytes:
        """gklhip_bgzf_inflate: the concatenated output of every member of a BGZF file image, each member's CRC32 and
        ISIZE checked; BgzfError (bad_member set) otherwise."""
        data = bytes(data)
        if out_cap is None:
            out_cap = int(bgzf_scan(data)[3].astype(np.int64).sum())
        buf = np.frombuffer(data or b"\0", dtype=np.uint8)
        out = np.zeros(max(int(out_cap), 1), np.uint8)
        n, bad = C.c_int64(0), C.c_int32(-1)
        st = self.lib.gklhip_bgzf_inflate(self.handle, buf.ctypes.data, len(data), out.ctypes.data, int(out_cap), C.byref(n), C.byref(bad))
        if st != OK:
            if bad.value >= 0:
                raise BgzfError((self.lib.gklhip_inflate_last_error() or b"").decode(), bad.value)
            self._raise(st)
        return out[:n.value].tobytes()

    def last_kernel_ms(self) -> float:
        return float(self.lib.gklhip_inflate_last_kernel_ms(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gklhip_inflate_done(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- batch deflate (include/deflate/gkl_hip_deflate.h)
DEFLATE_LIB_PATH = os.path.join(LIB_DIR, "libgklhip_deflate.so")
DEFLATE_OK, DEFLATE_OUT_OVERFLOW = range(2)
DEFLATE_DEFAULT_STRATEGY, DEFLATE_HUFFMAN_ONLY = range(2)
DEFLATE_STORED, DEFLATE_FIXED, DEFLATE_DYNAMIC = 1, 2, 4
_deflate_lib = None


def load_deflate_library(path: Optional[str] = None):
    global _deflate_lib
    if _deflate_lib is not None and path is None:
        return _deflate_lib
    p = path or DEFLATE_LIB_PATH
    try:
        import torch  # noqa: F401  (HIP runtime load order, see load_library)
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RuntimeException(f"{p} is not built (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    lib.gklhip_deflate_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.gklhip_deflate_init.restype = C.c_int
    lib.gklhip_deflate_done.argtypes = [C.c_void_p]
    lib.gklhip_deflate_done.restype = C.c_int
    lib.gklhip_deflate_bound.argtypes = [C.c_int64]
    lib.gklhip_deflate_bound.restype = C.c_int64
    lib.gklhip_deflate_set_strategy.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.gklhip_deflate_set_strategy.restype = C.c_int
    lib.gklhip_deflate_batch.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3
    lib.gklhip_deflate_batch.restype = C.c_int
    lib.gklhip_deflate_batch_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4
    lib.gklhip_deflate_batch_device.restype = C.c_int
    lib.gklhip_bgzf_bound.argtypes = [C.c_int64, C.c_int32]
    lib.gklhip_bgzf_bound.restype = C.c_int64
    lib.gklhip_bgzf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gklhip_bgzf_deflate.restype = C.c_int
    lib.gklhip_deflate_last_kernel_ms.argtypes = [C.c_void_p]
    lib.gklhip_deflate_last_kernel_ms.restype = C.c_float
    lib.gklhip_deflate_last_error.restype = C.c_char_p
    if path is None:
        _deflate_lib = lib
    return lib


def deflate_bound(length: int) -> int:
    """gklhip_deflate_bound (host arithmetic, no device needed): the stored size of `length` input bytes."""
    return int(load_deflate_library().gklhip_deflate_bound(int(length)))


def bgzf_bound(length: int, block_size: int = 0) -> int:
    """gklhip_bgzf_bound (host arithmetic): an output capacity that bgzf_deflate never exceeds; -1 for a bad block size."""
    return int(load_deflate_library().gklhip_bgzf_bound(int(length), int(block_size)))


class DeflateContext:
    """One gklhip_deflate context: batches of independent inputs, one wavefront per raw-deflate stream.  `level` of
    every call: 0 (stored blocks), 1 (the fast one) or 3 to 8 (hash chains, lazy matching from 4 on); 2, 9 and -1 raise
    RuntimeException ("... is not built")."""

    def __init__(self, device: int = -1):
        self.lib = load_deflate_library()
        h = C.c_void_p()
        st = self.lib.gklhip_deflate_init(device, C.byref(h))
        if st != OK:
            self._raise(st)
        self.handle = h

    def _raise(self, status):
        msg = (self.lib.gklhip_deflate_last_error() or b"").decode()
        if status == ERR_INVALID_ARG:
            raise IllegalArgumentException(msg)
        if status == ERR_OOM:
            raise OutOfMemoryError(msg)
        raise RuntimeException(msg)

    def set_strategy(self, strategy: int = DEFLATE_DEFAULT_STRATEGY, block_types: int = 0) -> None:
        """strategy 0 default, 1 Huffman only; block_types a mask of DEFLATE_STORED / _FIXED / _DYNAMIC, 0 = all."""
        st = self.lib.gklhip_deflate_set_strategy(self.handle, int(strategy), int(block_types))
        if st != OK:
            self._raise(st)

    def deflate_batch_raw(self, src: np.ndarray, src_off: np.ndarray, dst: np.ndarray, dst_off: np.ndarray, level: int = 1,
                          want_crc: bool = True):
        """gklhip_deflate_batch on flat arrays: src / dst uint8, src_off / dst_off int64[n + 1]; dst is written in place
        (only the bytes of the streams).  Returns (out_len int32[n], crc32 of the inputs uint32[n] or None,
        status int32[n])."""
        n = len(src_off) - 1
        if n < 0 or len(dst_off) != n + 1:
            raise IllegalArgumentException("n + 1 offsets each")
        src_off, dst_off = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(dst_off, np.int64)
        if src.dtype != np.uint8 or dst.dtype != np.uint8 or not src.flags.c_contiguous or not dst.flags.c_contiguous:
            raise IllegalArgumentException("src and dst must be contiguous uint8 arrays")
        if n and (src_off[-1] > src.size or dst_off[-1] > dst.size):
            raise IllegalArgumentException("offsets exceed the arrays")
        m = max(n, 1)
        out_len, status = np.zeros(m, np.int32), np.zeros(m, np.int32)
        crc = np.zeros(m, np.uint32) if want_crc else None
        st = self.lib.gklhip_deflate_batch(self.handle, n, src.ctypes.data, src_off.ctypes.data, dst.ctypes.data, dst_off.ctypes.data,
                                           int(level), out_len.ctypes.data, crc.ctypes.data if want_crc else None, status.ctypes.data)
        if st != OK:
            self._raise(st)
        return out_len[:n], (crc[:n] if want_crc else None), status[:n]

    def deflate_batch(self, inputs, level: int = 1, capacities=None):
        """Lists in, lists out: (streams, crcs of the inputs, statuses).  capacities default to deflate_bound of each
        input, which never overflows while stored blocks are allowed; streams[k] is b"" on DEFLATE_OUT_OVERFLOW."""
        inputs = [bytes(s) for s in inputs]
        n = len(inputs)
        if capacities is None:
            capacities = [deflate_bound(len(s)) for s in inputs]
        if len(capacities) != n:
            raise IllegalArgumentException("one capacity per input")
        so, do = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in inputs], out=so[1:])
        np.cumsum([int(c) for c in capacities], out=do[1:])
        src = np.frombuffer(b"".join(inputs) or b"\0", dtype=np.uint8)
        dst = np.zeros(max(int(do[-1]), 1), np.uint8)
        out_len, crc, status = self.deflate_batch_raw(src, so, dst, do, level)
        outs = [dst[do[k]:do[k] + out_len[k]].tobytes() for k in range(n)]
        return outs, [int(c) for c in crc], [int(s) for s in status]

    def deflate_batch_device(self, src, src_off, dst, dst_off, level: int = 1, want_crc: bool = True, stream=None):
        """gklhip_deflate_batch_device (synchronous): src and dst are contiguous torch uint8 CUDA tensors on the
        context's device, src_off / dst_off int64[n + 1] on the host; dst is written in place.  Returns torch tensors
        (out_len int32, crc32 of the inputs as int32 bit patterns or None, status int32) on that device."""
        import torch
        n = len(src_off) - 1
        if n < 0 or len(dst_off) != n + 1:
            raise IllegalArgumentException("n + 1 offsets each")
        for t in (src, dst):
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
                raise IllegalArgumentException("src and dst must be contiguous uint8 CUDA tensors")
        src_off, dst_off = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(dst_off, np.int64)
        if n and (src_off[-1] > src.numel() or dst_off[-1] > dst.numel()):
            raise IllegalArgumentException("offsets exceed the tensors")
        m = max(n, 1)
        out_len, status = (torch.zeros(m, dtype=torch.int32, device=dst.device) for _ in range(2))
        crc = torch.zeros(m, dtype=torch.int32, device=dst.device) if want_crc else None
        if stream is None:
            stream = torch.cuda.current_stream(dst.device)
        st = self.lib.gklhip_deflate_batch_device(self.handle, n, src.data_ptr(), src_off.ctypes.data, dst.data_ptr(),
                                                  dst_off.ctypes.data, int(level), out_len.data_ptr(),
                                                  crc.data_ptr() if want_crc else None, status.data_ptr(), stream.cuda_stream)
        if st != OK:
            self._raise(st)
        return out_len[:n], (crc[:n] if want_crc else None), status[:n]

    def bgzf_deflate(self, data, block_size: int = 0, level: int = 1, append_eof: bool = True):
        """gklhip_bgzf_deflate: the BGZF image of data (members of block_size input bytes, 0 = 65280) and its member count."""
        data = bytes(data)
        cap = bgzf_bound(len(data), block_size)
        if cap < 0:
            raise IllegalArgumentException(f"block_size {block_size}: 1 .. 65498, 0 = 65280")
        buf = np.frombuffer(data or b"\0", dtype=np.uint8)
        out = np.zeros(max(cap, 1), np.uint8)
        n, members = C.c_int64(0), C.c_int32(0)
        st = self.lib.gklhip_bgzf_deflate(self.handle, buf.ctypes.data, len(data), int(block_size), int(level), 1 if append_eof else 0,
                                          out.ctypes.data, cap, C.byref(n), C.byref(members))
        if st != OK:
            self._raise(st)
        return out[:n.value].tobytes(), members.value

    def last_kernel_ms(self) -> float:
        return float(self.lib.gklhip_deflate_last_kernel_ms(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gklhip_deflate_done(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

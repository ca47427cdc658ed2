"""ctypes binding of the native libraries (test / bench plumbing, not the product).

The product is the C ABI of ``include/hga.h`` (``lib/libhga.so``, HIP for gfx950) and the
C++ CLIs in ``bin/``.  This module only marshals numpy buffers through that ABI and through
``lib/libhga_host.so`` (host readers and seeded generators).  There is no fallback: if the
HIP library is missing or a call fails, an ``HgaError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
BIN_DIR = os.path.join(HERE, "bin")


class HgaError(RuntimeError):
    pass


_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p


class CountStats(C.Structure):
    _fields_ = [("instances", C.c_uint64), ("distinct_rows", C.c_uint64), ("bytes", C.c_uint64),
                ("buckets", C.c_uint32), ("max_split", C.c_uint32)]


class CountPassStats(C.Structure):   # hga_count_pass_stats
    _fields_ = [("passes", C.c_uint32), ("pad", C.c_uint32), ("work_bytes", C.c_uint64),
                ("max_pass_instances", C.c_uint64), ("min_pass_instances", C.c_uint64)]


class LookupSizes(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("windows", C.c_uint64), ("hits", C.c_uint64),
                ("firsts", C.c_uint64), ("reads_hit", C.c_uint64), ("n_sdk", C.c_uint32)]


class LookupBatchStats(C.Structure):   # hga_lookup_batch_stats
    _fields_ = [("batches", C.c_uint64), ("reads", C.c_uint64), ("bases", C.c_uint64), ("slot_bytes", C.c_uint64),
                ("result_bytes", C.c_uint64), ("regrowths", C.c_uint64), ("host_waits", C.c_uint64)]


class ComponentsSizes(C.Structure):
    _fields_ = [("index_entries", C.c_uint64), ("survivors", C.c_uint64), ("survivor_kmers", C.c_uint64),
                ("merges", C.c_uint64)]


class TreeEnds(C.Structure):   # hga_tree_ends
    _fields_ = [("right_id", C.c_uint32), ("right_dist", C.c_uint64), ("left_id", C.c_uint32),
                ("left_dist", C.c_uint64)]


class IngestInfo(C.Structure):
    _fields_ = [("layout", C.c_uint32), ("reserved", C.c_uint32), ("records", C.c_uint64), ("lines", C.c_uint64),
                ("seq_bytes", C.c_uint64)]


class LookupResult(C.Structure):
    _fields_ = [("hit_ptr", _u64p), ("hit_kid", _u32p), ("hit_pos", _u32p), ("sorted_kid", _u32p),
                ("first_ptr", _u64p), ("first_kid", _u32p), ("first_pos", _u32p),
                ("kci_ptr", _u64p), ("kci_read", _u32p)]


# hga_transport (include/hga.h): one collective all-to-all-v over host memory
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                           C.POINTER(C.c_void_p), C.POINTER(C.c_uint64))


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("alltoallv", ALLTOALLV_FN)]


# rows per workgroup of hga_connections_quality's kernels (hga_connections_quality_tile)
QUALITY_TILE = 2048

_lib = None
_host = None

# name -> (restype, argtypes) for every symbol include/hga.h declares
HGA_SYMBOLS = {
    "hga_last_error": (C.c_char_p, []),
    "hga_free": (None, [_vp]),
    "hga_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "hga_version": (C.c_char_p, []),
    "hga_ctx_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "hga_ctx_destroy": (C.c_int, [_vp]),
    "hga_count_begin": (C.c_int, [_vp, C.c_int, C.c_uint32]),
    "hga_count_add": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_uint64]),
    "hga_count_add_file": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(IngestInfo)]),
    "hga_count_seq": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), _u64p]),
    "hga_ingest_tile": (C.c_uint32, []),
    "hga_count_add_rows": (C.c_int, [_vp, C.c_uint32, _u64p, _u32p, C.c_uint64]),
    "hga_count_run": (C.c_int, [_vp, C.c_uint32]),
    "hga_count_get_stats": (C.c_int, [_vp, C.POINTER(CountStats)]),
    "hga_count_set_passes": (C.c_int, [_vp, C.c_uint32, C.c_uint64]),
    "hga_count_estimate": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _u64p]),
    "hga_count_get_pass_stats": (C.c_int, [_vp, C.POINTER(CountPassStats)]),
    "hga_count_spec_hist": (C.c_int, [_vp, C.POINTER(C.c_double), C.c_uint32, C.POINTER(_i64p), _u64p]),
    "hga_count_select": (C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(_u64p), _u64p, _u64p]),
    "hga_count_select_ex": (C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(_u64p), C.POINTER(_u8p), _u64p,
                                      _u64p]),
    "hga_count_select_device": (C.c_int, [_vp, C.c_int64, C.c_int64, _u64p, _u64p]),
    "hga_count_partition": (C.c_int, [_vp, _u64p, C.c_uint32, C.c_void_p, C.c_void_p, _u64p]),
    "hga_count_merge": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]),
    "hga_count_pack_bits": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "hga_count_partition_packed": (C.c_int, [_vp, _u64p, C.c_uint32, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    "hga_count_merge_packed": (C.c_int, [_vp, C.c_void_p, C.c_uint64, C.c_uint32]),
    "hga_count_rows": (C.c_int, [_vp, C.POINTER(_u64p), C.POINTER(_u32p), _u64p]),
    "hga_count_dump": (C.c_int, [_vp, C.c_uint32, C.POINTER(_u64p), C.POINTER(_u32p), _u64p]),
    "hga_lookup_load": (C.c_int, [_vp, C.c_int, _u64p, C.c_uint32]),
    "hga_lookup_set_reads": (C.c_int, [_vp, C.c_char_p, _u64p, C.c_uint64, C.c_uint32]),
    "hga_lookup_run": (C.c_int, [_vp]),
    "hga_lookup_begin": (C.c_int, [_vp, C.c_uint32]),
    "hga_lookup_add_reads": (C.c_int, [_vp, C.c_char_p, _u64p, C.c_uint64]),
    "hga_lookup_finish": (C.c_int, [_vp]),
    "hga_lookup_batch_estimate": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _u64p]),
    "hga_lookup_get_batch_stats": (C.c_int, [_vp, C.POINTER(LookupBatchStats)]),
    "hga_lookup_get_sizes": (C.c_int, [_vp, C.POINTER(LookupSizes)]),
    "hga_lookup_fetch": (C.c_int, [_vp, C.POINTER(LookupResult)]),
    "hga_connections_run": (C.c_int, [_vp, _u32p, C.c_uint64, C.c_uint32, C.c_uint64, _i32p, _u64p]),
    "hga_connections_fetch": (C.c_int, [_vp, _u32p, _u32p, _u64p, _u8p]),
    "hga_connections_fetch_range": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _u32p, _u32p, _u64p, _u8p]),
    "hga_connections_quality": (C.c_int, [_vp, _u32p, _u32p, _u64p, _u8p, C.c_uint64, C.c_int, _i32p, C.POINTER(_u64p),
                                          C.POINTER(_u64p), C.POINTER(_u64p), _u64p]),
    "hga_connections_quality_tile": (C.c_uint32, []),
    "hga_read_overlaps": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, _i32p, _u32p]),
    "hga_components_merge": (C.c_int, [_vp, _u64p, _u32p, C.c_uint64]),
    "hga_components_connections": (C.c_int, [_vp, _u32p, C.c_uint64, C.c_uint64, _u64p]),
    "hga_components_overlaps": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, _i32p, _u32p]),
    "hga_components_set_scores": (C.c_int, [_vp, _u64p, _u32p, C.c_uint64, _u32p, _u32p, C.c_uint64, _u64p, _u64p]),
    "hga_tree_tails": (C.c_int, [_vp, _u64p, _u32p, _u32p, C.c_uint64, _i32p, _u32p, C.c_uint64, _u64p, _u32p, _u64p,
                                 _u32p, C.POINTER(TreeEnds)]),
    "hga_spanning_forest": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint64, _u64p]),
    "hga_spanning_forest_restricted": (C.c_int, [_vp, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint64, _u32p, C.c_uint64,
                                                 _u64p]),
    "hga_spanning_forest_fetch": (C.c_int, [_vp, _u64p, _u32p, _u32p]),
    "hga_components_get_sizes": (C.c_int, [_vp, C.POINTER(ComponentsSizes)]),
    "hga_components_fetch_index": (C.c_int, [_vp, _u64p, _u32p]),
    "hga_components_fetch_kmers": (C.c_int, [_vp, C.c_uint32, _u32p, _u64p]),
    "hga_components_reset": (C.c_int, [_vp]),
    "hga_hll_registers": (C.c_int, [_vp, C.c_int, C.c_uint32, _u8p]),
    "hga_profile_enable": (C.c_int, [_vp, C.c_int]),
    "hga_profile_select": (C.c_int, [_vp, C.c_char_p]),
    "hga_profile_reset": (C.c_int, [_vp]),
    "hga_profile_get": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double), _u64p]),
    "hga_sync": (C.c_int, [_vp]),
    "hga_comm_unique_id": (C.c_int, [_vp]),
    "hga_comm_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "hga_comm_init_host": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(Transport)]),
    "hga_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hga_comm_destroy": (C.c_int, [_vp]),
    "hga_comm_set_root": (C.c_int, [_vp, C.c_int]),
    "hga_count_exchange": (C.c_int, [_vp, C.c_uint32]),
    "hga_lookup_gather": (C.c_int, [_vp]),
    "hga_connections_gather": (C.c_int, [_vp, _u64p]),
}

HOST_SYMBOLS = {
    "hgh_last_error": (C.c_char_p, []),
    "hgh_free": (None, [_vp]),
    "hgh_gen_genome": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "hgh_gen_haplotype": (C.c_int, [C.c_char_p, C.c_uint64, C.c_double, C.c_uint64, C.c_uint64,
                                    C.POINTER(_vp), _u64p]),
    "hgh_gen_art": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(_vp), _u64p,
                              C.POINTER(_vp), C.POINTER(_u64p), _u64p]),
    "hgh_gen_nanosim": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_vp), _u64p,
                                  C.POINTER(_vp), C.POINTER(_u64p), _u64p]),
    "hgh_write_art_fastq": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64,
                                      C.c_char_p]),
    "hgh_write_nanosim_fasta": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64,
                                          C.c_char_p]),
    "hgh_load_records": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_u64p),
                                   C.POINTER(_i32p), C.POINTER(_u32p), C.POINTER(_u32p), _u64p,
                                   C.POINTER(_u64p), C.POINTER(_vp)]),
    "hgh_jf_stream": (C.c_int, [C.c_char_p, C.POINTER(_vp), _u64p, _u64p]),
    "hgh_cut_records": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(_u64p), _u64p]),
    "hgh_fmt_double": (C.c_int, [C.c_double, C.c_char_p, C.c_int]),
    "hgh_hll_estimate": (C.c_double, [_u8p, C.c_int]),
    "hgh_set_threads": (None, [C.c_int]),
    "hgh_load_kmer_text": (C.c_int, [C.c_char_p, C.POINTER(_u64p), _u64p, C.POINTER(C.c_int)]),
    "hgh_unordered_set_order": (C.c_int, [_u64p, C.c_uint64, C.POINTER(_u64p), _u64p]),
    "hgh_write_kmer_dump": (C.c_int, [C.c_char_p, C.c_int, _u64p, _u32p, C.c_uint64]),
}


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def lib():
    """The HIP library (lib/libhga.so).  Raises if it was not built."""
    global _lib
    if _lib is None:
        path = os.environ.get("HGA_LIB") or os.path.join(LIB_DIR, "libhga.so")   # HGA_LIB: tuning variants
        if not os.path.exists(path):
            raise HgaError(f"{path} missing: build it with `make -C hybrid-genome-assembler_amd`")
        _lib = C.CDLL(path)
        _bind(_lib, HGA_SYMBOLS)
    return _lib


def host():
    global _host
    if _host is None:
        path = os.path.join(LIB_DIR, "libhga_host.so")
        if not os.path.exists(path):
            raise HgaError(f"{path} missing: build it with `make -C hybrid-genome-assembler_amd`")
        _host = C.CDLL(path)
        _bind(_host, HOST_SYMBOLS)
    return _host


def _ck(status):
    if status != 0:
        raise HgaError(f"hga status {status}: {lib().hga_last_error().decode()}")


def _hck(status):
    if status != 0:
        raise HgaError(f"host: {host().hgh_last_error().decode()}")


def _take(ptr, n, dtype, free):
    """Copy n items of dtype from a library-allocated pointer into numpy, then free it."""
    try:
        if n == 0:
            return np.zeros(0, dtype=dtype)
        addr = ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr)
        return np.frombuffer(buf, dtype=dtype).copy()
    finally:
        free(ptr)


def _p(arr, ct):
    return arr.ctypes.data_as(C.POINTER(ct))


def comm_unique_id() -> bytes:
    """RCCL unique id (HGA_UNIQUE_ID_BYTES) to hand to every rank's Ctx.comm_init."""
    b = C.create_string_buffer(128)
    _ck(lib().hga_comm_unique_id(b))
    return b.raw


def transport_of(alltoallv, nranks: int):
    """An hga_transport whose callback calls alltoallv(send, recv), each a list of (address, nbytes)
    per rank; an exception becomes a failed status.  Keep the returned object alive while in use."""
    def cb(_user, send, sb, recv, rb):
        try:
            alltoallv([(send[p] or 0, int(sb[p])) for p in range(nranks)],
                      [(recv[p] or 0, int(rb[p])) for p in range(nranks)])
            return 0
        except Exception as e:   # noqa: BLE001 - reported through the status
            import sys
            print(f"hga transport callback failed: {e!r}", file=sys.stderr)
            return 1
    fn = ALLTOALLV_FN(cb)
    t = Transport(None, fn)
    t._keep = fn
    return t


def device_count() -> int:
    n = C.c_int(0)
    _ck(lib().hga_device_count(C.byref(n)))
    return n.value


class Ctx:
    """One hga_ctx (one HIP stream on one device)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _ck(lib().hga_ctx_create(C.byref(self._h), device))
        self.n_files = 0

    def close(self):
        if self._h:
            lib().hga_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- multi-GPU (include/hga.h: hga_comm_*, hga_count_exchange)
    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        _ck(lib().hga_comm_init(self._h, C.c_char_p(unique_id), rank, nranks))

    def comm_init_host(self, rank: int, nranks: int, transport: "Transport"):
        self._transport = transport
        _ck(lib().hga_comm_init_host(self._h, rank, nranks, C.byref(transport)))

    def comm_set_root(self, root: int):
        """Gathered lists (select / select_ex / rows / dump after an exchange) on rank `root` only; the
        other ranks get empty ones (-1: every rank)."""
        _ck(lib().hga_comm_set_root(self._h, root))

    def comm_info(self):
        r, n = C.c_int(), C.c_int()
        _ck(lib().hga_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_destroy(self):
        _ck(lib().hga_comm_destroy(self._h))

    def count_exchange(self, min_per_file: int = 2):
        _ck(lib().hga_count_exchange(self._h, min_per_file))

    def lookup_gather(self):
        _ck(lib().hga_lookup_gather(self._h))

    def connections_gather(self) -> int:
        n = C.c_uint64()
        _ck(lib().hga_connections_gather(self._h, C.byref(n)))
        return n.value

    # ---- counting
    def count_begin(self, k: int, n_files: int):
        _ck(lib().hga_count_begin(self._h, k, n_files))
        self.n_files = n_files

    def count_add(self, file: int, seq: bytes):
        _ck(lib().hga_count_add(self._h, file, seq, len(seq)))

    def count_add_file(self, file: int, data: bytes) -> dict:
        """The raw bytes of a FASTA / FASTQ file (or a piece cut at a record start, cut_records), parsed on
        the device into the file's stream (hga_count_add_file).  Returns layout (0 empty, 1 FASTA, 2 FASTQ,
        3 refused: nothing added, parse on the host), records, lines and seq_bytes."""
        info = IngestInfo()
        _ck(lib().hga_count_add_file(self._h, file, data, len(data), C.byref(info)))
        return {"layout": info.layout, "records": info.records, "lines": info.lines, "seq_bytes": info.seq_bytes}

    def count_seq(self, file: int) -> bytes:
        """The resident stream of a file, as count_add / count_add_file left it."""
        p, n = _vp(), C.c_uint64()
        _ck(lib().hga_count_seq(self._h, file, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib().hga_free(p)

    def count_add_rows(self, file: int, keys, counts):
        """Rows of a cached `<reads>_<k>-mers_sorted` dump for `file` (summed in verbatim)."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if len(k) != len(c):
            raise ValueError("keys and counts differ in length")
        _ck(lib().hga_count_add_rows(self._h, file, k.ctypes.data_as(_u64p), c.ctypes.data_as(_u32p), len(k)))

    def count_run(self, min_per_file: int = 2):
        _ck(lib().hga_count_run(self._h, min_per_file))

    def count_stats(self) -> CountStats:
        s = CountStats()
        _ck(lib().hga_count_get_stats(self._h, C.byref(s)))
        return s

    def count_set_passes(self, passes: int = 0, budget: int = 0):
        """Key-range passes of the following count_run calls: `passes` (0: chosen from `budget`),
        `budget` = device bytes the work buffers and rows may use (0: the free device memory)."""
        _ck(lib().hga_count_set_passes(self._h, passes, budget))

    def count_estimate(self, min_count: int, passes: int) -> int:
        """Bytes count_run(min_count) would request at `passes` for what has been added (host arithmetic)."""
        b = C.c_uint64()
        _ck(lib().hga_count_estimate(self._h, min_count, passes, C.byref(b)))
        return b.value

    def count_pass_stats(self) -> CountPassStats:
        s = CountPassStats()
        _ck(lib().hga_count_get_pass_stats(self._h, C.byref(s)))
        return s

    def spec_hist(self, thresholds):
        thr = np.ascontiguousarray(thresholds, dtype=np.float64)
        p = _i64p()
        n = C.c_uint64()
        _ck(lib().hga_count_spec_hist(self._h, _p(thr, C.c_double), len(thr), C.byref(p), C.byref(n)))
        return _take(p, 3 * n.value, np.int64, lib().hga_free).reshape(-1, 3)

    def select(self, lower: int, upper: int):
        k = _u64p()
        f = _u8p()
        n = C.c_uint64()
        d = C.c_uint64()
        _ck(lib().hga_count_select_ex(self._h, lower, upper, C.byref(k), C.byref(f), C.byref(n), C.byref(d)))
        keys = _take(k, n.value, np.uint64, lib().hga_free)
        flags = _take(f, n.value, np.uint8, lib().hga_free)
        return keys, flags, d.value

    def select_device(self, lower: int, upper: int):
        n = C.c_uint64()
        d = C.c_uint64()
        _ck(lib().hga_count_select_device(self._h, lower, upper, C.byref(n), C.byref(d)))
        return n.value, d.value

    def count_partition(self, splitters, keys_out_ptr: int, counts_out_ptr: int):
        """Rows grouped by owner into device buffers (raw pointers, e.g. torch data_ptr()).
        Returns rows per owner (numpy u64)."""
        spl = np.ascontiguousarray(splitters, dtype=np.uint64)
        n_own = len(spl) + 1
        out = np.zeros(n_own, np.uint64)
        _ck(lib().hga_count_partition(self._h, _p(spl, C.c_uint64), n_own, C.c_void_p(keys_out_ptr),
                                      C.c_void_p(counts_out_ptr), _p(out, C.c_uint64)))
        return out

    def count_merge(self, keys_ptr: int, counts_ptr: int, n: int, min_per_file: int = 2):
        """Owner-side merge of received rows (device pointers); they become the ctx rows."""
        _ck(lib().hga_count_merge(self._h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), n, min_per_file))

    def count_pack_bits(self) -> int:
        b = C.c_int()
        _ck(lib().hga_count_pack_bits(self._h, C.byref(b)))
        return b.value

    def count_partition_packed(self, splitters, out_ptr: int, capacity: int):
        """Packed pieces grouped by owner into a device buffer.  Returns (pieces per owner, total);
        total > capacity means nothing was written (retry with more room)."""
        spl = np.ascontiguousarray(splitters, dtype=np.uint64)
        n_own = len(spl) + 1
        per = np.zeros(n_own, np.uint64)
        tot = C.c_uint64()
        st = lib().hga_count_partition_packed(self._h, _p(spl, C.c_uint64), n_own, C.c_void_p(out_ptr), capacity,
                                               _p(per, C.c_uint64), C.byref(tot))
        if st == 3 and tot.value > capacity:   # HGA_ERR_OOM: caller retries
            return per, tot.value
        _ck(st)
        return per, tot.value

    def count_merge_packed(self, pieces_ptr: int, n: int, min_per_file: int = 2):
        _ck(lib().hga_count_merge_packed(self._h, C.c_void_p(pieces_ptr), n, min_per_file))

    def rows(self):
        k = _u64p()
        c = _u32p()
        n = C.c_uint64()
        _ck(lib().hga_count_rows(self._h, C.byref(k), C.byref(c), C.byref(n)))
        keys = _take(k, n.value, np.uint64, lib().hga_free)
        cnts = _take(c, n.value * self.n_files, np.uint32, lib().hga_free).reshape(-1, self.n_files)
        return keys, cnts

    def dump(self, file: int):
        k = _u64p()
        c = _u32p()
        n = C.c_uint64()
        _ck(lib().hga_count_dump(self._h, file, C.byref(k), C.byref(c), C.byref(n)))
        return _take(k, n.value, np.uint64, lib().hga_free), _take(c, n.value, np.uint32, lib().hga_free)

    # ---- lookup
    def lookup_load(self, k: int, keys_in_id_order):
        keys = np.ascontiguousarray(keys_in_id_order, dtype=np.uint64)
        _ck(lib().hga_lookup_load(self._h, k, _p(keys, C.c_uint64), len(keys)))

    def lookup_set_reads(self, bases: bytes, offsets, first_read_id: int = 1):
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        _ck(lib().hga_lookup_set_reads(self._h, bases, _p(off, C.c_uint64), len(off) - 1, first_read_id))

    def lookup_run(self):
        _ck(lib().hga_lookup_run(self._h))

    # the lookup in read batches: begin, add_reads per batch (a CSR of whole reads), finish
    def lookup_begin(self, first_read_id: int = 1):
        _ck(lib().hga_lookup_begin(self._h, first_read_id))

    def lookup_add_reads(self, bases: bytes, offsets):
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        _ck(lib().hga_lookup_add_reads(self._h, bases, _p(off, C.c_uint64), len(off) - 1))

    def lookup_finish(self):
        _ck(lib().hga_lookup_finish(self._h))

    def lookup_batch_estimate(self, batch_bases: int, batch_reads: int) -> int:
        """Device bytes of a session's two slots for batches of at most this size (host arithmetic)."""
        b = C.c_uint64()
        _ck(lib().hga_lookup_batch_estimate(self._h, batch_bases, batch_reads, C.byref(b)))
        return b.value

    def lookup_batch_stats(self) -> LookupBatchStats:
        s = LookupBatchStats()
        _ck(lib().hga_lookup_get_batch_stats(self._h, C.byref(s)))
        return s

    def lookup_sizes(self) -> LookupSizes:
        s = LookupSizes()
        _ck(lib().hga_lookup_get_sizes(self._h, C.byref(s)))
        return s

    def lookup_fetch(self) -> dict:
        s = self.lookup_sizes()
        n, H, U, K = s.n_reads, s.hits, s.firsts, s.n_sdk
        out = {
            "hit_ptr": np.zeros(n + 1, np.uint64), "hit_kid": np.zeros(H, np.uint32),
            "hit_pos": np.zeros(H, np.uint32), "sorted_kid": np.zeros(H, np.uint32),
            "first_ptr": np.zeros(n + 1, np.uint64), "first_kid": np.zeros(U, np.uint32),
            "first_pos": np.zeros(U, np.uint32), "kci_ptr": np.zeros(K + 1, np.uint64),
            "kci_read": np.zeros(H, np.uint32),
        }
        r = LookupResult()
        for name, arr in out.items():
            setattr(r, name, _p(arr, C.c_uint64 if arr.dtype == np.uint64 else C.c_uint32))
        _ck(lib().hga_lookup_fetch(self._h, C.byref(r)))
        return out

    # ---- connections (get_connections / get_all_connections on the lookup's indices)
    def connections_run(self, pivots=None, min_kmers: int = 1, min_score: int = 1, categories=None) -> int:
        n = C.c_uint64()
        pv = None if pivots is None else np.ascontiguousarray(pivots, np.uint32)
        cat = None if categories is None else np.ascontiguousarray(categories, np.int32)
        self._keep = (pv, cat)
        _ck(lib().hga_connections_run(self._h, None if pv is None else _p(pv, C.c_uint32),
                                      0 if pv is None else len(pv), min_kmers, min_score,
                                      None if cat is None else _p(cat, C.c_int32), C.byref(n)))
        self._conn_n = n.value
        return n.value

    def connections(self, pivots=None, min_kmers: int = 1, min_score: int = 1, categories=None):
        """(x, y, score, is_good) ordered by score descending, then (x, y) ascending."""
        m = self.connections_run(pivots, min_kmers, min_score, categories)
        x, y = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        sc, g = np.zeros(m, np.uint64), np.zeros(m, np.uint8)
        _ck(lib().hga_connections_fetch(self._h, _p(x, C.c_uint32), _p(y, C.c_uint32), _p(sc, C.c_uint64),
                                        _p(g, C.c_uint8)))
        return x, y, sc, g

    def connections_range(self, first: int, count: int):
        """Entries [first, first + count) (clipped) of the last connections_run result."""
        m = max(0, min(count, self._conn_n - min(first, self._conn_n)))
        x, y = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        sc, g = np.zeros(m, np.uint64), np.zeros(m, np.uint8)
        _ck(lib().hga_connections_fetch_range(self._h, first, count, _p(x, C.c_uint32), _p(y, C.c_uint32),
                                              _p(sc, C.c_uint64), _p(g, C.c_uint8)))
        return x, y, sc, g

    # ---- connection quality (plot_connection_quality's histograms of an ordered list)
    def connections_quality(self, x=None, y=None, score=None, is_good=None, per_candidate: bool = False,
                            vertex_class=None):
        """(score uint64[r] ascending, good uint64[r], bad uint64[r]): per distinct score the counted
        connections that are good / bad.  x, y, score all None: the ctx's current ordered connection
        result; all given: rows in result order (score non-increasing), is_good None = all 0.
        per_candidate: one count per distinct y, from its row of the smallest position.  vertex_class:
        one int per read of the lookup; good = class[x] == class[y] then replaces the stored flag."""
        def arr(v, dt):
            return None if v is None else np.ascontiguousarray(v, dt).ravel()
        xv, yv, sv, gv = arr(x, np.uint32), arr(y, np.uint32), arr(score, np.uint64), arr(is_good, np.uint8)
        vc = arr(vertex_class, np.int32)
        lens = {len(v) for v in (xv, yv, sv, gv) if v is not None}
        if len(lens) > 1:
            raise ValueError("x, y, score and is_good must be of equal length")
        if vc is not None and len(vc) != self.lookup_sizes().n_reads:
            raise ValueError("vertex_class must hold one value per read of the lookup result")
        ps, pg, pb = _u64p(), _u64p(), _u64p()
        r = C.c_uint64()
        # (an empty list is still a given list: NULL would mean the ctx's result)
        ptr = lambda v, ct: None if v is None else _p(v if len(v) else np.zeros(1, v.dtype), ct)
        _ck(lib().hga_connections_quality(self._h, ptr(xv, C.c_uint32), ptr(yv, C.c_uint32), ptr(sv, C.c_uint64),
                                          ptr(gv, C.c_uint8), lens.pop() if lens else 0, 1 if per_candidate else 0,
                                          ptr(vc, C.c_int32), C.byref(ps), C.byref(pg), C.byref(pb), C.byref(r)))
        free = lib().hga_free
        return (_take(ps, r.value, np.uint64, free), _take(pg, r.value, np.uint64, free),
                _take(pb, r.value, np.uint64, free))

    # ---- read overlaps (approximate_read_overlap on the lookup's first-occurrence lists)
    def read_overlaps(self, x, y):
        """(overlap int32[n], shared uint32[n]) of the ReadID pairs (x[i], y[i])."""
        xv, yv = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
        if xv.shape != yv.shape or xv.ndim != 1:
            raise ValueError("x and y must be one-dimensional and of equal length")
        ov, sh = np.zeros(len(xv), np.int32), np.zeros(len(xv), np.uint32)
        _ck(lib().hga_read_overlaps(self._h, _p(xv, C.c_uint32), _p(yv, C.c_uint32), len(xv), _p(ov, C.c_int32),
                                    _p(sh, C.c_uint32)))
        return ov, sh

    # ---- merged components (merge_components / get_connections on the state merges leave)
    def components_merge(self, groups):
        """One merge_components call: groups is a list of ReadID lists, the first id of each survives."""
        gp = np.zeros(len(groups) + 1, np.uint64)
        gp[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64)
        ids = np.ascontiguousarray([i for g in groups for i in g], np.uint32)
        _ck(lib().hga_components_merge(self._h, _p(gp, C.c_uint64), _p(ids, C.c_uint32), len(groups)))

    def components_connections(self, pivots, min_score: int = 1) -> int:
        """get_connections of the pivots on the current component state; fetch with connections_range."""
        pv = np.ascontiguousarray(pivots, np.uint32)
        n = C.c_uint64()
        _ck(lib().hga_components_connections(self._h, _p(pv, C.c_uint32), len(pv), min_score, C.byref(n)))
        self._conn_n = n.value
        return n.value

    def components_overlaps(self, x, y):
        """(overlap int32[n], shared uint32[n]) of the id pairs (x[i], y[i]) on the current component lists."""
        xv, yv = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
        if xv.shape != yv.shape or xv.ndim != 1:
            raise ValueError("x and y must be one-dimensional and of equal length")
        ov, sh = np.zeros(len(xv), np.int32), np.zeros(len(xv), np.uint32)
        _ck(lib().hga_components_overlaps(self._h, _p(xv, C.c_uint32), _p(yv, C.c_uint32), len(xv), _p(ov, C.c_int32),
                                          _p(sh, C.c_uint32)))
        return ov, sh

    def components_set_scores(self, sets, pairs):
        """sets: a list of id lists, pairs: (n, 2) set indices.  (score uint64[n_pairs], set_size
        uint64[n_sets]): the sizes of the pairwise intersections of the sets' KmerID unions, and of the unions."""
        sp = np.zeros(len(sets) + 1, np.uint64)
        sp[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
        ids = np.ascontiguousarray([i for s in sets for i in s], np.uint32)
        pr = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        score, size = np.zeros(len(pr), np.uint64), np.zeros(len(sets), np.uint64)
        _ck(lib().hga_components_set_scores(self._h, _p(sp, C.c_uint64), _p(ids, C.c_uint32), len(sets), _p(pa, C.c_uint32),
                                            _p(pb, C.c_uint32), len(pr), _p(score, C.c_uint64), _p(size, C.c_uint64)))
        return score, size

    # ---- spanning-tree tails (get_spanning_tree_tails of every tree in one call)
    def tree_tails(self, trees, overlap=None, read_length=None, tail_length: int = 0):
        """trees: a list of edge lists [(x, y), ...].  overlap: one int per edge in the trees' order, or None
        for hga_components_overlaps' answers on the current component state; read_length: per read of the
        lookup result (by id - first_read_id), or None for the ctx's own reads.  Returns (left, right, ends):
        per tree the two ascending id arrays (uint32) and (right_id, right_dist, left_id, left_dist)."""
        nt = len(trees)
        tp = np.zeros(nt + 1, np.uint64)
        tp[1:] = np.cumsum([len(t) for t in trees], dtype=np.uint64)
        ne = int(tp[nt])
        xy = np.ascontiguousarray([e for t in trees for e in t], np.uint32).reshape(-1, 2)
        ex, ey = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
        ov = None if overlap is None else np.ascontiguousarray(overlap, np.int32)
        if ov is not None and ov.shape != (ne,):
            raise ValueError("overlap must hold one value per edge")
        rl = None if read_length is None else np.ascontiguousarray(read_length, np.uint32)
        if rl is not None and rl.shape != (self.lookup_sizes().n_reads,):
            raise ValueError("read_length must hold one value per read of the lookup result")
        lp, rp = np.zeros(nt + 1, np.uint64), np.zeros(nt + 1, np.uint64)
        left, right = np.zeros(ne + nt, np.uint32), np.zeros(ne + nt, np.uint32)
        ends = (TreeEnds * max(nt, 1))()
        _ck(lib().hga_tree_tails(self._h, _p(tp, C.c_uint64), _p(ex, C.c_uint32), _p(ey, C.c_uint32), nt,
                                 None if ov is None else _p(ov, C.c_int32), None if rl is None else _p(rl, C.c_uint32),
                                 tail_length, _p(lp, C.c_uint64), _p(left, C.c_uint32), _p(rp, C.c_uint64),
                                 _p(right, C.c_uint32), ends))
        return ([left[int(lp[t]):int(lp[t + 1])].copy() for t in range(nt)],
                [right[int(rp[t]):int(rp[t + 1])].copy() for t in range(nt)],
                [(e.right_id, e.right_dist, e.left_id, e.left_dist) for e in ends[:nt]])

    # ---- spanning forest (the connections an uncapped union_find accepts)
    def spanning_forest(self, x=None, y=None, first: int = 0, count=None, restricted=None):
        """(pos uint64[m], x uint32[m], y uint32[m]): the ascending positions in [first, first + count)
        (clipped; count None: to the end) at which union_find joins two components, and the connections
        there.  x, y: ReadID arrays, or both None for the ctx's current ordered connection result.
        restricted: ReadIDs of which no two may end in one component (union_find's restricted set), through
        hga_spanning_forest_restricted; None: hga_spanning_forest."""
        if (x is None) != (y is None):
            raise ValueError("x and y must both be given or both be None")
        xv = yv = None
        if x is not None:
            xv, yv = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
            if xv.shape != yv.shape or xv.ndim != 1:
                raise ValueError("x and y must be one-dimensional and of equal length")
        m = C.c_uint64()
        edges = (self._h, None if xv is None else _p(xv, C.c_uint32), None if yv is None else _p(yv, C.c_uint32),
                 0 if xv is None else len(xv), first, 2 ** 64 - 1 if count is None else count)
        if restricted is None:
            _ck(lib().hga_spanning_forest(*edges, C.byref(m)))
        else:
            rv = np.ascontiguousarray(restricted, np.uint32).ravel()
            _ck(lib().hga_spanning_forest_restricted(*edges, _p(rv, C.c_uint32) if len(rv) else None, len(rv), C.byref(m)))
        pos, ox, oy = np.zeros(m.value, np.uint64), np.zeros(m.value, np.uint32), np.zeros(m.value, np.uint32)
        _ck(lib().hga_spanning_forest_fetch(self._h, _p(pos, C.c_uint64), _p(ox, C.c_uint32), _p(oy, C.c_uint32)))
        return pos, ox, oy

    def components_sizes(self) -> ComponentsSizes:
        s = ComponentsSizes()
        _ck(lib().hga_components_get_sizes(self._h, C.byref(s)))
        return s

    def components_index(self):
        """The current kmer_component_index as a CSR of ReadIDs: (ptr uint64[K + 1], ids uint32[entries])."""
        ptr = np.zeros(self.lookup_sizes().n_sdk + 1, np.uint64)
        ids = np.zeros(self.components_sizes().index_entries, np.uint32)
        _ck(lib().hga_components_fetch_index(self._h, _p(ptr, C.c_uint64), _p(ids, C.c_uint32)))
        return ptr, ids

    def components_kmers(self, id: int):
        """The current KmerID list of one id (uint32, ascending)."""
        n = C.c_uint64()
        _ck(lib().hga_components_fetch_kmers(self._h, id, None, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        _ck(lib().hga_components_fetch_kmers(self._h, id, _p(out, C.c_uint32), C.byref(n)))
        return out

    def components_reset(self):
        _ck(lib().hga_components_reset(self._h))

    # ---- HyperLogLog auto-k (KmerAnalysis.cpp:15-56) on the reads of lookup_set_reads
    def hll_registers(self, k: int, b: int = 10):
        """hll::HyperLogLog(b) registers over every KmerIterator window (HyperLogLog.hpp:96-106)."""
        regs = np.zeros(1 << b, np.uint8)
        _ck(lib().hga_hll_registers(self._h, k, b, _p(regs, C.c_uint8)))
        return regs

    def approximate_kmer_count(self, k: int) -> int:
        """get_approximate_kmer_count (KmerAnalysis.cpp:26-38): the estimate truncated to uint64."""
        return int(hll_estimate(self.hll_registers(k, 10), 10))

    def unique_k_length(self):
        """get_unique_k_length (KmerAnalysis.cpp:41-56): ((k, count), the printed lines)."""
        lines = []
        k = 11
        prev = self.approximate_kmer_count(k)
        lines.append(f"k=11 : ~{prev} kmers")
        while k < 33:
            cnt = self.approximate_kmer_count(k + 2)
            lines.append(f"k={k + 2} : ~{cnt} kmers")
            if cnt + prev and abs(cnt - prev) / ((cnt + prev) / 2.0) < 0.1:
                return (k, prev), lines
            k += 2
            prev = cnt
        return (k, prev), lines

    # ---- measurement
    def profile(self, on: bool = True):
        _ck(lib().hga_profile_enable(self._h, 1 if on else 0))

    def profile_select(self, names=()):
        """Time only these launch names (empty: all)."""
        _ck(lib().hga_profile_select(self._h, ",".join(names).encode()))

    def profile_reset(self):
        _ck(lib().hga_profile_reset(self._h))

    def profile_get(self, name: str):
        ms = C.c_double()
        n = C.c_uint64()
        _ck(lib().hga_profile_get(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sync(self):
        _ck(lib().hga_sync(self._h))


# ---------------------------------------------------------------- host helpers
def gen_genome(length: int, seed: int) -> bytes:
    p = C.c_void_p()
    _hck(host().hgh_gen_genome(length, seed, C.byref(p)))
    return bytes(_take(p.value, length, np.uint8, host().hgh_free))


def gen_haplotype(src: bytes, d: float, extra: int, seed: int) -> bytes:
    p = C.c_void_p()
    n = C.c_uint64()
    _hck(host().hgh_gen_haplotype(src, len(src), d, extra, seed, C.byref(p), C.byref(n)))
    return bytes(_take(p.value, n.value, np.uint8, host().hgh_free))


@dataclass
class Reads:
    seq: bytes               # '\n'-joined stream (counting input)
    bases: bytes             # concatenated sequences (lookup input)
    offsets: np.ndarray      # CSR, n+1

    @property
    def n(self):
        return len(self.offsets) - 1


def _reads_from(fn, *args) -> Reads:
    sp, bp = C.c_void_p(), C.c_void_p()
    sl = C.c_uint64()
    op = _u64p()
    nr = C.c_uint64()
    _hck(fn(*args, C.byref(sp), C.byref(sl), C.byref(bp), C.byref(op), C.byref(nr)))
    offsets = _take(op, nr.value + 1, np.uint64, host().hgh_free)
    seq = bytes(_take(sp.value, sl.value, np.uint8, host().hgh_free))
    bases = bytes(_take(bp.value, int(offsets[-1]), np.uint8, host().hgh_free)) if offsets[-1] else (
        host().hgh_free(bp.value) or b"")
    return Reads(seq, bases, offsets)


def gen_art(genome: bytes, n_reads: int, read_len: int, seed: int) -> Reads:
    return _reads_from(host().hgh_gen_art, genome, len(genome), n_reads, read_len, seed)


def gen_nanosim(genome: bytes, n_reads: int, seed: int) -> Reads:
    return _reads_from(host().hgh_gen_nanosim, genome, len(genome), n_reads, seed)


def write_art_fastq(genome: bytes, name: str, n_reads: int, read_len: int, seed: int, path: str):
    _hck(host().hgh_write_art_fastq(genome, len(genome), name.encode(), n_reads, read_len, seed, path.encode()))


def write_nanosim_fasta(genome: bytes, name: str, n_reads: int, seed: int, path: str):
    _hck(host().hgh_write_nanosim_fasta(genome, len(genome), name.encode(), n_reads, seed, path.encode()))


def write_kmer_dump(path: str, k: int, keys, counts):
    """The jf_occurrences dump cache writer ("KMER COUNT" lines, host/seqio.cpp write_kmer_dump)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    _hck(host().hgh_write_kmer_dump(path.encode(), k, keys.ctypes.data_as(_u64p), counts.ctypes.data_as(_u32p), len(keys)))


def load_kmer_text(path: str):
    """categorization's SDK loader (load_text_file_kmers, read_clustering.cpp:18-33): (codes in KmerID
    order, k)."""
    p, n, k = _u64p(), C.c_uint64(), C.c_int()
    _hck(host().hgh_load_kmer_text(path.encode(), C.byref(p), C.byref(n), C.byref(k)))
    return _take(p, n.value, np.uint64, host().hgh_free), k.value


def unordered_set_order(keys):
    """The iteration order of a std::unordered_set<uint64_t> filled with `keys` in order."""
    keys = np.ascontiguousarray(keys, np.uint64)
    p, m = _u64p(), C.c_uint64()
    _hck(host().hgh_unordered_set_order(keys.ctypes.data_as(_u64p), len(keys), C.byref(p), C.byref(m)))
    return _take(p, m.value, np.uint64, host().hgh_free)


def set_host_threads(n: int):
    """Reader threads of load_records / jf_stream (1 = the sequential readers, 0 = default)."""
    host().hgh_set_threads(n)


def load_records(paths, annotate: bool):
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    bp = C.c_void_p()
    op, sp, ep = _u64p(), _u32p(), _u32p()
    cp = _i32p()
    n = C.c_uint64()
    mp = _u64p()
    fp = C.c_void_p()
    _hck(host().hgh_load_records(arr, len(paths), 1 if annotate else 0, C.byref(bp), C.byref(op), C.byref(cp),
                                 C.byref(sp), C.byref(ep), C.byref(n), C.byref(mp), C.byref(fp)))
    nr = n.value
    offsets = _take(op, nr + 1, np.uint64, host().hgh_free)
    bases = bytes(_take(bp.value, int(offsets[-1]), np.uint8, host().hgh_free))
    meta = _take(mp, (len(paths) + 1) * 5, np.uint64, host().hgh_free).reshape(-1, 5)
    fname = C.string_at(fp.value).decode()
    host().hgh_free(fp.value)
    return {
        "bases": bases, "offsets": offsets,
        "category": _take(cp, nr, np.int32, host().hgh_free),
        "start": _take(sp, nr, np.uint32, host().hgh_free),
        "end": _take(ep, nr, np.uint32, host().hgh_free),
        "meta": meta, "filename": fname,
    }


def ingest_tile() -> int:
    """Input bytes per workgroup of hga_count_add_file's kernels."""
    return int(lib().hga_ingest_tile())


def cut_records(data: bytes, piece: int) -> np.ndarray:
    """Piece starts of a FASTA / FASTQ file for Ctx.count_add_file: 0, then the first record start at or
    after each multiple of `piece` (seqio.h cut_records)."""
    p, n = _u64p(), C.c_uint64()
    _hck(host().hgh_cut_records(data, len(data), piece, C.byref(p), C.byref(n)))
    return _take(p, n.value, np.uint64, host().hgh_free)


def jf_stream(path: str) -> bytes:
    p = C.c_void_p()
    n = C.c_uint64()
    r = C.c_uint64()
    _hck(host().hgh_jf_stream(path.encode(), C.byref(p), C.byref(n), C.byref(r)))
    return bytes(_take(p.value, n.value, np.uint8, host().hgh_free)) if n.value else (
        host().hgh_free(p.value) or b"")


def hll_estimate(regs, b: int = 10) -> float:
    """hll::HyperLogLog::estimate (src/lib/HyperLogLog.hpp:113-132), host C++ (host/hll.cpp)."""
    r = np.ascontiguousarray(regs, np.uint8)
    return float(host().hgh_hll_estimate(_p(r, C.c_uint8), b))


def fmt_double(v: float) -> str:
    buf = C.create_string_buffer(64)
    n = host().hgh_fmt_double(v, buf, 64)
    return buf.value.decode() if n >= 0 else ""


# ---------------------------------------------------------------------------- clustering stages
# lib/libhga_cluster.so: ReadClusteringEngine after construct_indices (host/clustering.cpp).
class ClusterConfig(C.Structure):
    """ReadClusteringConfig (src/clustering/ReadClusteringEngine.h:138-148)."""
    _fields_ = [("sc_min_size", C.c_int), ("sc_max_size", C.c_int), ("sc_fraction", C.c_double),
                ("sc_score", C.c_uint64), ("core_enrichment", C.c_uint64), ("tail_amplification", C.c_uint64),
                ("threads", C.c_int), ("spectral_dims", C.c_int), ("force_spectral", C.c_int)]


def cluster_config(sc_min=30, sc_max=-1, sc_fraction=0.15, sc_score=0, enrich=20, tail=40, threads=1, dims=16,
                   force_spectral=False) -> ClusterConfig:
    return ClusterConfig(sc_min, sc_max, sc_fraction, sc_score, enrich, tail, threads, dims, 1 if force_spectral else 0)


CLUSTER_SYMBOLS = {
    "hgc_last_error": (C.c_char_p, []),
    "hgc_free": (None, [_vp]),
    "hgc_cluster": (C.c_int, [C.c_char_p, _u64p, _i32p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p, _u64p,
                              _u32p, _u32p, _u64p, _u32p, C.c_uint32, C.POINTER(ClusterConfig), C.c_int,
                              C.POINTER(_u32p), _u64p, C.POINTER(_u32p), C.POINTER(_vp)]),
    "hgc_cluster_batched": (C.c_int, [C.c_char_p, _u64p, _i32p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p,
                                      _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32, C.POINTER(ClusterConfig), C.c_int,
                                      C.POINTER(_u32p), _u64p, C.POINTER(_u32p), C.POINTER(_vp), C.c_int, _u64p]),
    "hgc_cluster_plots": (C.c_int, [C.c_char_p, _u64p, _i32p, _u32p, _u32p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p, _u32p,
                                    _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32, C.POINTER(ClusterConfig), C.c_int,
                                    C.POINTER(_u32p), _u64p, C.POINTER(_u32p), C.POINTER(_vp), C.c_int, _u64p, C.c_int,
                                    C.POINTER(_vp), _u64p, _u64p, _u64p]),
    "hgc_plot_connection_histogram": (C.c_int, [_u64p, _u64p, _u64p, C.c_uint64, C.POINTER(_vp)]),
    "hgc_plot_component_coverage": (C.c_int, [_u64p, _u32p, _u32p, C.c_uint64, C.POINTER(_vp)]),
    "hgc_plot_spectral_graph": (C.c_int, [_u32p, _u32p, _u64p, _i32p, _i32p, C.c_uint64, _u64p, _u32p, C.c_uint64,
                                          C.POINTER(_vp)]),
    "hgc_forest_calls": (C.c_uint64, []),
    "hgc_enrich_forest_calls": (C.c_uint64, []),
    "hgc_union_find": (C.c_int, [_u32p, _u32p, _u64p, C.c_uint64, _u32p, C.c_uint64, C.c_int, C.c_int,
                                 C.POINTER(_u64p), C.POINTER(_u32p), _u64p, C.POINTER(_u64p), C.POINTER(_u32p)]),
    "hgc_spectral": (C.c_int, [_u32p, _u32p, _u64p, C.c_uint64, C.c_int, C.POINTER(_u64p), C.POINTER(_u32p), _u64p]),
    "hgc_sym_eigen": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}
_cl = None


def cluster_lib():
    global _cl
    if _cl is None:
        path = os.path.join(LIB_DIR, "libhga_cluster.so")
        if not os.path.exists(path):
            raise HgaError(f"{path} missing: build it with `make -C hybrid-genome-assembler_amd`")
        _cl = C.CDLL(path)
        _bind(_cl, CLUSTER_SYMBOLS)
    return _cl


def _cck(status):
    if status != 0:
        raise HgaError(f"clustering: {cluster_lib().hgc_last_error().decode()}")


def _conn_arrays(conns):
    x = np.ascontiguousarray([c[0] for c in conns], np.uint32)
    y = np.ascontiguousarray([c[1] for c in conns], np.uint32)
    s = np.ascontiguousarray([c[2] for c in conns], np.uint64)
    return x, y, s


def _components(ptr, ids, n):
    L = cluster_lib()
    p = _take(ptr, n.value + 1, np.uint64, L.hgc_free)
    v = _take(ids, int(p[-1]), np.uint32, L.hgc_free)
    return [v[p[i]:p[i + 1]].tolist() for i in range(n.value)]


def union_find(conns, restricted=(), min_size=1, max_size=-1):
    """union_find (ReadClusteringEngine.cpp:424-489): [(component ids, spanning-tree edges)]."""
    x, y, s = _conn_arrays(conns)
    r = np.ascontiguousarray(sorted(restricted), np.uint32)
    cp, ci, tp, txy = _u64p(), _u32p(), _u64p(), _u32p()
    n = C.c_uint64()
    _cck(cluster_lib().hgc_union_find(_p(x, C.c_uint32), _p(y, C.c_uint32), _p(s, C.c_uint64), len(x),
                                      _p(r, C.c_uint32), len(r), min_size, max_size, C.byref(cp), C.byref(ci),
                                      C.byref(n), C.byref(tp), C.byref(txy)))
    comps = _components(cp, ci, n)
    tptr = _take(tp, n.value + 1, np.uint64, cluster_lib().hgc_free)
    t = _take(txy, 2 * int(tptr[-1]), np.uint32, cluster_lib().hgc_free).reshape(-1, 2)
    return [(comps[i], [tuple(e) for e in t[tptr[i]:tptr[i + 1]].tolist()]) for i in range(n.value)]


def spectral_clustering(conns, dims=16):
    """spectral_clustering (ReadClusteringEngine.cpp:653-697)."""
    x, y, s = _conn_arrays(conns)
    cp, ci = _u64p(), _u32p()
    n = C.c_uint64()
    _cck(cluster_lib().hgc_spectral(_p(x, C.c_uint32), _p(y, C.c_uint32), _p(s, C.c_uint64), len(x), dims,
                                    C.byref(cp), C.byref(ci), C.byref(n)))
    return _components(cp, ci, n)


def sym_eigen(a):
    a = np.ascontiguousarray(a, np.float64)
    n = a.shape[0]
    val, vec = np.zeros(n), np.zeros((n, n))
    _cck(cluster_lib().hgc_sym_eigen(_p(a, C.c_double), n, _p(val, C.c_double), _p(vec, C.c_double)))
    return val, vec


def _taken_string(p):
    s = C.string_at(p.value).decode()
    cluster_lib().hgc_free(p.value)
    return s


def plot_connection_histogram(score, good, bad) -> str:
    """plot_connection_quality's wire string (ReadClusteringEngine.cpp:32, :122) of histogram rows."""
    sv, gv, bv = (np.ascontiguousarray(v, np.uint64) for v in (score, good, bad))
    out = C.c_void_p()
    _cck(cluster_lib().hgc_plot_connection_histogram(_p(sv, C.c_uint64), _p(gv, C.c_uint64), _p(bv, C.c_uint64), len(sv),
                                                     C.byref(out)))
    return _taken_string(out)


def plot_component_coverage(components) -> str:
    """plot_read_coverage's wire string (:37-73); components: per component a list of (start, end) per read."""
    cp = np.zeros(len(components) + 1, np.uint64)
    cp[1:] = np.cumsum([len(c) for c in components], dtype=np.uint64)
    st = np.ascontiguousarray([r[0] for c in components for r in c], np.uint32)
    en = np.ascontiguousarray([r[1] for c in components for r in c], np.uint32)
    out = C.c_void_p()
    _cck(cluster_lib().hgc_plot_component_coverage(_p(cp, C.c_uint64), _p(st, C.c_uint32), _p(en, C.c_uint32),
                                                   len(components), C.byref(out)))
    return _taken_string(out)


def plot_spectral_graph(conns, first_category, partition) -> str:
    """plot_spectral's wire string (:77-98); conns: (x, y, score, ...), first_category: id -> the first
    category of its component, partition: a list of id lists."""
    x, y, s = _conn_arrays(conns)
    cx = np.ascontiguousarray([first_category[int(v)] for v in x], np.int32)
    cy = np.ascontiguousarray([first_category[int(v)] for v in y], np.int32)
    pp = np.zeros(len(partition) + 1, np.uint64)
    pp[1:] = np.cumsum([len(c) for c in partition], dtype=np.uint64)
    ids = np.ascontiguousarray([i for c in partition for i in c], np.uint32)
    out = C.c_void_p()
    _cck(cluster_lib().hgc_plot_spectral_graph(_p(x, C.c_uint32), _p(y, C.c_uint32), _p(s, C.c_uint64), _p(cx, C.c_int32),
                                               _p(cy, C.c_int32), len(x), _p(pp, C.c_uint64), _p(ids, C.c_uint32),
                                               len(partition), C.byref(out)))
    return _taken_string(out)


def cluster_host(bases: bytes, offsets, category, idx, avg_read_length, cfg=None, debug=False, first_read_id=1,
                 start=None, end=None, batched_overlaps=False, stats=None, device_sets=False, device_tails=False,
                 device_forest=False, device_enrich=False, plots=None, plot_sink=True, device_quality=False):
    """run_clustering after construct_indices on the host (no device state): (component ids,
    per-read component id (0 = none), log text).  start / end: the reads' simulator coordinates
    (print_components' intervals under debug), None = 0.
    batched_overlaps: the tail stage takes its spanning-tree edge overlaps through the batched hook
    (the device path's batching and eligibility rule) with hga_read_overlaps' semantics computed on
    the host.  stats: a dict that receives "overlap_edges_batched" and "overlap_edges_host".
    device_sets: the tail stage runs the batching of HGA_DEVICE_SETS=1 (every spanning-tree edge in one
    component-overlap call, one set-score call over the tail ids still in the index) through hooks bound
    to the engine's host implementations.
    device_tails: the tails of all scaffold trees come from one call of the tree-tails hook (the batching of
    HGA_DEVICE_TAILS=1), bound to the engine's host implementation.
    device_forest: the first union_find replays only the connections it would accept, taken from the
    spanning-forest hook (the path of HGA_DEVICE_FOREST=1), bound to the engine's host implementation;
    stats then also receives "forest_calls".
    device_enrich: the enrichment union_find replays only the connections it would accept, taken from the
    enrichment-forest hook (the path of HGA_DEVICE_ENRICH=1), bound to the engine's host implementation;
    stats then also receives "enrich_forest_calls".
    plots: a list that receives the debug plots as (kind, wire) pairs in emission order (the engine runs with a
    plot sink; plot_sink=False runs the same entry point without one); stats then also receives
    "quality_calls_device" and "quality_calls_host".  device_quality: the two connection histograms come
    through the quality hook (the path taken where the list stays on the device), bound to the engine's
    host implementation."""
    L = cluster_lib()
    cfg = cfg or cluster_config()
    off = np.ascontiguousarray(offsets, np.uint64)
    cat = np.ascontiguousarray(category, np.int32)
    a = {k: np.ascontiguousarray(idx[k], np.uint64 if k.endswith("ptr") else np.uint32)
         for k in ("hit_ptr", "sorted_kid", "first_ptr", "first_kid", "first_pos", "kci_ptr", "kci_read")}
    n = len(off) - 1
    ip, op = _u32p(), _u32p()
    lp = C.c_void_p()
    ni = C.c_uint64()
    st = None if start is None else np.ascontiguousarray(start, np.uint32)
    en = None if end is None else np.ascontiguousarray(end, np.uint32)
    ove = np.zeros(2, np.uint64)
    entry, extra = L.hgc_cluster_batched, ()
    if plots is not None:
        pp, pbytes, pn, qc = C.c_void_p(), C.c_uint64(), C.c_uint64(), np.zeros(2, np.uint64)
        entry = L.hgc_cluster_plots
        extra = (1 if plot_sink else 0, C.byref(pp), C.byref(pbytes), C.byref(pn), _p(qc, C.c_uint64))
    _cck(entry(bases, _p(off, C.c_uint64), _p(cat, C.c_int32),
                               None if st is None else _p(st, C.c_uint32), None if en is None else _p(en, C.c_uint32),
                               n, avg_read_length, first_read_id,
                               _p(a["hit_ptr"], C.c_uint64), _p(a["sorted_kid"], C.c_uint32), _p(a["first_ptr"], C.c_uint64),
                               _p(a["first_kid"], C.c_uint32), _p(a["first_pos"], C.c_uint32), _p(a["kci_ptr"], C.c_uint64),
                               _p(a["kci_read"], C.c_uint32), len(a["kci_ptr"]) - 1, C.byref(cfg), 1 if debug else 0,
                               C.byref(ip), C.byref(ni), C.byref(op), C.byref(lp),
                               (1 if batched_overlaps else 0) | (2 if device_sets else 0) | (4 if device_tails else 0) |
                               (8 if device_forest else 0) | (16 if device_enrich else 0) | (32 if device_quality else 0),
                               _p(ove, C.c_uint64), *extra))
    if plots is not None:
        blob = C.string_at(pp.value, pbytes.value)
        L.hgc_free(pp.value)
        parts = blob.split(b"\0")[:-1] if blob else []
        assert len(parts) == 2 * pn.value
        plots.extend((parts[2 * i].decode(), parts[2 * i + 1].decode()) for i in range(pn.value))
        if stats is not None:
            stats["quality_calls_device"], stats["quality_calls_host"] = int(qc[0]), int(qc[1])
    if stats is not None:
        stats["overlap_edges_batched"], stats["overlap_edges_host"] = int(ove[0]), int(ove[1])
        if device_forest:
            stats["forest_calls"] = int(L.hgc_forest_calls())
        if device_enrich:
            stats["enrich_forest_calls"] = int(L.hgc_enrich_forest_calls())
    ids = _take(ip, ni.value, np.uint32, L.hgc_free)
    owner = _take(op, n, np.uint32, L.hgc_free)
    log = C.string_at(lp.value).decode()
    L.hgc_free(lp.value)
    return ids, owner, log

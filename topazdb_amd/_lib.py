"""ctypes binding of topazdb_amd/libtpz_gpu.so (the C ABI in include/tpz_gpu.h).

The product path has no CPU fallback: if the HIP library is missing or no gfx950 device is
visible, these calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# TPZ_LIB_PATH: diagnostic override (ablation builds under topazdb_amd/variants/)
LIB_PATH = os.environ.get("TPZ_LIB_PATH") or os.path.join(HERE, "libtpz_gpu.so")
HEADER = os.path.join(ROOT, "include", "tpz_gpu.h")

# tpz_err
SUCCESS, ERR_INVALID_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_NOMEM, ERR_INTERNAL, ERR_SIZES = \
    0, -1, -2, -3, -4, -5, -6
# tpz_block_status
(BLOCK_OK, BLOCK_EMPTY, BLOCK_BAD_TAG, BLOCK_UNSUPPORTED_CODEC, BLOCK_CHECKSUM_MISMATCH,
 BLOCK_MALFORMED, BLOCK_OK_SPILLED, BLOCK_SPILL_FULL, BLOCK_CODEC_ERROR, BLOCK_BAD_ENTRY) = range(10)
# tpz_entry_class (BAD_ENTRY blocks)
ENTRY_OK, ENTRY_BAD_VALUE, ENTRY_BAD_KEY = 0, 1, 2
ABI_VERSION = 8           # TPZ_ABI_VERSION this binding was written against
GET_MAX_LEVELS = 16       # TPZ_GET_MAX_LEVELS
GET_ABSENT, GET_FOUND, GET_DELETED, GET_ERROR = range(4)   # tpz_get_keys' d_result (TPZ_GET_*)
GET_NONE = 0xFFFFFFFF     # d_table / d_block / d_entry of a walk that ended nowhere
SCAN_MAX_TABLES = 64      # TPZ_SCAN_MAX_TABLES
LEVEL_SCAN_MAX_CURSORS = 64   # TPZ_LEVEL_SCAN_MAX_CURSORS
MEM_MAX_RUNS = 16         # TPZ_MEM_MAX_RUNS
HIT_MEM = 0x80000000      # TPZ_HIT_MEM: d_table = HIT_MEM | run for a hit in a memtable run
BOUND_UNBOUNDED, BOUND_INCLUDED, BOUND_EXCLUDED, BOUND_AFTER = range(4)   # TPZ_BOUND_*
SCAN_DONE, SCAN_MORE, SCAN_ERROR = range(3)    # tpz_scan_ranges' d_result (TPZ_SCAN_*)
CUT_NONE, CUT_FOUND, CUT_BAD_ENTRY = range(3)   # tpz_table_cut's d_cut[0] (TPZ_CUT_*)
MERGE_MAX_RUNS = 256      # TPZ_MERGE_MAX_RUNS
MEM_REPLAY, MEM_PUT = 0, 1   # tpz_mem_build's mode (TPZ_MEM_REPLAY, TPZ_MEM_PUT)
WAL_END_IMAGE, WAL_END_EMPTY_KEY, WAL_TRUNCATED = range(3)   # tpz_wal_index's h_info[1] (TPZ_WAL_*)
MERGE_TILE = 1024         # entries per tile-merge workgroup of tpz_merge_runs (csrc kMergeTile)
MERGE_LANE_COPY_MAX = 256  # longer keys / values are copied by the whole wave (csrc kLaneCopyMax)
BLOOM_SLICE_BITS = 1 << 19  # bits per slice of tpz_bloom_build's partitioned path (csrc kBloomSliceBits)
BLOOM_MAX_SLICES = 1024   # filters of more slices take the atomic kernel (csrc kBloomMaxSlices)
BLOOM_WG_PROBES = 12288   # a workgroup takes BLOOM_WG_PROBES // k keys (csrc kBloomWgProbes)
OPEN_TILE = 4096          # TPZ_OPEN_TILE: bytes of meta section per checkpoint of tpz_open_index
# tpz_open_index's d_info[8f] (TPZ_OPEN_*)
(OPEN_OK, OPEN_SHORT, OPEN_BLOOM_RANGE, OPEN_META_RANGE, OPEN_META_TRUNCATED, OPEN_BAD_EXTENTS,
 OPEN_NO_BLOCKS, OPEN_UNSUPPORTED) = range(8)
HAS_RAW_TABLES = 1        # TPZ_HAS_RAW_TABLES: the tpz_raw_* calls over in-place tables
LDS_BLOCK_BYTES = 94192  # TPZ_LDS_BLOCK_BYTES: longer blocks with 64+ entries take the spill path
BIGWAVE_BLOCK_BYTES = 0x40000000   # TPZ_BIGWAVE_BLOCK_BYTES


class TpzError(RuntimeError):
    pass


class Batch(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("d_ext", C.c_void_p), ("n_blocks", C.c_uint32),
                ("src_bytes", C.c_uint64)]


class Columns(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("d_ends", C.c_void_p), ("d_count", C.c_void_p),
                ("d_status", C.c_void_p), ("d_crc", C.c_void_p), ("d_spill", C.c_void_p),
                ("spill_cap", C.c_uint64), ("d_spill_off", C.c_void_p),
                ("d_spill_used", C.c_void_p), ("d_entry_first", C.c_void_p)]

COLUMN_FIELDS = ("data", "ends", "count", "status", "crc", "spill", "spill_cap", "spill_off",
                 "spill_used", "entry_first")


class FlatColumns(C.Structure):
    """tpz_flat_columns: the flat layout (one key column, one value column, exact ends)."""
    _fields_ = [("d_keys", C.c_void_p), ("d_values", C.c_void_p), ("d_ends", C.c_void_p),
                ("d_first", C.c_void_p), ("d_count", C.c_void_p), ("d_status", C.c_void_p),
                ("d_crc", C.c_void_p), ("d_spill", C.c_void_p), ("spill_cap", C.c_uint64),
                ("d_spill_off", C.c_void_p), ("d_spill_used", C.c_void_p)]

FLAT_FIELDS = ("keys", "values", "ends", "first", "count", "status", "crc", "spill", "spill_cap",
               "spill_off", "spill_used")


class Table(C.Structure):
    """tpz_table: block first keys + the columns tpz_decode_blocks wrote for the table."""
    _fields_ = [("d_first_keys", C.c_void_p), ("d_first_pos", C.c_void_p), ("d_ext", C.c_void_p),
                ("n_blocks", C.c_uint32), ("d_data", C.c_void_p), ("d_ends", C.c_void_p),
                ("d_count", C.c_void_p), ("d_status", C.c_void_p), ("d_spill", C.c_void_p),
                ("d_spill_off", C.c_void_p), ("d_entry_first", C.c_void_p)]


class GetTable(C.Structure):
    """tpz_get_table: a resident table of tpz_get_keys (its tpz_table plus its bloom filter;
    d_filter None: no filter)."""
    _fields_ = [("table", Table), ("d_filter", C.c_void_p), ("filter_len", C.c_uint64)]


class RawTable(C.Structure):
    """tpz_raw_table: an in-place table (its encoded blocks where they lie, tpz_raw_verify's
    status column, its block first keys and its bloom filter; d_filter None: no filter)."""
    _fields_ = [("d_first_keys", C.c_void_p), ("d_first_pos", C.c_void_p), ("d_src", C.c_void_p),
                ("d_ext", C.c_void_p), ("n_blocks", C.c_uint32), ("d_status", C.c_void_p),
                ("d_filter", C.c_void_p), ("filter_len", C.c_uint64)]


class Entries(C.Structure):
    """tpz_entries: sorted entries in HBM for the device write side."""
    _fields_ = [("d_keys", C.c_void_p), ("d_kpos", C.c_void_p), ("d_vals", C.c_void_p),
                ("d_vpos", C.c_void_p), ("n_entries", C.c_uint32), ("key_bytes", C.c_uint64),
                ("val_bytes", C.c_uint64)]


class MemRun(C.Structure):
    """tpz_mem_run: one memtable's sorted snapshot in HBM (d_prefix None: no prefix column)."""
    _fields_ = [("entries", Entries), ("d_prefix", C.c_void_p)]


class SstImage(C.Structure):
    """tpz_sst_image: one output table of tpz_sst_finish (its data region already at d_image)."""
    _fields_ = [("d_image", C.c_void_p), ("data_bytes", C.c_uint64), ("d_first", C.c_void_p),
                ("d_ext", C.c_void_p), ("n_blocks", C.c_uint32), ("entry_base", C.c_uint32),
                ("d_filter", C.c_void_p), ("filter_len", C.c_uint64)]


class HostColumns(C.Structure):
    """tpz_host_columns: tpz_decode_blocks_host's outputs in host memory."""
    _fields_ = [("h_data", C.c_void_p), ("h_ends", C.c_void_p), ("ends_cap", C.c_uint64),
                ("h_first", C.c_void_p), ("h_count", C.c_void_p), ("h_status", C.c_void_p),
                ("h_crc", C.c_void_p), ("h_spill", C.c_void_p), ("spill_cap", C.c_uint64),
                ("h_spill_off", C.c_void_p), ("h_spill_used", C.c_void_p),
                ("h_dext", C.c_void_p), ("data_cap", C.c_uint64)]


_lib = None


def header_functions() -> list[str]:
    """Names of every function include/tpz_gpu.h declares (non-inline)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"static inline[^{]*\{[^}]*\}", "", src)
    return re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\**\s*(tpz_[a-z_0-9]+)\s*\(", src, flags=re.M)


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TpzError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C "
                           "topazdb_amd/csrc); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.tpz_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.tpz_ctx_create.restype = C.c_int
        L.tpz_ctx_destroy.argtypes = [C.c_void_p]
        L.tpz_ctx_destroy.restype = None
        L.tpz_ctx_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.tpz_ctx_reserve.restype = C.c_int
        L.tpz_decode_blocks.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Columns),
                                        C.c_void_p]
        L.tpz_decode_blocks.restype = C.c_int
        L.tpz_decode_check.argtypes = [C.c_void_p, C.c_void_p]
        L.tpz_decode_check.restype = C.c_int
        # diagnostic (not in tpz_gpu.h): bench.py's flat copy probe for roofline.copy_ceiling
        if hasattr(L, "tpz_debug_copy"):   # (diagnostic builds from older trees lack it)
            L.tpz_debug_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p]
            L.tpz_debug_copy.restype = C.c_int
        for f in ("tpz_crc32_ranges",):
            getattr(L, f).argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
            getattr(L, f).restype = C.c_int
        L.tpz_verify_files.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p,
                                       C.c_void_p]
        L.tpz_verify_files.restype = C.c_int
        try:   # (absent from diagnostic builds of earlier commits, TPZ_LIB_PATH)
            L.tpz_verify_files_flat_layout.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p,
                                                       C.POINTER(Batch)] + [C.c_void_p] * 4
            L.tpz_verify_files_flat_layout.restype = C.c_int
        except AttributeError:
            pass
        for f in ("tpz_decompressed_sizes", "tpz_decompressed_sizes_claimed"):
            getattr(L, f).argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
            getattr(L, f).restype = C.c_int
        L.tpz_decompress_check.argtypes = [C.c_void_p, C.c_void_p]
        L.tpz_decompress_check.restype = C.c_int
        L.tpz_decompress_blocks.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
        L.tpz_decompress_blocks.restype = C.c_int
        L.tpz_format_block_error.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p,
                                             C.c_size_t]
        L.tpz_last_error.restype = C.c_char_p
        L.tpz_seek_keys.argtypes = [C.c_void_p, C.POINTER(Table), C.c_void_p, C.c_void_p,
                                    C.c_uint32] + [C.c_void_p] * 5
        L.tpz_seek_keys.restype = C.c_int
        L.tpz_bloom_may_contain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.tpz_bloom_may_contain.restype = C.c_int
        L.tpz_pack_ends.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Columns),
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.tpz_pack_ends.restype = C.c_int
        L.tpz_entry_first.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
        L.tpz_entry_first.restype = C.c_int
        L.tpz_compress_blocks.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.tpz_compress_blocks.restype = C.c_int
        L.tpz_layout_compress_bound.argtypes = [C.c_uint64, C.c_uint64]
        L.tpz_layout_compress_bound.restype = C.c_uint64
        L.tpz_flat_layout.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
        L.tpz_flat_layout.restype = C.c_int
        L.tpz_decode_blocks_flat.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(FlatColumns),
                                             C.c_void_p]
        L.tpz_decode_blocks_flat.restype = C.c_int
        L.tpz_decode_blocks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.POINTER(HostColumns), C.c_uint32]
        L.tpz_decode_blocks_host.restype = C.c_int
        try:   # (absent from diagnostic builds of earlier commits, TPZ_LIB_PATH)
            L.tpz_verify_blocks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, C.c_void_p, C.c_uint32]
            L.tpz_verify_blocks_host.restype = C.c_int
        except AttributeError:
            pass
        L.tpz_host_decoded_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.POINTER(C.c_uint64)]
        L.tpz_host_decoded_bound.restype = C.c_int
        L.tpz_plan_blocks.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                      C.c_void_p]
        L.tpz_plan_blocks.restype = C.c_int
        L.tpz_encode_blocks.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_void_p]
        L.tpz_encode_blocks.restype = C.c_int
        L.tpz_plan_blocks_async.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_uint32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.tpz_plan_blocks_async.restype = C.c_int
        L.tpz_encode_blocks_async.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tpz_encode_blocks_async.restype = C.c_int
        L.tpz_merge_runs.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p, C.c_uint32] + \
            [C.c_void_p] * 7
        L.tpz_merge_runs.restype = C.c_int
        L.tpz_flat_entry_pos.argtypes = [C.c_void_p, C.POINTER(FlatColumns), C.c_uint32] + \
            [C.c_void_p] * 4
        L.tpz_flat_entry_pos.restype = C.c_int
        L.tpz_get_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
        L.tpz_get_keys.restype = C.c_int
        L.tpz_get_values.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p]
        L.tpz_get_values.restype = C.c_int
        if not hasattr(L, "tpz_scan_ranges"):     # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_scan_ranges: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_scan_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + \
            [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 11
        L.tpz_scan_ranges.restype = C.c_int
        L.tpz_scan_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + \
            [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                C.c_void_p]
        L.tpz_scan_entries.restype = C.c_int
        if not hasattr(L, "tpz_sst_finish"):      # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_sst_finish: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_entries_bound.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.tpz_entries_bound.restype = C.c_int
        L.tpz_table_cut.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.tpz_table_cut.restype = C.c_int
        L.tpz_sst_image_bytes.argtypes = [C.c_uint64] * 4
        L.tpz_sst_image_bytes.restype = C.c_uint64
        L.tpz_sst_finish.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.tpz_sst_finish.restype = C.c_int
        if not hasattr(L, "tpz_lsm_get_keys"):    # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_lsm_get_keys: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_mem_prefix.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_void_p, C.c_void_p]
        L.tpz_mem_prefix.restype = C.c_int
        L.tpz_lsm_get_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + \
            list(L.tpz_get_keys.argtypes[1:])
        L.tpz_lsm_get_keys.restype = C.c_int
        L.tpz_lsm_get_values.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + \
            list(L.tpz_get_values.argtypes[1:])
        L.tpz_lsm_get_values.restype = C.c_int
        L.tpz_lsm_scan_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + \
            list(L.tpz_scan_ranges.argtypes[1:])
        L.tpz_lsm_scan_ranges.restype = C.c_int
        L.tpz_lsm_scan_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + \
            list(L.tpz_scan_entries.argtypes[1:])
        L.tpz_lsm_scan_entries.restype = C.c_int
        if not hasattr(L, "tpz_level_scan_ranges"):   # (additive within ABI 8)
            raise TpzError(f"{LIB_PATH} does not export tpz_level_scan_ranges: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_level_scan_ranges.argtypes = list(L.tpz_lsm_scan_ranges.argtypes)
        L.tpz_level_scan_ranges.restype = C.c_int
        if hasattr(L, "tpz_debug_level_scan"):    # diagnostic (not in tpz_gpu.h): levelscan_probe.py
            L.tpz_debug_level_scan.argtypes = list(L.tpz_lsm_scan_ranges.argtypes) + [C.c_uint32]
            L.tpz_debug_level_scan.restype = C.c_int
        L.tpz_level_scan_entries.argtypes = list(L.tpz_lsm_scan_entries.argtypes)
        L.tpz_level_scan_entries.restype = C.c_int
        if not hasattr(L, "tpz_mem_build"):       # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_mem_build: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_mem_build.argtypes = [C.c_void_p, C.POINTER(Entries), C.c_uint32] + [C.c_void_p] * 10
        L.tpz_mem_build.restype = C.c_int
        if hasattr(L, "tpz_debug_mem_build"):     # diagnostic (not in tpz_gpu.h): membuild_probe.py
            L.tpz_debug_mem_build.argtypes = list(L.tpz_mem_build.argtypes) + [C.c_uint32]
            L.tpz_debug_mem_build.restype = C.c_int
        L.tpz_wal_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.tpz_wal_index.restype = C.c_int
        L.tpz_wal_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32] + \
            [C.c_void_p] * 6
        L.tpz_wal_entries.restype = C.c_int
        if not hasattr(L, "tpz_open_index"):      # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_open_index: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_open_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32] + \
            [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
        L.tpz_open_index.restype = C.c_int
        L.tpz_open_metas.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32] + \
            [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64, C.c_uint64, C.c_void_p]
        L.tpz_open_metas.restype = C.c_int
        if not hasattr(L, "tpz_table_runs_layout"):   # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_table_runs_layout: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_table_runs_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        L.tpz_table_runs_layout.restype = C.c_int
        L.tpz_table_runs_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                             C.c_void_p]
        L.tpz_table_runs_entries.restype = C.c_int
        if not hasattr(L, "tpz_raw_verify"):      # (additive within ABI 8: an older build lacks it)
            raise TpzError(f"{LIB_PATH} does not export tpz_raw_verify: rebuild (make -C "
                           "topazdb_amd/csrc)")
        L.tpz_raw_verify.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        L.tpz_raw_verify.restype = C.c_int
        L.tpz_raw_seek_keys.argtypes = [C.c_void_p, C.POINTER(RawTable)] + \
            list(L.tpz_seek_keys.argtypes[2:])
        L.tpz_raw_seek_keys.restype = C.c_int
        for f in ("get_keys", "get_values", "lsm_get_keys", "lsm_get_values"):
            getattr(L, "tpz_raw_" + f).argtypes = list(getattr(L, "tpz_" + f).argtypes)
            getattr(L, "tpz_raw_" + f).restype = C.c_int
        if hasattr(L, "tpz_debug_table_runs_entries"):   # diagnostic (not in tpz_gpu.h): runs_probe.py
            L.tpz_debug_table_runs_entries.argtypes = \
                list(L.tpz_table_runs_entries.argtypes[:-1]) + [C.c_uint32, C.c_void_p]
            L.tpz_debug_table_runs_entries.restype = C.c_int
        L.tpz_bloom_geometry.argtypes = [C.c_uint64, C.c_double, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]
        L.tpz_bloom_geometry.restype = C.c_int
        L.tpz_bloom_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double,
                                      C.c_void_p, C.c_void_p]
        L.tpz_bloom_build.restype = C.c_int
        L.tpz_host_xxh3_64.argtypes = [C.c_char_p, C.c_uint64]
        L.tpz_host_xxh3_64.restype = C.c_uint64
        L.tpz_layout_spill_stream.argtypes = [C.c_uint64]
        L.tpz_layout_spill_stream.restype = C.c_uint64
        L.tpz_layout_spill_classes.argtypes = [C.c_uint64] * 3
        L.tpz_layout_spill_classes.restype = C.c_uint64
        L.tpz_abi_version.restype = C.c_int
        if L.tpz_abi_version() != ABI_VERSION:
            raise TpzError(f"{LIB_PATH}: ABI version {L.tpz_abi_version()}, this binding "
                           f"needs {ABI_VERSION}: rebuild (make -C topazdb_amd/csrc)")
        for f in ("slot_base", "entry_base", "data_capacity", "entry_capacity"):
            fn = getattr(L, "tpz_layout_" + f)
            fn.argtypes = [C.c_uint64, C.c_uint64]
            fn.restype = C.c_uint64
        L.tpz_layout_value_start.argtypes = [C.c_uint64]
        L.tpz_layout_value_start.restype = C.c_uint64
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != SUCCESS:
        raise TpzError(f"{what} failed ({rc}): {lib().tpz_last_error().decode()}")


def format_block_error(status: int, crc_expected: int = 0, crc_actual: int = 0) -> str:
    buf = C.create_string_buffer(128)
    lib().tpz_format_block_error(status, crc_expected, crc_actual, buf, 128)
    return buf.value.decode()


# layout (mirrors the static inline helpers of include/tpz_gpu.h; works on ints and numpy int64)
def slot_base(ext_i, i):
    return ((ext_i + 127) & ~127) + 256 * i


def value_start(key_bytes):
    return (key_bytes + 15) & ~15


def entry_base(ext_i, i):
    return 16 * (ext_i // 96 + i)


def spill_stream(n):
    """tpz_spill_stream: a spill record's stream starts after its 2n u32 ends, 128-aligned."""
    return (8 * n + 127) & ~127


def spill_classes(n, k, v):
    """tpz_spill_classes: a BAD_ENTRY record's class bytes follow its ends and stream."""
    return spill_stream(n) + ((value_start(k) + v + 127) & ~127)


def block_decoded(status) -> bool:
    """Ok(Block) in the reference: TPZ_BLOCK_OK, OK_SPILLED (decoded into the spill arena) or
    BAD_ENTRY (Ok, with entries that panic when an iterator reaches them)."""
    return status in (BLOCK_OK, BLOCK_OK_SPILLED, BLOCK_BAD_ENTRY)


def data_capacity(src_bytes: int, n_blocks: int) -> int:
    return slot_base(src_bytes, n_blocks) + 128


def entry_capacity(src_bytes: int, n_blocks: int) -> int:
    return entry_base(src_bytes, n_blocks) + 16


class Context:
    """One tpz_ctx per device (tpz_ctx_create / tpz_ctx_destroy)."""

    def __init__(self, device: int = 0):
        self.device = device
        h = C.c_void_p()
        check(lib().tpz_ctx_create(device, C.byref(h)), "tpz_ctx_create")
        self.handle = h

    def reserve(self, max_blocks: int, stream: int = 0) -> None:
        check(lib().tpz_ctx_reserve(self.handle, max_blocks, C.c_void_p(stream)),
              "tpz_ctx_reserve")

    def close(self) -> None:
        if getattr(self, "handle", None):
            lib().tpz_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int, cols: dict,
                    stream: int = 0) -> None:
        """tpz_decode_blocks on raw device pointers; cols maps field name -> device pointer."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        c = Columns(*[cols[f] for f in COLUMN_FIELDS])
        check(lib().tpz_decode_blocks(self.handle, C.byref(b), C.byref(c), C.c_void_p(stream)),
              "tpz_decode_blocks")

    def decode_check(self, stream: int = 0) -> None:
        """tpz_decode_check: synchronizes the stream; raises TpzError if a decode on it did not
        run to completion (a tail workgroup's bounded wait timed out)."""
        check(lib().tpz_decode_check(self.handle, C.c_void_p(stream)), "tpz_decode_check")

    def entry_first_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int,
                         d_first: int, stream: int = 0) -> None:
        """tpz_entry_first: the exact ends layout's per-block pair offsets (n_blocks + 1 u64)."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        check(lib().tpz_entry_first(self.handle, C.byref(b), C.c_void_p(d_first),
                                    C.c_void_p(stream)), "tpz_entry_first")

    def flat_layout_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int,
                         d_first: int, stream: int = 0) -> None:
        """tpz_flat_layout: 3 x (n_blocks + 1) u64 of per-block entry / key-byte / value-byte
        prefixes (the flat layout's sizes)."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        check(lib().tpz_flat_layout(self.handle, C.byref(b), C.c_void_p(d_first),
                                    C.c_void_p(stream)), "tpz_flat_layout")

    def decode_flat_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int, cols: dict,
                         stream: int = 0) -> None:
        """tpz_decode_blocks_flat on raw device pointers; cols maps FLAT_FIELDS -> pointer."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        c = FlatColumns(*[cols[f] for f in FLAT_FIELDS])
        check(lib().tpz_decode_blocks_flat(self.handle, C.byref(b), C.byref(c), C.c_void_p(stream)),
              "tpz_decode_blocks_flat")

    def decode_host_ptrs(self, h_src: int, h_ext: int, n_blocks: int, cols: HostColumns,
                         chunk_blocks: int = 0) -> int:
        """tpz_decode_blocks_host (blocks in host memory; H2D, decode, D2H inside the library).
        Returns the tpz_err (SUCCESS, or ERR_NOMEM when the ends, spill or data capacity was
        short)."""
        rc = lib().tpz_decode_blocks_host(self.handle, C.c_void_p(h_src), C.c_void_p(h_ext),
                                          n_blocks, C.byref(cols), chunk_blocks)
        if rc not in (SUCCESS, ERR_NOMEM):
            check(rc, "tpz_decode_blocks_host")
        return rc

    def verify_host(self, region, ext, chunk_blocks: int = 0):
        """tpz_verify_blocks_host over blocks in host memory: the device's verdict (status, crc,
        count) with the decoded columns left on the device, and for a run with snappy / lz4
        blocks the decoded extents and bytes (every block's Uncompress form). Returns
        (status, crc, count, dext, plain); dext / plain are None for an Uncompress run."""
        import numpy as np
        if not hasattr(lib(), "tpz_verify_blocks_host"):
            raise RuntimeError(f"{LIB_PATH} has no tpz_verify_blocks_host (ABI 6, round 5 on): "
                               "a library built from an earlier tree")
        src = np.ascontiguousarray(np.frombuffer(bytes(region), np.uint8) if not isinstance(region, np.ndarray) else region, np.uint8)
        e = np.ascontiguousarray(ext, np.uint64)
        n = len(e) - 1
        status = np.zeros(n, np.uint8)
        crc = np.zeros(n, np.uint32)
        count = np.zeros(n, np.uint32)
        dext = np.zeros(n + 1, np.uint64)
        codec = bool(n) and any(e[i + 1] > e[i] and src[int(e[i + 1]) - 1] in (2, 3) for i in range(n))
        plain = None
        if codec:
            bound = C.c_uint64(0)
            check(lib().tpz_host_decoded_bound(C.c_void_p(src.ctypes.data), C.c_void_p(e.ctypes.data), n,
                                               C.byref(bound)), "tpz_host_decoded_bound")
            plain = np.zeros(max(int(bound.value), 1), np.uint8)
        while True:
            rc = lib().tpz_verify_blocks_host(
                self.handle, C.c_void_p(src.ctypes.data if src.size else None), C.c_void_p(e.ctypes.data), n,
                C.c_void_p(status.ctypes.data), C.c_void_p(crc.ctypes.data),
                C.c_void_p(count.ctypes.data), C.c_void_p(plain.ctypes.data if codec else None),
                plain.size if codec else 0, C.c_void_p(dext.ctypes.data), chunk_blocks)
            # (NOMEM means h_plain was short: dext[n] holds the bytes needed; grow only then)
            if rc == ERR_NOMEM and codec and int(dext[n]) > plain.size:
                plain = np.zeros(int(dext[n]), np.uint8)
                continue
            check(rc, "tpz_verify_blocks_host")
            break
        if not codec:
            return status, crc, count, None, None
        return status, crc, count, dext, plain[:int(dext[n])]

    def decompressed_sizes_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int,
                                d_size: int, stream: int = 0, claimed: bool = False) -> None:
        """tpz_decompressed_sizes (compress::decode's codec step, compress.rs:95-113); claimed:
        tpz_decompressed_sizes_claimed (LZ4 blocks take their size prefix, checked by
        decompress_check after the decompress)."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        name = "tpz_decompressed_sizes_claimed" if claimed else "tpz_decompressed_sizes"
        check(getattr(lib(), name)(self.handle, C.byref(b), C.c_void_p(d_size), C.c_void_p(stream)),
              name)

    def decompress_check(self, stream: int = 0) -> bool:
        """tpz_decompress_check: synchronizes the stream; False when a decompress on it since the
        last check ran over claimed sizes that were not exact (the caller sizes the batch exactly
        and decompresses it again), True otherwise."""
        rc = lib().tpz_decompress_check(self.handle, C.c_void_p(stream))
        if rc == ERR_SIZES:
            return False
        check(rc, "tpz_decompress_check")
        return True

    def decompress_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int, d_dst: int,
                        d_dst_ext: int, d_status: int, stream: int = 0) -> None:
        """tpz_decompress_blocks: snappy blocks to their Uncompress form."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        check(lib().tpz_decompress_blocks(self.handle, C.byref(b), C.c_void_p(d_dst),
                                          C.c_void_p(d_dst_ext), C.c_void_p(d_status),
                                          C.c_void_p(stream)), "tpz_decompress_blocks")

    def crc32_ptrs(self, d_src: int, d_ext: int, n_ranges: int, src_bytes: int, d_crc: int,
                   stream: int = 0) -> None:
        """tpz_crc32_ranges: CRC-32 of every range [ext[i], ext[i+1]) (checksum.rs:6-10)."""
        b = Batch(d_src, d_ext, n_ranges, src_bytes)
        check(lib().tpz_crc32_ranges(self.handle, C.byref(b), C.c_void_p(d_crc),
                                     C.c_void_p(stream)), "tpz_crc32_ranges")

    def verify_files_ptrs(self, d_src: int, d_ext: int, n_files: int, src_bytes: int,
                          d_crc: int, d_status: int, stream: int = 0) -> None:
        """tpz_verify_files: FileObject::open's whole-file CRC check (file_object.rs:57-78)."""
        b = Batch(d_src, d_ext, n_files, src_bytes)
        check(lib().tpz_verify_files(self.handle, C.byref(b), C.c_void_p(d_crc),
                                     C.c_void_p(d_status), C.c_void_p(stream)),
              "tpz_verify_files")

    def open_flat_layout_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int,
                              d_file_block: int, d_tsrc: int, d_text: int, n_files: int,
                              tail_bytes: int, d_crc: int, d_status: int, d_first: int,
                              stream: int = 0) -> None:
        """tpz_verify_files_flat_layout: tpz_verify_files over the files (data region + tail) and
        tpz_flat_layout over their blocks from one read of the blocks (file_object.rs:57-78,
        iterator.rs:74-82)."""
        if not hasattr(lib(), "tpz_verify_files_flat_layout"):
            raise RuntimeError("libtpz_gpu.so lacks tpz_verify_files_flat_layout (an older build)")
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        t = Batch(d_tsrc, d_text, n_files, tail_bytes)
        check(lib().tpz_verify_files_flat_layout(self.handle, C.byref(b), C.c_void_p(d_file_block),
                                                 C.byref(t), C.c_void_p(d_crc),
                                                 C.c_void_p(d_status), C.c_void_p(d_first),
                                                 C.c_void_p(stream)),
              "tpz_verify_files_flat_layout")

    def seek_keys_ptrs(self, table: Table, d_keys: int, d_key_pos: int, n_keys: int,
                       d_block: int, d_entry: int, d_status: int, d_valid: int,
                       stream: int = 0) -> None:
        """tpz_seek_keys: SsTableIterator::seek_to_key for every key (table/iterator.rs:44-72)."""
        check(lib().tpz_seek_keys(self.handle, C.byref(table), C.c_void_p(d_keys),
                                  C.c_void_p(d_key_pos), n_keys, C.c_void_p(d_block),
                                  C.c_void_p(d_entry), C.c_void_p(d_status), C.c_void_p(d_valid),
                                  C.c_void_p(stream)), "tpz_seek_keys")

    def raw_verify_ptrs(self, d_src: int, d_ext: int, n_blocks: int, src_bytes: int,
                        d_status: int, d_crc: int, stream: int = 0) -> None:
        """tpz_raw_verify: Block::decode's checks ahead of the entries (tag, CRC, n and the
        offsets readable) for every block of the batch; no decoded bytes anywhere."""
        b = Batch(d_src, d_ext, n_blocks, src_bytes)
        check(lib().tpz_raw_verify(self.handle, C.byref(b), C.c_void_p(d_status),
                                   C.c_void_p(d_crc), C.c_void_p(stream)), "tpz_raw_verify")

    def raw_seek_keys_ptrs(self, table: RawTable, d_keys: int, d_key_pos: int, n_keys: int,
                           d_block: int, d_entry: int, d_status: int, d_valid: int,
                           stream: int = 0) -> None:
        """tpz_raw_seek_keys: tpz_seek_keys over an in-place table."""
        check(lib().tpz_raw_seek_keys(self.handle, C.byref(table), C.c_void_p(d_keys),
                                      C.c_void_p(d_key_pos), n_keys, C.c_void_p(d_block),
                                      C.c_void_p(d_entry), C.c_void_p(d_status),
                                      C.c_void_p(d_valid), C.c_void_p(stream)),
              "tpz_raw_seek_keys")

    def raw_get_keys_ptrs(self, d_tables: int, n_tables: int, h_level_first: int, n_levels: int,
                          d_keys: int, d_key_pos: int, n_keys: int, d_result: int, d_status: int,
                          d_table: int, d_block: int, d_entry: int, d_val_pos: int,
                          stream: int = 0) -> None:
        """tpz_raw_get_keys: tpz_get_keys over the n_tables tpz_raw_table descriptors at
        d_tables."""
        check(lib().tpz_raw_get_keys(self.handle, C.c_void_p(d_tables), n_tables,
                                     C.c_void_p(h_level_first), n_levels, C.c_void_p(d_keys),
                                     C.c_void_p(d_key_pos), n_keys, C.c_void_p(d_result),
                                     C.c_void_p(d_status), C.c_void_p(d_table),
                                     C.c_void_p(d_block), C.c_void_p(d_entry),
                                     C.c_void_p(d_val_pos), C.c_void_p(stream)),
              "tpz_raw_get_keys")

    def raw_get_values_ptrs(self, d_tables: int, n_tables: int, n_keys: int, d_result: int,
                            d_table: int, d_block: int, d_entry: int, d_val_pos: int, d_vals: int,
                            val_cap: int, stream: int = 0) -> None:
        """tpz_raw_get_values: the values of tpz_raw_get_keys' FOUND queries."""
        check(lib().tpz_raw_get_values(self.handle, C.c_void_p(d_tables), n_tables, n_keys,
                                       C.c_void_p(d_result), C.c_void_p(d_table),
                                       C.c_void_p(d_block), C.c_void_p(d_entry),
                                       C.c_void_p(d_val_pos), C.c_void_p(d_vals), val_cap,
                                       C.c_void_p(stream)), "tpz_raw_get_values")

    def raw_lsm_get_keys_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                              h_level_first: int, n_levels: int, d_keys: int, d_key_pos: int,
                              n_keys: int, d_result: int, d_status: int, d_table: int,
                              d_block: int, d_entry: int, d_val_pos: int, stream: int = 0) -> None:
        """tpz_raw_lsm_get_keys: tpz_lsm_get_keys with in-place tables under the runs."""
        check(lib().tpz_raw_lsm_get_keys(self.handle, C.c_void_p(d_runs), n_runs,
                                         C.c_void_p(d_tables), n_tables,
                                         C.c_void_p(h_level_first), n_levels, C.c_void_p(d_keys),
                                         C.c_void_p(d_key_pos), n_keys, C.c_void_p(d_result),
                                         C.c_void_p(d_status), C.c_void_p(d_table),
                                         C.c_void_p(d_block), C.c_void_p(d_entry),
                                         C.c_void_p(d_val_pos), C.c_void_p(stream)),
              "tpz_raw_lsm_get_keys")

    def raw_lsm_get_values_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                                n_keys: int, d_result: int, d_table: int, d_block: int,
                                d_entry: int, d_val_pos: int, d_vals: int, val_cap: int,
                                stream: int = 0) -> None:
        """tpz_raw_lsm_get_values: the values of tpz_raw_lsm_get_keys' FOUND queries."""
        check(lib().tpz_raw_lsm_get_values(self.handle, C.c_void_p(d_runs), n_runs,
                                           C.c_void_p(d_tables), n_tables, n_keys,
                                           C.c_void_p(d_result), C.c_void_p(d_table),
                                           C.c_void_p(d_block), C.c_void_p(d_entry),
                                           C.c_void_p(d_val_pos), C.c_void_p(d_vals), val_cap,
                                           C.c_void_p(stream)), "tpz_raw_lsm_get_values")

    def bloom_ptrs(self, d_filter: int, filter_len: int, d_keys: int, d_key_pos: int,
                   n_keys: int, d_out: int, stream: int = 0) -> None:
        """tpz_bloom_may_contain: SsTable::may_contain for every key (table.rs:114-119)."""
        check(lib().tpz_bloom_may_contain(self.handle, C.c_void_p(d_filter), filter_len,
                                          C.c_void_p(d_keys), C.c_void_p(d_key_pos), n_keys,
                                          C.c_void_p(d_out), C.c_void_p(stream)),
              "tpz_bloom_may_contain")

    def plan_blocks_ptrs(self, ent: Entries, block_size: int, d_first: int, d_ext: int,
                         stream: int = 0) -> tuple[int, int]:
        """tpz_plan_blocks (synchronous): BlockBuilder's fill rule over the entries. Returns
        (rc, n_blocks or the first bad entry): rc ERR_INVALID_ARG with a bad entry index when an
        entry has an empty key or fits no block (the reference asserts / recurses forever)."""
        nb, bad = C.c_uint32(), C.c_uint64()
        rc = lib().tpz_plan_blocks(self.handle, C.byref(ent), block_size, C.c_void_p(d_first),
                                   C.c_void_p(d_ext), C.byref(nb), C.byref(bad),
                                   C.c_void_p(stream))
        if rc == ERR_INVALID_ARG and bad.value != 2**64 - 1:
            return rc, int(bad.value)
        check(rc, "tpz_plan_blocks")
        return rc, int(nb.value)

    def plan_blocks_async_ptrs(self, ent: Entries, block_size: int, d_first: int, d_ext: int,
                               d_info: int, stream: int = 0) -> None:
        """tpz_plan_blocks_async: the plan on `stream`, its {widest block start, first bad entry,
        n_blocks} left in d_info (4 u32 of device memory); no host round trip for block sizes up
        to TPZ_PLAN_ASYNC_MAX_BLOCK."""
        check(lib().tpz_plan_blocks_async(self.handle, C.byref(ent), block_size, C.c_void_p(d_first),
                                          C.c_void_p(d_ext), C.c_void_p(d_info),
                                          C.c_void_p(stream)), "tpz_plan_blocks_async")

    def encode_blocks_async_ptrs(self, ent: Entries, d_first: int, d_ext: int, d_info: int,
                                 d_out: int, stream: int = 0) -> None:
        """tpz_encode_blocks_async: the encode with the block count read from d_info."""
        check(lib().tpz_encode_blocks_async(self.handle, C.byref(ent), C.c_void_p(d_first),
                                            C.c_void_p(d_ext), C.c_void_p(d_info), C.c_void_p(d_out),
                                            C.c_void_p(stream)), "tpz_encode_blocks_async")

    def merge_runs_ptrs(self, ent: Entries, h_run_first: int, n_runs: int, d_out_keys: int,
                        d_out_kpos: int, d_out_vals: int, d_out_vpos: int, d_src_entry: int,
                        d_info: int, stream: int = 0) -> None:
        """tpz_merge_runs: MergeIterator over n_runs sorted runs of `ent` (merge_iterator.rs:41-106);
        h_run_first is a host pointer to n_runs + 1 u32."""
        check(lib().tpz_merge_runs(self.handle, C.byref(ent), C.c_void_p(h_run_first), n_runs,
                                   C.c_void_p(d_out_keys), C.c_void_p(d_out_kpos),
                                   C.c_void_p(d_out_vals), C.c_void_p(d_out_vpos),
                                   C.c_void_p(d_src_entry), C.c_void_p(d_info),
                                   C.c_void_p(stream)), "tpz_merge_runs")

    def get_keys_ptrs(self, d_tables: int, n_tables: int, h_level_first: int, n_levels: int,
                      d_keys: int, d_key_pos: int, n_keys: int, d_result: int, d_status: int,
                      d_table: int, d_block: int, d_entry: int, d_val_pos: int,
                      stream: int = 0) -> None:
        """tpz_get_keys: LevelController::get's walk for every key (level.rs:427-465) over the
        n_tables tpz_get_table descriptors at d_tables; h_level_first is a host pointer to
        n_levels + 1 u32."""
        check(lib().tpz_get_keys(self.handle, C.c_void_p(d_tables), n_tables,
                                 C.c_void_p(h_level_first), n_levels, C.c_void_p(d_keys),
                                 C.c_void_p(d_key_pos), n_keys, C.c_void_p(d_result),
                                 C.c_void_p(d_status), C.c_void_p(d_table), C.c_void_p(d_block),
                                 C.c_void_p(d_entry), C.c_void_p(d_val_pos), C.c_void_p(stream)),
              "tpz_get_keys")

    def get_values_ptrs(self, d_tables: int, n_tables: int, n_keys: int, d_result: int,
                        d_table: int, d_block: int, d_entry: int, d_val_pos: int, d_vals: int,
                        val_cap: int, stream: int = 0) -> None:
        """tpz_get_values: the values of tpz_get_keys' FOUND queries, packed at d_val_pos."""
        check(lib().tpz_get_values(self.handle, C.c_void_p(d_tables), n_tables, n_keys,
                                   C.c_void_p(d_result), C.c_void_p(d_table), C.c_void_p(d_block),
                                   C.c_void_p(d_entry), C.c_void_p(d_val_pos), C.c_void_p(d_vals),
                                   val_cap, C.c_void_p(stream)), "tpz_get_values")

    def mem_prefix_ptrs(self, ent: Entries, d_prefix: int, stream: int = 0) -> None:
        """tpz_mem_prefix: the prefix column of a memtable run (n_entries u64 at d_prefix)."""
        check(lib().tpz_mem_prefix(self.handle, C.byref(ent), C.c_void_p(d_prefix),
                                   C.c_void_p(stream)), "tpz_mem_prefix")

    def mem_build_ptrs(self, ent: Entries, mode: int, d_version: int, d_out_keys: int,
                       d_out_kpos: int, d_out_vals: int, d_out_vpos: int, d_out_prefix: int,
                       d_src_entry: int, d_out_version: int, d_info: int, stream: int = 0) -> None:
        """tpz_mem_build: `ent` in arrival order becomes a memtable run under MemTable::open's
        (MEM_REPLAY) or do_mem_put's (MEM_PUT, d_version: n u64) rule; d_info: 8 u64."""
        check(lib().tpz_mem_build(self.handle, C.byref(ent), mode, C.c_void_p(d_version),
                                  C.c_void_p(d_out_keys), C.c_void_p(d_out_kpos),
                                  C.c_void_p(d_out_vals), C.c_void_p(d_out_vpos),
                                  C.c_void_p(d_out_prefix), C.c_void_p(d_src_entry),
                                  C.c_void_p(d_out_version), C.c_void_p(d_info),
                                  C.c_void_p(stream)), "tpz_mem_build")

    def wal_entries_ptrs(self, d_image: int, image_bytes: int, d_rec: int, n_records: int,
                         d_keys: int, d_kpos: int, d_vals: int, d_vpos: int, d_info: int,
                         stream: int = 0) -> None:
        """tpz_wal_entries: the records of a WAL image in HBM (d_rec: tpz_wal_index's n_records + 1
        starts) as packed key and value columns in arrival order; d_info: 4 u64."""
        check(lib().tpz_wal_entries(self.handle, C.c_void_p(d_image), image_bytes,
                                    C.c_void_p(d_rec), n_records, C.c_void_p(d_keys),
                                    C.c_void_p(d_kpos), C.c_void_p(d_vals), C.c_void_p(d_vpos),
                                    C.c_void_p(d_info), C.c_void_p(stream)), "tpz_wal_entries")

    def lsm_get_keys_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                          h_level_first: int, n_levels: int, d_keys: int, d_key_pos: int,
                          n_keys: int, d_result: int, d_status: int, d_table: int, d_block: int,
                          d_entry: int, d_val_pos: int, stream: int = 0) -> None:
        """tpz_lsm_get_keys: LsmStorage::get (lsm_storage.rs:198-213) for every key: the n_runs
        tpz_mem_run descriptors at d_runs newest first, then tpz_get_keys' walk."""
        check(lib().tpz_lsm_get_keys(self.handle, C.c_void_p(d_runs), n_runs, C.c_void_p(d_tables),
                                     n_tables, C.c_void_p(h_level_first), n_levels,
                                     C.c_void_p(d_keys), C.c_void_p(d_key_pos), n_keys,
                                     C.c_void_p(d_result), C.c_void_p(d_status),
                                     C.c_void_p(d_table), C.c_void_p(d_block), C.c_void_p(d_entry),
                                     C.c_void_p(d_val_pos), C.c_void_p(stream)),
              "tpz_lsm_get_keys")

    def lsm_get_values_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                            n_keys: int, d_result: int, d_table: int, d_block: int, d_entry: int,
                            d_val_pos: int, d_vals: int, val_cap: int, stream: int = 0) -> None:
        """tpz_lsm_get_values: the values of tpz_lsm_get_keys' FOUND queries, from runs and
        tables, packed at d_val_pos."""
        check(lib().tpz_lsm_get_values(self.handle, C.c_void_p(d_runs), n_runs,
                                       C.c_void_p(d_tables), n_tables, n_keys,
                                       C.c_void_p(d_result), C.c_void_p(d_table),
                                       C.c_void_p(d_block), C.c_void_p(d_entry),
                                       C.c_void_p(d_val_pos), C.c_void_p(d_vals), val_cap,
                                       C.c_void_p(stream)), "tpz_lsm_get_values")

    def lsm_scan_ranges_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                             h_level_first: int, n_levels: int, d_lo_keys: int, d_lo_pos: int,
                             d_lo_kind: int, d_hi_keys: int, d_hi_pos: int, d_hi_kind: int,
                             n_scans: int, limit: int, d_result: int, d_status: int, d_where: int,
                             d_hit_table: int, d_hit_block: int, d_hit_entry: int, d_first: int,
                             d_key_first: int, d_val_first: int, d_info: int,
                             stream: int = 0) -> None:
        """tpz_lsm_scan_ranges: LsmStorage::scan whole (lsm_storage.rs:335-374) for every range:
        the n_runs tpz_mem_run descriptors at d_runs merged over the tables (TwoMergeIterator)."""
        ptrs = [C.c_void_p(x) for x in (d_result, d_status, d_where, d_hit_table, d_hit_block,
                                        d_hit_entry, d_first, d_key_first, d_val_first, d_info)]
        check(lib().tpz_lsm_scan_ranges(self.handle, C.c_void_p(d_runs), n_runs,
                                        C.c_void_p(d_tables), n_tables, C.c_void_p(h_level_first),
                                        n_levels, C.c_void_p(d_lo_keys), C.c_void_p(d_lo_pos),
                                        C.c_void_p(d_lo_kind), C.c_void_p(d_hi_keys),
                                        C.c_void_p(d_hi_pos), C.c_void_p(d_hi_kind), n_scans, limit,
                                        *ptrs, C.c_void_p(stream)), "tpz_lsm_scan_ranges")

    def lsm_scan_entries_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                              n_scans: int, limit: int, d_hit_table: int, d_hit_block: int,
                              d_hit_entry: int, d_first: int, d_keys: int, key_cap: int,
                              d_kpos: int, d_vals: int, val_cap: int, d_vpos: int,
                              stream: int = 0) -> None:
        """tpz_lsm_scan_entries: the entries tpz_lsm_scan_ranges yielded, from runs and tables."""
        check(lib().tpz_lsm_scan_entries(self.handle, C.c_void_p(d_runs), n_runs,
                                         C.c_void_p(d_tables), n_tables, n_scans, limit,
                                         C.c_void_p(d_hit_table), C.c_void_p(d_hit_block),
                                         C.c_void_p(d_hit_entry), C.c_void_p(d_first),
                                         C.c_void_p(d_keys), key_cap, C.c_void_p(d_kpos),
                                         C.c_void_p(d_vals), val_cap, C.c_void_p(d_vpos),
                                         C.c_void_p(stream)), "tpz_lsm_scan_entries")

    def level_scan_ranges_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                               h_level_first: int, n_levels: int, d_lo_keys: int, d_lo_pos: int,
                               d_lo_kind: int, d_hi_keys: int, d_hi_pos: int, d_hi_kind: int,
                               n_scans: int, limit: int, d_result: int, d_status: int,
                               d_where: int, d_hit_table: int, d_hit_block: int, d_hit_entry: int,
                               d_first: int, d_key_first: int, d_val_first: int, d_info: int,
                               stream: int = 0) -> None:
        """tpz_level_scan_ranges: tpz_lsm_scan_ranges with one merge cursor per run, per L0 table
        and per non-empty level below L0 (sorted and disjoint), so any number of tables."""
        ptrs = [C.c_void_p(x) for x in (d_result, d_status, d_where, d_hit_table, d_hit_block,
                                        d_hit_entry, d_first, d_key_first, d_val_first, d_info)]
        check(lib().tpz_level_scan_ranges(self.handle, C.c_void_p(d_runs), n_runs,
                                          C.c_void_p(d_tables), n_tables,
                                          C.c_void_p(h_level_first), n_levels,
                                          C.c_void_p(d_lo_keys), C.c_void_p(d_lo_pos),
                                          C.c_void_p(d_lo_kind), C.c_void_p(d_hi_keys),
                                          C.c_void_p(d_hi_pos), C.c_void_p(d_hi_kind), n_scans,
                                          limit, *ptrs, C.c_void_p(stream)),
              "tpz_level_scan_ranges")

    def level_scan_entries_ptrs(self, d_runs: int, n_runs: int, d_tables: int, n_tables: int,
                                n_scans: int, limit: int, d_hit_table: int, d_hit_block: int,
                                d_hit_entry: int, d_first: int, d_keys: int, key_cap: int,
                                d_kpos: int, d_vals: int, val_cap: int, d_vpos: int,
                                stream: int = 0) -> None:
        """tpz_level_scan_entries: the entries tpz_level_scan_ranges yielded."""
        check(lib().tpz_level_scan_entries(self.handle, C.c_void_p(d_runs), n_runs,
                                           C.c_void_p(d_tables), n_tables, n_scans, limit,
                                           C.c_void_p(d_hit_table), C.c_void_p(d_hit_block),
                                           C.c_void_p(d_hit_entry), C.c_void_p(d_first),
                                           C.c_void_p(d_keys), key_cap, C.c_void_p(d_kpos),
                                           C.c_void_p(d_vals), val_cap, C.c_void_p(d_vpos),
                                           C.c_void_p(stream)), "tpz_level_scan_entries")

    def scan_ranges_ptrs(self, d_tables: int, n_tables: int, h_level_first: int, n_levels: int,
                         d_lo_keys: int, d_lo_pos: int, d_lo_kind: int, d_hi_keys: int,
                         d_hi_pos: int, d_hi_kind: int, n_scans: int, limit: int, d_result: int,
                         d_status: int, d_where: int, d_hit_table: int, d_hit_block: int,
                         d_hit_entry: int, d_first: int, d_key_first: int, d_val_first: int,
                         d_info: int, stream: int = 0) -> None:
        """tpz_scan_ranges: LsmStorage::scan's SST half (lsm_storage.rs:335-374) for every range
        over the n_tables tpz_get_table descriptors at d_tables: the yielded entries' positions,
        at most `limit` per scan."""
        ptrs = [C.c_void_p(x) for x in (d_result, d_status, d_where, d_hit_table, d_hit_block,
                                        d_hit_entry, d_first, d_key_first, d_val_first, d_info)]
        check(lib().tpz_scan_ranges(self.handle, C.c_void_p(d_tables), n_tables,
                                    C.c_void_p(h_level_first), n_levels, C.c_void_p(d_lo_keys),
                                    C.c_void_p(d_lo_pos), C.c_void_p(d_lo_kind),
                                    C.c_void_p(d_hi_keys), C.c_void_p(d_hi_pos),
                                    C.c_void_p(d_hi_kind), n_scans, limit, *ptrs,
                                    C.c_void_p(stream)), "tpz_scan_ranges")

    def scan_entries_ptrs(self, d_tables: int, n_tables: int, n_scans: int, limit: int,
                          d_hit_table: int, d_hit_block: int, d_hit_entry: int, d_first: int,
                          d_keys: int, key_cap: int, d_kpos: int, d_vals: int, val_cap: int,
                          d_vpos: int, stream: int = 0) -> None:
        """tpz_scan_entries: the entries tpz_scan_ranges yielded, as a tpz_entries."""
        check(lib().tpz_scan_entries(self.handle, C.c_void_p(d_tables), n_tables, n_scans, limit,
                                     C.c_void_p(d_hit_table), C.c_void_p(d_hit_block),
                                     C.c_void_p(d_hit_entry), C.c_void_p(d_first),
                                     C.c_void_p(d_keys), key_cap, C.c_void_p(d_kpos),
                                     C.c_void_p(d_vals), val_cap, C.c_void_p(d_vpos),
                                     C.c_void_p(stream)), "tpz_scan_entries")

    def entries_bound_ptrs(self, ent: Entries, d_keys: int, d_key_pos: int, d_inclusive: int,
                           n_probes: int, d_out: int, stream: int = 0) -> None:
        """tpz_entries_bound: per probe key the number of entries below it (or at it, where its
        flag is set): sub_compact's seek and key_vaild (level.rs:188-206) over merged entries."""
        check(lib().tpz_entries_bound(self.handle, C.byref(ent), C.c_void_p(d_keys),
                                      C.c_void_p(d_key_pos), C.c_void_p(d_inclusive), n_probes,
                                      C.c_void_p(d_out), C.c_void_p(stream)), "tpz_entries_bound")

    def table_cut_ptrs(self, ent: Entries, start: int, win_entries: int, seg_end: int,
                       d_first: int, d_ext: int, d_cut_ext: int, d_plan_info: int, block_size: int,
                       capacity: int, d_cut: int, stream: int = 0) -> None:
        """tpz_table_cut: reach_capacity's cut (builder.rs:88-94) inside a planned window of the
        table that starts at entry `start`; d_cut: 8 u64 of device memory."""
        check(lib().tpz_table_cut(self.handle, C.byref(ent), start, win_entries, seg_end,
                                  C.c_void_p(d_first), C.c_void_p(d_ext), C.c_void_p(d_cut_ext),
                                  C.c_void_p(d_plan_info), block_size, capacity,
                                  C.c_void_p(d_cut), C.c_void_p(stream)), "tpz_table_cut")

    def sst_finish_ptrs(self, ent: Entries, d_images: int, n_images: int, max_blocks: int,
                        d_base: int, span_bytes: int, d_info: int, stream: int = 0) -> None:
        """tpz_sst_finish: metas, offsets, bloom section and the CRC trailer of n_images SST file
        images (builder.rs:97-141, file_object.rs:33-48); d_images: SstImage descriptors in device
        memory; d_info: 4 u64 per image."""
        check(lib().tpz_sst_finish(self.handle, C.byref(ent), C.c_void_p(d_images), n_images,
                                   max_blocks, C.c_void_p(d_base), span_bytes, C.c_void_p(d_info),
                                   C.c_void_p(stream)), "tpz_sst_finish")

    def open_index_ptrs(self, d_src: int, span_bytes: int, d_span: int, n_files: int, d_info: int,
                        d_file_block: int, d_file_key: int, d_scratch: int, scratch_bytes: int,
                        stream: int = 0) -> None:
        """tpz_open_index: SsTable::open's footer checks and meta walk (table.rs:75-112) for
        n_files resident file images; d_info: 8 u64 per file."""
        check(lib().tpz_open_index(self.handle, C.c_void_p(d_src), span_bytes, C.c_void_p(d_span),
                                   n_files, C.c_void_p(d_info), C.c_void_p(d_file_block),
                                   C.c_void_p(d_file_key), C.c_void_p(d_scratch), scratch_bytes,
                                   C.c_void_p(stream)), "tpz_open_index")

    def open_metas_ptrs(self, d_src: int, span_bytes: int, d_span: int, n_files: int, d_info: int,
                        d_file_block: int, d_file_key: int, d_scratch: int, scratch_bytes: int,
                        d_ext: int, d_first_pos: int, d_first_keys: int, block_cap: int,
                        key_cap: int, stream: int = 0) -> None:
        """tpz_open_metas: every opened file's extents, first-key positions and first keys from
        tpz_open_index's checkpoints, and the codec flag in d_info."""
        check(lib().tpz_open_metas(self.handle, C.c_void_p(d_src), span_bytes, C.c_void_p(d_span),
                                   n_files, C.c_void_p(d_info), C.c_void_p(d_file_block),
                                   C.c_void_p(d_file_key), C.c_void_p(d_scratch), scratch_bytes,
                                   C.c_void_p(d_ext), C.c_void_p(d_first_pos),
                                   C.c_void_p(d_first_keys), block_cap, key_cap,
                                   C.c_void_p(stream)), "tpz_open_metas")

    def table_runs_layout_ptrs(self, d_tables: int, n_runs: int, h_block_first: int,
                               d_block_first: int, d_run_first: int, d_info: int,
                               stream: int = 0) -> None:
        """tpz_table_runs_layout: the entries, key bytes and value bytes before every block of
        n_runs resident tables (Table descriptors in device memory) in run order, the run table
        and the totals; d_info: 4 u64."""
        check(lib().tpz_table_runs_layout(self.handle, C.c_void_p(d_tables), n_runs,
                                          C.c_void_p(h_block_first), C.c_void_p(d_block_first),
                                          C.c_void_p(d_run_first), C.c_void_p(d_info),
                                          C.c_void_p(stream)), "tpz_table_runs_layout")

    def table_runs_entries_ptrs(self, d_tables: int, n_runs: int, h_block_first: int,
                                d_block_first: int, d_keys: int, key_cap: int, d_kpos: int,
                                d_vals: int, val_cap: int, d_vpos: int, entry_cap: int,
                                stream: int = 0, aligned: int | None = None) -> None:
        """tpz_table_runs_entries: the tables' keys, values and entry positions gathered into one
        tpz_entries, a run per table. aligned (0 / 1): the diagnostic export with the gather's
        form chosen (1: aligned loads and a funnel shift; 0: the product's wave_copy;
        tools/runs_probe.py)."""
        args = (self.handle, C.c_void_p(d_tables), n_runs, C.c_void_p(h_block_first),
                C.c_void_p(d_block_first), C.c_void_p(d_keys), key_cap, C.c_void_p(d_kpos),
                C.c_void_p(d_vals), val_cap, C.c_void_p(d_vpos), entry_cap)
        if aligned is None:
            check(lib().tpz_table_runs_entries(*args, C.c_void_p(stream)), "tpz_table_runs_entries")
        else:
            check(lib().tpz_debug_table_runs_entries(*args, int(aligned), C.c_void_p(stream)),
                  "tpz_debug_table_runs_entries")

    def flat_entry_pos_ptrs(self, cols: dict, n_blocks: int, d_kpos: int, d_vpos: int,
                            d_info: int, stream: int = 0) -> None:
        """tpz_flat_entry_pos: the flat columns' entry positions (cols maps FLAT_FIELDS -> pointer)."""
        c = FlatColumns(*[cols[f] for f in FLAT_FIELDS])
        check(lib().tpz_flat_entry_pos(self.handle, C.byref(c), n_blocks, C.c_void_p(d_kpos),
                                       C.c_void_p(d_vpos), C.c_void_p(d_info), C.c_void_p(stream)),
              "tpz_flat_entry_pos")

    def encode_blocks_ptrs(self, ent: Entries, d_first: int, d_ext: int, n_blocks: int,
                           d_out: int, stream: int = 0) -> None:
        """tpz_encode_blocks: Block::encode + CRC + Uncompress tag for every planned block."""
        check(lib().tpz_encode_blocks(self.handle, C.byref(ent), C.c_void_p(d_first),
                                      C.c_void_p(d_ext), n_blocks, C.c_void_p(d_out),
                                      C.c_void_p(stream)), "tpz_encode_blocks")


def _pack_ends(ctx, d_ext: int, n_blocks: int, src_bytes: int, cols: dict, d_first: int,
               d_dense: int, stream: int = 0) -> None:
    b = Batch(None, d_ext, n_blocks, src_bytes)
    c = Columns(*[cols[f] for f in COLUMN_FIELDS])
    check(lib().tpz_pack_ends(ctx.handle, C.byref(b), C.byref(c), C.c_void_p(d_first),
                              C.c_void_p(d_dense), C.c_void_p(stream)), "tpz_pack_ends")


def host_decoded_bound(h_src: int, h_ext: int, n_blocks: int) -> int:
    """tpz_host_decoded_bound: an upper bound of the decoded bytes of blocks in host memory."""
    b = C.c_uint64()
    check(lib().tpz_host_decoded_bound(C.c_void_p(h_src), C.c_void_p(h_ext), n_blocks,
                                       C.byref(b)), "tpz_host_decoded_bound")
    return int(b.value)


def bloom_geometry(n_keys: int, fpp: float):
    """tpz_bloom_geometry: (filter length in bytes, k) of Bloom::from_keys (bloom.rs:48-70), or
    None where the reference asserts (fpp outside [0, 1)) or divides by zero (fpp 0 with keys)."""
    ln, k = C.c_uint64(), C.c_uint32()
    rc = lib().tpz_bloom_geometry(n_keys, fpp, C.byref(ln), C.byref(k))
    return None if rc != SUCCESS else (int(ln.value), int(k.value))


def sst_image_bytes(data_bytes: int, n_blocks: int, first_key_bytes: int, filter_len: int) -> int:
    """tpz_sst_image_bytes: the size of an SST file image (filter_len 0: no bloom section)."""
    return int(lib().tpz_sst_image_bytes(data_bytes, n_blocks, first_key_bytes, filter_len))


def open_scratch_bytes(span_bytes: int, n_files: int) -> int:
    """tpz_open_scratch_bytes: 16 bytes per TPZ_OPEN_TILE of the span plus two tiles per file."""
    return (span_bytes // OPEN_TILE + 2 * n_files) * 16


def xxh3_64(b: bytes) -> int:
    """xxh3_64 on the host through the library (tpz_host_xxh3_64)."""
    return int(lib().tpz_host_xxh3_64(b, len(b)))

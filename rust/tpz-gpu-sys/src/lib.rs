//! `extern "C"` binding of `libtpz_gpu.so`, the C ABI declared in `include/tpz_gpu.h`.
//!
//! Every item mirrors one declaration of the header (same name, same field order, same
//! argument types); `tests/test_rust_binding.py` parses both files and fails when they drift
//! apart. The safe layer topazdb uses sits in `rust/topazdb-gpu` (`Block::from_columns`,
//! `SsTable::read_blocks_gpu`), which replaces the reference's `SsTable::read_block` +
//! `Block::decode` (`src/table.rs:154-164`, `src/block.rs:46-65`) for batches of blocks.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

/// `tpz_err`: an API failure (a per-block outcome is a `TPZ_BLOCK_*` status, not an error).
pub type TpzErr = c_int;
pub const TPZ_SUCCESS: TpzErr = 0;
pub const TPZ_ERR_INVALID_ARG: TpzErr = -1;
pub const TPZ_ERR_HIP: TpzErr = -2;
pub const TPZ_ERR_NO_DEVICE: TpzErr = -3;
pub const TPZ_ERR_NOMEM: TpzErr = -4;
pub const TPZ_ERR_INTERNAL: TpzErr = -5;
pub const TPZ_ERR_SIZES: TpzErr = -6;

/// `tpz_block_status`, one byte per block in `d_status` / `h_status`.
pub const TPZ_BLOCK_OK: u8 = 0;
pub const TPZ_BLOCK_EMPTY: u8 = 1;
pub const TPZ_BLOCK_BAD_TAG: u8 = 2;
pub const TPZ_BLOCK_UNSUPPORTED_CODEC: u8 = 3;
pub const TPZ_BLOCK_CHECKSUM_MISMATCH: u8 = 4;
pub const TPZ_BLOCK_MALFORMED: u8 = 5;
pub const TPZ_BLOCK_OK_SPILLED: u8 = 6;
pub const TPZ_BLOCK_SPILL_FULL: u8 = 7;
pub const TPZ_BLOCK_CODEC_ERROR: u8 = 8;
pub const TPZ_BLOCK_BAD_ENTRY: u8 = 9;

/// `tpz_entry_class`: per-entry class byte of a `TPZ_BLOCK_BAD_ENTRY` block's spill record.
pub const TPZ_ENTRY_OK: u8 = 0;
pub const TPZ_ENTRY_BAD_VALUE: u8 = 1;
pub const TPZ_ENTRY_BAD_KEY: u8 = 2;

pub const TPZ_ABI_VERSION: c_int = 8;
pub const TPZ_LDS_BLOCK_BYTES: u32 = 94192;
pub const TPZ_BIGWAVE_BLOCK_BYTES: u32 = 0x40000000;
pub const TPZ_PLAN_ASYNC_MAX_BLOCK: u32 = 10242;
pub const TPZ_MERGE_MAX_RUNS: u32 = 256;
pub const TPZ_GET_MAX_LEVELS: u32 = 16;

/// `tpz_get_keys`' `d_result`, one byte per query.
pub const TPZ_GET_ABSENT: u8 = 0;
pub const TPZ_GET_FOUND: u8 = 1;
pub const TPZ_GET_DELETED: u8 = 2;
pub const TPZ_GET_ERROR: u8 = 3;

/// The header declares `tpz_scan_ranges` / `tpz_scan_entries` (additive within ABI 8).
pub const TPZ_HAS_SCAN: u32 = 1;
/// One wave merges a scan, a cursor per lane.
pub const TPZ_SCAN_MAX_TABLES: u32 = 64;
/// `tpz_scan_ranges`' `d_lo_kind` / `d_hi_kind`, one byte per scan (`std::ops::Bound`; AFTER,
/// lower only, continues a scan that reported MORE from its last yielded key).
pub const TPZ_BOUND_UNBOUNDED: u8 = 0;
pub const TPZ_BOUND_INCLUDED: u8 = 1;
pub const TPZ_BOUND_EXCLUDED: u8 = 2;
pub const TPZ_BOUND_AFTER: u8 = 3;
/// `tpz_scan_ranges`' `d_result`, one byte per scan.
pub const TPZ_SCAN_DONE: u8 = 0;
pub const TPZ_SCAN_MORE: u8 = 1;
pub const TPZ_SCAN_ERROR: u8 = 2;

/// The header declares `tpz_entries_bound` / `tpz_table_cut` / `tpz_sst_finish` (additive within
/// ABI 8).
pub const TPZ_HAS_TABLES: u32 = 1;
/// `tpz_table_cut`'s `d_cut[0]`.
pub const TPZ_CUT_NONE: u64 = 0;
pub const TPZ_CUT_FOUND: u64 = 1;
pub const TPZ_CUT_BAD_ENTRY: u64 = 2;

/// The header declares `tpz_mem_prefix`, `tpz_lsm_get_keys` / `tpz_lsm_get_values` and
/// `tpz_lsm_scan_ranges` / `tpz_lsm_scan_entries` (additive within ABI 8).
pub const TPZ_HAS_MEM: u32 = 1;
/// The most memtable runs one call takes.
pub const TPZ_MEM_MAX_RUNS: u32 = 16;
/// `d_table = TPZ_HIT_MEM | run` for a hit in a memtable run.
pub const TPZ_HIT_MEM: u32 = 0x80000000;
/// The header declares `tpz_level_scan_ranges` / `tpz_level_scan_entries` (additive within ABI 8):
/// the scan with one merge cursor per level below L0, so a level may hold any number of tables.
pub const TPZ_HAS_LEVEL_SCAN: u32 = 1;
/// The most cursors of one scan: runs + L0 tables + non-empty levels below L0.
pub const TPZ_LEVEL_SCAN_MAX_CURSORS: u32 = 64;

/// The header declares `tpz_mem_build`, `tpz_wal_index` and `tpz_wal_entries` (additive within
/// ABI 8): a memtable run built on the device from a write batch or a WAL image.
pub const TPZ_HAS_MEM_BUILD: u32 = 1;
/// `tpz_mem_build`'s `mode`: `MemTable::open`'s rule (the last record of a key wins, the first
/// empty key ends the replay) or `do_mem_put`'s (the first entry of the highest version wins).
pub const TPZ_MEM_REPLAY: u32 = 0;
pub const TPZ_MEM_PUT: u32 = 1;
/// `tpz_wal_index`'s `h_info[1]`: how the walk ended.
pub const TPZ_WAL_END_IMAGE: u64 = 0;
pub const TPZ_WAL_END_EMPTY_KEY: u64 = 1;
pub const TPZ_WAL_TRUNCATED: u64 = 2;

/// The header declares `tpz_open_index` / `tpz_open_metas` (additive within ABI 8): `SsTable::open`'s
/// parse over file images that are resident in HBM.
pub const TPZ_HAS_OPEN: u32 = 1;
/// Bytes of meta section per checkpoint of `tpz_open_index`'s scratch.
pub const TPZ_OPEN_TILE: u32 = 4096;
/// `tpz_open_index`'s `d_info[8 f]`: the file's status, `SsTable::open`'s checks in order.
pub const TPZ_OPEN_OK: u64 = 0;
pub const TPZ_OPEN_SHORT: u64 = 1;
pub const TPZ_OPEN_BLOOM_RANGE: u64 = 2;
pub const TPZ_OPEN_META_RANGE: u64 = 3;
pub const TPZ_OPEN_META_TRUNCATED: u64 = 4;
pub const TPZ_OPEN_BAD_EXTENTS: u64 = 5;
pub const TPZ_OPEN_NO_BLOCKS: u64 = 6;
pub const TPZ_OPEN_UNSUPPORTED: u64 = 7;

/// The header declares `tpz_table_runs_layout` / `tpz_table_runs_entries` (additive within ABI 8):
/// resident tables gathered into the runs `tpz_merge_runs` takes.
pub const TPZ_HAS_TABLE_RUNS: u32 = 1;

/// The header declares `tpz_raw_verify` and the `tpz_raw_*` seek and get calls (additive within
/// ABI 8): point gets served from the encoded blocks in place, without decoded columns.
pub const TPZ_HAS_RAW_TABLES: u32 = 1;

/// `tpz_open_scratch_bytes` (a static inline of the header): 16 bytes per tile of the span plus
/// two tiles per file.
pub const fn tpz_open_scratch_bytes(span_bytes: u64, n_files: u64) -> u64 {
    (span_bytes / TPZ_OPEN_TILE as u64 + 2 * n_files) * 16
}

/// `tpz_batch`: blocks (or ranges, or files) back to back in HBM; block i is
/// `d_src[d_ext[i] .. d_ext[i + 1])`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzBatch {
    pub d_src: *const u8,
    pub d_ext: *const u64,
    pub n_blocks: u32,
    pub src_bytes: u64,
}

/// `tpz_columns`: the decode's outputs in HBM (slotted layout: block i's keys, then its values
/// from the next 16-byte boundary, at `tpz_layout_slot_base(ext[i], i)`).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzColumns {
    pub d_data: *mut u8,
    pub d_ends: *mut u32,
    pub d_count: *mut u32,
    pub d_status: *mut u8,
    pub d_crc: *mut u32,
    pub d_spill: *mut u8,
    pub spill_cap: u64,
    pub d_spill_off: *mut u64,
    pub d_spill_used: *mut u64,
    pub d_entry_first: *const u64,
}

/// `tpz_flat_columns`: the flat layout (one dense key column and one dense value column for the
/// batch, exact `{kend, vend}` pairs); `d_first` from `tpz_flat_layout`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzFlatColumns {
    pub d_keys: *mut u8,
    pub d_values: *mut u8,
    pub d_ends: *mut u32,
    pub d_first: *const u64,
    pub d_count: *mut u32,
    pub d_status: *mut u8,
    pub d_crc: *mut u32,
    pub d_spill: *mut u8,
    pub spill_cap: u64,
    pub d_spill_off: *mut u64,
    pub d_spill_used: *mut u64,
}

/// `tpz_host_columns`: `tpz_decode_blocks_host`'s outputs in host memory.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzHostColumns {
    pub h_data: *mut u8,
    pub h_ends: *mut u32,
    pub ends_cap: u64,
    pub h_first: *mut u64,
    pub h_count: *mut u32,
    pub h_status: *mut u8,
    pub h_crc: *mut u32,
    pub h_spill: *mut u8,
    pub spill_cap: u64,
    pub h_spill_off: *mut u64,
    pub h_spill_used: *mut u64,
    pub h_dext: *mut u64,
    pub data_cap: u64,
}

/// `tpz_table`: a table decoded on the device plus its block metas' first keys.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzTable {
    pub d_first_keys: *const u8,
    pub d_first_pos: *const u64,
    pub d_ext: *const u64,
    pub n_blocks: u32,
    pub d_data: *const u8,
    pub d_ends: *const u32,
    pub d_count: *const u32,
    pub d_status: *const u8,
    pub d_spill: *const u8,
    pub d_spill_off: *const u64,
    pub d_entry_first: *const u64,
}

/// `tpz_get_table`: a resident table of `tpz_get_keys`: its `tpz_table` plus its bloom filter
/// (`d_filter` null: the table has none and `may_contain` is true).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzGetTable {
    pub table: TpzTable,
    pub d_filter: *const u8,
    pub filter_len: u64,
}
/// The header declares this struct with a tag, so the extern block names it as the header does.
#[allow(non_camel_case_types)]
pub type tpz_get_table = TpzGetTable;

/// `tpz_raw_table`: an in-place table: its encoded blocks where they lie in HBM (Uncompress form),
/// `tpz_raw_verify`'s status column, its block first keys and its bloom filter (`d_filter` null:
/// no filter).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzRawTable {
    pub d_first_keys: *const u8,
    pub d_first_pos: *const u64,
    pub d_src: *const u8,
    pub d_ext: *const u64,
    pub n_blocks: u32,
    pub d_status: *const u8,
    pub d_filter: *const u8,
    pub filter_len: u64,
}
/// Declared with a tag in the header, as `tpz_get_table` is.
#[allow(non_camel_case_types)]
pub type tpz_raw_table = TpzRawTable;

/// `tpz_sst_image`: one output table of `tpz_sst_finish`; its data region sits at `d_image`
/// already (`d_filter` null: no bloom section).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzSstImage {
    pub d_image: *mut u8,
    pub data_bytes: u64,
    pub d_first: *const u32,
    pub d_ext: *const u64,
    pub n_blocks: u32,
    pub entry_base: u32,
    pub d_filter: *const u8,
    pub filter_len: u64,
}
/// Declared with a tag in the header, as `tpz_get_table` is.
#[allow(non_camel_case_types)]
pub type tpz_sst_image = TpzSstImage;

/// `tpz_entries`: sorted entries in HBM (the write side).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzEntries {
    pub d_keys: *const u8,
    pub d_kpos: *const u64,
    pub d_vals: *const u8,
    pub d_vpos: *const u64,
    pub n_entries: u32,
    pub key_bytes: u64,
    pub val_bytes: u64,
}

/// `tpz_mem_run`: one memtable's sorted snapshot in HBM (`MemTables::view()` order in `d_runs`:
/// immutable memtables oldest first, the mutable one last); `d_prefix` null: no prefix column.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct TpzMemRun {
    pub entries: TpzEntries,
    pub d_prefix: *const u64,
}
/// Declared with a tag in the header, as `tpz_get_table` is.
#[allow(non_camel_case_types)]
pub type tpz_mem_run = TpzMemRun;

/// `tpz_ctx` (opaque).
#[repr(C)]
pub struct TpzCtx {
    _private: [u8; 0],
}

extern "C" {
    pub fn tpz_abi_version() -> c_int;
    pub fn tpz_layout_slot_base(ext_i: u64, i: u64) -> u64;
    pub fn tpz_layout_value_start(key_bytes: u64) -> u64;
    pub fn tpz_layout_entry_base(ext_i: u64, i: u64) -> u64;
    pub fn tpz_layout_data_capacity(src_bytes: u64, n_blocks: u64) -> u64;
    pub fn tpz_layout_entry_capacity(src_bytes: u64, n_blocks: u64) -> u64;
    pub fn tpz_layout_spill_stream(n: u64) -> u64;
    pub fn tpz_layout_spill_classes(n: u64, k: u64, v: u64) -> u64;
    pub fn tpz_ctx_create(device: c_int, out: *mut *mut TpzCtx) -> TpzErr;
    pub fn tpz_ctx_destroy(ctx: *mut TpzCtx);
    pub fn tpz_ctx_reserve(ctx: *mut TpzCtx, max_blocks: u32, stream: *mut c_void) -> TpzErr;
    pub fn tpz_decode_blocks(ctx: *mut TpzCtx, batch: *const TpzBatch, out: *const TpzColumns,
                             stream: *mut c_void) -> TpzErr;
    pub fn tpz_decode_check(ctx: *mut TpzCtx, stream: *mut c_void) -> TpzErr;
    pub fn tpz_entry_first(ctx: *mut TpzCtx, batch: *const TpzBatch, d_first: *mut u64,
                           stream: *mut c_void) -> TpzErr;
    pub fn tpz_pack_ends(ctx: *mut TpzCtx, batch: *const TpzBatch, cols: *const TpzColumns,
                         d_first: *const u64, d_dense: *mut u32, stream: *mut c_void) -> TpzErr;
    pub fn tpz_layout_compress_bound(src_bytes: u64, n_blocks: u64) -> u64;
    pub fn tpz_compress_blocks(ctx: *mut TpzCtx, batch: *const TpzBatch, codec: u32, d_dst: *mut u8,
                               d_dst_ext: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_flat_layout(ctx: *mut TpzCtx, batch: *const TpzBatch, d_first: *mut u64,
                           stream: *mut c_void) -> TpzErr;
    pub fn tpz_decode_blocks_flat(ctx: *mut TpzCtx, batch: *const TpzBatch,
                                  out: *const TpzFlatColumns, stream: *mut c_void) -> TpzErr;
    pub fn tpz_host_decoded_bound(h_src: *const u8, h_ext: *const u64, n_blocks: u32,
                                  bound: *mut u64) -> TpzErr;
    pub fn tpz_decode_blocks_host(ctx: *mut TpzCtx, h_src: *const u8, h_ext: *const u64,
                                  n_blocks: u32, out: *const TpzHostColumns,
                                  chunk_blocks: u32) -> TpzErr;
    pub fn tpz_verify_blocks_host(ctx: *mut TpzCtx, h_src: *const u8, h_ext: *const u64,
                                  n_blocks: u32, h_status: *mut u8, h_crc: *mut u32,
                                  h_count: *mut u32, h_plain: *mut u8, plain_cap: u64,
                                  h_dext: *mut u64, chunk_blocks: u32) -> TpzErr;
    pub fn tpz_crc32_ranges(ctx: *mut TpzCtx, ranges: *const TpzBatch, d_crc: *mut u32,
                            stream: *mut c_void) -> TpzErr;
    pub fn tpz_verify_files(ctx: *mut TpzCtx, files: *const TpzBatch, d_crc: *mut u32,
                            d_status: *mut u8, stream: *mut c_void) -> TpzErr;
    pub fn tpz_verify_files_flat_layout(ctx: *mut TpzCtx, blocks: *const TpzBatch,
                                        d_file_block: *const u32, tails: *const TpzBatch,
                                        d_crc: *mut u32, d_status: *mut u8, d_first: *mut u64,
                                        stream: *mut c_void) -> TpzErr;
    pub fn tpz_decompressed_sizes(ctx: *mut TpzCtx, batch: *const TpzBatch, d_size: *mut u64,
                                  stream: *mut c_void) -> TpzErr;
    pub fn tpz_decompressed_sizes_claimed(ctx: *mut TpzCtx, batch: *const TpzBatch,
                                          d_size: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_decompress_check(ctx: *mut TpzCtx, stream: *mut c_void) -> TpzErr;
    pub fn tpz_decompress_blocks(ctx: *mut TpzCtx, batch: *const TpzBatch, d_dst: *mut u8,
                                 d_dst_ext: *const u64, d_status: *mut u8,
                                 stream: *mut c_void) -> TpzErr;
    pub fn tpz_seek_keys(ctx: *mut TpzCtx, table: *const TpzTable, d_keys: *const u8,
                         d_key_pos: *const u64, n_keys: u32, d_block: *mut u32,
                         d_entry: *mut u32, d_status: *mut u8, d_valid: *mut u8,
                         stream: *mut c_void) -> TpzErr;
    pub fn tpz_bloom_may_contain(ctx: *mut TpzCtx, d_filter: *const u8, filter_len: u64,
                                 d_keys: *const u8, d_key_pos: *const u64, n_keys: u32,
                                 d_out: *mut u8, stream: *mut c_void) -> TpzErr;
    pub fn tpz_host_xxh3_64(h_buf: *const u8, len: u64) -> u64;
    pub fn tpz_bloom_geometry(n_keys: u64, fpp: f64, filter_len: *mut u64, k: *mut u32) -> TpzErr;
    pub fn tpz_bloom_build(ctx: *mut TpzCtx, d_keys: *const u8, d_key_pos: *const u64,
                           n_keys: u32, fpp: f64, d_filter: *mut u8, stream: *mut c_void) -> TpzErr;
    pub fn tpz_plan_blocks(ctx: *mut TpzCtx, entries: *const TpzEntries, block_size: u32,
                           d_first: *mut u32, d_ext: *mut u64, h_n_blocks: *mut u32,
                           h_bad_entry: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_encode_blocks(ctx: *mut TpzCtx, entries: *const TpzEntries, d_first: *const u32,
                             d_ext: *const u64, n_blocks: u32, d_out: *mut u8,
                             stream: *mut c_void) -> TpzErr;
    pub fn tpz_plan_blocks_async(ctx: *mut TpzCtx, entries: *const TpzEntries, block_size: u32,
                                 d_first: *mut u32, d_ext: *mut u64, d_info: *mut u32,
                                 stream: *mut c_void) -> TpzErr;
    pub fn tpz_encode_blocks_async(ctx: *mut TpzCtx, entries: *const TpzEntries,
                                   d_first: *const u32, d_ext: *const u64, d_info: *const u32,
                                   d_out: *mut u8, stream: *mut c_void) -> TpzErr;
    pub fn tpz_merge_runs(ctx: *mut TpzCtx, entries: *const TpzEntries, h_run_first: *const u32,
                          n_runs: u32, d_out_keys: *mut u8, d_out_kpos: *mut u64,
                          d_out_vals: *mut u8, d_out_vpos: *mut u64, d_src_entry: *mut u32,
                          d_info: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_get_keys(ctx: *mut TpzCtx, d_tables: *const tpz_get_table, n_tables: u32,
                        h_level_first: *const u32, n_levels: u32, d_keys: *const u8,
                        d_key_pos: *const u64, n_keys: u32, d_result: *mut u8, d_status: *mut u8,
                        d_table: *mut u32, d_block: *mut u32, d_entry: *mut u32,
                        d_val_pos: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_get_values(ctx: *mut TpzCtx, d_tables: *const tpz_get_table, n_tables: u32,
                          n_keys: u32, d_result: *const u8, d_table: *const u32,
                          d_block: *const u32, d_entry: *const u32, d_val_pos: *const u64,
                          d_vals: *mut u8, val_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_mem_prefix(ctx: *mut TpzCtx, entries: *const TpzEntries, d_prefix: *mut u64,
                          stream: *mut c_void) -> TpzErr;
    pub fn tpz_mem_build(ctx: *mut TpzCtx, entries: *const TpzEntries, mode: u32,
                         d_version: *const u64, d_out_keys: *mut u8, d_out_kpos: *mut u64,
                         d_out_vals: *mut u8, d_out_vpos: *mut u64, d_out_prefix: *mut u64,
                         d_src_entry: *mut u32, d_out_version: *mut u64, d_info: *mut u64,
                         stream: *mut c_void) -> TpzErr;
    pub fn tpz_wal_index(h_image: *const u8, image_bytes: u64, h_rec: *mut u64, rec_cap: u64,
                         h_info: *mut u64) -> TpzErr;
    pub fn tpz_wal_entries(ctx: *mut TpzCtx, d_image: *const u8, image_bytes: u64,
                           d_rec: *const u64, n_records: u32, d_keys: *mut u8, d_kpos: *mut u64,
                           d_vals: *mut u8, d_vpos: *mut u64, d_info: *mut u64,
                           stream: *mut c_void) -> TpzErr;
    pub fn tpz_lsm_get_keys(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                            d_tables: *const tpz_get_table, n_tables: u32,
                            h_level_first: *const u32, n_levels: u32, d_keys: *const u8,
                            d_key_pos: *const u64, n_keys: u32, d_result: *mut u8,
                            d_status: *mut u8, d_table: *mut u32, d_block: *mut u32,
                            d_entry: *mut u32, d_val_pos: *mut u64,
                            stream: *mut c_void) -> TpzErr;
    pub fn tpz_lsm_get_values(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                              d_tables: *const tpz_get_table, n_tables: u32, n_keys: u32,
                              d_result: *const u8, d_table: *const u32, d_block: *const u32,
                              d_entry: *const u32, d_val_pos: *const u64, d_vals: *mut u8,
                              val_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_lsm_scan_ranges(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                               d_tables: *const tpz_get_table, n_tables: u32,
                               h_level_first: *const u32, n_levels: u32, d_lo_keys: *const u8,
                               d_lo_pos: *const u64, d_lo_kind: *const u8, d_hi_keys: *const u8,
                               d_hi_pos: *const u64, d_hi_kind: *const u8, n_scans: u32,
                               limit: u32, d_result: *mut u8, d_status: *mut u8,
                               d_where: *mut u32, d_hit_table: *mut u32, d_hit_block: *mut u32,
                               d_hit_entry: *mut u32, d_first: *mut u64, d_key_first: *mut u64,
                               d_val_first: *mut u64, d_info: *mut u64,
                               stream: *mut c_void) -> TpzErr;
    pub fn tpz_lsm_scan_entries(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                                d_tables: *const tpz_get_table, n_tables: u32, n_scans: u32,
                                limit: u32, d_hit_table: *const u32, d_hit_block: *const u32,
                                d_hit_entry: *const u32, d_first: *const u64, d_keys: *mut u8,
                                key_cap: u64, d_kpos: *mut u64, d_vals: *mut u8, val_cap: u64,
                                d_vpos: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_level_scan_ranges(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                                 d_tables: *const tpz_get_table, n_tables: u32,
                                 h_level_first: *const u32, n_levels: u32, d_lo_keys: *const u8,
                                 d_lo_pos: *const u64, d_lo_kind: *const u8,
                                 d_hi_keys: *const u8, d_hi_pos: *const u64,
                                 d_hi_kind: *const u8, n_scans: u32, limit: u32,
                                 d_result: *mut u8, d_status: *mut u8, d_where: *mut u32,
                                 d_hit_table: *mut u32, d_hit_block: *mut u32,
                                 d_hit_entry: *mut u32, d_first: *mut u64,
                                 d_key_first: *mut u64, d_val_first: *mut u64, d_info: *mut u64,
                                 stream: *mut c_void) -> TpzErr;
    pub fn tpz_level_scan_entries(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                                  d_tables: *const tpz_get_table, n_tables: u32, n_scans: u32,
                                  limit: u32, d_hit_table: *const u32, d_hit_block: *const u32,
                                  d_hit_entry: *const u32, d_first: *const u64, d_keys: *mut u8,
                                  key_cap: u64, d_kpos: *mut u64, d_vals: *mut u8, val_cap: u64,
                                  d_vpos: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_scan_ranges(ctx: *mut TpzCtx, d_tables: *const tpz_get_table, n_tables: u32,
                           h_level_first: *const u32, n_levels: u32, d_lo_keys: *const u8,
                           d_lo_pos: *const u64, d_lo_kind: *const u8, d_hi_keys: *const u8,
                           d_hi_pos: *const u64, d_hi_kind: *const u8, n_scans: u32, limit: u32,
                           d_result: *mut u8, d_status: *mut u8, d_where: *mut u32,
                           d_hit_table: *mut u32, d_hit_block: *mut u32, d_hit_entry: *mut u32,
                           d_first: *mut u64, d_key_first: *mut u64, d_val_first: *mut u64,
                           d_info: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_scan_entries(ctx: *mut TpzCtx, d_tables: *const tpz_get_table, n_tables: u32,
                            n_scans: u32, limit: u32, d_hit_table: *const u32,
                            d_hit_block: *const u32, d_hit_entry: *const u32,
                            d_first: *const u64, d_keys: *mut u8, key_cap: u64,
                            d_kpos: *mut u64, d_vals: *mut u8, val_cap: u64, d_vpos: *mut u64,
                            stream: *mut c_void) -> TpzErr;
    pub fn tpz_flat_entry_pos(ctx: *mut TpzCtx, cols: *const TpzFlatColumns, n_blocks: u32,
                              d_kpos: *mut u64, d_vpos: *mut u64, d_info: *mut u32,
                              stream: *mut c_void) -> TpzErr;
    pub fn tpz_entries_bound(ctx: *mut TpzCtx, entries: *const TpzEntries, d_keys: *const u8,
                             d_key_pos: *const u64, d_inclusive: *const u8, n_probes: u32,
                             d_out: *mut u32, stream: *mut c_void) -> TpzErr;
    pub fn tpz_table_cut(ctx: *mut TpzCtx, entries: *const TpzEntries, start: u32,
                         win_entries: u32, seg_end: u32, d_first: *mut u32, d_ext: *mut u64,
                         d_cut_ext: *const u64, d_plan_info: *mut u32, block_size: u32,
                         capacity: u64, d_cut: *mut u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_sst_image_bytes(data_bytes: u64, n_blocks: u64, first_key_bytes: u64,
                               filter_len: u64) -> u64;
    pub fn tpz_sst_finish(ctx: *mut TpzCtx, entries: *const TpzEntries,
                          d_images: *const tpz_sst_image, n_images: u32, max_blocks: u32,
                          d_base: *mut u8, span_bytes: u64, d_info: *mut u64,
                          stream: *mut c_void) -> TpzErr;
    pub fn tpz_open_index(ctx: *mut TpzCtx, d_src: *const u8, span_bytes: u64,
                          d_span: *const u64, n_files: u32, d_info: *mut u64,
                          d_file_block: *mut u64, d_file_key: *mut u64, d_scratch: *mut u8,
                          scratch_bytes: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_open_metas(ctx: *mut TpzCtx, d_src: *const u8, span_bytes: u64,
                          d_span: *const u64, n_files: u32, d_info: *mut u64,
                          d_file_block: *const u64, d_file_key: *const u64,
                          d_scratch: *const u8, scratch_bytes: u64, d_ext: *mut u64,
                          d_first_pos: *mut u64, d_first_keys: *mut u8, block_cap: u64,
                          key_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_table_runs_layout(ctx: *mut TpzCtx, d_tables: *const TpzTable, n_runs: u32,
                                 h_block_first: *const u32, d_block_first: *mut u64,
                                 d_run_first: *mut u32, d_info: *mut u64,
                                 stream: *mut c_void) -> TpzErr;
    pub fn tpz_table_runs_entries(ctx: *mut TpzCtx, d_tables: *const TpzTable, n_runs: u32,
                                  h_block_first: *const u32, d_block_first: *const u64,
                                  d_keys: *mut u8, key_cap: u64, d_kpos: *mut u64,
                                  d_vals: *mut u8, val_cap: u64, d_vpos: *mut u64,
                                  entry_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_verify(ctx: *mut TpzCtx, batch: *const TpzBatch, d_status: *mut u8,
                          d_crc: *mut u32, stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_seek_keys(ctx: *mut TpzCtx, table: *const tpz_raw_table, d_keys: *const u8,
                             d_key_pos: *const u64, n_keys: u32, d_block: *mut u32,
                             d_entry: *mut u32, d_status: *mut u8, d_valid: *mut u8,
                             stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_get_keys(ctx: *mut TpzCtx, d_tables: *const tpz_raw_table, n_tables: u32,
                            h_level_first: *const u32, n_levels: u32, d_keys: *const u8,
                            d_key_pos: *const u64, n_keys: u32, d_result: *mut u8,
                            d_status: *mut u8, d_table: *mut u32, d_block: *mut u32,
                            d_entry: *mut u32, d_val_pos: *mut u64,
                            stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_get_values(ctx: *mut TpzCtx, d_tables: *const tpz_raw_table, n_tables: u32,
                              n_keys: u32, d_result: *const u8, d_table: *const u32,
                              d_block: *const u32, d_entry: *const u32, d_val_pos: *const u64,
                              d_vals: *mut u8, val_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_lsm_get_keys(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                                d_tables: *const tpz_raw_table, n_tables: u32,
                                h_level_first: *const u32, n_levels: u32, d_keys: *const u8,
                                d_key_pos: *const u64, n_keys: u32, d_result: *mut u8,
                                d_status: *mut u8, d_table: *mut u32, d_block: *mut u32,
                                d_entry: *mut u32, d_val_pos: *mut u64,
                                stream: *mut c_void) -> TpzErr;
    pub fn tpz_raw_lsm_get_values(ctx: *mut TpzCtx, d_runs: *const tpz_mem_run, n_runs: u32,
                                  d_tables: *const tpz_raw_table, n_tables: u32, n_keys: u32,
                                  d_result: *const u8, d_table: *const u32, d_block: *const u32,
                                  d_entry: *const u32, d_val_pos: *const u64, d_vals: *mut u8,
                                  val_cap: u64, stream: *mut c_void) -> TpzErr;
    pub fn tpz_build_blocks(h_keys: *const u8, h_kpos: *const u64, h_vals: *const u8,
                            h_vpos: *const u64, n_entries: u64, block_size: u32, h_out: *mut u8,
                            out_cap: u64, h_ext: *mut u64, ext_cap: u64, n_blocks: *mut u64,
                            out_len: *mut u64) -> c_int;
    pub fn tpz_snappy_encode_blocks(h_src: *const u8, h_ext: *const u64, n_blocks: u64,
                                    h_out: *mut u8, out_cap: u64, h_out_ext: *mut u64,
                                    out_len: *mut u64) -> c_int;
    pub fn tpz_lz4_encode_blocks(h_src: *const u8, h_ext: *const u64, n_blocks: u64,
                                 h_out: *mut u8, out_cap: u64, h_out_ext: *mut u64,
                                 out_len: *mut u64) -> c_int;
    pub fn tpz_host_crc32(h_buf: *const u8, len: u64) -> u32;
    pub fn tpz_format_block_error(status: c_int, crc_expected: u32, crc_actual: u32,
                                  buf: *mut c_char, cap: usize) -> c_int;
    pub fn tpz_last_error() -> *const c_char;
}

/// The header's inline layout helpers, restated (the exported `tpz_layout_*` functions compute
/// the same values; `tests/test_abi.py` checks those against the header's definitions).
pub mod layout {
    /// Block i's output slot: its keys, then its values from `value_start(K)`.
    pub fn slot_base(ext_i: u64, i: u64) -> u64 {
        ((ext_i + 127) & !127) + 256 * i
    }
    pub fn value_start(key_bytes: u64) -> u64 {
        (key_bytes + 15) & !15
    }
    /// Block i's first {kend, vend} pair in the slotted ends.
    pub fn entry_base(ext_i: u64, i: u64) -> u64 {
        16 * (ext_i / 96 + i)
    }
}

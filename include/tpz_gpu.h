/*
 * tpz_gpu.h — C ABI of the MI355X (gfx950) SSTable block decode + checksum path.
 *
 * This is the drop-in boundary for topazdb's read hot path. The reference has no FFI (it is a
 * plain Rust API); each entry point below replaces the reference items it names, and
 * INTEGRATION.md shows the `extern "C"` binding a topazdb maintainer adds on the Rust side.
 *
 *   tpz_decode_blocks_host  the same from host memory: H2D, decode and D2H pipelined in the
 *                           library (SsTable::read_block + FileObject::read, table.rs:154-164,
 *                           file_object.rs:23-27)
 *   tpz_decode_blocks       SsTable::read_block (src/table.rs:154-164) batched over many
 *                           blocks -> Block::decode (src/block.rs:46-65) -> compress::decode
 *                           tag dispatch (src/block/compress.rs:95-113) -> checksum::
 *                           verify_checksum (src/checksum.rs:12-21) -> every
 *                           BlockIterator::seek_to materialised (src/block/iterator.rs:63-83)
 *   tpz_crc32_ranges        checksum::calculate_checksum (src/checksum.rs:6-10) over many ranges
 *   tpz_verify_files        FileObject::open's whole-file CRC (src/table/file_object.rs:57-78),
 *                           batched over SST file images (SsTable::open, src/table.rs:91-112)
 *   tpz_decompress_blocks   compress::decode's codec step: snappy (src/block/compress.rs:104-107)
 *                           and lz4 (:108-111) blocks to their Uncompress form
 *   tpz_format_block_error  the reference's error strings (checksum.rs:18-21, compress.rs:97,102)
 *   tpz_plan_blocks +       the write side for compaction output: SsTableBuilder::add +
 *   tpz_encode_blocks       block_build (src/table/builder.rs:49-85) over entries in HBM
 *   tpz_merge_runs          MergeIterator over one SsTableIterator per input table, as sub_compact
 *                           drives it (src/iterators/merge_iterator.rs:41-106, src/level.rs:178-222)
 *   tpz_mem_build +         a memtable run from entries in arrival order: MemTable::open's replay
 *   tpz_wal_index +         (src/mem_table.rs:119-143, over WalIterator, src/wal/iterator.rs) and
 *   tpz_wal_entries         do_mem_put's versions (:155-196), with MemTable::size()
 *   tpz_get_keys +          LevelController::get (src/level.rs:427-465) for a batch of keys over
 *   tpz_get_values          tables resident in HBM: the walk over L0 and the levels, then the values
 *   tpz_entries_bound +     do_compact around the merge (src/level.rs:133-222): sub_compact's key
 *   tpz_table_cut +         range, SsTableBuilder::reach_capacity's table cuts (src/table/
 *   tpz_sst_finish          builder.rs:88-94) and SsTableBuilder::build + FileObject::create's
 *                           file bytes (builder.rs:97-141, src/table/file_object.rs:33-48)
 *
 * Plain pointers and sizes only. Pointers named d_* are device (HBM) pointers of the context's
 * device; h_* are host pointers. `stream` is a hipStream_t passed as void* (NULL = default).
 * Every call is asynchronous on `stream` unless it says otherwise; the library never frees
 * caller memory and holds no global mutable state (one context per device; many host threads
 * may share it, and decodes on different streams run concurrently: every stream gets its own
 * device workspace).
 */
#ifndef TPZ_GPU_H
#define TPZ_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ABI version -------------------------------------------------------------------------
 * Bumped on every incompatible change of a status value, a struct layout or a record format:
 *   1  round 1: statuses 0..7 with 6 = OVERLAP, 7 = TOO_LARGE (device limits); 5-field columns
 *   2  6 = OK_SPILLED, 7 = SPILL_FULL, 8 = CODEC_ERROR; spill arena fields in tpz_columns
 *   3  9 = BAD_ENTRY (a CRC-valid block with out-of-range entries decodes, with per-entry
 *      classes in its spill record, instead of MALFORMED); MALFORMED is now only the block-level
 *      panic of Block::decode
 *   4  tpz_decode_blocks_host takes snappy / lz4 blocks (tpz_host_columns.h_dext, data_cap);
 *      the exact ends layout (tpz_columns.d_entry_first, tpz_table.d_entry_first)
 *   5  the flat layout: tpz_flat_layout + tpz_decode_blocks_flat (tpz_flat_columns); no
 *      existing struct or status changed
 *   6  claimed LZ4 sizes: tpz_decompressed_sizes_claimed, tpz_decompress_check, TPZ_ERR_SIZES;
 *      tpz_verify_blocks_host (the host pipeline's verdict without the column downloads, for
 *      Block views of the caller's bytes). Round 6, same ABI: tpz_decode_blocks_host /
 *      tpz_verify_blocks_host return TPZ_ERR_NOMEM only for a short caller buffer (an internal
 *      chunk overflow is TPZ_ERR_INTERNAL), and tpz_decode_check also fails for a wave path row
 *      claim that timed out or was overwritten; new entry point tpz_verify_files_flat_layout
 *      (open + flat layout from one read of the blocks)
 *   7  compaction's merge step: tpz_merge_runs (MergeIterator over sorted runs in HBM) and
 *      tpz_flat_entry_pos (flat columns -> tpz_entries), TPZ_MERGE_MAX_RUNS; no existing struct
 *      or status changed. The bump also covers the three round-6 changes that version 6 took in
 *      without one: the export tpz_verify_files_flat_layout, tpz_decode_check failing for a wave
 *      path row claim, and TPZ_ERR_NOMEM of the host pipeline meaning a short caller buffer only
 *   8  batched point gets over resident tables: tpz_get_keys (LevelController::get's walk over
 *      L0 and the levels) and tpz_get_values (the gather of the values found), tpz_get_table,
 *      TPZ_GET_*; no existing struct or status changed. Same ABI, additive: tpz_scan_ranges and
 *      tpz_scan_entries (LsmStorage::scan's SST half), TPZ_BOUND_*, TPZ_SCAN_*; a consumer tests
 *      TPZ_HAS_SCAN. Same ABI, additive: tpz_entries_bound, tpz_table_cut, tpz_sst_finish and
 *      tpz_sst_image_bytes (a compaction task's key ranges, table cuts and SST file images),
 *      tpz_sst_image, TPZ_CUT_*; a consumer tests TPZ_HAS_TABLES. Same ABI, additive: memtable
 *      runs as a resident input (tpz_mem_run, tpz_mem_prefix, TPZ_MEM_MAX_RUNS, TPZ_HIT_MEM) and
 *      LsmStorage::get and LsmStorage::scan over runs plus tables (tpz_lsm_get_keys,
 *      tpz_lsm_get_values, tpz_lsm_scan_ranges, tpz_lsm_scan_entries); a consumer tests
 *      TPZ_HAS_MEM. Same ABI, additive: building a memtable run on the device from a write batch
 *      or a WAL image (tpz_mem_build, tpz_wal_index, tpz_wal_entries, TPZ_MEM_REPLAY / TPZ_MEM_PUT,
 *      TPZ_WAL_*); a consumer tests TPZ_HAS_MEM_BUILD
 * A consumer compiled against one header checks tpz_abi_version() == TPZ_ABI_VERSION. */
#define TPZ_ABI_VERSION 8
int tpz_abi_version(void);

/* ---- API return codes ------------------------------------------------------------------- */
typedef enum {
  TPZ_SUCCESS = 0,
  TPZ_ERR_INVALID_ARG = -1, /* null pointer, inconsistent sizes                               */
  TPZ_ERR_HIP = -2,         /* a HIP runtime call failed (tpz_last_error has the text)        */
  TPZ_ERR_NO_DEVICE = -3,   /* no gfx950 device with that index                               */
  TPZ_ERR_NOMEM = -4,
  TPZ_ERR_INTERNAL = -5,    /* a device-side consistency check failed (tpz_decode_check)      */
  TPZ_ERR_SIZES = -6        /* claimed codec sizes were not exact (tpz_decompress_check)      */
} tpz_err;

/* ---- per-block outcome (written to columns.status[i]) ------------------------------------
 * Maps one-to-one onto what Block::decode + iterating every entry does in the reference. */
typedef enum {
  TPZ_BLOCK_OK = 0,                /* Ok(Block); all entries decoded                         */
  TPZ_BLOCK_EMPTY = 1,             /* Err("data is empty")          compress.rs:96-98        */
  TPZ_BLOCK_BAD_TAG = 2,           /* Err("invaild data")           compress.rs:102          */
  TPZ_BLOCK_UNSUPPORTED_CODEC = 3, /* tag 2 (snappy) / 3 (lz4) given to tpz_decode_blocks
                                      without the codec step (tpz_decompress_blocks) first    */
  TPZ_BLOCK_CHECKSUM_MISMATCH = 4, /* Err("checksum: expected E, actual A") checksum.rs:18-21 */
  TPZ_BLOCK_MALFORMED = 5,         /* CRC-valid, but Block::decode itself panics on it: the
                                      decompressed block is shorter than its CRC, or the payload
                                      is too short for n / the n offsets (block.rs:49-59)      */
  TPZ_BLOCK_OK_SPILLED = 6,        /* Ok(Block); all entries decoded, into the spill arena
                                      (tpz_columns.d_spill) instead of the block's slot: the
                                      decoded bytes do not fit the slot (entries that overlap or
                                      repeat, which iterator.rs:63-83 accepts: 6*n > len or
                                      value_start(K) + V > len + 2), or the block is too long
                                      for the LDS paths (longer than TPZ_LDS_BLOCK_BYTES with
                                      64+ entries, or longer than TPZ_BIGWAVE_BLOCK_BYTES).
                                      Same answer as TPZ_BLOCK_OK.                             */
  TPZ_BLOCK_SPILL_FULL = 7,        /* Ok(Block) in the reference, but the caller's spill arena
                                      was too small for this block's record:
                                      d_spill_off[i] = the bytes it needs. Decode again with
                                      spill_cap >= *d_spill_used.                               */
  TPZ_BLOCK_CODEC_ERROR = 8,       /* Err of the codec: snap's decompress_vec rejects the
                                      stream (compress.rs:104-107)                           */
  TPZ_BLOCK_BAD_ENTRY = 9          /* Ok(Block): Block::decode succeeds (block.rs:46-65 checks
                                      no entry), but at least one entry lies out of range, and
                                      BlockIterator panics when it reaches that entry
                                      (iterator.rs:74-82, :91-109). Decoded into the spill arena
                                      like OK_SPILLED, count[i] = n, with one class byte per
                                      entry in the record (tpz_entry_class, below), so that a
                                      reader fails exactly where the reference's iterator does:
                                      a scan stopped by an empty key before the bad entry, a seek
                                      whose bisection never touches it and SsTable::open's first
                                      and last entry all succeed.                              */
} tpz_block_status;

/* Per-entry class of a TPZ_BLOCK_BAD_ENTRY block (its spill record), in the reference's terms
 * for entry i at o = offsets[i] in data (L = data.len(), src/block/iterator.rs:74-82):
 *   OK         the entry reads whole: key and value are in the record
 *   BAD_VALUE  key readable (o + 2 + klen <= L), value not (o + 4 + klen + vlen > L): the key is
 *              in the record, the value is empty; seek_to(i) panics, while seek_to_key's
 *              bisection (which reads keys only, :95-98) may compare against the key
 *   BAD_KEY    o + 2 > L or o + 2 + klen > L: key and value empty; any read of entry i panics */
typedef enum {
  TPZ_ENTRY_OK = 0,
  TPZ_ENTRY_BAD_VALUE = 1,
  TPZ_ENTRY_BAD_KEY = 2
} tpz_entry_class;

/* The largest block the LDS decode paths stage whole (every block a block_size <= 64 KiB
 * BlockBuilder emits fits); longer blocks with 64 or more entries are decoded by the spill path,
 * straight from HBM. */
#define TPZ_LDS_BLOCK_BYTES 94192u
/* Longer blocks with fewer than 64 entries are decoded one wave per block straight from HBM
 * (the bigwave path, as OK) up to this length; past it by the spill path (OK_SPILLED). No block
 * length limit exists: the spill path decodes any length the extents can express. */
#define TPZ_BIGWAVE_BLOCK_BYTES 0x40000000u

/* ---- batch input -------------------------------------------------------------------------
 * Encoded blocks back to back in one device buffer (an SST data region [0, meta_off), or the
 * data regions of many SSTs concatenated). Block i is d_src[d_ext[i] .. d_ext[i+1]); d_ext has
 * n_blocks+1 entries and is non-decreasing. src_bytes = d_ext[n_blocks] (host copy). Blocks may
 * start at any byte offset; d_src itself must be 16-byte aligned for tpz_decode_blocks and the
 * codec step (hipMalloc returns 256-byte aligned memory; TPZ_ERR_INVALID_ARG otherwise). The
 * CRC entry points take any d_src. */
typedef struct {
  const uint8_t* d_src;
  const uint64_t* d_ext;
  uint32_t n_blocks;
  uint64_t src_bytes;
} tpz_batch;

/* ---- decoded columns (the "slotted" layout) ----------------------------------------------
 * No global prefix pass: every block owns a slot derived from its input extent, so blocks
 * decode independently (and shard across GPUs) with no cross-block communication. Every slot
 * starts on a 128-byte line and is written in whole lines (HBM3E then never sees a partial-line
 * write from two different workgroups).
 *   data  : block i's slot starts at s = tpz_slot_base(ext[i], i). It holds the block's key
 *           bytes (every entry's key, in entry order) at data[s .. s + K), K = the block's key
 *           bytes, then its value bytes from data[s + tpz_value_start(K)] on (K rounded up to
 *           16; the bytes in between are unspecified). One stream per block: the copy writes it
 *           with whole-wave stores, and a consumer moves one contiguous range per block.
 *   ends  : entry j of block i (j < count[i]) has its exclusive end offsets at ends[2*(e+j)]
 *           (key, relative to s) and ends[2*(e+j)+1] (value, relative to s + vs),
 *           e = tpz_entry_base(ext[i], i), K = ends[2*(e+count[i]-1)] (0 when count is 0),
 *           vs = tpz_value_start(K):
 *             key_j   = data[s +      (j ? ends[2(e+j-1)]   : 0) .. s +      ends[2(e+j)]]
 *             value_j = data[s + vs + (j ? ends[2(e+j-1)+1] : 0) .. s + vs + ends[2(e+j)+1]]
 *   count[i]  : entries in block i (n) for OK, OK_SPILLED, BAD_ENTRY and SPILL_FULL, else 0
 *   status[i] : tpz_block_status
 *   crc[i]    : CRC-32 the device computed over the payload (valid for OK, OK_SPILLED,
 *               BAD_ENTRY, SPILL_FULL, MALFORMED (n / offsets too short), CHECKSUM_MISMATCH;
 *               the stored one is the payload's trailing u32)
 * Bytes of a slot beyond the block's own data are unspecified. A slot spans at most
 * len + 129 bytes (len = the block's encoded length), which never reaches the next slot.
 *
 * Spill arena. A block whose decoded bytes do not fit its slot (the reference iterator accepts
 * offsets that overlap or repeat, so n entries may materialise up to n * 65535 key and value
 * bytes each), one too long for the LDS paths, or one with out-of-range entries is decoded into
 * the caller's spill arena and reported TPZ_BLOCK_OK_SPILLED (TPZ_BLOCK_BAD_ENTRY for the last
 * kind). Its record starts at r = d_spill_off[i] (128-aligned):
 *   u32 ends[2*count[i]] at d_spill[r ..]         {kend, vend} pairs, exactly as in the slot
 *   stream at d_spill[r + tpz_spill_stream(count[i]) ..]: keys, then values from
 *                                                 tpz_value_start(K), as in the slot
 *   BAD_ENTRY only: count[i] class bytes (tpz_entry_class) at
 *                   d_spill[r + tpz_spill_classes(count[i], K, V) ..], K / V = the last kend /
 *                   vend; an entry's unreadable key or value is empty in ends and stream
 * (K and V each fit in 32 bits: at most 65535 entries of at most 65535 bytes.) Records are
 * placed by an atomic cursor; *d_spill_used = the bytes every spilled block of the call asked
 * for (the library zeroes it first). A record that does not fit spill_cap leaves the block
 * TPZ_BLOCK_SPILL_FULL with d_spill_off[i] = its size: decode the batch again with
 * spill_cap >= *d_spill_used. Batches written by topazdb's BlockBuilder with block_size <= 64 KiB
 * never spill; d_spill may then be NULL with spill_cap 0. */
typedef struct {
  uint8_t* d_data;          /* capacity tpz_data_capacity(src_bytes, n_blocks) bytes        */
  uint32_t* d_ends;         /* capacity 2 * tpz_entry_capacity(src_bytes, n_blocks) u32      */
  uint32_t* d_count;        /* n_blocks */
  uint8_t* d_status;        /* n_blocks */
  uint32_t* d_crc;          /* n_blocks */
  uint8_t* d_spill;         /* spill arena (see above), spill_cap bytes; may be NULL if 0   */
  uint64_t spill_cap;
  uint64_t* d_spill_off;    /* n_blocks: written for OK_SPILLED, BAD_ENTRY, SPILL_FULL only   */
  uint64_t* d_spill_used;   /* one u64                                                      */
  const uint64_t* d_entry_first; /* NULL: the slotted ends (tpz_entry_base). Else the exact
                                    ends layout: block i's {kend, vend} pairs at
                                    d_ends[2*d_entry_first[i] ..], d_ends holding
                                    2*d_entry_first[n_blocks] u32, d_entry_first from
                                    tpz_entry_first (see below)                             */
} tpz_columns;

/* Offset of a spilled record's stream from the record start: its 2*n u32 ends, 128-aligned. */
static inline uint64_t tpz_spill_stream(uint64_t n) {
  return (8u * n + 127u) & ~(uint64_t)127u;
}
/* Bytes of a spilled record with n entries, K key and V value bytes (128-aligned). */
static inline uint64_t tpz_spill_record_bytes(uint64_t n, uint64_t k, uint64_t v) {
  return tpz_spill_stream(n) + ((((k + 15u) & ~(uint64_t)15u) + v + 127u) & ~(uint64_t)127u);
}
/* Offset of a BAD_ENTRY record's class bytes from the record start (its ends and stream come
 * first); the record then spans tpz_spill_classes(n, K, V) + n bytes, 128-aligned. */
static inline uint64_t tpz_spill_classes(uint64_t n, uint64_t k, uint64_t v) {
  return tpz_spill_record_bytes(n, k, v);
}

static inline uint64_t tpz_slot_base(uint64_t ext_i, uint64_t i) {
  return ((ext_i + 127u) & ~(uint64_t)127u) + 256u * i;
}
static inline uint64_t tpz_value_start(uint64_t key_bytes) {
  return (key_bytes + 15u) & ~(uint64_t)15u;
}
static inline uint64_t tpz_entry_base(uint64_t ext_i, uint64_t i) {
  return 16u * (ext_i / 96u + i);
}
static inline uint64_t tpz_data_capacity(uint64_t src_bytes, uint64_t n_blocks) {
  return tpz_slot_base(src_bytes, n_blocks) + 128u;
}
static inline uint64_t tpz_entry_capacity(uint64_t src_bytes, uint64_t n_blocks) {
  return tpz_entry_base(src_bytes, n_blocks) + 16u;
}

/* Exported copies of the layout helpers for FFI callers that cannot use static inline. */
uint64_t tpz_layout_slot_base(uint64_t ext_i, uint64_t i);
uint64_t tpz_layout_value_start(uint64_t key_bytes);
uint64_t tpz_layout_entry_base(uint64_t ext_i, uint64_t i);
uint64_t tpz_layout_data_capacity(uint64_t src_bytes, uint64_t n_blocks);
uint64_t tpz_layout_entry_capacity(uint64_t src_bytes, uint64_t n_blocks);
uint64_t tpz_layout_spill_stream(uint64_t n);
uint64_t tpz_layout_spill_classes(uint64_t n, uint64_t k, uint64_t v);

/* ---- context ------------------------------------------------------------------------------ */
typedef struct tpz_ctx tpz_ctx;

/* Creates a context on HIP device `device` (uploads the CRC tables, sizes the launch grid for
 * the device's CU count). Fails with TPZ_ERR_NO_DEVICE unless the device is gfx950. */
tpz_err tpz_ctx_create(int device, tpz_ctx** out);
void tpz_ctx_destroy(tpz_ctx* ctx);

/* Pre-sizes the device workspace `stream` uses for batches of up to max_blocks blocks, so that
 * tpz_decode_blocks on that stream never allocates (needed before capturing it in a hipGraph).
 * Each stream gets its own workspace, so decodes on different streams may run concurrently.
 * Every call on one stream reuses that stream's workspace (worklists, plan buffers and the
 * pinned word tpz_plan_blocks reads back): calls that share a stream must not be made from
 * several host threads at once. Give each host thread its own stream. */
tpz_err tpz_ctx_reserve(tpz_ctx* ctx, uint32_t max_blocks, void* stream);

/* ---- the hot path ------------------------------------------------------------------------ */
/* Checksum-verify and decode every block of `batch` into `out`. Asynchronous on `stream`;
 * per-block outcomes land in out->d_status (no host sync, no host-visible error for a bad
 * block: that is data, not an API failure). */
tpz_err tpz_decode_blocks(tpz_ctx* ctx, const tpz_batch* batch, const tpz_columns* out,
                          void* stream);

/* Synchronizes `stream` and reports whether every decode on it so far ran to completion:
 * TPZ_ERR_INTERNAL (and the flag cleared) when a tail workgroup's bounded wait for the big
 * path timed out, so that blocks of the spill worklist may have been left undecoded (their
 * status/count/crc are then unspecified). The wait only times out if the device stalls for
 * about a second. The flag is sticky per stream: it covers every decode queued on `stream`
 * since the previous check, so a device-resident integration calls this once per batch (after
 * the batch's decode, before it trusts the outputs; tpz_decode_blocks_host and the Python layer
 * do). The flag is read and cleared in stream order (no null-stream copy). */
tpz_err tpz_decode_check(tpz_ctx* ctx, void* stream);

/* The exact ends layout. The slotted ends reserve the worst case (a pair per 6 input bytes,
 * ~1.36x the input in ends alone for 4 KiB blocks) so that blocks need no prefix pass; a caller
 * that keeps the decoded columns resident (a block cache in HBM) can instead reserve exactly n
 * pairs per block, 8 bytes per entry: d_first[i] = the sum over blocks 0..i-1 of the header n
 * (u16 at the block's first two bytes) of each block the decode parses in place (last byte 1,
 * len >= 7 + 2n, 6n <= len; 0 for any other block, whose pairs, if any, live in its spill
 * record), d_first[n_blocks] = the total, computed on the device (a header pass and a scan, no
 * host sync). A block that decodes in place has count == its header n, so its pairs fit. Pass
 * d_first as tpz_columns.d_entry_first / tpz_table.d_entry_first. The batch must be the one
 * the decode runs over (after the codec step). Asynchronous on `stream`; uses the stream's
 * workspace. */
tpz_err tpz_entry_first(tpz_ctx* ctx, const tpz_batch* batch, uint64_t* d_first, void* stream);

/* Dense entry ends for consumers that copy a batch out (e.g. back to the host): the slotted
 * ends reserve the worst case (a pair per 6 input bytes, ~1.33x the input) so that blocks need no
 * prefix pass; this packs the used pairs. d_first = exclusive prefix sums of out->d_count
 * (n_blocks + 1 entries, from the caller's device scan); block i's count[i] {kend, vend} pairs go
 * to d_dense[2*d_first[i] .. 2*d_first[i+1]) (for OK_SPILLED and BAD_ENTRY blocks from their
 * spill records; zeros for a block whose status is none of OK, OK_SPILLED, BAD_ENTRY). */
tpz_err tpz_pack_ends(tpz_ctx* ctx, const tpz_batch* batch, const tpz_columns* cols,
                      const uint64_t* d_first, uint32_t* d_dense, void* stream);

/* ---- the flat layout ---------------------------------------------------------------------
 * One dense key column and one dense value column for the whole batch: every key of every
 * block, in SsTableIterator order (blocks in batch order, entries in block order: what
 * BlockIterator::key() returns for each entry, src/block/iterator.rs:63-83), back to back, and
 * likewise every value; the {kend, vend} pairs give each entry's end within its block's run.
 *
 * tpz_flat_layout sizes the columns on the device (one pass over the batch and three scans, no
 * host sync): d_first holds 3 * (n_blocks + 1) u64, with st = n_blocks + 1:
 *   d_first[i]          entries of blocks 0..i-1 (the exact ends layout's d_entry_first)
 *   d_first[st + i]     key bytes of blocks 0..i-1: block i's keys start at d_keys[d_first[st + i]]
 *   d_first[2 st + i]   value bytes of blocks 0..i-1, likewise in d_values
 * and the totals at i = n_blocks (read them back to size the columns). A block's reservation is
 * what decoding it yields when its CRC matches: its header n entries and the bytes of every key
 * and value that reads whole (src/block/iterator.rs:74-82: an unreadable key or value reserves
 * nothing, as in TPZ_BLOCK_BAD_ENTRY), for a block with tag 1 and len >= 7 + 2n; nothing for any
 * other block (EMPTY, BAD_TAG, UNSUPPORTED_CODEC, MALFORMED). Run the codec step first for
 * snappy / lz4 batches. Asynchronous on `stream`; uses the stream's workspace. */
tpz_err tpz_flat_layout(tpz_ctx* ctx, const tpz_batch* batch, uint64_t* d_first, void* stream);

/* tpz_decode_blocks_flat: tpz_decode_blocks into the flat layout. Per block i (st as above):
 *   keys:   key_j   = d_keys  [kb + (j ? ends[2(e+j-1)]   : 0) .. kb + ends[2(e+j)]]
 *   values: value_j = d_values[vb + (j ? ends[2(e+j-1)+1] : 0) .. vb + ends[2(e+j)+1]]
 *   with e = d_first[i], kb = d_first[st + i], vb = d_first[2 st + i], j < count[i]
 *   d_count, d_status, d_crc: as tpz_columns. Every decoded block reports TPZ_BLOCK_OK or
 *   TPZ_BLOCK_BAD_ENTRY (no OK_SPILLED: the spill path writes the columns too); a block that
 *   fails its CRC keeps its reserved bytes, unspecified.
 *   d_spill / spill_cap / d_spill_off / d_spill_used: a BAD_ENTRY block's count[i] class bytes
 *   (tpz_entry_class) at d_spill[d_spill_off[i] ..] (records of n bytes rounded up to 128; the
 *   entry's unreadable key or value is empty in the columns), SPILL_FULL as in tpz_columns.
 *   May be NULL / 0 for batches without bad entries.
 * d_keys and d_values must be 16-byte aligned, with d_first[st + n_blocks] and
 * d_first[2 st + n_blocks] bytes; d_ends 2 * d_first[n_blocks] u32. Blocks share 16-byte chunks
 * of the columns at their boundaries: the decode writes those chunks byte-exactly (each block
 * its own bytes), so blocks still decode independently. Asynchronous on `stream`. */
typedef struct {
  uint8_t* d_keys;
  uint8_t* d_values;
  uint32_t* d_ends;
  const uint64_t* d_first;  /* from tpz_flat_layout over the same batch */
  uint32_t* d_count;
  uint8_t* d_status;
  uint32_t* d_crc;
  uint8_t* d_spill;
  uint64_t spill_cap;
  uint64_t* d_spill_off;
  uint64_t* d_spill_used;
} tpz_flat_columns;

tpz_err tpz_decode_blocks_flat(tpz_ctx* ctx, const tpz_batch* batch, const tpz_flat_columns* out,
                               void* stream);

/* ---- the host pipeline -------------------------------------------------------------------
 * SsTable::read_block for a whole run of blocks that sit in HOST memory (src/table.rs:154-164;
 * the bytes FileObject::read's pread returns, src/table/file_object.rs:23-27): the library
 * copies the blocks to the device in chunks, runs compress::decode's codec step on them where a
 * block is snappy or lz4 (src/block/compress.rs:104-111; topazdb's default codec is snappy,
 * src/opt.rs:48), decodes them (tpz_decode_blocks), packs the used entry ends (tpz_pack_ends)
 * and copies every output back, on three streams (upload, decode, download) so that both PCIe
 * directions stay busy. Synchronous: returns when every output is in host memory. The caller's
 * buffers are page-locked for the duration of the call when they are not already
 * (hipHostRegister); pinned buffers (hipHostMalloc) avoid that cost.
 *
 * Block i = h_src[h_ext[i] .. h_ext[i+1]) (h_ext non-decreasing, any alignment, any mix of
 * codec tags). The decoded layout is that of tpz_columns over the DECODED extents h_dext: for
 * a batch of Uncompress blocks h_dext = h_ext; when any block is snappy or lz4, h_dext[i+1] -
 * h_dext[i] = the block's length after the codec step (its Uncompress form; the codec's Err
 * leaves a 1-byte stub, tpz_decompressed_sizes), computed on the device chunk by chunk with no
 * whole-batch host sync. Outputs:
 *   h_data    data_cap bytes (0 = tpz_data_capacity(h_ext[n], n), enough for Uncompress
 *             batches; for snappy / lz4 blocks use tpz_data_capacity(bound, n) with bound from
 *             tpz_host_decoded_bound): the slotted stream layout, block i's slot at
 *             tpz_slot_base(h_dext[i], i)
 *   h_dext    n + 1 decoded extents (may be NULL for a batch without snappy / lz4 blocks)
 *   h_ends    every decoded block's {kend, vend} pairs, dense in block order: block i's at
 *             h_ends[2*h_first[i] ..]; ends_cap = its capacity in u32
 *   h_first   n + 1 entries: h_first[i] = pairs before block i (OK, OK_SPILLED and BAD_ENTRY
 *             blocks only)
 *   h_count, h_status, h_crc    n each, as tpz_columns; a block whose codec step failed has
 *             status TPZ_BLOCK_CODEC_ERROR (the reference's Err of the codec), count 0
 *   h_spill, spill_cap, h_spill_off, h_spill_used   as tpz_columns, in host memory: spilled
 *             blocks' records (the library's device arenas grow as needed)
 * Returns TPZ_ERR_NOMEM when ends_cap, spill_cap or data_cap is too small: h_first[n],
 * *h_spill_used and h_dext[n] then hold the sizes needed (the call can be repeated with larger
 * buffers; NOMEM has no other cause, so a repeat with buffers of those sizes succeeds). chunk_blocks = 0 picks the default (8,192 blocks per chunk: 34 MB of 4 KiB blocks,
 * the fastest of 4K..64K on MI355X, profiles/r2/e2e_sweep.jsonl). The streams and device buffers
 * of a call are kept by the context and reused by its next calls (one set per concurrent
 * caller). */
typedef struct {
  uint8_t* h_data;
  uint32_t* h_ends;
  uint64_t ends_cap;
  uint64_t* h_first;
  uint32_t* h_count;
  uint8_t* h_status;
  uint32_t* h_crc;
  uint8_t* h_spill;
  uint64_t spill_cap;
  uint64_t* h_spill_off;
  uint64_t* h_spill_used;
  uint64_t* h_dext;         /* n + 1 decoded extents, or NULL (see above)                   */
  uint64_t data_cap;        /* bytes at h_data; 0 = tpz_data_capacity(h_ext[n], n)          */
} tpz_host_columns;

/* An upper bound of h_dext[n] for blocks in host memory, from their headers alone: a snappy
 * block's preamble length + 1, an lz4 block's size prefix + 1 (lz4::block::decompress may keep
 * fewer bytes), any other block's own length. Size h_data with tpz_data_capacity(bound, n). */
tpz_err tpz_host_decoded_bound(const uint8_t* h_src, const uint64_t* h_ext, uint32_t n_blocks,
                               uint64_t* bound);

tpz_err tpz_decode_blocks_host(tpz_ctx* ctx, const uint8_t* h_src, const uint64_t* h_ext,
                               uint32_t n_blocks, const tpz_host_columns* out,
                               uint32_t chunk_blocks);

/* SsTable::read_block's checks for a run of blocks in host memory, with the decoded columns left
 * on the device: the reference's Block is {data: payload[2 + 2n ..], offsets} of the block's
 * Uncompress form (src/block.rs:46-65), so a host that holds the block bytes needs only the
 * device's verdict (CRC, tag, header) and, for snappy / lz4 blocks, the decompressed bytes to
 * build it without a copy (rust/topazdb-gpu/src/table/gpu.rs, read_blocks_gpu). Same pipeline as
 * tpz_decode_blocks_host (chunked H2D, codec step, decode) without the slot, ends and spill
 * downloads. Outputs: h_status, h_crc, h_count (n each, as tpz_host_columns); h_dext (n + 1, may
 * be NULL for a batch without snappy / lz4 blocks; h_ext is then the decoded layout); h_plain /
 * plain_cap: for a batch with snappy / lz4 blocks, h_dext[n] bytes receiving every block's
 * Uncompress form at h_dext[i] (tpz_host_decoded_bound bounds it); unused (may be NULL)
 * otherwise. Returns TPZ_ERR_NOMEM when plain_cap < h_dext[n] (h_dext[n] then holds the size
 * needed). */
tpz_err tpz_verify_blocks_host(tpz_ctx* ctx, const uint8_t* h_src, const uint64_t* h_ext,
                               uint32_t n_blocks, uint8_t* h_status, uint32_t* h_crc,
                               uint32_t* h_count, uint8_t* h_plain, uint64_t plain_cap,
                               uint64_t* h_dext, uint32_t chunk_blocks);

/* ---- whole-range CRC-32 ------------------------------------------------------------------
 * Ranges use the batch type: range i is d_src[d_ext[i] .. d_ext[i+1]) (d_ext non-decreasing,
 * n_blocks = number of ranges, src_bytes = d_ext[n]). Each range may be up to 2^35 bytes.
 *
 * checksum::calculate_checksum (src/checksum.rs:6-10) of every range: d_crc[i] = CRC-32/ISO-HDLC
 * of range i. Asynchronous on `stream`. */
tpz_err tpz_crc32_ranges(tpz_ctx* ctx, const tpz_batch* ranges, uint32_t* d_crc, void* stream);

/* FileObject::open's whole-file check (src/table/file_object.rs:57-78) for SST file images in
 * HBM: range i is a whole file; its CRC-32 over all but the last 4 bytes goes to d_crc[i] and
 * is compared with the big-endian u32 in those 4 bytes. d_status[i] = TPZ_BLOCK_OK,
 * TPZ_BLOCK_CHECKSUM_MISMATCH ("checksum: expected E, actual A", checksum.rs:18-21, with
 * A = d_crc[i]) or TPZ_BLOCK_MALFORMED (file shorter than 4 bytes: the reference's
 * `buf[size - CHECKSUM_SIZE..]` panics). Asynchronous on `stream`. */
tpz_err tpz_verify_files(tpz_ctx* ctx, const tpz_batch* files, uint32_t* d_crc,
                         uint8_t* d_status, void* stream);

/* SsTable::open for every file + tpz_flat_layout of their data blocks, from ONE read of the
 * blocks (the reference's open reads every byte for FileObject::open's CRC, src/table.rs:91-112,
 * src/table/file_object.rs:57-78, before the blocks are read again to decode them): the outputs of
 * tpz_verify_files over the files and of tpz_flat_layout(blocks, d_first).
 *   blocks : every file's data region (its blocks, [0, meta offset) of an SST), the files' regions
 *            back to back: the batch tpz_decode_blocks_flat then decodes
 *   d_file_block : n_files + 1 u32; file f's blocks are blocks d_file_block[f] ..
 *            d_file_block[f + 1] - 1 (d_file_block[n_files] = n_blocks)
 *   tails  : n_files ranges; tail f = the rest of file f after its data region (meta block,
 *            bloom filter, offsets and the 4-byte CRC trailer), so that file f is its data region
 *            followed by tail f. Each tail holds at least the trailer (a file whose tail is
 *            shorter than 4 bytes reports TPZ_BLOCK_MALFORMED with crc 0, as a file shorter than
 *            its trailer does in tpz_verify_files)
 *   d_crc, d_status : n_files, as tpz_verify_files
 * Both d_src 16-byte aligned. Asynchronous on `stream`; uses the stream's workspace. */
tpz_err tpz_verify_files_flat_layout(tpz_ctx* ctx, const tpz_batch* blocks,
                                     const uint32_t* d_file_block, const tpz_batch* tails,
                                     uint32_t* d_crc, uint8_t* d_status, uint64_t* d_first,
                                     void* stream);

/* ---- codec step of compress::decode (src/block/compress.rs:95-113) ------------------------
 * Snappy (tag 2) and LZ4 (tag 3) blocks are decompressed on the device into their Uncompress
 * (tag 1) form, so tpz_decode_blocks then verifies and decodes them like any block:
 *   1. tpz_decompressed_sizes: d_size[i] = the length block i has once decompressed and
 *      re-tagged: for tag 2 the snappy preamble's length + 1 (0 if the preamble is invalid);
 *      for tag 3 the length LZ4_decompress_safe decodes + 1 (lz4::block::decompress keeps only
 *      the decoded bytes, which may be fewer than the size prefix; 1 for an Err); the block's
 *      own length for any other block. No size limit: blocks past the LDS windows are
 *      decompressed straight from HBM to HBM.
 *   2. the caller forms d_dst_ext = exclusive prefix sums of d_size (n_blocks + 1 entries) and
 *      allocates d_dst (d_dst_ext[n] bytes). d_dst_ext[0] may be any position (the blocks then
 *      follow other data in d_dst); every position is 64-bit, as in tpz_batch.
 *   3. tpz_decompress_blocks writes block i's uncompressed form to d_dst[d_dst_ext[i] ..
 *      d_dst_ext[i+1]) (other tags are copied unchanged) and d_status[i] = TPZ_BLOCK_OK,
 *      or TPZ_BLOCK_CODEC_ERROR (the codec's Err). A failed block's range
 *      ends in tag 0, so decoding it reports BAD_TAG; its d_status is the reference's outcome.
 *   4. tpz_decode_blocks over (d_dst, d_dst_ext).
 * LZ4 acceptance is liblz4 1.9.3's LZ4_decompress_safe (the library the reference's lz4 crate
 * binds; restated in oracle/tpz_lz4.c and pinned against liblz4 in tests/test_lz4_oracle.py). */
tpz_err tpz_decompressed_sizes(tpz_ctx* ctx, const tpz_batch* batch, uint64_t* d_size,
                               void* stream);
/* Step 1 without LZ4's walk: a tag-3 block reports its size prefix + 1 (what
 * lz4::block::decompress allocates, compress.rs:108-111; the exact length of every stream
 * lz4::block::compress writes) instead of the length its stream decodes to; the exact walk only
 * where the prefix is invalid or larger than any stream of that length can decode to. Every other
 * block as tpz_decompressed_sizes. A stream that then decodes to another length or fails sets a
 * sticky word of the stream's workspace in tpz_decompress_blocks (that block's output is
 * CODEC_ERROR, the layout is not the exact one): tpz_decompress_check reports it, and the caller
 * sizes the batch with tpz_decompressed_sizes and decompresses it again. Asynchronous on
 * `stream`. */
tpz_err tpz_decompressed_sizes_claimed(tpz_ctx* ctx, const tpz_batch* batch, uint64_t* d_size,
                                       void* stream);
/* Synchronizes `stream`; TPZ_ERR_SIZES (and the word cleared) when a tpz_decompress_blocks on it
 * since the previous check ran over claimed sizes that were not exact, TPZ_SUCCESS otherwise. */
tpz_err tpz_decompress_check(tpz_ctx* ctx, void* stream);
tpz_err tpz_decompress_blocks(tpz_ctx* ctx, const tpz_batch* batch, uint8_t* d_dst,
                              const uint64_t* d_dst_ext, uint8_t* d_status, void* stream);

/* ---- batched point-get side ----------------------------------------
 * A table = its block metas' first keys plus the columns tpz_decode_blocks wrote for its
 * blocks (d_ext: the extents of the batch that decode ran over, i.e. after the codec step).
 *   tpz_seek_keys: for every query key, SsTableIterator::seek_to_key (src/table/iterator.rs:
 *     44-72): find_block_idx (src/table.rs:178-182, partition_point(first_key <= key) - 1,
 *     saturating; the lower-bound bisection), BlockIterator::seek_to_key in that block
 *     (src/block/iterator.rs:91-109: binary search, an equal key returns at once), then the
 *     next block's first entry when that iterator is invalid and a next block exists.
 *     d_block/d_entry = the position, d_valid = is_valid() (iterator.rs:50-52: the current key
 *     is non-empty), d_status = the status of the last block the seek read (non-OK: the
 *     reference's read_block_cached Err, or its panic for MALFORMED; a table with no blocks
 *     gives MALFORMED: block_metas[0] panics; so does a seek whose bisection reads the key of
 *     a BAD_KEY entry or which lands on a BAD_KEY / BAD_VALUE entry (iterator.rs:91-109, the
 *     reference's panic; entries of a BAD_ENTRY block the seek does not touch do not matter);
 *     OK_SPILLED and BAD_ENTRY blocks are read from their spill
 *     records and report OK).
 *   tpz_bloom_may_contain: SsTable::may_contain (src/table.rs:114-119) = Bloom::may_contain
 *     (src/bloom.rs:72-84) of xxh3_64(key) for every key; d_filter = Bloom::encode (the bit
 *     array, then k). d_out = 1 (may contain), 0 (absent), 2 (the reference panics: an empty
 *     filter, or no bit array with k > 0).
 * Keys are packed: key i = d_keys[d_key_pos[i] .. d_key_pos[i+1]). */
typedef struct {
  const uint8_t* d_first_keys;
  const uint64_t* d_first_pos; /* n_blocks + 1 */
  const uint64_t* d_ext;       /* n_blocks + 1 */
  uint32_t n_blocks;
  const uint8_t* d_data;
  const uint32_t* d_ends;
  const uint32_t* d_count;
  const uint8_t* d_status;
  const uint8_t* d_spill;      /* the decode's spill arena and record offsets (OK_SPILLED,
                                  BAD_ENTRY)                                               */
  const uint64_t* d_spill_off;
  const uint64_t* d_entry_first; /* the decode's tpz_columns.d_entry_first (NULL: slotted)   */
} tpz_table;

tpz_err tpz_seek_keys(tpz_ctx* ctx, const tpz_table* table, const uint8_t* d_keys,
                      const uint64_t* d_key_pos, uint32_t n_keys, uint32_t* d_block,
                      uint32_t* d_entry, uint8_t* d_status, uint8_t* d_valid, void* stream);
tpz_err tpz_bloom_may_contain(tpz_ctx* ctx, const uint8_t* d_filter, uint64_t filter_len,
                              const uint8_t* d_keys, const uint64_t* d_key_pos, uint32_t n_keys,
                              uint8_t* d_out, void* stream);
/* xxh3_64 (seed 0) on the host: the hash the reference's bloom uses (xxhash-rust 0.8.5). */
uint64_t tpz_host_xxh3_64(const uint8_t* h_buf, uint64_t len);

/* Bloom::from_keys (src/bloom.rs:48-70) for keys in HBM (SsTableBuilder::build_bloom,
 * src/table/builder.rs:132-141, over xxh3_64 of every added key):
 *   tpz_bloom_geometry (host): the filter's length in bytes (bit array + the k byte) and k for
 *     n_keys keys and false-positive rate fpp, with the reference's f64 arithmetic and saturating
 *     casts; TPZ_ERR_INVALID_ARG unless 0 <= fpp < 1 (bloom.rs:49 asserts).
 *   tpz_bloom_build: writes the filter (Bloom::encode) to d_filter[0 .. filter_len). d_filter must
 *     be 4-byte aligned with room for (filter_len + 3) & ~3 bytes. Asynchronous on `stream`;
 *     uses the stream's grow-only workspace (4 B per probe: n_keys * k * 4 bytes plus slice
 *     histograms), so one build at a time per stream, as with the other workspace users. */
tpz_err tpz_bloom_geometry(uint64_t n_keys, double fpp, uint64_t* filter_len, uint32_t* k);
tpz_err tpz_bloom_build(tpz_ctx* ctx, const uint8_t* d_keys, const uint64_t* d_key_pos,
                        uint32_t n_keys, double fpp, uint8_t* d_filter, void* stream);

/* ---- device write side (SURVEY.md §8f row 4's alternative: compaction output) ------------
 * A run of sorted entries in HBM becomes SST data-region blocks, byte for byte what
 * SsTableBuilder::add + block_build (src/table/builder.rs:49-85) writes with
 * CompressOptions::Uncompress: BlockBuilder's fill rule (src/block/builder.rs:26-41: an entry
 * joins the block while size + encode_len + 2 <= block_size), Block::encode (src/block.rs:31-44),
 * Entry::encode (builder.rs:72-81), the CRC (src/checksum.rs:6-10) and the tag
 * (src/block/compress.rs:85-89). Entry e: key = d_keys[d_kpos[e] .. d_kpos[e+1]), value =
 * d_vals[d_vpos[e] .. d_vpos[e+1]) (d_kpos/d_vpos: n_entries + 1 non-decreasing offsets; key_bytes
 * and val_bytes = the readable bytes at d_keys / d_vals, at least d_kpos[n] / d_vpos[n]).
 *   tpz_plan_blocks: the block cuts. d_first[b] = first entry of block b, d_ext[b] = its byte
 *     offset in the data region (SsTableBuilder's data.len() when it was built, i.e.
 *     BlockMeta::offset), for b <= n_blocks (d_first[n_blocks] = n_entries, d_ext[n_blocks] = the
 *     region's length); both need n_entries + 1 entries. SYNCHRONOUS on `stream` (it returns
 *     *h_n_blocks). An empty key (builder.rs:27 asserts) or an entry no block can hold (encode_len
 *     + 2 > block_size: SsTableBuilder::add recurses without end, table/builder.rs:57-60) makes it
 *     return TPZ_ERR_INVALID_ARG with *h_bad_entry = the first such entry (UINT64_MAX otherwise).
 *     block_size must be in (2, 65536]: past 64 KiB the reference's u16 offsets wrap.
 *   tpz_encode_blocks: writes block b to d_out[d_ext[b] .. d_ext[b+1]) (d_out 16-byte aligned,
 *     d_ext[n_blocks] bytes; no byte outside the blocks is written) for d_first / d_ext /
 *     n_blocks exactly as tpz_plan_blocks returned them for these entries and block_size.
 *     Asynchronous on `stream`; uses the stream's workspace (like tpz_decode_blocks).
 *   tpz_plan_blocks_async: tpz_plan_blocks with its results left on the device:
 *     d_info[0] = the most entries a block starting at any entry would take (>= the longest
 *     block; the plan's chunk tables are that wide), d_info[1] = the first entry the reference rejects
 *     (0xFFFFFFFF: none; d_first / d_ext are then meaningless), d_info[2] = n_blocks (4 u32 of
 *     device memory). No host round trip for block_size <= TPZ_PLAN_ASYNC_MAX_BLOCK (every block
 *     then holds at most 2048 entries, the transfer tables are sized from that bound); a larger
 *     block size reads the longest block back once (its plan chunks follow it). tpz_plan_blocks
 *     is this call plus one read of d_info.
 *   tpz_encode_blocks_async: tpz_encode_blocks with the block count read on the device from
 *     tpz_plan_blocks_async's d_info (a plan with a rejected entry encodes nothing). d_out needs
 *     d_ext[n_blocks] bytes; key_bytes + val_bytes + 13 * n_entries bounds that without reading it.
 * BlockMeta::first_key of block b is entry d_first[b]'s key. */
#define TPZ_PLAN_ASYNC_MAX_BLOCK 10242u
typedef struct {
  const uint8_t* d_keys;
  const uint64_t* d_kpos;
  const uint8_t* d_vals;
  const uint64_t* d_vpos;
  uint32_t n_entries;
  uint64_t key_bytes;
  uint64_t val_bytes;
} tpz_entries;

tpz_err tpz_plan_blocks(tpz_ctx* ctx, const tpz_entries* entries, uint32_t block_size,
                        uint32_t* d_first, uint64_t* d_ext, uint32_t* h_n_blocks,
                        uint64_t* h_bad_entry, void* stream);
tpz_err tpz_encode_blocks(tpz_ctx* ctx, const tpz_entries* entries, const uint32_t* d_first,
                          const uint64_t* d_ext, uint32_t n_blocks, uint8_t* d_out, void* stream);
tpz_err tpz_plan_blocks_async(tpz_ctx* ctx, const tpz_entries* entries, uint32_t block_size,
                              uint32_t* d_first, uint64_t* d_ext, uint32_t* d_info, void* stream);
tpz_err tpz_encode_blocks_async(tpz_ctx* ctx, const tpz_entries* entries, const uint32_t* d_first,
                                const uint64_t* d_ext, const uint32_t* d_info, uint8_t* d_out,
                                void* stream);

/* ---- compaction's merge step, on the device ----------------------------------------------
 * The step between the read side (tpz_decode_blocks_flat) and the write side (tpz_plan_blocks):
 * sub_compact's MergeIterator over one SsTableIterator per input table (src/level.rs:178-222,
 * src/iterators/merge_iterator.rs:41-106), with the entries staying in HBM.
 *
 * tpz_merge_runs: MergeIterator over n_runs sorted runs (merge_iterator.rs:41-106, as sub_compact
 * drives it, level.rs:188-212). `entries` holds every run's entries back to back; run r is entries
 * [h_run_first[r], h_run_first[r+1]) (h_run_first: n_runs + 1 non-decreasing u32 in HOST memory,
 * h_run_first[0] = 0, h_run_first[n_runs] = entries->n_entries; a run may be empty: create()
 * filters those out before it numbers the rest, :48-53). Every run is sorted non-decreasing by
 * key (Rust's [u8] Ord: bytewise, unsigned, a proper prefix is smaller). The iterator then yields
 *   - input entry (run r, position j) iff no run with a lower index holds an equal key (every copy
 *     of a key repeated inside the winning run is yielded, every copy in the other runs is not);
 *   - in the order (key, r, j).
 * Empty values (tombstones) are entries like any other: sub_compact adds them to the builder.
 *   d_out_keys, d_out_vals : the yielded keys / values, packed; 16-byte aligned, capacity
 *                            entries->key_bytes / entries->val_bytes
 *   d_out_kpos, d_out_vpos : capacity n_entries + 1 u64, valid up to index n_out: with the two
 *                            byte columns a tpz_entries for tpz_plan_blocks_async
 *   d_src_entry            : NULL, or capacity n_entries u32: d_src_entry[o] = the input entry
 *                            output entry o is
 *   d_info                 : 4 u64 of device memory: [0] = n_out, [1] = output key bytes,
 *                            [2] = output value bytes, [3] = the first input entry with an empty
 *                            key or UINT64_MAX (SsTableIterator::is_valid is false there and
 *                            BlockBuilder::add asserts, builder.rs:27); when one is reported, the
 *                            other outputs are unspecified (and stay within their capacities)
 * Asynchronous on `stream`; uses the stream's grow-only workspace (about 40 bytes per entry).
 * n_runs == 0 or n_entries == 0 gives n_out = 0. TPZ_ERR_INVALID_ARG for n_runs >
 * TPZ_MERGE_MAX_RUNS, an h_run_first that breaks the rules above, or a misaligned output. Runs
 * that are not sorted are a precondition violation: the outputs are then unspecified, but every
 * loop is bounded, every index clamped, and nothing is written outside the stated capacities. */
#define TPZ_MERGE_MAX_RUNS 256u
tpz_err tpz_merge_runs(tpz_ctx* ctx, const tpz_entries* entries, const uint32_t* h_run_first,
                       uint32_t n_runs, uint8_t* d_out_keys, uint64_t* d_out_kpos,
                       uint8_t* d_out_vals, uint64_t* d_out_vpos, uint32_t* d_src_entry,
                       uint64_t* d_info, void* stream);

/* Flat columns -> the write side's entry positions: for the batch tpz_decode_blocks_flat decoded
 * into `cols`, d_kpos[e] / d_vpos[e] (e <= n = d_first[n_blocks]; n + 1 u64 each) = the absolute
 * start of entry e's key in cols->d_keys / value in cols->d_values, so that {d_keys, d_kpos,
 * d_values, d_vpos, n} is a tpz_entries in SsTableIterator order. Block i, entry j < count[i]
 * (e = d_first[i] + j): kpos = d_first[st + i] + (j ? ends[2(e-1)] : 0), vpos likewise;
 * kpos[n] / vpos[n] = the column totals. A TPZ_BLOCK_BAD_ENTRY block reads as decoded (an
 * unreadable key or value is empty). A block that decoded nothing (count[i] == 0 with its header's
 * n slots reserved) gives its first slot the block's reserved byte range and leaves the others
 * empty. d_info[0] (one u32) = the first block whose status is not TPZ_BLOCK_OK, or 0xFFFFFFFF:
 * sub_compact's `?` fails the compaction at such a block (and the reference panics at a
 * BAD_ENTRY block's bad entry), so the caller checks it. Asynchronous on `stream`. */
tpz_err tpz_flat_entry_pos(tpz_ctx* ctx, const tpz_flat_columns* cols, uint32_t n_blocks,
                           uint64_t* d_kpos, uint64_t* d_vpos, uint32_t* d_info, void* stream);

/* ---- batched LevelController::get over resident tables -----------------------------------
 * LevelController::get(key) (src/level.rs:427-465) for a batch of keys, over tables that stay in
 * HBM after they were opened (their decoded columns, block first keys and bloom filters):
 *   1. L0 (:428-442): the tables of level 0 from the last one down (l0_push_sstable appends, so
 *      the last is the newest). For each: SsTable::may_contain(key) false -> the next table
 *      (src/table.rs:114-119: no filter means true); else SsTableIterator::create_and_seek_to_key,
 *      whose Err ends the get; a valid iterator at an equal key ends it too: an empty value is
 *      Ok(None) (a tombstone), any other Ok(Some(value)); otherwise the next table.
 *   2. levels 1.. (:444-463): an empty level is skipped; in any other only tables[idx] is tried,
 *      idx = partition_point(smallest_key <= key).saturating_sub(1) over the level's tables in
 *      their stored order, with the same three steps. smallest_key is block_metas[0].first_key
 *      (src/table.rs:143-151): the first entry of tpz_table.d_first_keys.
 *   3. nothing found: Ok(None).
 * The probe is tpz_bloom_may_contain's and the seek is tpz_seek_keys', with their panic classes.
 *
 * d_tables: n_tables descriptors in DEVICE memory (their pointers are device pointers). Level l
 * is tables [h_level_first[l], h_level_first[l+1]); h_level_first: n_levels + 1 non-decreasing
 * u32 in HOST memory, h_level_first[0] = 0, h_level_first[n_levels] = n_tables (read during the
 * call: it travels in the kernel's arguments). Level 0 is stored in push order (oldest first);
 * the levels below are stored sorted by smallest key, which is a precondition: with an unsorted
 * level the results are unspecified, but every loop is bounded and every index clamped.
 * Keys are packed as for tpz_seek_keys; an empty key is legal and takes the same walk.
 *
 * tpz_get_keys, per query i:
 *   d_result[i]  TPZ_GET_ABSENT / FOUND / DELETED / ERROR
 *   d_status[i]  TPZ_BLOCK_OK unless the result is ERROR; then the status tpz_seek_keys reports
 *                for the seek that failed, or TPZ_BLOCK_MALFORMED where tpz_bloom_may_contain
 *                reports 2 or the selected table has no blocks
 *   d_table[i], d_block[i], d_entry[i]
 *                where the walk ended: the hit, the tombstone, or the failing table and the block
 *                and entry its seek reports; 0xFFFFFFFF each for ABSENT; a bloom panic gives
 *                d_block = d_entry = 0xFFFFFFFF
 *   d_val_pos    n_keys + 1 u64: the exclusive prefix sums of the value lengths (0 unless FOUND);
 *                d_val_pos[n_keys] is the total, which the caller reads back to size d_vals
 * tpz_get_values copies the value of every FOUND query i to d_vals[d_val_pos[i] ..
 * d_val_pos[i+1]) (packed back to back, d_vals 16-byte aligned), from tpz_get_keys' outputs over
 * the same d_tables; nothing is written at or past val_cap.
 * Both are asynchronous on `stream`; tpz_get_keys uses the stream's grow-only workspace (the
 * scan's partial sums). TPZ_ERR_INVALID_ARG, before any device work, for n_levels >
 * TPZ_GET_MAX_LEVELS, an h_level_first that breaks the rules above, or null or misaligned
 * pointers. n_keys == 0 and n_tables == 0 are valid: with no tables every query is ABSENT. */
#define TPZ_GET_MAX_LEVELS 16u /* the reference's MAX_LEVEL is 6 (src/level.rs:34) */
#define TPZ_GET_ABSENT 0       /* Ok(None): no table holds the key */
#define TPZ_GET_FOUND 1        /* Ok(Some(value)) */
#define TPZ_GET_DELETED 2      /* Ok(None): the first table holding it has an empty value */
#define TPZ_GET_ERROR 3        /* the reference's Err / panic; d_status says which */
/* (declared with a tag: tests/test_rust_binding.py's parser takes every anonymous struct
 * typedef for one of the six structs it knows by name) */
struct tpz_get_table {
  tpz_table table;         /* as for tpz_seek_keys */
  const uint8_t* d_filter; /* Bloom::encode, or NULL: no filter, may_contain is true */
  uint64_t filter_len;
};
typedef struct tpz_get_table tpz_get_table;

tpz_err tpz_get_keys(tpz_ctx* ctx, const tpz_get_table* d_tables, uint32_t n_tables,
                     const uint32_t* h_level_first, uint32_t n_levels, const uint8_t* d_keys,
                     const uint64_t* d_key_pos, uint32_t n_keys, uint8_t* d_result,
                     uint8_t* d_status, uint32_t* d_table, uint32_t* d_block, uint32_t* d_entry,
                     uint64_t* d_val_pos, void* stream);
tpz_err tpz_get_values(tpz_ctx* ctx, const tpz_get_table* d_tables, uint32_t n_tables,
                       uint32_t n_keys, const uint8_t* d_result, const uint32_t* d_table,
                       const uint32_t* d_block, const uint32_t* d_entry, const uint64_t* d_val_pos,
                       uint8_t* d_vals, uint64_t val_cap, void* stream);

/* ---- batched LsmStorage::scan over resident tables ---------------------------------------
 * The SST half of LsmStorage::scan(lower, upper) (src/lsm_storage.rs:335-374) for a batch of
 * ranges, over the tables tpz_get_keys walks. Additive within ABI 8: new symbols and constants
 * only (TPZ_HAS_SCAN tells a consumer the header has them). Per scan, with no memtables:
 *   1. LevelController::level_tables_sorted (src/level.rs:538-579): L0 reversed (newest first),
 *      then every level in stored order; that is the cursors' priority order. A table is dropped
 *      iff biggest_key < the lower key (Included and Excluded alike) or smallest_key > the upper
 *      key; Unbounded drops nothing. smallest_key is block_metas[0].first_key, biggest_key the
 *      last entry's key of the last block (src/table.rs:143-151); both are resident already.
 *   2. One SsTableIterator per surviving table: create_and_seek_to_key for Included,
 *      create_and_seek_to_first for Unbounded; Excluded seeks and takes one next() when the
 *      cursor is valid at an equal key. next() (src/table/iterator.rs:88-95) steps into the next
 *      block when the block iterator ends, and that block's read can be an Err. A cursor is valid
 *      iff its current key is non-empty.
 *   3. MergeIterator (src/iterators/merge_iterator.rs:41-106) drops invalid cursors, yields the
 *      smallest (key, priority), and on next advances every other cursor at an equal key first,
 *      in increasing priority, until its key differs, then the current cursor once. An Err from
 *      any of these steps ends the scan.
 *   4. TwoMergeIterator with an always-invalid memtable side passes that sequence e0, e1, ..
 *      through; the host merges its memtables over the device's output, or hands them over as
 *      runs (tpz_lsm_scan_ranges, below: the real TwoMergeIterator).
 *   5. LsmIterator (src/lsm_iterator.rs): entries with an empty value are skipped; every element
 *      AFTER e0, tombstones included, is tested against the end bound (Included stops at the
 *      first key > upper, Excluded at the first key >= upper) and the first failure ends the scan.
 *      e0 is never end-checked (LsmIterator::new, :22-33): over one table {a, d},
 *      scan(Included(b), Included(c)) yields d. The device reproduces this.
 *
 * d_tables, h_level_first, n_levels: exactly tpz_get_keys', with its preconditions and its
 * "unspecified, but bounded and clamped" clause for an unsorted level (and likewise for a table
 * whose keys decrease). Bound keys are packed as for tpz_seek_keys (an Unbounded bound has an
 * empty key); d_lo_kind / d_hi_kind hold one TPZ_BOUND_* byte per scan. `limit` >= 1 is the most
 * entries a scan yields in this call, uniform per call; n_scans * limit < 2^32.
 *
 * tpz_scan_ranges, per scan i:
 *   d_result[i]  TPZ_SCAN_DONE / MORE / ERROR
 *   d_status[i]  TPZ_BLOCK_OK unless the result is ERROR
 *   d_where[3i .. 3i+3)
 *                the table (an index into d_tables), block and entry of the failure, as
 *                tpz_get_keys reports them; 0xFFFFFFFF each unless the result is ERROR. A failure
 *                while the cursors are created reports the first failing table in priority
 *                order; one during a next, the first failing cursor in the order of step 3.
 *   d_hit_table / d_hit_block / d_hit_entry [i * limit + j]
 *                the j-th yielded entry (columns of n_scans * limit u32; the slots past a scan's
 *                count are not written)
 *   d_first, d_key_first, d_val_first
 *                n_scans + 1 u64 each: the exclusive prefix sums of the scans' yielded entry
 *                counts, key bytes and value bytes; on ERROR the count is the number of entries
 *                yielded before the failing step
 *   d_info       3 u64: the three totals, which the caller reads back once to size the gather
 * A table the reference could not have opened (SsTable::open fails on it: no blocks, or a last
 * block that cannot be read or whose first or last entry cannot) makes every scan an ERROR at
 * that table, found by the filter and so before any seek: status MALFORMED, or the last block's
 * status when its read is an Err; d_where block = the last block (0xFFFFFFFF without blocks),
 * entry = 0xFFFFFFFF.
 * Paging: TPZ_BOUND_AFTER as the lower kind means Excluded with the first merged element
 * end-checked like every later one: it continues a scan that reported MORE from its last yielded
 * key, and with every block readable the pages concatenate to the unpaged scan. It is not valid
 * as an upper kind. Kinds live in device memory: an out-of-range kind gives that scan ERROR with
 * TPZ_BLOCK_MALFORMED and d_where all 0xFFFFFFFF.
 *
 * tpz_scan_entries writes the yielded entries as a tpz_entries: d_kpos and d_vpos
 * (d_first[n_scans] + 1 u64 each) and the packed key and value bytes (d_keys, d_vals 16-byte
 * aligned); scan i owns entries [d_first[i], d_first[i+1]) in iterator order. Nothing is written
 * at or past key_cap / val_cap; table, block and entry are checked against the descriptors.
 *
 * Both are asynchronous on `stream` and use the stream's grow-only workspace (tpz_scan_ranges:
 * the cursors, 8 B per scan and table, plus a status byte each and the scans' partial sums).
 * TPZ_ERR_INVALID_ARG, before any device work, for n_tables > TPZ_SCAN_MAX_TABLES (one wave
 * merges a scan, a cursor per lane; lifting the limit is a later change), the h_level_first rules
 * of tpz_get_keys, limit == 0, n_scans * limit >= 2^32, or null or misaligned pointers (u64
 * columns 8-byte, u32 columns 4-byte, d_keys and d_vals 16-byte). n_scans == 0 and n_tables == 0
 * are valid: with no tables every scan is DONE with nothing yielded. */
#define TPZ_HAS_SCAN 1
#define TPZ_SCAN_MAX_TABLES 64u
#define TPZ_BOUND_UNBOUNDED 0
#define TPZ_BOUND_INCLUDED 1
#define TPZ_BOUND_EXCLUDED 2
#define TPZ_BOUND_AFTER 3 /* lower only: see paging */
#define TPZ_SCAN_DONE 0   /* the iterator became invalid within `limit` entries */
#define TPZ_SCAN_MORE 1   /* `limit` entries yielded and the iterator is still valid */
#define TPZ_SCAN_ERROR 2  /* the reference's Err / panic; d_status says which */

tpz_err tpz_scan_ranges(tpz_ctx* ctx, const tpz_get_table* d_tables, uint32_t n_tables,
                        const uint32_t* h_level_first, uint32_t n_levels,
                        const uint8_t* d_lo_keys, const uint64_t* d_lo_pos,
                        const uint8_t* d_lo_kind, const uint8_t* d_hi_keys,
                        const uint64_t* d_hi_pos, const uint8_t* d_hi_kind, uint32_t n_scans,
                        uint32_t limit, uint8_t* d_result, uint8_t* d_status, uint32_t* d_where,
                        uint32_t* d_hit_table, uint32_t* d_hit_block, uint32_t* d_hit_entry,
                        uint64_t* d_first, uint64_t* d_key_first, uint64_t* d_val_first,
                        uint64_t* d_info, void* stream);
tpz_err tpz_scan_entries(tpz_ctx* ctx, const tpz_get_table* d_tables, uint32_t n_tables,
                         uint32_t n_scans, uint32_t limit, const uint32_t* d_hit_table,
                         const uint32_t* d_hit_block, const uint32_t* d_hit_entry,
                         const uint64_t* d_first, uint8_t* d_keys, uint64_t key_cap,
                         uint64_t* d_kpos, uint8_t* d_vals, uint64_t val_cap, uint64_t* d_vpos,
                         void* stream);

/* ---- memtable runs: LsmStorage::get and LsmStorage::scan over runs plus tables -------------
 * What a user of the store calls: LsmStorage::get (src/lsm_storage.rs:198-213) looks in the
 * memtables first, newest first, and only then in the tables (LevelController::get, above);
 * LsmStorage::scan (:335-374) merges the memtables in with TwoMergeIterator. Additive within
 * ABI 8: new symbols and constants only (TPZ_HAS_MEM tells a consumer the header has them).
 *
 * A run is one memtable's SkipMap (src/mem_table.rs) as a tpz_entries in DEVICE memory: its keys
 * strictly increasing (a map; Rust's [u8] Ord), a tombstone an entry with an empty value.
 * d_prefix is NULL or n_entries u64: entry j's key's first 8 bytes, big-endian, zero padded, which
 * tpz_mem_prefix builds (asynchronous on `stream`; n_entries == 0 does nothing). It is the index
 * of a lookup: a bisection step over it is one 8-byte load, and key bytes are read only among
 * entries whose prefix ties with the probe's. A tie decides nothing (`a` and `a\0` share a
 * prefix, long keys share 8-byte prefixes): the full comparison follows. With d_prefix NULL the
 * same bisection reads the keys; both forms give identical answers.
 * d_runs: n_runs descriptors in DEVICE memory, in MemTables::view() order (src/mem_table.rs:74-81):
 * the immutable memtables oldest first, the mutable one last. Priority is the reverse.
 * Unsorted or repeated keys in a run, or a d_prefix that is not the keys' prefix column, are a
 * precondition violation: the results are then unspecified, but every loop is bounded, every
 * index clamped, and nothing is written outside the stated capacities.
 *
 * tpz_lsm_get_keys: tpz_get_keys' arguments with d_runs, n_runs in front, and its output
 * columns. Per query:
 *   - an empty key: LsmStorage::get asserts (:199). TPZ_GET_ERROR with TPZ_BLOCK_MALFORMED and
 *     d_table = d_block = d_entry = 0xFFFFFFFF (tpz_get_keys keeps accepting empty keys);
 *   - the runs from n_runs - 1 down to 0 with an exact match (MemTable::get, src/mem_table.rs:
 *     150-152). The first run holding the key ends the get (:202-209): an empty value is
 *     TPZ_GET_DELETED, any other TPZ_GET_FOUND, with d_table = TPZ_HIT_MEM | run, d_block = 0,
 *     d_entry = the index in the run, and the value length in d_val_pos as for a table hit;
 *   - no run holds it: tpz_get_keys' walk, unchanged (:211).
 * tpz_lsm_get_values is tpz_get_values over both sources in one pass: run and entry are checked
 * against the run descriptors as table, block and entry are against the tables', and nothing is
 * written at or past val_cap.
 * With n_runs == 0 both give tpz_get_keys' / tpz_get_values' outputs byte for byte for non-empty
 * keys. TPZ_ERR_INVALID_ARG, before any device work, for n_runs > TPZ_MEM_MAX_RUNS, a null or
 * misaligned d_runs with n_runs > 0, and everything tpz_get_keys / tpz_get_values reject.
 *
 * tpz_lsm_scan_ranges / tpz_lsm_scan_entries: tpz_scan_ranges' / tpz_scan_entries' arguments with
 * d_runs, n_runs in front, and their outputs: LsmStorage::scan whole. Step 4 of the scan section
 * above becomes the real TwoMergeIterator (src/iterators/two_merge_iterator.rs), A = the
 * MergeIterator over one cursor per memtable, newest first (lsm_storage.rs:340-346), B = the SST
 * MergeIterator of steps 1-3. One wave still merges a scan, a cursor per lane: the runs newest
 * first, then the tables in level_tables_sorted order; n_runs + n_tables > TPZ_SCAN_MAX_TABLES is
 * TPZ_ERR_INVALID_ARG.
 *   - A run's cursor is map.range((lower, upper)) (src/mem_table.rs:199-219): unlike an SST
 *     cursor it is bounded on both sides. It covers the run's entries [lb, ub): lb = 0 for
 *     Unbounded, the number of keys < lower for Included, of keys <= lower for Excluded and
 *     After; ub = n_entries for Unbounded, the number of keys <= upper for Included, of keys
 *     < upper for Excluded. With lower > upper, or equal keys and an Excluded side, the cursor is
 *     empty. (BTreeMap::range panics on such bounds; this header takes crossbeam-skiplist's range
 *     to yield nothing there, which is a decision: its source was not at hand.) Run cursors
 *     never fail.
 *   - The cursor is valid iff lb < ub and the key at lb is non-empty (MemTableIterator::is_valid,
 *     :263-265). batch_put and the channel writers do not assert on keys, so a run can hold the
 *     empty key as its first entry; a cursor that starts on it is invalid, MergeIterator::create
 *     drops it, and that memtable contributes nothing to the scan. The device reproduces this.
 *   - The yielded sequence is what one flat merge over all lanes in that priority order yields:
 *     TwoMergeIterator prefers A on a tie and skips B's equal keys. Where the work happens
 *     differs, and errors show it: create() and every next() step B past every key equal to A's
 *     current key BEFORE that key is yielded (two_merge_iterator.rs:20-24, :64-68), with B's own
 *     "others first" order. An Err from a block read during that skip therefore ends the scan one
 *     element earlier than a flat merge would report it; if the skip happens in create(), or in
 *     LsmIterator::new's tombstone skip, scan() itself returns the Err and the count is 0.
 *     d_first on ERROR stays "entries the reference's iterator yielded before the failing step",
 *     and d_where is the failing SST cursor in MergeIterator::next's order.
 *   - LsmIterator is unchanged (step 5): e0 is never end-checked unless the lower kind is After;
 *     because run cursors are bounded above, that quirk can only fire from an SST lane.
 *     TPZ_BOUND_AFTER applies Excluded to run cursors too. TPZ_SCAN_MORE keeps its meaning (an
 *     Err in the step after the last yielded entry is ERROR with count `limit`), and pages
 *     concatenate to the unpaged scan when every block is readable and the runs are the same
 *     snapshot.
 * A yielded run entry reports d_hit_table = TPZ_HIT_MEM | run, d_hit_block = 0, d_hit_entry = its
 * index; tpz_lsm_scan_entries gathers from both kinds with tpz_scan_entries' checks (run and
 * entry against the run descriptors). With n_runs == 0 both reproduce tpz_scan_ranges /
 * tpz_scan_entries byte for byte. The workspace holds a cursor per scan and run too. */
#define TPZ_HAS_MEM 1
#define TPZ_MEM_MAX_RUNS 16u    /* the reference's default max_memtable_num is 5 (src/opt.rs:41) */
#define TPZ_HIT_MEM 0x80000000u /* d_table = TPZ_HIT_MEM | run for a hit in a memtable run */
/* (declared with a tag, as tpz_get_table is) */
struct tpz_mem_run {
  tpz_entries entries;
  const uint64_t* d_prefix; /* n_entries u64, or NULL */
};
typedef struct tpz_mem_run tpz_mem_run;

tpz_err tpz_mem_prefix(tpz_ctx* ctx, const tpz_entries* entries, uint64_t* d_prefix, void* stream);
tpz_err tpz_lsm_get_keys(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                         const tpz_get_table* d_tables, uint32_t n_tables,
                         const uint32_t* h_level_first, uint32_t n_levels, const uint8_t* d_keys,
                         const uint64_t* d_key_pos, uint32_t n_keys, uint8_t* d_result,
                         uint8_t* d_status, uint32_t* d_table, uint32_t* d_block,
                         uint32_t* d_entry, uint64_t* d_val_pos, void* stream);
tpz_err tpz_lsm_get_values(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                           const tpz_get_table* d_tables, uint32_t n_tables, uint32_t n_keys,
                           const uint8_t* d_result, const uint32_t* d_table,
                           const uint32_t* d_block, const uint32_t* d_entry,
                           const uint64_t* d_val_pos, uint8_t* d_vals, uint64_t val_cap,
                           void* stream);
tpz_err tpz_lsm_scan_ranges(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                            const tpz_get_table* d_tables, uint32_t n_tables,
                            const uint32_t* h_level_first, uint32_t n_levels,
                            const uint8_t* d_lo_keys, const uint64_t* d_lo_pos,
                            const uint8_t* d_lo_kind, const uint8_t* d_hi_keys,
                            const uint64_t* d_hi_pos, const uint8_t* d_hi_kind, uint32_t n_scans,
                            uint32_t limit, uint8_t* d_result, uint8_t* d_status,
                            uint32_t* d_where, uint32_t* d_hit_table, uint32_t* d_hit_block,
                            uint32_t* d_hit_entry, uint64_t* d_first, uint64_t* d_key_first,
                            uint64_t* d_val_first, uint64_t* d_info, void* stream);
tpz_err tpz_lsm_scan_entries(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                             const tpz_get_table* d_tables, uint32_t n_tables, uint32_t n_scans,
                             uint32_t limit, const uint32_t* d_hit_table,
                             const uint32_t* d_hit_block, const uint32_t* d_hit_entry,
                             const uint64_t* d_first, uint8_t* d_keys, uint64_t key_cap,
                             uint64_t* d_kpos, uint8_t* d_vals, uint64_t val_cap, uint64_t* d_vpos,
                             void* stream);

/* ---- scanning levels of any width: one merge cursor per level below L0 ----------------------
 * tpz_lsm_scan_ranges gives every table a lane of the one wave that merges a scan, hence its 64.
 * Under the reference's defaults (src/opt.rs:31-54, TABLE_CAPACITY in src/table/builder.rs:27) L1
 * alone holds about 40 tables and L2 about 400. tpz_level_scan_ranges / tpz_level_scan_entries
 * take tpz_lsm_scan_ranges' / tpz_lsm_scan_entries' arguments (n_runs may be 0) and give their
 * outputs, with any number of tables inside a level below L0. Additive within ABI 8: new symbols
 * and constants only (TPZ_HAS_LEVEL_SCAN tells a consumer the header has them).
 *
 * Precondition (tpz_get_keys' words): the levels below L0 are stored sorted by smallest key and
 * are disjoint, and keys increase inside a table. The reference still builds one SsTableIterator
 * per table that passes the filter (level_tables_sorted, src/level.rs:538-579; lsm_storage.rs:
 * 350-365), but over such a level those iterators, merged, yield exactly the concatenation of the
 * surviving tables, so one cursor per level yields the same sequence. A scan's cursors, in
 * priority order: the runs, newest first; the L0 tables, newest first; one per non-empty level
 * 1.., in level order. Run and L0 cursors are tpz_lsm_scan_ranges'. A level cursor over the
 * tables T[0..m) of its level stands for the reference's per-table cursors:
 *   - Survivors. a = the first table with biggest_key >= lower (0 for Unbounded), z = the last
 *     with smallest_key <= upper (m - 1 for Unbounded); T[a..z] survive, and with a > z or no
 *     such table the level contributes nothing. That is level_tables_sorted's filter
 *     (level.rs:554-568) over a sorted, disjoint level. Both are found by bisection on the
 *     smallest keys (LevelController::get's partition_point, level.rs:449-451) and one look at a
 *     biggest key.
 *   - Creation. T[a] takes the real seek: create_and_seek_to_key and the Excluded / After step
 *     (lsm_storage.rs:356-362), or create_and_seek_to_first for Unbounded. Every T[j], a < j <= z,
 *     has smallest_key > biggest_key(T[a]) >= lower, so its create_and_seek_to_key finds block 0
 *     and bisects there below every key (table/iterator.rs:44-72): the outcome does not depend on
 *     the scan. It is the table's head record, computed once per call: valid at a (block, entry),
 *     invalid (MergeIterator::create drops the cursor, merge_iterator.rs:47-57), or failing with
 *     the status, block and entry tpz_seek_keys reports for a key below all of the table's keys.
 *     With an Unbounded lower bound the head is create_and_seek_to_first's (table/iterator.rs:
 *     39-42: block 0, entry 0 and no bisection), kept beside the other.
 *   - Errors at creation. The reference creates every cursor before it merges, so a failing head
 *     anywhere in T[a+1..z] makes the scan TPZ_SCAN_ERROR with nothing yielded, however small
 *     `limit` is; a failing head outside it does nothing. Among several failures the first in the
 *     reference's per-table cursor order is reported: runs, L0 newest first, the levels, within a
 *     level the stored order, T[a]'s own seek before any head. A table the reference could not
 *     have opened keeps tpz_scan_ranges' rule: every scan is an ERROR at the first such table in
 *     priority order, found before any seek, wherever the scan's range lies.
 *   - Stepping. When the cursor's table ends (SsTableIterator::next, table/iterator.rs:88-95,
 *     leaves the last block invalid), the cursor moves to the next table of (current, z] whose
 *     head is valid and stands at that head; tables with an invalid head are passed over. It never
 *     enters T[z + 1]: the reference dropped that table, and entering it could yield an element
 *     through the unchecked-e0 rule (L1 = {a, d}, {f, g}: scan(Excluded(d), Included(e)) yields
 *     nothing). A T[a] whose own seek is invalid (Excluded at its biggest key) starts at the next
 *     valid head of (a, z]. The merge is otherwise tpz_lsm_scan_ranges': the tie rule,
 *     TwoMergeIterator's eager skip (which can carry a level cursor into its next table), the e0
 *     quirk, TPZ_BOUND_AFTER paging and MergeIterator::next's failure order.
 *   - Reporting. d_hit_table and d_where name indices into d_tables, never lanes. Over sorted,
 *     disjoint levels every output equals tpz_lsm_scan_ranges' byte for byte wherever that call
 *     accepts the set.
 * With the precondition broken the results are unspecified, but every loop is bounded, every
 * index clamped, and nothing is written outside the stated capacities. (tpz_scan_ranges and
 * tpz_lsm_scan_ranges keep merging overlapping lower levels table by table.)
 *
 * TPZ_ERR_INVALID_ARG, before any device work: n_runs + L0 tables + non-empty levels below L0 >
 * TPZ_LEVEL_SCAN_MAX_CURSORS, counted from h_level_first; and everything tpz_lsm_scan_ranges /
 * tpz_lsm_scan_entries reject apart from their table count. Both calls are asynchronous on
 * `stream` and use the stream's grow-only workspace; h_level_first is read during the call.
 * tpz_level_scan_ranges' workspace: per table a 40-byte index record and four u32 links (built on
 * the device at the start of every call: one thread per table, then one wave per level), then 16
 * bytes and a status byte per scan and cursor, and the scans' partial sums. A scan reads
 * O(log tables) smallest keys, one biggest key and two links per level when it is created.
 * tpz_level_scan_entries is tpz_lsm_scan_entries without the table cap (the gather checks table,
 * block and entry against the descriptors). */
#define TPZ_HAS_LEVEL_SCAN 1
#define TPZ_LEVEL_SCAN_MAX_CURSORS 64u

tpz_err tpz_level_scan_ranges(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                              const tpz_get_table* d_tables, uint32_t n_tables,
                              const uint32_t* h_level_first, uint32_t n_levels,
                              const uint8_t* d_lo_keys, const uint64_t* d_lo_pos,
                              const uint8_t* d_lo_kind, const uint8_t* d_hi_keys,
                              const uint64_t* d_hi_pos, const uint8_t* d_hi_kind, uint32_t n_scans,
                              uint32_t limit, uint8_t* d_result, uint8_t* d_status,
                              uint32_t* d_where, uint32_t* d_hit_table, uint32_t* d_hit_block,
                              uint32_t* d_hit_entry, uint64_t* d_first, uint64_t* d_key_first,
                              uint64_t* d_val_first, uint64_t* d_info, void* stream);
tpz_err tpz_level_scan_entries(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                               const tpz_get_table* d_tables, uint32_t n_tables, uint32_t n_scans,
                               uint32_t limit, const uint32_t* d_hit_table,
                               const uint32_t* d_hit_block, const uint32_t* d_hit_entry,
                               const uint64_t* d_first, uint8_t* d_keys, uint64_t key_cap,
                               uint64_t* d_kpos, uint8_t* d_vals, uint64_t val_cap,
                               uint64_t* d_vpos, void* stream);

/* ---- building a memtable run: write batches and WAL images ----------------------------------
 * The stage in front of the runs above: entries in ARRIVAL order (a write batch, or the records
 * of a WAL image) become a run (keys strictly increasing, one entry per distinct key) with the
 * reference's replacement rules and its MemTable::size(), ready for tpz_mem_run. Additive within
 * ABI 8: new symbols and constants only (TPZ_HAS_MEM_BUILD tells a consumer the header has them).
 *
 * tpz_mem_build. `entries` is a tpz_entries whose keys are in arrival order, not sorted. Two rules
 * (src/mem_table.rs), chosen by `mode`:
 *   TPZ_MEM_REPLAY  MemTable::open (:119-143) over WalIterator (src/wal/iterator.rs). Records are
 *     read while is_valid() (:125; iterator.rs:30-32: the key is non-empty): the FIRST entry with
 *     an empty key ends the replay and it and every entry after it are ignored. map.insert (:129)
 *     replaces: the LAST entry of a key wins. size (:128) = the sum of klen + vlen over every
 *     entry read, replaced ones included. d_version is ignored.
 *   TPZ_MEM_PUT     MemTable::put / put_entries -> do_mem_put (:155-196). d_version: n u64 in
 *     device memory, entry i's WAL append version (all entries of one put_entries batch share
 *     one, :162-165), non-decreasing in arrival order (a precondition; it suffices that the
 *     entries of each key have non-decreasing versions, which is what lets a built run's own
 *     d_out_version column stand in front of a later batch). compare_insert(.., |x|
 *     x.version < version) (:179-181) replaces only on a strictly greater version: the winner of
 *     a key is the FIRST entry, in arrival order, among those with the key's highest version
 *     (inside one batch the first duplicate wins, where replaying that batch's WAL lets the last
 *     win: the reference's behaviour, kept). An empty key is an ordinary key (MemTable does not
 *     check it). size: compare_insert returns the entry the map holds afterwards, and the update
 *     (:185-195) runs when that entry's version equals this entry's: for the entry that inserted
 *     or replaced, and also for a later entry of the same key and version, which was turned away.
 *     With h = the entry the map held before entry e arrived (the first entry of e's version if
 *     that is not e itself, else the first entry of the key's previous version):
 *       no h:                  size += klen + vlen
 *       vlen >= vlen_h (:189): size += vlen - vlen_h
 *       otherwise (:193):      size -= old_size - klen + vlen, which is vlen_h + vlen (the
 *                              reference's operator precedence, kept)
 *     The sum wraps as usize does.
 * Outputs: d_out_keys / d_out_vals (16-byte aligned, capacities entries->key_bytes / val_bytes),
 * d_out_kpos / d_out_vpos (n + 1 u64 each; [n_out] = the byte totals): the winners in Rust's [u8]
 * order (bytewise, unsigned, a proper prefix first) with their values; empty values (tombstones)
 * are kept. Optional, NULL to skip: d_out_prefix (n u64: tpz_mem_prefix of the output keys, so the
 * result is a tpz_mem_run without a second call), d_src_entry (n u32: the input entry each output
 * entry is), d_out_version (n u64: the winners' versions, 0 under REPLAY as open() stores, :133;
 * a later batch is applied by building over {this run's entries and versions, then the batch};
 * size is then the sum of the calls' sizes minus the first output's klen + vlen total, which the
 * second call counts again as inserts).
 * d_info, 8 u64: [0] n_out, [1] output key bytes, [2] output value bytes, [3] the first input
 * entry with an empty key or UINT64_MAX, [4] size, [5] entries consumed (REPLAY: [3] if there is
 * an empty key, else n; PUT: n), [6], [7] zero.
 * Asynchronous on `stream`; uses the stream's grow-only workspace: 40 bytes per entry (the prefix,
 * two id lists, three scan words) plus under 1 % for partial sums and tile partitions.
 * n_entries == 0 gives all-zero counts ([3] = UINT64_MAX). TPZ_ERR_INVALID_ARG, before any device
 * work, for null or misaligned pointers, an unknown mode, PUT without d_version, or n_entries ==
 * 0xFFFFFFFF. Versions that decrease or positions that are not monotone leave the outputs
 * unspecified but in bounds: every loop is bounded, every id and span clamped, and nothing is
 * written past the stated capacities.
 *
 * tpz_wal_index (host code, no GPU): WalIterator's chain over a WAL image in host memory, a record
 * being BE u16 klen | key | BE u16 vlen | value (Entry::encode, src/block/builder.rs:72-81;
 * iterator.rs:34-45). Writes the record starts h_rec[0 .. n] (h_rec[n] = the end of the last
 * record read; rec_cap = the u64 h_rec holds, TPZ_ERR_NOMEM if n + 1 exceed it); with h_rec NULL
 * it only counts. It stops after the first empty-key record, as MemTable::open does; that record
 * is parsed (its value too: next() reads it) and counted. h_info, 4 u64: [0] n, [1] how the walk
 * ended (TPZ_WAL_END_IMAGE, TPZ_WAL_END_EMPTY_KEY, TPZ_WAL_TRUNCATED), [2] the end of the last
 * record read, [3] UINT64_MAX, or for TPZ_WAL_TRUNCATED the byte offset of the record at which the
 * reference panics (get_u16 on fewer than 2 bytes, iterator.rs:39 / :42; a slice past the end,
 * :40 / :43); the call then returns TPZ_ERR_SIZES, with [0] the records before it. Never reads
 * outside the image. The chain is serial and has no checksum, so it stays on the host, where the
 * file arrives anyway.
 *
 * tpz_wal_entries (device): d_image (image_bytes in HBM) and d_rec (n_records + 1 record starts,
 * tpz_wal_index's) become packed key and value columns with d_kpos / d_vpos (n_records + 1 u64
 * each): a tpz_entries in arrival order for tpz_mem_build(TPZ_MEM_REPLAY). One thread per record
 * re-reads klen and vlen and checks rec[i] + 4 + klen + vlen == rec[i + 1] inside the image; a
 * record that fails contributes empty spans. d_info, 4 u64: [0] n_records, [1] key bytes, [2]
 * value bytes, [3] the first record that fails or UINT64_MAX. d_keys / d_vals: 16-byte aligned,
 * image_bytes of capacity each suffice and nothing is written past them. Asynchronous on
 * `stream`. TPZ_ERR_INVALID_ARG for null or misaligned pointers or n_records == 0xFFFFFFFF. */
#define TPZ_HAS_MEM_BUILD 1
#define TPZ_MEM_REPLAY 0u
#define TPZ_MEM_PUT 1u
#define TPZ_WAL_END_IMAGE 0u
#define TPZ_WAL_END_EMPTY_KEY 1u
#define TPZ_WAL_TRUNCATED 2u

tpz_err tpz_mem_build(tpz_ctx* ctx, const tpz_entries* entries, uint32_t mode,
                      const uint64_t* d_version, uint8_t* d_out_keys, uint64_t* d_out_kpos,
                      uint8_t* d_out_vals, uint64_t* d_out_vpos, uint64_t* d_out_prefix,
                      uint32_t* d_src_entry, uint64_t* d_out_version, uint64_t* d_info,
                      void* stream);
tpz_err tpz_wal_index(const uint8_t* h_image, uint64_t image_bytes, uint64_t* h_rec,
                      uint64_t rec_cap, uint64_t* h_info);
tpz_err tpz_wal_entries(tpz_ctx* ctx, const uint8_t* d_image, uint64_t image_bytes,
                        const uint64_t* d_rec, uint32_t n_records, uint8_t* d_keys,
                        uint64_t* d_kpos, uint8_t* d_vals, uint64_t* d_vpos, uint64_t* d_info,
                        void* stream);

/* ---- a whole compaction task's output tables ----------------------------------------------
 * What do_compact (src/level.rs:133-222) does around the merge and the block loop: the key ranges
 * of its sub-compactions, SsTableBuilder's table cuts and the bytes of every output file. Additive
 * within ABI 8: new symbols and constants only (TPZ_HAS_TABLES tells a consumer the header has
 * them). The caller merges the task's input tables once (tpz_merge_runs) and then, per range and
 * per output table, plans a window of blocks, cuts it, encodes it at the table's image start and
 * finishes the images.
 *
 * tpz_entries_bound replaces sub_compact's seeks and its key_vaild test (src/level.rs:188-206:
 * SsTableIterator::create_and_seek_to_key(table, lower) on every input, `iter.key() <= key` for an
 * Included upper, `<` for an Excluded one), over the merged entries: d_out[i] = the number of
 * entries whose key is < probe i, or <= probe i where d_inclusive[i] != 0. A range's entries are
 * [bound(lower, 0), bound(upper, upper is Included)). Keys compare as Rust's [u8] Ord (bytewise,
 * unsigned, a proper prefix first). Probe keys are packed as for tpz_seek_keys. That equals seeking
 * every input and merging provided every input table's keys are strictly increasing
 * (BlockIterator::seek_to_key returns any equal position otherwise): a precondition. On entries
 * that are not sorted the counts are unspecified, but every loop is bounded and every index
 * clamped. TPZ_ERR_INVALID_ARG, before any device work, for null or misaligned pointers (u64
 * positions 8-byte, d_out 4-byte). n_probes == 0 is valid. Asynchronous on `stream`.
 *
 * tpz_table_cut replaces reach_capacity() in sub_compact's inner loop (src/level.rs:209,
 * src/table/builder.rs:27,88-94: data.len() + 2 * meta.len() >= capacity, tested before each add;
 * the size only changes when add() builds a block, builder.rs:54-57). `entries` are the merged
 * entries; the table starts at entry `start`, and [start, start + win_entries) is the window that
 * tpz_plan_blocks_async planned as its own tpz_entries (d_kpos + start, d_vpos + start,
 * n_entries = win_entries) into d_first / d_ext / d_plan_info; the window ends at or before
 * seg_end, the end of the sub-compaction's range. d_cut_ext holds the stored extents of the
 * window's blocks, the ones the capacity is tested against: d_ext itself for Uncompress,
 * tpz_compress_blocks' extents for Snappy / Lz4. With e_j = the first entry of block j, the cut is
 * the smallest k with d_cut_ext[k + 1] + 2 (k + 1) >= capacity and e_{k+1} inside the window (the
 * window's last block may be cut short by the window, so it never counts). The table then holds
 * blocks 0..k and one more block with e_{k+1} alone (the add that built block k put it into a
 * fresh block before the loop tested the size again), and the next table starts at e_{k+1} + 1.
 * The call patches d_first[k + 2], d_ext[k + 2] (the closed form of the plan: entry bytes + 2 per
 * entry + 7 per block) and d_plan_info[2] = k + 2, so that tpz_encode_blocks_async writes exactly
 * the table. Without a cut the plan is left alone: a window that ends at seg_end is then the whole
 * table, a shorter one has to be planned again over the window the call proposes.
 *   d_cut  8 u64: [0] TPZ_CUT_NONE / FOUND / BAD_ENTRY, [1] k (BAD_ENTRY: the rejected entry, an
 *          index into `entries`), [2] the table's blocks, [3] its entries, [4] its Uncompress
 *          data bytes (d_ext at its block count), [5] the sum of its blocks' first-key lengths,
 *          [6] where the next window starts (FOUND: the next table; else `start`), [7] where it
 *          ends: the first entry by which its raw bytes (4 + key + value per entry) reach
 *          capacity + block_size, which always holds the cut for Uncompress, or twice the bytes of
 *          the window that held no cut plus that; clamped to seg_end.
 * win_entries == 0 plans nothing (the plan pointers may be NULL): the call only proposes the
 * window of a table starting at `start`. One workgroup; asynchronous on `stream`.
 * TPZ_ERR_INVALID_ARG, before any device work, for null or misaligned pointers, capacity 0 (the
 * reference then builds a table of no entries and panics on it), a block size outside
 * tpz_plan_blocks' range, or start + win_entries > seg_end or seg_end > n_entries.
 *
 * tpz_sst_finish replaces SsTableBuilder::build (src/table/builder.rs:97-141) and
 * FileObject::create's checksum (src/table/file_object.rs:33-48) for n_images tables whose data
 * regions already sit at their image starts:
 *   data | metas (BE u32 offset, BE u16 key length, key; src/table.rs:33-46) | BE u32 meta offset
 *        | [Bloom::encode | BE u32 bloom offset] | BE u32 CRC-32 of everything before it
 * The bloom section is there iff the descriptor has a filter (the caller builds one iff
 * false_positive_rate.is_sign_positive(), builder.rs:111; the reference's own SsTable::open
 * misreads a file without one, src/table.rs:75-87). d_images: n_images descriptors in DEVICE
 * memory, in increasing address order, all inside [d_base, d_base + span_bytes): one allocation,
 * because the CRC runs over the span as one batch of ranges and reads (never writes) the bytes
 * between two images. max_blocks bounds every descriptor's n_blocks. A descriptor that breaks
 * these rules is skipped and reports size 0.
 *   d_info  4 u64 per image: {size (CRC trailer included), meta offset, bloom offset or
 *           UINT64_MAX, the CRC}
 * Asynchronous on `stream`; uses the stream's workspace (the key-length scan's partial sums, the
 * CRC's ranges and accumulators). TPZ_ERR_INVALID_ARG, before any device work, for null or
 * misaligned pointers (descriptors and d_info 8-byte) or span_bytes past 2^35. n_images == 0 is
 * valid. tpz_sst_image_bytes (host) is the size such an image has. */
#define TPZ_HAS_TABLES 1
#define TPZ_CUT_NONE 0      /* no cut inside the window */
#define TPZ_CUT_FOUND 1
#define TPZ_CUT_BAD_ENTRY 2 /* the window's plan rejected an entry (tpz_plan_blocks_async's d_info[1]) */
/* (declared with a tag, as tpz_get_table is) */
struct tpz_sst_image {
  uint8_t* d_image;        /* the image's first byte; its data region is there already */
  uint64_t data_bytes;     /* the data region's length: the meta offset */
  const uint32_t* d_first; /* n_blocks: each block's first entry, relative to entry_base */
  const uint64_t* d_ext;   /* n_blocks: each block's offset in the data region */
  uint32_t n_blocks;
  uint32_t entry_base;     /* the table's first entry in `entries` */
  const uint8_t* d_filter; /* Bloom::encode (tpz_bloom_build's 4-byte aligned output), or NULL */
  uint64_t filter_len;
};
typedef struct tpz_sst_image tpz_sst_image;

tpz_err tpz_entries_bound(tpz_ctx* ctx, const tpz_entries* entries, const uint8_t* d_keys,
                          const uint64_t* d_key_pos, const uint8_t* d_inclusive,
                          uint32_t n_probes, uint32_t* d_out, void* stream);
tpz_err tpz_table_cut(tpz_ctx* ctx, const tpz_entries* entries, uint32_t start,
                      uint32_t win_entries, uint32_t seg_end, uint32_t* d_first, uint64_t* d_ext,
                      const uint64_t* d_cut_ext, uint32_t* d_plan_info, uint32_t block_size,
                      uint64_t capacity, uint64_t* d_cut, void* stream);
uint64_t tpz_sst_image_bytes(uint64_t data_bytes, uint64_t n_blocks, uint64_t first_key_bytes,
                             uint64_t filter_len);
tpz_err tpz_sst_finish(tpz_ctx* ctx, const tpz_entries* entries, const tpz_sst_image* d_images,
                       uint32_t n_images, uint32_t max_blocks, uint8_t* d_base,
                       uint64_t span_bytes, uint64_t* d_info, void* stream);

/* ---- opening SST file images that are resident in HBM -------------------------------------
 * SsTable::open's parse (src/table.rs:91-112: read_bloom :75-87, the meta offset :93-97,
 * BlockMeta::decode_block_meta :49-59) for a batch of whole file images that already lie in one
 * device buffer, as tpz_sst_finish leaves them or as tpz_verify_files takes them. Additive within
 * ABI 8: new symbols and constants only (TPZ_HAS_OPEN tells a consumer the header has them). The
 * outputs are what a tpz_table / tpz_get_table needs besides the decoded columns: every block's
 * extent (the decode's d_ext), the block first keys with their positions, and where the bloom
 * filter lies in the image; nothing is copied to the host and the image is never written.
 *
 * File f is d_src[d_span[2f] .. d_span[2f] + d_span[2f + 1]): the whole file, its 4-byte CRC
 * trailer included (FileObject::size() = len - 4, src/table/file_object.rs:29-31, :63). The spans
 * lie inside [0, span_bytes), in increasing address order, and do not overlap; any bytes may lie
 * between them. The calls read nothing outside the spans. A file that starts before its
 * predecessor ends, or ends past span_bytes, is TPZ_OPEN_UNSUPPORTED; whatever the spans hold,
 * every access stays inside the spans, the scratch and the stated capacities.
 *
 * tpz_open_index, per file:
 *   d_info  8 u64: {status, size, meta offset, meta bytes, bloom offset or UINT64_MAX,
 *           filter_len, n_blocks, flags}; size = len - 4 (0 when len < 4); with a status other
 *           than TPZ_OPEN_OK every field after size is 0. flags bit 0 is set by tpz_open_metas.
 *   status, check by check in the reference's order:
 *     TPZ_OPEN_SHORT           len < 8: read_bloom's `size - SIZEOF_U32` underflows (:78), or there
 *                              is no trailer
 *     TPZ_OPEN_BLOOM_RANGE     offset + 4 > size, offset = the BE u32 at size - 4 (:84: `size -
 *                              SIZEOF_U32 - offset` underflows). size == offset + 4: no bloom
 *                              section (:81-83); otherwise the filter is [offset, size - 4)
 *     TPZ_OPEN_META_RANGE      offset < 4 (:94), or the BE u32 at offset - 4 is > offset - 4 (:97)
 *     TPZ_OPEN_META_TRUNCATED  decode_block_meta's panics (:52-54): fewer than 6 bytes left for a
 *                              record's offset and key length, or a key running past offset - 4.
 *                              The reference decodes the whole section before anything looks at
 *                              the offsets, so this wins over BAD_EXTENTS
 *     TPZ_OPEN_BAD_EXTENTS     the block offsets followed by the meta offset are not
 *                              non-decreasing (read_block's `end - offset`, :154-164)
 *     TPZ_OPEN_NO_BLOCKS       an empty meta section (init_samllest_biggest_key's block_metas[0],
 *                              :143-151)
 *     TPZ_OPEN_UNSUPPORTED     not a reference outcome: len > 2^34 (this keeps n_blocks below
 *                              2^32), or a span that breaks the rules above
 *   d_file_block, d_file_key  n_files + 1 u64 each: exclusive prefix sums over the files of
 *           n_blocks and of the first keys' bytes; only OK files count; the last element is the
 *           total. The caller reads both totals back to size tpz_open_metas' outputs.
 *   d_scratch  tpz_open_scratch_bytes(span_bytes, n_files) bytes, 8-byte aligned: one 16-byte
 *           checkpoint per TPZ_OPEN_TILE bytes of every meta section, handed to tpz_open_metas.
 *
 * tpz_open_metas, for an OK file f with n blocks, b = d_file_block[f] + f:
 *   d_ext[b + j], j = 0..n        the block offsets, then the meta offset, relative to the image's
 *                                 first byte: block j is image[d_ext[b + j] .. d_ext[b + j + 1])
 *   d_first_pos[b + j], j = 0..n  positions local to the file, starting at 0: block j's first key
 *                                 is d_first_keys[d_file_key[f] + d_first_pos[b + j] ..
 *                                 d_file_key[f] + d_first_pos[b + j + 1])
 * so a tpz_table for file f is three pointer offsets into the shared arrays. d_info[8f + 7] bit 0
 * is set when some block's last byte is tag 2 or 3 (compress.rs:104-111: the codec step is
 * needed). Nothing is written at or past block_cap + n_files entries of d_ext / d_first_pos or
 * key_cap bytes of d_first_keys; the caller passes the totals tpz_open_index reported.
 *
 * Both calls are asynchronous on `stream` and use no workspace but d_scratch.
 * TPZ_ERR_INVALID_ARG, before any device work, for null pointers, misaligned pointers (u64 arrays
 * and d_scratch 8-byte) or scratch_bytes < tpz_open_scratch_bytes(span_bytes, n_files).
 * n_files == 0 is valid and does nothing. */
#define TPZ_HAS_OPEN 1
#define TPZ_OPEN_TILE 4096u /* bytes of meta section per checkpoint */
#define TPZ_OPEN_OK 0
#define TPZ_OPEN_SHORT 1
#define TPZ_OPEN_BLOOM_RANGE 2
#define TPZ_OPEN_META_RANGE 3
#define TPZ_OPEN_META_TRUNCATED 4
#define TPZ_OPEN_BAD_EXTENTS 5
#define TPZ_OPEN_NO_BLOCKS 6
#define TPZ_OPEN_UNSUPPORTED 7
static inline uint64_t tpz_open_scratch_bytes(uint64_t span_bytes, uint64_t n_files) {
  return (span_bytes / TPZ_OPEN_TILE + 2 * n_files) * 16;
}
tpz_err tpz_open_index(tpz_ctx* ctx, const uint8_t* d_src, uint64_t span_bytes,
                       const uint64_t* d_span, uint32_t n_files, uint64_t* d_info,
                       uint64_t* d_file_block, uint64_t* d_file_key, uint8_t* d_scratch,
                       uint64_t scratch_bytes, void* stream);
tpz_err tpz_open_metas(tpz_ctx* ctx, const uint8_t* d_src, uint64_t span_bytes,
                       const uint64_t* d_span, uint32_t n_files, uint64_t* d_info,
                       const uint64_t* d_file_block, const uint64_t* d_file_key,
                       const uint8_t* d_scratch, uint64_t scratch_bytes, uint64_t* d_ext,
                       uint64_t* d_first_pos, uint8_t* d_first_keys, uint64_t block_cap,
                       uint64_t key_cap, void* stream);

/* ---- resident tables as merge runs --------------------------------------------------------
 * The device's SsTableIterator (src/table/iterator.rs:10-96) over tables whose decoded columns
 * already lie in HBM behind tpz_table descriptors: for a list of tables in priority order
 * (sub_compact's this_tables + next_tables, src/level.rs:184-197: an earlier table wins a key) the
 * entries of every table, block after block, as one tpz_entries holding a run per table: dense key
 * and value columns plus absolute entry positions, what tpz_merge_runs and the write side take.
 * A compaction's inputs then come from the columns that serve the gets, with no host
 * concatenation, upload or second decode. Additive within ABI 8: new symbols only
 * (TPZ_HAS_TABLE_RUNS tells a consumer the header has them).
 *
 * d_tables: n_runs <= TPZ_MERGE_MAX_RUNS descriptors in device memory, in run order. h_block_first
 * (host, n_runs + 1 u32, read during the call) starts at 0 and is non-decreasing; B =
 * h_block_first[n_runs]. Run r is the blocks [h_block_first[r], h_block_first[r + 1]) of table r,
 * counted from the table's block 0, in block order. A table may have no blocks; n_runs == 0 is
 * valid and gives all totals 0.
 *
 * tpz_table_runs_layout (the sizing pass), with g = h_block_first[r] + b for block b of run r:
 *   d_block_first  3 x (B + 1) u64: d_block_first[g] = the entries before block g in run order,
 *           d_block_first[B + 1 + g] the key bytes, d_block_first[2 (B + 1) + g] the value bytes;
 *           the totals at g = B. A block counts its n entries and its K key and V value bytes (the
 *           last {kend, vend} pair) when its status is TPZ_BLOCK_OK or TPZ_BLOCK_OK_SPILLED; a
 *           block of any other status (BAD_ENTRY, CHECKSUM_MISMATCH, CODEC_ERROR, MALFORMED, EMPTY,
 *           BAD_TAG, SPILL_FULL), and a block past its descriptor's n_blocks, holds nothing. The
 *           ends of a block with count 0 are not read.
 *   d_run_first    n_runs + 1 u32: the entries before every run, tpz_merge_runs' h_run_first once
 *           read back (saturated at UINT32_MAX).
 *   d_info  4 u64: {entries, key bytes, value bytes, first bad block}. The entry count is a true
 *           u64: the caller refuses 2^32 or more, tpz_entries.n_entries being u32. d_info[3] =
 *           run << 32 | block of the first block in run order that holds nothing for its status,
 *           or UINT64_MAX; the other outputs are as defined above either way (sub_compact's `?`
 *           fails the compaction at that block: the caller decides).
 *   Uses the stream's grow-only workspace for the scans' partial sums.
 *
 * tpz_table_runs_entries (the gather pass), over the same tables and d_block_first:
 *   d_keys / d_vals  block g's K key bytes at d_keys[kb ..], kb = d_block_first[B + 1 + g], and its
 *           V value bytes at d_vals[vb ..]: two byte-range copies per block out of its slot or its
 *           spill record (one wave per block, 16-byte stores, the pieces a range shares with its
 *           neighbours byte by byte: no two blocks store the same byte).
 *   d_kpos / d_vpos  entry_cap + 1 u64 each: entry j of block g is e = d_block_first[g] + j,
 *           d_kpos[e] = kb + (j ? kend[j - 1] : 0), d_vpos likewise; d_kpos[n] / d_vpos[n] = the
 *           totals (n = d_info[0]), so (d_keys, d_kpos, d_vals, d_vpos, n, key bytes, value bytes)
 *           is a tpz_entries and d_run_first its run table.
 *   Nothing is written at or past key_cap / val_cap bytes, nor past index entry_cap of d_kpos /
 *   d_vpos; a caller passes the totals of d_info. Empty keys are tpz_merge_runs' business.
 * All position arithmetic is u64 (slot bases and spill offsets pass 2^32 for tables over 4 GiB).
 * Every index read from device memory is clamped (n to the block's reserved pairs, K and V to the
 * slot, an entry's end to K / V, a block to what the layout reserved), so tables whose columns
 * were overwritten give wrong entries, not stray accesses outside the slot or the outputs.
 *
 * Both calls are asynchronous on `stream`. TPZ_ERR_INVALID_ARG, before any device work, for null
 * pointers (d_keys / d_vals may be NULL with a capacity of 0, d_tables with n_runs 0), misaligned
 * pointers (d_keys / d_vals 16-byte; d_tables and the u64 arrays 8-byte; d_run_first 4-byte), an
 * h_block_first that does not start at 0 or decreases, or n_runs > TPZ_MERGE_MAX_RUNS. */
#define TPZ_HAS_TABLE_RUNS 1
tpz_err tpz_table_runs_layout(tpz_ctx* ctx, const tpz_table* d_tables, uint32_t n_runs,
                              const uint32_t* h_block_first, uint64_t* d_block_first,
                              uint32_t* d_run_first, uint64_t* d_info, void* stream);
tpz_err tpz_table_runs_entries(tpz_ctx* ctx, const tpz_table* d_tables, uint32_t n_runs,
                               const uint32_t* h_block_first, const uint64_t* d_block_first,
                               uint8_t* d_keys, uint64_t key_cap, uint64_t* d_kpos,
                               uint8_t* d_vals, uint64_t val_cap, uint64_t* d_vpos,
                               uint64_t entry_cap, void* stream);

/* ---- point gets from encoded blocks in place ---------------------------------------------
 * An in-place table is a resident table without decoded columns: its blocks are read where they
 * lie, in the Uncompress form payload | crc u32 BE | tag 1 with payload = n u16 BE | n offsets
 * u16 BE | data (src/block.rs:31-44, src/block/compress.rs:85-89); blocks stored with a codec
 * take tpz_decompress_blocks first, whose output is that form. The device does on those bytes
 * what BlockIterator does (src/block/iterator.rs:63-109): seek_to_key bisects over offsets[mid],
 * reads klen and compares the key (:91-109); seek_to reads vlen and the value (:74-82). A served
 * table then costs its encoded bytes plus 17 bytes per block (d_ext, d_first_pos, d_status) and
 * its first keys, not the decoded columns on top. Additive within ABI 8: new symbols only
 * (TPZ_HAS_RAW_TABLES tells a consumer the header has them). Scans, level scans and compaction
 * inputs still take decoded tables (tpz_table).
 *
 * tpz_raw_verify: what Block::decode does before any entry is read (src/block.rs:46-59,
 * src/block/compress.rs:95-113), for every block of `batch`: the tag dispatch, the CRC over the
 * payload, n and the n offsets readable.
 *   d_status[b]  what tpz_decode_blocks reports for the same batch, except that
 *                TPZ_BLOCK_OK_SPILLED and TPZ_BLOCK_BAD_ENTRY read as TPZ_BLOCK_OK (no entry is
 *                read: a bad entry fails lazily, where a seek touches it, as in the reference)
 *   d_crc[b]     the CRC-32 computed over the payload, as tpz_decode_blocks' d_crc (0 for EMPTY,
 *                BAD_TAG, UNSUPPORTED_CODEC and a block shorter than 5 bytes)
 * Device memory: the caller's two columns and n_blocks u32 of the stream's workspace; nothing
 * proportional to the data bytes. batch->d_src may have any alignment. n_blocks == 0 is valid.
 *
 * tpz_raw_table: d_first_keys / d_first_pos as tpz_table; block b is d_src[d_ext[b] ..
 * d_ext[b + 1]) (any byte offset; extents may pass 2^32); d_status = tpz_raw_verify's column;
 * d_filter as tpz_get_table's. An entry is named (block, entry index) as in a decoded table.
 *
 * tpz_raw_seek_keys = tpz_seek_keys, tpz_raw_get_keys / tpz_raw_get_values = tpz_get_keys /
 * tpz_get_values, tpz_raw_lsm_get_keys / tpz_raw_lsm_get_values = tpz_lsm_get_keys /
 * tpz_lsm_get_values (memtable runs in front, the TPZ_HIT_MEM convention), each over in-place
 * tables: the same outputs, statuses, panics classes, preconditions and TPZ_ERR_INVALID_ARG rules
 * (n_levels > TPZ_GET_MAX_LEVELS, a bad h_level_first, n_runs > TPZ_MEM_MAX_RUNS, null or
 * misaligned pointers; n_keys == 0 and n_tables == 0 are valid). An entry whose key read panics
 * in the reference (offset past the data, klen unreadable or past the end: :97-100) gives
 * TPZ_BLOCK_MALFORMED where the bisection reads it, one whose value read panics (:80-82) where
 * the seek lands on it; entries the seek does not touch do not matter. With descriptors or block
 * bytes that changed after tpz_raw_verify the results are unspecified, but every loop is bounded
 * and no byte outside a block's extent is read. */
#define TPZ_HAS_RAW_TABLES 1
/* (declared with a tag, as tpz_get_table is) */
struct tpz_raw_table {
  const uint8_t* d_first_keys; /* as tpz_table */
  const uint64_t* d_first_pos; /* n_blocks + 1 */
  const uint8_t* d_src;        /* the blocks where they lie (Uncompress form, tag 1) */
  const uint64_t* d_ext;       /* n_blocks + 1 extents into d_src */
  uint32_t n_blocks;
  const uint8_t* d_status;     /* tpz_raw_verify's, one byte per block */
  const uint8_t* d_filter;     /* Bloom::encode or NULL */
  uint64_t filter_len;
};
typedef struct tpz_raw_table tpz_raw_table;

tpz_err tpz_raw_verify(tpz_ctx* ctx, const tpz_batch* batch, uint8_t* d_status, uint32_t* d_crc,
                       void* stream);
tpz_err tpz_raw_seek_keys(tpz_ctx* ctx, const tpz_raw_table* table, const uint8_t* d_keys,
                          const uint64_t* d_key_pos, uint32_t n_keys, uint32_t* d_block,
                          uint32_t* d_entry, uint8_t* d_status, uint8_t* d_valid, void* stream);
tpz_err tpz_raw_get_keys(tpz_ctx* ctx, const tpz_raw_table* d_tables, uint32_t n_tables,
                         const uint32_t* h_level_first, uint32_t n_levels, const uint8_t* d_keys,
                         const uint64_t* d_key_pos, uint32_t n_keys, uint8_t* d_result,
                         uint8_t* d_status, uint32_t* d_table, uint32_t* d_block,
                         uint32_t* d_entry, uint64_t* d_val_pos, void* stream);
tpz_err tpz_raw_get_values(tpz_ctx* ctx, const tpz_raw_table* d_tables, uint32_t n_tables,
                           uint32_t n_keys, const uint8_t* d_result, const uint32_t* d_table,
                           const uint32_t* d_block, const uint32_t* d_entry,
                           const uint64_t* d_val_pos, uint8_t* d_vals, uint64_t val_cap,
                           void* stream);
tpz_err tpz_raw_lsm_get_keys(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                             const tpz_raw_table* d_tables, uint32_t n_tables,
                             const uint32_t* h_level_first, uint32_t n_levels,
                             const uint8_t* d_keys, const uint64_t* d_key_pos, uint32_t n_keys,
                             uint8_t* d_result, uint8_t* d_status, uint32_t* d_table,
                             uint32_t* d_block, uint32_t* d_entry, uint64_t* d_val_pos,
                             void* stream);
tpz_err tpz_raw_lsm_get_values(tpz_ctx* ctx, const tpz_mem_run* d_runs, uint32_t n_runs,
                               const tpz_raw_table* d_tables, uint32_t n_tables, uint32_t n_keys,
                               const uint8_t* d_result, const uint32_t* d_table,
                               const uint32_t* d_block, const uint32_t* d_entry,
                               const uint64_t* d_val_pos, uint8_t* d_vals, uint64_t val_cap,
                               void* stream);

/* ---- host write side (inputs for benches and the table facade) ---------------------------
 * SsTableBuilder::add + block_build (src/table/builder.rs:49-85) with BlockBuilder's fill rule
 * (src/block/builder.rs:26-41) and Block::encode + Uncompress (src/block.rs:31-44,
 * src/block/compress.rs:85-89): packs entries e (key = keys[kpos[e]..kpos[e+1]), value likewise)
 * into blocks written back to back into h_out, block i = [ext[i], ext[i+1]). Host memory only.
 * Returns TPZ_ERR_INVALID_ARG for an empty key or an entry no block can hold, TPZ_ERR_NOMEM
 * when out_cap / ext_cap are too small. */
int tpz_build_blocks(const uint8_t* h_keys, const uint64_t* h_kpos, const uint8_t* h_vals,
                     const uint64_t* h_vpos, uint64_t n_entries, uint32_t block_size,
                     uint8_t* h_out, uint64_t out_cap, uint64_t* h_ext, uint64_t ext_cap,
                     uint64_t* n_blocks, uint64_t* out_len);
/* compress::encode with CompressOptions::Snappy (src/block/compress.rs:66-71) over a batch of
 * Uncompress blocks: every tag-1 block i = h_src[h_ext[i] .. h_ext[i+1]) is written to h_out as
 * snappy_raw(payload | crc) | 2, other blocks unchanged; h_out_ext gets n_blocks + 1 extents.
 * Host memory only; out_cap >= 32 * n_blocks + 2 * h_ext[n_blocks] always suffices. */
int tpz_snappy_encode_blocks(const uint8_t* h_src, const uint64_t* h_ext, uint64_t n_blocks,
                             uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_ext,
                             uint64_t* out_len);
/* compress::encode with CompressOptions::Lz4 (src/block/compress.rs:73-77): every tag-1 block
 * becomes u32 LE size (payload | crc) | lz4_block(payload | crc) | 3 (lz4::block::compress with
 * prepend_size), other blocks unchanged. Host memory only; out_cap >= 32 * n_blocks +
 * 2 * h_ext[n_blocks] always suffices. */
int tpz_lz4_encode_blocks(const uint8_t* h_src, const uint64_t* h_ext, uint64_t n_blocks,
                          uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_ext,
                          uint64_t* out_len);
/* ---- compaction output with a codec, on the device ---------------------------------------
 * compress::encode(data, opt) (src/block/compress.rs:66-77, :82-93) for every block of a batch
 * of Uncompress blocks in HBM (tpz_encode_blocks' output), opt = the SST's compress_option
 * (src/table/builder.rs:74; Snappy by default, src/opt.rs:48):
 *   codec 2 (Snappy): block i = payload | crc | 1 becomes snappy_raw(payload | crc) | 2
 *   codec 3 (Lz4):    u32 LE size | lz4_block(payload | crc) | 3 (lz4::block::compress with
 *                     prepend_size; every match ends 5 bytes and starts 12 bytes before the
 *                     end, as LZ4_decompress_safe requires)
 * written back to back into d_dst; d_dst_ext gets n_blocks + 1 extents (its last entry = the
 * bytes written), so BlockMeta::offset of block i is d_dst_ext[i] (src/table/builder.rs:74-84).
 * Blocks with another tag are copied unchanged; any other codec is TPZ_ERR_INVALID_ARG. The
 * streams decode with snap / liblz4 to exactly payload | crc; they are not byte-identical to
 * those libraries' encoders. Blocks whose payload is longer than 4,336 bytes (block_size past
 * 4 KiB) are emitted as literal elements only: valid streams, a few bytes larger than the
 * payload (the match finder works on blocks staged whole in LDS). d_dst needs
 * tpz_layout_compress_bound(src_bytes, n_blocks) bytes. batch->d_src and d_dst must be 16-byte
 * aligned (TPZ_ERR_INVALID_ARG otherwise). Asynchronous on `stream`; uses the stream's workspace
 * (scratch of that bound). */
uint64_t tpz_layout_compress_bound(uint64_t src_bytes, uint64_t n_blocks);
tpz_err tpz_compress_blocks(tpz_ctx* ctx, const tpz_batch* batch, uint32_t codec, uint8_t* d_dst,
                            uint64_t* d_dst_ext, void* stream);

/* CRC-32/ISO-HDLC on the host (checksum::calculate_checksum, src/checksum.rs:6-10). */
uint32_t tpz_host_crc32(const uint8_t* h_buf, uint64_t len);

/* ---- errors ------------------------------------------------------------------------------ */
/* Writes the reference's error text for a block outcome into buf (NUL-terminated):
 * "data is empty", "invaild data", "checksum: expected E, actual A" (decimal, as Rust's {}),
 * "unsupported codec", "malformed block", "spill arena too small", "decompression failed",
 * "" for OK, OK_SPILLED and BAD_ENTRY (an Ok(Block); its bad entries panic on access).
 * Returns the text length. */
int tpz_format_block_error(int status, uint32_t crc_expected, uint32_t crc_actual, char* buf,
                           size_t cap);
/* Last HIP error text seen by this thread (empty if none). */
const char* tpz_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TPZ_GPU_H */

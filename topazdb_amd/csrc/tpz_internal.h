// tpz_internal.h — shared between the C ABI (tpz_api.cpp) and the kernels (tpz_decode.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tpz_gpu.h"

// Context accessors for the host pipeline (tpz_host_pipeline.cpp; defined in tpz_api.cpp).
int tpz_internal_device(tpz_ctx* c);
tpz_err tpz_internal_hip_fail(hipError_t e, const char* what);
// Sets tpz_last_error's text and returns err.
tpz_err tpz_internal_fail(tpz_err err, const char* what);
// The context's pool of host pipelines (streams + buffers of tpz_decode_blocks_host, reused
// across calls; one per concurrent caller): acquire returns a free one or nullptr; release puts
// one back (fresh = created by this call: the context takes ownership); the context destroys
// them with tpz_internal_pipe_destroy (tpz_host_pipeline.cpp).
void* tpz_internal_pipe_acquire(tpz_ctx* c);
void tpz_internal_pipe_release(tpz_ctx* c, void* pipe, bool fresh);
void tpz_internal_pipe_destroy(void* pipe);

namespace tpz {

// CRC-32 lookup tables of the block decode, uploaded once per context (tpz_api.cpp):
// ids 0..15 = T_0..T_15 (slice-by-16); ids 16+4j+i = T_{n_j-1-i}: the shift-by-n_j operator,
// n_j = kCrcShiftBytes[j] = 80 * 2^j (the lane-position shifts of the CRC combine; 2 x 2560 B
// chains the 5120-B super-rounds of long blocks);
// id 40 = kCrcInvTable: inv[t] = the byte b whose T_0[b] has top byte t (one zero byte un-shifted).
constexpr int kNumCrcTables = 41;
constexpr int kCrcInvTable = 40;
constexpr int kCrcLaneBytes = 80;
constexpr int kCrcShiftBytes[6] = {80, 160, 320, 640, 1280, 2560};
// Big path entry-table capacity per block and column: slots are only written when 6n <= len
// (the unified key+value table holds 2 x this).
constexpr uint32_t kBigMaxSlots = TPZ_LDS_BLOCK_BYTES / 6 + 16;

// Range CRC (tpz_crc.hip): shift-by-16*2^j operators j = 0..kRangeShiftOps-1 in the global
// range tables (ranges up to 16 * 2^kRangeShiftOps bytes), and the 32-fold replicated
// slice-by-4 table (4 x 256 x 32 u32).
constexpr int kRangeShiftOps = 32;
constexpr int kRangeTables = 16 + 4 * kRangeShiftOps;
// ... followed by 4 power tables: id kPowTable + i, entry j = x^(8 j 256^i) mod P (the shift by
// j * 256^i bytes as a GF(2)[x] factor: tpz_flat.hip open_finish_kernel)
constexpr int kPowTable = kRangeTables;
constexpr int kRangeTablesAll = kRangeTables + 4;
constexpr int kCrcRepWords = 4 * 256 * 32;

// Slotted layout (include/tpz_gpu.h), callable from device code.
__host__ __device__ inline uint64_t slot_base(uint64_t ext_i, uint64_t i) {
  return ((ext_i + 127u) & ~(uint64_t)127u) + 256u * i;
}
__host__ __device__ inline uint64_t entry_base(uint64_t ext_i, uint64_t i) {
  return 16u * (ext_i / 96u + i);
}
__host__ __device__ inline uint64_t value_start(uint64_t key_bytes) {
  return (key_bytes + 15u) & ~(uint64_t)15u;
}
// Spill records (include/tpz_gpu.h): u32 ends[2n], then the stream from spill_stream(n).
__host__ __device__ inline uint64_t spill_stream(uint64_t n) {
  return (8u * n + 127u) & ~(uint64_t)127u;
}
__host__ __device__ inline uint64_t spill_record_bytes(uint64_t n, uint64_t k, uint64_t v) {
  return spill_stream(n) + ((value_start(k) + v + 127u) & ~(uint64_t)127u);
}
// A TPZ_BLOCK_BAD_ENTRY record's class bytes follow its ends and stream.
__host__ __device__ inline uint64_t spill_classes(uint64_t n, uint64_t k, uint64_t v) {
  return spill_record_bytes(n, k, v);
}
// Readers of decoded blocks: a block whose entries are in its slot or in a spill record.
__host__ __device__ inline bool block_decoded(uint32_t st) {
  return st == TPZ_BLOCK_OK || st == TPZ_BLOCK_OK_SPILLED || st == TPZ_BLOCK_BAD_ENTRY;
}
__host__ __device__ inline bool block_in_spill(uint32_t st) {
  return st == TPZ_BLOCK_OK_SPILLED || st == TPZ_BLOCK_BAD_ENTRY;
}

struct LaunchArgs {
  const uint8_t* src;
  const uint64_t* ext;
  uint64_t src_bytes;
  uint32_t n_blocks;
  const uint32_t* crc_tables;
  uint8_t* data;
  uint32_t* ends;
  uint32_t* count;
  uint8_t* status;
  uint32_t* crc;
  uint32_t* defer_list;   // workspace: n_blocks entries
  uint32_t* defer_count;  // tail + kTailBig
  uint32_t num_cus;
  uint64_t* big_scratch;  // big_grid x 2 x kBigMaxSlots
  uint32_t big_grid;
  uint32_t* spill_list;   // workspace: n_blocks entries (blocks for the spill path)
  uint32_t* spill_count;  // tail + kTailSpill
  uint8_t* spill;         // the caller's spill arena (tpz_columns)
  uint64_t spill_cap;
  uint64_t* spill_off;
  uint64_t* spill_used;   // zeroed before the launch
  uint32_t* bw_list;      // workspace: n_blocks entries (blocks for the bigwave kernel)
  uint32_t* bw_count;     // tail + kTailBw
  const uint32_t* rep;    // replicated slice-by-4 tables (the bigwave phase's CRC)
  const uint64_t* efirst; // exact ends layout (tpz_columns.d_entry_first) or null
  // flat layout (tpz_decode_blocks_flat): key / value columns and the blocks' first key / value
  // byte in them; null: slotted (data)
  uint8_t* keys;
  uint8_t* vals;
  const uint64_t* kfirst;
  const uint64_t* vfirst;
  uint32_t* tail;         // workspace: kTailCounters, zero at the launch (the tail kernel
                          // leaves them zero)
};
// Pair index of block b's first {kend, vend}: the exact layout's d_entry_first[b], or the
// slotted tpz_entry_base.
__host__ __device__ inline uint64_t ends_base(const uint64_t* efirst, uint64_t ext_b, uint64_t b) {
  return efirst ? efirst[b] : entry_base(ext_b, b);
}

void launch_decode(const LaunchArgs& a, hipStream_t stream);

// The decode's worklist counters (tpz_decode.hip decode_tail_kernel): zero before a decode, and
// zeroed again by the tail kernel's last workgroup.
enum TailCounter : int {
  kTailBig = 0,        // big list length
  kTailSpill,          // spill list length
  kTailBw,             // bigwave list length
  kTailBigTicket,      // big blocks claimed
  kTailBigDone,        // big blocks finished
  kTailSpillTicket,    // spill blocks claimed
  kTailExit,           // tail-kernel workgroups finished
  kTailRow,            // wave path: rows of 16 blocks claimed (decode_wave_kernel)
  kTailCounters,
  // Sticky, past the counters the tail kernel zeroes: set when a tail workgroup's wait for the
  // big phase timed out (tpz_decode_check reports it and clears it)
  kTailError = kTailCounters,
  // Sticky: set when tpz_decompress_blocks gave an LZ4 block a range that is not its exact length
  // (claimed sizes, tpz_decompressed_sizes_claimed); tpz_decompress_check reports and clears it
  kTailCodecInexact,
  kTailWords
};
__device__ __forceinline__ uint32_t tail_load(const uint32_t* c) {
  return __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Every thread of the workgroup: wait until *done reaches n, then see what the finished blocks
// wrote. Workgroups only wait for blocks that running workgroups hold (tickets), so the wait
// ends; it is still bounded (about a second), so that a counting bug cannot hang the device.
// A wait that times out is not passed over: it sets the sticky error word (tpz_decode_check
// returns TPZ_ERR_INTERNAL) and returns false, and the caller skips what depended on it.
__device__ __forceinline__ bool tail_wait(const uint32_t* done, uint32_t n, uint32_t* err,
                                          uint32_t* flag) {
  if (threadIdx.x == 0) {
    uint32_t i = 0;
    for (; i < (1u << 22) && tail_load(done) < n; i++) __builtin_amdgcn_s_sleep(2);
#ifdef TPZ_ABL_TAILLATE
    const bool late = true;   // diagnostic build (tests/test_gpu_tail_check.py): every wait times out
#else
    const bool late = tail_load(done) < n;
#endif
    if (late) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = late ? 0u : 1u;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return __builtin_amdgcn_readfirstlane(*flag) != 0;
}

// Long blocks with few entries (tpz_bigwave.hip): one wave per block, straight from HBM.
struct BigWaveLaunch {
  const uint8_t* src;
  const uint64_t* ext;
  uint64_t src_bytes;
  const uint32_t* rep;          // replicated slice-by-4 tables
  const uint32_t* crc_tables;   // the decode tables (small shifts, inverse table)
  const uint32_t* list;
  uint8_t* data;
  uint32_t* ends;
  uint32_t* count;
  uint8_t* status;
  uint32_t* crc;
  uint32_t* spill_list;
  uint32_t* spill_count;
  uint32_t* big_list;
  uint32_t* big_count;
  const uint64_t* efirst;
};
// Launched between the wave kernel and decode_tail_kernel; ctr = the decode's tail counters.
void launch_bigwave(const BigWaveLaunch& a, uint32_t* ctr, uint32_t grid, hipStream_t stream);

// The spill path (tpz_spill.hip, phase C of the tail kernel): blocks the LDS paths hand over,
// decoded into the arena.
struct SpillLaunch {
  const uint8_t* src;
  const uint64_t* ext;
  uint64_t src_bytes;
  const uint32_t* crc_tables;
  const uint32_t* list;
  uint8_t* spill;
  uint64_t spill_cap;
  uint64_t* spill_off;
  uint64_t* spill_used;
  uint32_t* count;
  uint8_t* status;
  uint32_t* crc;
  // flat layout (keys non-null): the spill path writes the block's ends to
  // ends[2 * efirst[b] ..], its keys to keys[kfirst[b] ..] and its values to vals[vfirst[b] ..];
  // its arena record holds only a BAD_ENTRY block's class bytes
  uint32_t* ends;
  const uint64_t* efirst;
  uint8_t* keys;
  uint8_t* vals;
  const uint64_t* kfirst;
  const uint64_t* vfirst;
};

struct CrcLaunch {
  const uint8_t* src;
  const uint64_t* ext;
  uint64_t src_bytes;
  uint32_t n_ranges;
  uint32_t trailer;       // 0 (plain ranges), 4 (FileObject: BE u32 trailer after the CRC) or 5
                          // (a block: the BE u32 CRC and the tag byte, tpz_raw_verify)
  const uint32_t* tables; // kRangeTables x 256
  const uint32_t* rep;    // kCrcRepWords
  uint32_t* acc;          // workspace: n_ranges, zeroed before the launch
  uint32_t* crc;
  uint8_t* status;        // null for plain ranges
  uint32_t num_cus;
  bool acc_only;          // leave R0 of every range's main part in acc (no finish kernel:
                          // tpz_flat.hip open_finish_kernel finishes the files' tails)
};

void launch_crc_ranges(const CrcLaunch& a, hipStream_t stream);

struct SeekLaunch {
  const uint8_t* fk;
  const uint64_t* fk_pos;
  uint32_t n_blocks;
  const uint64_t* ext;
  const uint8_t* data;
  const uint32_t* ends;
  const uint32_t* count;
  const uint8_t* bstatus;
  const uint8_t* spill;
  const uint64_t* spill_off;
  const uint8_t* q;
  const uint64_t* q_pos;
  uint32_t n_q;
  uint32_t* out_block;
  uint32_t* out_entry;
  uint8_t* out_status;
  uint8_t* out_valid;
  const uint64_t* efirst;
};
void launch_seek(const SeekLaunch& a, hipStream_t stream);

struct BloomLaunch {
  const uint8_t* filter;
  uint64_t filter_len;
  const uint8_t* q;
  const uint64_t* q_pos;
  uint32_t n_q;
  uint8_t* out;
};
void launch_bloom(const BloomLaunch& a, hipStream_t stream);

struct BloomBuildLaunch {
  const uint8_t* keys;
  const uint64_t* key_pos;
  uint32_t n_keys;
  uint32_t k;
  uint64_t limit;       // bits in the array: (filter_len - 1) * 8
  uint8_t* filter;      // zeroed bit array, 4-byte aligned, padded to whole words
  uint64_t filter_words;  // (filter_len + 3) / 4
  void* work;           // bloom_build_work_bytes() of device scratch (the partitioned build)
};
// Scratch for the partitioned build (0: the filter is too big for it and the atomic kernel runs).
uint64_t bloom_build_work_bytes(uint32_t n_keys, uint32_t k, uint64_t limit);
void launch_bloom_build(const BloomBuildLaunch& a, hipStream_t stream);

struct PackLaunch {
  const uint64_t* ext;
  uint32_t n_blocks;
  const uint32_t* ends;
  const uint32_t* count;
  const uint8_t* status;
  const uint8_t* spill;
  const uint64_t* spill_off;
  const uint64_t* first;
  uint32_t* dense;
  const uint64_t* efirst;
};
void launch_pack_ends(const PackLaunch& a, hipStream_t stream);
// d_first[i] = sum of the header n of blocks < i (tpz_entry_first); `part` = workspace of
// entry_first_parts(n_blocks) u64.
uint64_t entry_first_parts(uint32_t n_blocks);
// tpz_flat_layout (tpz_flat.hip): first = 3 x (n_blocks + 1) u64 (entries, key bytes, value
// bytes: exclusive prefixes, totals at [n_blocks]); `part` = flat_scan_parts_words(n_blocks) u64.
uint64_t flat_scan_parts_words(uint32_t n_blocks);
// In place: a[i] = sum of a[j < i], a[n] = the total (n + 1 u64; part = flat_scan_parts_words(n)
// / 3 u64 suffices).
void launch_scan_u64(uint64_t* a, uint32_t n, uint64_t* part, hipStream_t stream);
// Three arrays of n + 1 u64 back to back (a, a + n + 1, a + 2 (n + 1)), each scanned in place as
// launch_scan_u64 does (the flat layout's scan); part = flat_scan_parts_words(n) u64. n > 0.
void launch_scan3_u64(uint64_t* a, uint32_t n, uint64_t* part, hipStream_t stream);
// tpz_flat_entry_pos (tpz_flat.hip): the flat columns' entry positions as a tpz_entries.
struct EntryPosLaunch {
  const uint64_t* first;   // tpz_flat_layout's 3 x (n_blocks + 1)
  const uint32_t* ends;
  const uint32_t* count;
  const uint8_t* status;
  uint32_t n_blocks;
  uint64_t* kpos;
  uint64_t* vpos;
  uint32_t* info;          // [0] = first block whose status is not OK (0xFFFFFFFF: none)
};
void launch_flat_entry_pos(const EntryPosLaunch& a, hipStream_t stream);

// tpz_merge_runs (tpz_merge.hip): MergeIterator over sorted runs of entries in HBM.
constexpr uint32_t kMergeTile = 1024;   // entries per tile-merge workgroup (256 threads x 4)
struct MergeLaunch {
  const uint8_t* keys;
  const uint64_t* kpos;
  uint64_t key_bytes;
  const uint8_t* vals;
  const uint64_t* vpos;
  uint64_t val_bytes;
  uint32_t n;                 // > 0
  uint32_t n_runs;            // 1 .. TPZ_MERGE_MAX_RUNS
  const uint32_t* run_first;  // host: n_runs + 1, checked by the caller
  uint8_t* out_keys;
  uint64_t* out_kpos;
  uint8_t* out_vals;
  uint64_t* out_vpos;
  uint32_t* src_entry;        // or null
  uint64_t* info;             // 4 u64
  void* work;                 // merge_work_bytes(n, n_runs) of device scratch
};
uint64_t merge_work_bytes(uint32_t n, uint32_t n_runs);
hipError_t launch_merge(const MergeLaunch& a, hipStream_t stream);

// tpz_mem_build (tpz_membuild.hip): a memtable run from entries in arrival order.
struct MemBuildLaunch {
  const uint8_t* keys;
  const uint64_t* kpos;
  uint64_t key_bytes;
  const uint8_t* vals;
  const uint64_t* vpos;
  uint64_t val_bytes;
  uint32_t n;                 // > 0
  uint32_t mode;              // TPZ_MEM_REPLAY / TPZ_MEM_PUT
  const uint64_t* version;    // n u64 (PUT)
  uint8_t* out_keys;
  uint64_t* out_kpos;
  uint8_t* out_vals;
  uint64_t* out_vpos;
  uint64_t* out_prefix;       // or null
  uint32_t* src_entry;        // or null
  uint64_t* out_version;      // or null
  uint64_t* info;             // 8 u64
  void* work;                 // membuild_work_bytes(n) of device scratch
  uint32_t stop_after;        // 0; diagnostic: 1 ends after the sort passes, 2 after pick + scan
};
uint64_t membuild_work_bytes(uint32_t n);
hipError_t launch_membuild(const MemBuildLaunch& a, hipStream_t stream);
// tpz_wal_entries (tpz_membuild.hip): a WAL image's records as packed columns.
struct WalEntriesLaunch {
  const uint8_t* img;
  uint64_t img_bytes;
  const uint64_t* rec;        // n + 1
  uint32_t n;                 // > 0
  uint8_t* keys;
  uint64_t* kpos;
  uint8_t* vals;
  uint64_t* vpos;
  uint64_t* info;             // 4 u64
  void* work;                 // wal_entries_work_bytes(n) of device scratch
};
uint64_t wal_entries_work_bytes(uint32_t n);
hipError_t launch_wal_entries(const WalEntriesLaunch& a, hipStream_t stream);

// Which query call a launch serves: the tables alone (tpz_get_* / tpz_scan_*), memtable runs in
// front of them (tpz_lsm_*), or runs plus one merge cursor per level (tpz_level_scan_*). It picks
// the kernels and is never inferred from n_runs: the lsm kernels run with no runs too (they apply
// LsmStorage::get's empty-key assert, which tpz_get_keys does not).
enum class Flavour : uint32_t { kTables, kLsm, kLevel };
// Which kind of resident table a get launch reads: decoded columns (tpz_get_table) or the encoded
// blocks in place (tpz_raw_table; the kernels of tpz_raw.hip). It travels beside the flavour and
// is never inferred from the pointers.
enum class TableKind : uint32_t { kDecoded, kRaw };

// tpz_get_keys / tpz_get_values / tpz_lsm_get_keys / tpz_lsm_get_values (tpz_get.hip; the lsm
// walk's kernel is tpz_mem.hip's): LevelController::get over resident tables, and LsmStorage::get
// over memtable runs plus them.
struct GetLaunch {
  Flavour flavour;              // kTables / kLsm
  TableKind kind;
  const tpz_mem_run* runs;      // device (kLsm)
  uint32_t n_runs;              // <= TPZ_MEM_MAX_RUNS
  const void* tabs;             // device: tpz_get_table (kDecoded) or tpz_raw_table (kRaw)
  uint32_t n_tables;
  const uint32_t* level_first;  // host: n_levels + 1, checked by the caller
  uint32_t n_levels;            // <= TPZ_GET_MAX_LEVELS
  const uint8_t* q;
  const uint64_t* q_pos;
  uint32_t n_q;                 // > 0
  uint8_t* result;
  uint8_t* status;
  uint32_t* table;
  uint32_t* block;
  uint32_t* entry;
  uint64_t* val_pos;            // n_q + 1: the value lengths, then scanned in place
  uint64_t* part;               // flat_scan_parts_words(n_q) / 3 u64 of device scratch
};
void launch_get_walk(const GetLaunch& a, hipStream_t stream);
struct GetGatherLaunch {
  Flavour flavour;              // kTables / kLsm
  TableKind kind;
  const tpz_mem_run* runs;
  uint32_t n_runs;
  const void* tabs;             // tpz_get_table (kDecoded) or tpz_raw_table (kRaw)
  uint32_t n_tables;
  uint32_t n_q;                 // > 0
  const uint8_t* result;
  const uint32_t* table;
  const uint32_t* block;
  const uint32_t* entry;
  const uint64_t* val_pos;
  uint8_t* vals;
  uint64_t val_cap;
};
void launch_get_gather(const GetGatherLaunch& a, hipStream_t stream);
// The same over in-place tables (tpz_raw.hip; a.kind == kRaw: launch_get_walk / launch_get_gather
// hand over to them), tpz_raw_seek_keys, and tpz_raw_verify's header checks after the range CRC
// (launch_crc_ranges with trailer 5 left its CRCs and OK / CHECKSUM_MISMATCH / MALFORMED).
void launch_raw_get_walk(const GetLaunch& a, hipStream_t stream);
void launch_raw_get_gather(const GetGatherLaunch& a, hipStream_t stream);
struct RawSeekLaunch {
  tpz_raw_table t;
  const uint8_t* q;
  const uint64_t* q_pos;
  uint32_t n_q;                 // > 0
  uint32_t* out_block;
  uint32_t* out_entry;
  uint8_t* out_status;
  uint8_t* out_valid;
};
void launch_raw_seek(const RawSeekLaunch& a, hipStream_t stream);
void launch_raw_verify_headers(const uint8_t* src, const uint64_t* ext, uint32_t n_blocks,
                               uint8_t* status, uint32_t* crc, hipStream_t stream);

// tpz_mem_prefix (tpz_mem.hip): the prefix column of a memtable run resident in HBM.
void launch_mem_prefix(const tpz_entries& e, uint64_t* prefix, hipStream_t stream);   // n_entries > 0

// tpz_scan_ranges / tpz_lsm_scan_ranges (tpz_scan.hip) and tpz_level_scan_ranges
// (tpz_levelscan.hip): LsmStorage::scan over resident tables; kLsm and kLevel put the memtable
// runs' cursors in front of the tables', kLevel takes one cursor per run, per L0 table and per
// non-empty level below L0.
struct ScanLaunch {
  Flavour flavour;
  const tpz_mem_run* runs;      // device (kLsm, kLevel)
  uint32_t n_runs;              // <= TPZ_MEM_MAX_RUNS; kLsm: n_runs + n_tables <= TPZ_SCAN_MAX_TABLES
  const tpz_get_table* tabs;    // device
  uint32_t n_tables;            // <= TPZ_SCAN_MAX_TABLES; kLevel: any number
  const uint32_t* level_first;  // host: n_levels + 1, checked by the caller
  uint32_t n_levels;
  const uint8_t* lo;
  const uint64_t* lo_pos;
  const uint8_t* lo_kind;
  const uint8_t* hi;
  const uint64_t* hi_pos;
  const uint8_t* hi_kind;
  uint32_t n_scans;             // > 0
  uint32_t limit;               // > 0, n_scans * limit < 2^32
  uint8_t* result;
  uint8_t* status;
  uint32_t* where;              // 3 x n_scans
  uint32_t* hit_table;          // n_scans x limit each
  uint32_t* hit_block;
  uint32_t* hit_entry;
  uint64_t* first;              // n_scans + 1 each: the counts and byte totals, scanned in place
  uint64_t* key_first;
  uint64_t* val_first;
  uint64_t* info;               // 3 u64
  void* work;                   // device scratch: scan_ranges_work_bytes(n_scans, n_runs +
                                // n_tables); kLevel: level_scan_work_bytes(n_scans,
                                // level_scan_cursors(..), n_tables)
  uint32_t stop_after;          // 0; kLevel diagnostic: 1 ends after the index pass, 2 after the links
  uint32_t l0() const { return n_levels ? level_first[1] : 0u; }   // the number of L0 tables
};
uint64_t scan_ranges_work_bytes(uint32_t n_scans, uint32_t n_cursors);
uint64_t level_scan_cursors(const uint32_t* level_first, uint32_t n_levels, uint32_t n_runs);
uint64_t level_scan_work_bytes(uint32_t n_scans, uint32_t n_cursors, uint32_t n_tables);
// Every flavour (kLevel: through launch_level_scan_ranges).
void launch_scan_ranges(const ScanLaunch& a, hipStream_t stream);
void launch_level_scan_ranges(const ScanLaunch& a, hipStream_t stream);
// The scans of d_first / d_key_first / d_val_first and d_info (the tail of both).
void launch_scan_totals(const ScanLaunch& a, uint64_t* part, hipStream_t stream);
// tpz_scan_entries / tpz_lsm_scan_entries / tpz_level_scan_entries (tpz_scan.hip): the gather of
// the hits; kLsm and kLevel take the same kernels (hits in runs as well as in tables).
struct ScanEntriesLaunch {
  Flavour flavour;
  const tpz_mem_run* runs;
  uint32_t n_runs;
  const tpz_get_table* tabs;
  uint32_t n_tables;
  uint32_t n_scans;             // > 0
  uint32_t limit;
  const uint32_t* hit_table;
  const uint32_t* hit_block;
  const uint32_t* hit_entry;
  const uint64_t* first;
  uint8_t* keys;
  uint64_t key_cap;
  uint64_t* kpos;
  uint8_t* vals;
  uint64_t val_cap;
  uint64_t* vpos;
  void* work;                   // scan_entries_work_bytes(n_scans) of device scratch
};
uint64_t scan_entries_work_bytes(uint32_t n_scans);
void launch_scan_entries(const ScanEntriesLaunch& a, hipStream_t stream);

// tpz_entries_bound / tpz_table_cut / tpz_sst_finish (tpz_tables.hip): a compaction task's key
// ranges, table cuts and SST file images.
struct BoundLaunch {
  const uint8_t* keys;
  const uint64_t* kpos;
  uint64_t key_bytes;
  uint32_t n;
  const uint8_t* q;
  const uint64_t* q_pos;
  const uint8_t* incl;
  uint32_t n_q;                 // > 0
  uint32_t* out;
};
void launch_entries_bound(const BoundLaunch& a, hipStream_t stream);
struct CutLaunch {
  const uint64_t* kpos;
  const uint64_t* vpos;
  uint32_t start;
  uint32_t win;
  uint32_t seg_end;
  uint32_t* first;
  uint64_t* ext;
  const uint64_t* cut_ext;
  uint32_t* info;
  uint32_t block_size;
  uint64_t capacity;
  uint64_t* cut;                // 8 u64
};
void launch_table_cut(const CutLaunch& a, hipStream_t stream);
struct FinishLaunch {
  const uint8_t* keys;
  const uint64_t* kpos;
  uint64_t key_bytes;
  uint32_t n_entries;
  const tpz_sst_image* images;  // device
  uint32_t n_images;            // 1 .. 65535 (a grid dimension)
  uint32_t max_blocks;
  uint8_t* base;
  uint64_t span;
  uint64_t* part;               // workspace: n_images x finish_parts(max_blocks) u64
  uint64_t* crc_ext;            // workspace: 2 n_images + 1 u64 (the CRC's ranges)
  const uint32_t* crc;          // workspace: 2 n_images u32 (the CRC's output)
  uint64_t* info;               // 4 u64 per image
};
uint32_t finish_parts(uint32_t max_blocks);
// The metas, offsets and filters of every image and the CRC's ranges; then, after
// launch_crc_ranges over crc_ext (trailer 4), the images' CRC bytes.
void launch_finish_layout(const FinishLaunch& a, hipStream_t stream);
void launch_finish_crc(const FinishLaunch& a, hipStream_t stream);

// tpz_open_index / tpz_open_metas (tpz_open.hip): SsTable::open's parse over resident file
// images. launch_open_index: the footer checks, the walk of every meta section with its
// checkpoints (ck, filled with 0xFF by the caller), the prefix sums over the files; the output
// fields are unused. launch_open_metas: extents, first keys and positions from the checkpoints,
// then the codec flags.
struct OpenIndexLaunch {
  const uint8_t* src;
  uint64_t span_bytes;
  const uint64_t* span;         // {start, len} per file
  uint32_t n_files;             // 1 .. 2^31 - 1 (a grid dimension)
  uint64_t* info;               // 8 u64 per file
  uint64_t* file_block;         // n_files + 1
  uint64_t* file_key;           // n_files + 1
  uint64_t* ck;                 // n_ck checkpoints of 2 u64
  uint64_t n_ck;
  uint64_t* ext;
  uint64_t* first_pos;
  uint8_t* first_keys;
  uint64_t block_cap;
  uint64_t key_cap;
};
void launch_open_index(const OpenIndexLaunch& a, hipStream_t stream);
void launch_open_metas(const OpenIndexLaunch& a, hipStream_t stream);

// tpz_table_runs_layout / tpz_table_runs_entries (tpz_runs.hip): resident tables as merge runs.
// h_block_first: host, n_runs + 1, checked by the caller; first: 3 x (B + 1) u64; part =
// flat_scan_parts_words(B) u64 of device scratch. aligned: the aligned-load form of the gather
// (the diagnostic export's; false: copydev::wave_copy, the product's).
void launch_table_runs_layout(const tpz_table* tabs, uint32_t n_runs, const uint32_t* h_block_first,
                              uint64_t* first, uint32_t* run_first, uint64_t* info, uint64_t* part,
                              hipStream_t stream);
void launch_table_runs_entries(const tpz_table* tabs, uint32_t n_runs, const uint32_t* h_block_first,
                               const uint64_t* first, uint8_t* keys, uint64_t key_cap, uint64_t* kpos,
                               uint8_t* vals, uint64_t val_cap, uint64_t* vpos, uint64_t entry_cap,
                               bool aligned, hipStream_t stream);

// tpz_compress_blocks (tpz_compress.hip): scratch bytes for the per-block slots; the snappy
// encode, the scan of the sizes into dst_ext and the packing into dst.
uint64_t compress_scratch_bytes(uint64_t src_bytes, uint32_t n_blocks);
void launch_compress(const uint8_t* src, const uint64_t* ext, uint64_t src_bytes, uint32_t n_blocks,
                     uint32_t codec, uint8_t* scratch, uint64_t* dst_ext, uint64_t* part, uint8_t* dst,
                     uint32_t num_cus, hipStream_t stream);
void launch_flat_layout(const uint8_t* src, const uint64_t* ext, uint64_t src_bytes,
                        uint32_t n_blocks, uint64_t* first, uint64_t* part, uint32_t num_cus,
                        hipStream_t stream);
// tpz_verify_files_flat_layout (tpz_flat.hip): the whole-file CRC of n_files SST files (data
// region = blocks fblock[f] .. fblock[f + 1] - 1, then the tail) and the flat reservations of
// their data blocks from one read of the blocks.
struct OpenLaunch {
  const uint8_t* src;
  const uint64_t* bext;
  uint64_t src_bytes;
  uint32_t n_blocks;
  const uint32_t* fblock;   // n_files + 1
  uint32_t n_files;
  const uint8_t* tsrc;      // the files' tails (meta, bloom, offsets, trailer)
  const uint64_t* text;
  uint64_t tail_bytes;
  uint64_t* first;        // 3 x (n_blocks + 1)
  uint64_t* part;         // workspace: flat_scan_parts_words(n_blocks) u64
  uint32_t* cb;           // workspace: n_blocks
  uint32_t* tacc;         // workspace: n_files, zeroed (the tails' main-part R0, crc_window_kernel)
  const uint32_t* rep;    // the replicated slice-by-4 tables (crc_window_kernel)
  const uint32_t* dtab;   // decode tables
  const uint32_t* rtab;   // range tables
  uint32_t* crc;
  uint8_t* status;
  uint32_t num_cus;
};
void launch_open_flat(const OpenLaunch& a, hipStream_t stream);
void launch_entry_first(const uint8_t* src, const uint64_t* ext, uint64_t src_bytes,
                        uint32_t n_blocks, uint64_t* first, uint64_t* part, hipStream_t stream);
// first[i] = exclusive prefix of count over decoded (OK / OK_SPILLED) blocks, first[n] = total.
void launch_count_prefix(const uint32_t* count, const uint8_t* status, uint32_t n,
                         uint64_t* first, hipStream_t stream);

struct CodecLaunch {
  const uint8_t* src;
  const uint64_t* ext;
  uint64_t src_bytes;
  uint32_t n_blocks;
  uint64_t* size;          // tpz_decompressed_sizes output
  uint8_t* dst;            // tpz_decompress_blocks output
  const uint64_t* dst_ext;
  uint8_t* status;
  uint32_t* defer_list;    // workspace: n_blocks entries
  uint32_t* defer_count;   // workspace: zeroed before the launch
  uint32_t num_cus;
  bool claimed;            // tpz_decompressed_sizes_claimed
  uint32_t* inexact;       // workspace: sticky, read and cleared by tpz_decompress_check
};

void launch_codec_sizes(const CodecLaunch& a, hipStream_t stream);
void launch_decompress(const CodecLaunch& a, hipStream_t stream);

// The write side (tpz_encode.hip): block cuts (phase 0: nx + info; phase 1: the chain) and the
// block encode.
struct PlanLaunch {
  int phase;
  const uint64_t* kpos;
  const uint64_t* vpos;
  uint32_t n;
  uint32_t block_size;
  uint32_t* nx;        // workspace: n + 2 (n / 2048 + 1) (nx, per-workgroup maxima and bad entries)
  uint32_t* info;      // {max nx (w), first bad entry, n_blocks}: written by the kernels
  uint32_t w;          // phase 1: an upper bound of info[0] (the tables' row capacity)
  uint32_t chunk;      // phase 1: entries per chunk (>= w)
  int* tab_a;          // phase 1 workspace: 2 x K x w
  int* tab_b;
  uint32_t* cnt;       // phase 1 workspace: K
  uint32_t* first;
  uint64_t* ext;
  uint32_t* n_blocks;  // workspace: one u32
};
hipError_t launch_plan(const PlanLaunch& a, hipStream_t stream);
constexpr uint32_t kPlanChunk = 2048;  // minimum entries per plan chunk
constexpr uint32_t kPlanNextPer = 4096; // entries per plan_next_kernel workgroup

struct EncodeLaunch {
  const uint8_t* keys;
  const uint64_t* kpos;
  uint64_t key_bytes;
  const uint8_t* vals;
  const uint64_t* vpos;
  uint64_t val_bytes;
  const uint32_t* first;
  const uint64_t* ext;
  uint32_t n_blocks;            // or its bound, when plan_info is set
  const uint32_t* plan_info;    // tpz_plan_blocks_async's d_info (block count on the device), or null
  const uint32_t* crc_tables;
  uint8_t* out;
  uint32_t* big_list;   // workspace: n_blocks
  uint32_t* big_count;  // workspace: one u32
  uint32_t num_cus;
};
hipError_t launch_encode(const EncodeLaunch& a, hipStream_t stream);

}  // namespace tpz

// tpz_scan.hip — gfx950 kernels of the batched LsmStorage::scan (src/lsm_storage.rs:335-374) over
// tables resident in HBM: its SST half (tpz_scan_ranges, tpz_scan_entries; include/tpz_gpu.h) and
// the whole scan, memtable runs merged in (tpz_lsm_scan_ranges, tpz_lsm_scan_entries;
// tpz_level_scan_entries is the same gather). One launcher per operation picks the kernels by
// flavour; the level flavour's ranges call goes on to tpz_levelscan.hip.
//
//   scan_seek_kernel     One thread per (scan, table), the threads of a scan adjacent in priority
//                        order (L0 newest first, then the levels as stored: level.rs:538-579). It
//                        checks that the reference could have opened the table (its biggest key
//                        is the last entry of the last block, table.rs:143-151), applies the
//                        filter (dropped iff biggest_key < lower or smallest_key > upper), seeks
//                        the lower bound (tpz_seek_dev.h seek_table; block 0 / entry 0 for
//                        Unbounded) and takes the Excluded / After step. It stores the cursor
//                        (block, entry; 0xFFFFFFFF: dropped or invalid) and a status byte (non-OK:
//                        where the reference fails, the cursor then naming the block and entry).
//   scan_merge_kernel    One wave per scan, one cursor per lane in priority order (hence at most
//                        64 tables). A step: the wave's minimum (key, lane) by an 8-byte
//                        big-endian prefix reduced with shuffles, the full comparison only among
//                        the lanes a ballot shows tied on it; the end check (not on element 0
//                        unless the lower kind is After: LsmIterator::new, lsm_iterator.rs:22-33);
//                        the tombstone rule; the leader's lane records the hit; then
//                        MergeIterator::next (merge_iterator.rs:73-105): every other lane at an
//                        equal key moves on until its key differs, the leader takes one step. A
//                        cursor only moves forward, so the loops end with the tables' entries.
//   (scan)               The scans' entry counts, key bytes and value bytes become d_first,
//                        d_key_first and d_val_first with launch_scan_u64 (tpz_flat.hip).
//   scan_entries_kernel  One wave per scan, twice: a length pass (the scan's key and value bytes,
//                        scanned into per-scan bases), then the pass that writes d_kpos / d_vpos
//                        and copies keys and values in 16-byte pieces of the destination
//                        (tpz_copy.h, as get_gather_kernel): by their own lane up to kLaneCopyMax
//                        bytes, longer ones by the whole wave.
//   lsm_scan_*_kernel    The same three kernels with the memtable side, from the same bodies
//                        (tpz_scan_dev.h, kMem): the seek pass also bisects every run twice per
//                        scan (map.range's two ends), the merge gives lanes 0 .. n_runs - 1 to the
//                        runs, newest first, and takes TwoMergeIterator's eager step (the SST
//                        cursors leave a key a run holds before that key is looked at), and the
//                        gather reads run entries too.
//
// No kernel needs a workgroup barrier. The gather trusts nothing it is handed: table, block and
// entry are checked against the descriptors, counts are clamped to `limit` and to d_first's total,
// and every copy is clipped to its capacity.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "tpz_copy.h"
#include "tpz_internal.h"
#include "tpz_scan_dev.h"

namespace tpz {

namespace {

using scandev::EntriesParams;
using scandev::kWaves;
using scandev::MergeParams;
using scandev::SeekParams;
using seekdev::u32;
using seekdev::u64;

// The bodies are tpz_scan_dev.h's, without the memtable side (the lsm_scan_* kernels below run
// them with it).
__global__ __launch_bounds__(256) void scan_seek_kernel(SeekParams p) {
  scandev::seek_body<false>(p, scandev::Runs{nullptr, 0});
}

__global__ __launch_bounds__(256) void scan_merge_kernel(MergeParams p) {
  scandev::merge_body<false>(p, scandev::Runs{nullptr, 0});
}

__global__ void scan_info_kernel(const u64* first, const u64* key_first, const u64* val_first,
                                 u32 n_scans, u64* info) {
  if (threadIdx.x == 0) {
    info[0] = first[n_scans];
    info[1] = key_first[n_scans];
    info[2] = val_first[n_scans];
  }
}

template <bool kCopy>
__global__ __launch_bounds__(256) void scan_entries_kernel(EntriesParams p) {
  scandev::entries_body<kCopy, false>(p, scandev::Runs{nullptr, 0});
}

// LsmStorage::scan whole: the same bodies with the memtable side.
struct LsmSeekParams {
  scandev::SeekParams s;
  scandev::Runs m;
};
__global__ __launch_bounds__(256) void lsm_scan_seek_kernel(LsmSeekParams p) {
  scandev::seek_body<true>(p.s, p.m);
}

struct LsmMergeParams {
  scandev::MergeParams s;
  scandev::Runs m;
};
__global__ __launch_bounds__(256) void lsm_scan_merge_kernel(LsmMergeParams p) {
  scandev::merge_body<true>(p.s, p.m);
}

struct LsmEntriesParams {
  scandev::EntriesParams s;
  scandev::Runs m;
};
template <bool kCopy>
__global__ __launch_bounds__(256) void lsm_scan_entries_kernel(LsmEntriesParams p) {
  scandev::entries_body<kCopy, true>(p.s, p.m);
}

}  // namespace

uint64_t scan_ranges_work_bytes(uint32_t n_scans, uint32_t n_cursors) {
  return scandev::cursor_work_bytes(n_scans, (uint64_t)n_scans * n_cursors, 2);
}

uint64_t scan_entries_work_bytes(uint32_t n_scans) {
  return 8 * (2 * ((uint64_t)n_scans + 1) + flat_scan_parts_words(n_scans) / 3);
}

void launch_scan_totals(const ScanLaunch& a, uint64_t* part, hipStream_t stream) {
  launch_scan_u64(a.first, a.n_scans, part, stream);
  launch_scan_u64(a.key_first, a.n_scans, part, stream);
  launch_scan_u64(a.val_first, a.n_scans, part, stream);
  hipLaunchKernelGGL(scan_info_kernel, dim3(1), dim3(64), 0, stream, a.first, a.key_first,
                     a.val_first, a.n_scans, a.info);
}

void launch_scan_ranges(const ScanLaunch& a, hipStream_t stream) {
  if (a.flavour == Flavour::kLevel) return launch_level_scan_ranges(a, stream);
  const bool mem = a.flavour == Flavour::kLsm;
  const uint64_t cells = (uint64_t)a.n_scans * (a.n_tables + (mem ? a.n_runs : 0u));
  const scandev::CursorWork w = scandev::carve_cursors(a.work, cells, 2);
  const SeekParams sp = scandev::seek_params(a, w);
  const MergeParams mp = scandev::merge_params(a, w);
  const scandev::Runs m{a.runs, a.n_runs};
  const dim3 seek_grid((u32)((cells + 255) / 256)), merge_grid((a.n_scans + kWaves - 1) / kWaves);
  if (mem) {
    const LsmSeekParams ls{sp, m};
    const LsmMergeParams lm{mp, m};
    if (cells) hipLaunchKernelGGL(lsm_scan_seek_kernel, seek_grid, dim3(256), 0, stream, ls);
    hipLaunchKernelGGL(lsm_scan_merge_kernel, merge_grid, dim3(256), 0, stream, lm);
  } else {
    if (cells) hipLaunchKernelGGL(scan_seek_kernel, seek_grid, dim3(256), 0, stream, sp);
    hipLaunchKernelGGL(scan_merge_kernel, merge_grid, dim3(256), 0, stream, mp);
  }
  launch_scan_totals(a, w.part, stream);
}

void launch_scan_entries(const ScanEntriesLaunch& a, hipStream_t stream) {
  u64* kbase = static_cast<u64*>(a.work);
  u64* vbase = kbase + a.n_scans + 1;
  u64* part = vbase + a.n_scans + 1;
  const EntriesParams p{a.tabs, a.n_tables, a.n_scans, a.limit, a.hit_table, a.hit_block,
                        a.hit_entry, a.first, kbase, vbase, a.keys, a.key_cap, a.kpos, a.vals,
                        a.val_cap, a.vpos};
  const LsmEntriesParams lp{p, {a.runs, a.n_runs}};
  const bool mem = a.flavour != Flavour::kTables;   // kLsm and kLevel: hits in runs too
  const dim3 grid((a.n_scans + kWaves - 1) / kWaves);
  auto pass = [&](auto copy) {
    constexpr bool kCopy = decltype(copy)::value;
    if (mem)
      hipLaunchKernelGGL(lsm_scan_entries_kernel<kCopy>, grid, dim3(256), 0, stream, lp);
    else
      hipLaunchKernelGGL(scan_entries_kernel<kCopy>, grid, dim3(256), 0, stream, p);
  };
  pass(std::false_type{});                          // the lengths
  launch_scan_u64(kbase, a.n_scans, part, stream);
  launch_scan_u64(vbase, a.n_scans, part, stream);
  pass(std::true_type{});                           // the positions and the copies
}

}  // namespace tpz

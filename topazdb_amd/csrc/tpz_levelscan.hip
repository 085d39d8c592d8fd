// tpz_levelscan.hip — gfx950 kernels of the level scan (tpz_level_scan_ranges; include/tpz_gpu.h):
// LsmStorage::scan (src/lsm_storage.rs:335-374) over memtable runs plus resident tables with one
// merge cursor per run, per L0 table and per non-empty level below L0, so a level may hold any
// number of tables. tpz_level_scan_entries is tpz_mem.hip's gather (launch_lsm_scan_entries).
//
//   level_index_kernel   One thread per table, once per call: can the reference open it and its
//                        biggest key (table.rs:143-151), and its head records (tpz_levelscan_dev.h).
//   level_links_kernel   One wave per non-empty level below L0: per table the next failing and the
//                        next valid head at or after it; one more wave finds the first table that
//                        cannot be opened, in priority order.
//   level_seek_kernel    One thread per (scan, cursor). A level's cursor bisects the smallest keys
//                        for the surviving tables T[a..z] (level_tables_sorted's filter over a
//                        sorted, disjoint level), seeks T[a] as scan_seek_kernel seeks a table, and
//                        reads two links: a failing head in (a, z] fails the scan as the reference's
//                        cursor creation does, and a T[a] left invalid starts at the next valid head.
//   level_merge_kernel   tpz_scan_dev.h's merge_body with kLvl: one wave per scan, one cursor per
//                        lane; a level's lane enters the next table when its table ends.
//
// Workspace (the stream's scan buffer): the index (40 B per table), the links (4 u32 per table),
// the first unopenable table (one u32, padded to 16 B), then per scan and cursor 16 B and a
// status byte, and the scans' partial sums.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"
#include "tpz_levelscan_dev.h"
#include "tpz_scan_dev.h"

namespace tpz {

namespace {

using lvldev::Shape;
using scandev::Levels;
using scandev::TabIndex;
using seekdev::u32;
using seekdev::u64;

__global__ __launch_bounds__(256) void level_index_kernel(Shape s, TabIndex* idx) {
  lvldev::index_body(s, idx);
}

__global__ __launch_bounds__(64) void level_links_kernel(Shape s, const TabIndex* idx, u32* nf,
                                                         u32* nv, u32* first_unopened) {
  lvldev::links_body(s, idx, nf, nv, first_unopened);
}

struct LevelSeekParams {
  scandev::SeekParams s;
  scandev::Runs m;
  Shape shape;
  Levels lv;
};
__global__ __launch_bounds__(256) void level_seek_kernel(LevelSeekParams p) {
  lvldev::seek_body<true>(p.s, p.m, p.shape, p.lv);
}

struct LevelMergeParams {
  scandev::MergeParams s;
  scandev::Runs m;
  Levels lv;
};
__global__ __launch_bounds__(256) void level_merge_kernel(LevelMergeParams p) {
  scandev::merge_body<true, true>(p.s, p.m, p.lv);
}

uint64_t up8(uint64_t x) { return (x + 7) & ~7ull; }
uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

}  // namespace

uint64_t level_scan_cursors(const uint32_t* level_first, uint32_t n_levels, uint32_t n_runs) {
  uint64_t n = (uint64_t)n_runs + (n_levels ? level_first[1] : 0u);
  for (uint32_t l = 1; l < n_levels; l++) n += level_first[l + 1] > level_first[l];
  return n;
}

uint64_t level_scan_work_bytes(uint32_t n_scans, uint32_t n_cursors, uint32_t n_tables) {
  const uint64_t cells = (uint64_t)n_scans * n_cursors;
  return up16(sizeof(TabIndex) * (uint64_t)n_tables) + 16 * (uint64_t)n_tables + 16 + 16 * cells +
         up8(cells) + 8 * (flat_scan_parts_words(n_scans) / 3);
}

void launch_level_scan_ranges(const LevelScanLaunch& l, hipStream_t stream) {
  const ScanLaunch& a = l.lsm.scan;
  Shape sh{};
  sh.tabs = a.tabs;
  sh.n_tables = a.n_tables;
  sh.l0 = a.l0;
  sh.cf[0] = a.l0;
  for (u32 lv = 1; lv < l.n_levels; lv++)
    if (l.level_first[lv + 1] > l.level_first[lv]) sh.cf[++sh.n_lv] = l.level_first[lv + 1];
  for (u32 k = sh.n_lv + 1; k <= TPZ_GET_MAX_LEVELS; k++) sh.cf[k] = a.n_tables;
  const u32 n_cur = l.lsm.n_runs + a.l0 + sh.n_lv;
  const uint64_t cells = (uint64_t)a.n_scans * n_cur;

  uint8_t* w = static_cast<uint8_t*>(a.work);
  TabIndex* idx = reinterpret_cast<TabIndex*>(w);
  w += up16(sizeof(TabIndex) * (uint64_t)a.n_tables);
  u32* nf = reinterpret_cast<u32*>(w);
  u32* nv = nf + 2 * (uint64_t)a.n_tables;
  w += 16 * (uint64_t)a.n_tables;
  u32* first_unopened = reinterpret_cast<u32*>(w);
  w += 16;                                       // (the cursors are read 16 bytes at a time)
  u32* cur = reinterpret_cast<u32*>(w);
  w += 16 * cells;
  uint8_t* cst = w;
  u64* part = reinterpret_cast<u64*>(w + up8(cells));

  if (a.n_tables)
    hipLaunchKernelGGL(level_index_kernel, dim3((a.n_tables + 255) / 256), dim3(256), 0, stream, sh,
                       idx);
  if (l.stop_after == 1) return;
  hipLaunchKernelGGL(level_links_kernel, dim3(sh.n_lv + 1), dim3(64), 0, stream, sh, idx, nf, nv,
                     first_unopened);
  if (l.stop_after == 2) return;
  const scandev::Runs m{l.lsm.runs, l.lsm.n_runs};
  const Levels lv{a.tabs, a.n_tables, idx, nf, nv, first_unopened, n_cur};
  if (cells) {
    LevelSeekParams s{{a.tabs, a.n_tables, a.l0, a.lo, a.lo_pos, a.lo_kind, a.hi, a.hi_pos,
                       a.hi_kind, a.n_scans, cur, cst}, m, sh, lv};
    hipLaunchKernelGGL(level_seek_kernel, dim3((u32)((cells + 255) / 256)), dim3(256), 0, stream,
                       s);
  }
  LevelMergeParams mp{{a.tabs, a.n_tables, a.l0, a.hi, a.hi_pos, a.lo_kind, a.hi_kind, a.n_scans,
                       a.limit, cur, cst, a.result, a.status, a.where, a.hit_table, a.hit_block,
                       a.hit_entry, a.first, a.key_first, a.val_first}, m, lv};
  hipLaunchKernelGGL(level_merge_kernel,
                     dim3((a.n_scans + scandev::kWaves - 1) / scandev::kWaves), dim3(256), 0, stream,
                     mp);
  launch_scan_totals(a, part, stream);
}

}  // namespace tpz

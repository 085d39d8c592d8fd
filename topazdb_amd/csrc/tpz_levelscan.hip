// tpz_levelscan.hip — gfx950 kernels of the level scan (tpz_level_scan_ranges; include/tpz_gpu.h):
// LsmStorage::scan (src/lsm_storage.rs:335-374) over memtable runs plus resident tables with one
// merge cursor per run, per L0 table and per non-empty level below L0, so a level may hold any
// number of tables. launch_scan_ranges (tpz_scan.hip) hands the level flavour's ScanLaunch on to
// launch_level_scan_ranges here; tpz_level_scan_entries is tpz_scan.hip's gather with the runs.
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

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

}  // namespace

uint64_t level_scan_cursors(const uint32_t* level_first, uint32_t n_levels, uint32_t n_runs) {
  uint64_t n = (uint64_t)n_runs + (n_levels ? level_first[1] : 0u);
  for (uint32_t l = 1; l < n_levels; l++) n += level_first[l + 1] > level_first[l];
  return n;
}

uint64_t level_scan_work_bytes(uint32_t n_scans, uint32_t n_cursors, uint32_t n_tables) {
  return up16(sizeof(TabIndex) * (uint64_t)n_tables) + 16 * (uint64_t)n_tables + 16 +
         scandev::cursor_work_bytes(n_scans, (uint64_t)n_scans * n_cursors, 4);
}

void launch_level_scan_ranges(const ScanLaunch& a, hipStream_t stream) {
  Shape sh{};
  sh.tabs = a.tabs;
  sh.n_tables = a.n_tables;
  sh.l0 = a.l0();
  sh.cf[0] = a.l0();
  for (u32 lv = 1; lv < a.n_levels; lv++)
    if (a.level_first[lv + 1] > a.level_first[lv]) sh.cf[++sh.n_lv] = a.level_first[lv + 1];
  for (u32 k = sh.n_lv + 1; k <= TPZ_GET_MAX_LEVELS; k++) sh.cf[k] = a.n_tables;
  const u32 n_cur = a.n_runs + a.l0() + sh.n_lv;
  const uint64_t cells = (uint64_t)a.n_scans * n_cur;

  uint8_t* w = static_cast<uint8_t*>(a.work);
  TabIndex* idx = reinterpret_cast<TabIndex*>(w);
  w += up16(sizeof(TabIndex) * (uint64_t)a.n_tables);
  u32* nf = reinterpret_cast<u32*>(w);
  u32* nv = nf + 2 * (uint64_t)a.n_tables;
  w += 16 * (uint64_t)a.n_tables;
  u32* first_unopened = reinterpret_cast<u32*>(w);
  w += 16;                                       // (the cursors are read 16 bytes at a time)
  const scandev::CursorWork cw = scandev::carve_cursors(w, cells, 4);

  if (a.n_tables)
    hipLaunchKernelGGL(level_index_kernel, dim3((a.n_tables + 255) / 256), dim3(256), 0, stream, sh,
                       idx);
  if (a.stop_after == 1) return;
  hipLaunchKernelGGL(level_links_kernel, dim3(sh.n_lv + 1), dim3(64), 0, stream, sh, idx, nf, nv,
                     first_unopened);
  if (a.stop_after == 2) return;
  const scandev::Runs m{a.runs, a.n_runs};
  const Levels lv{a.tabs, a.n_tables, idx, nf, nv, first_unopened, n_cur};
  if (cells) {
    const LevelSeekParams s{scandev::seek_params(a, cw), m, sh, lv};
    hipLaunchKernelGGL(level_seek_kernel, dim3((u32)((cells + 255) / 256)), dim3(256), 0, stream,
                       s);
  }
  const LevelMergeParams mp{scandev::merge_params(a, cw), m, lv};
  hipLaunchKernelGGL(level_merge_kernel,
                     dim3((a.n_scans + scandev::kWaves - 1) / scandev::kWaves), dim3(256), 0, stream,
                     mp);
  launch_scan_totals(a, cw.part, stream);
}

}  // namespace tpz

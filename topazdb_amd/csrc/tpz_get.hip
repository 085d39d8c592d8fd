// tpz_get.hip — gfx950 kernels of the batched LevelController::get (src/level.rs:427-465) over
// tables resident in HBM (tpz_get_keys, tpz_get_values; include/tpz_gpu.h), and of the batched
// LsmStorage::get (src/lsm_storage.rs:198-213) over memtable runs plus those tables
// (tpz_lsm_get_keys, tpz_lsm_get_values). One launcher per operation picks the kernel by flavour.
//
//   get_walk_kernel    One thread per query: the walk over L0 (newest table first) and then one
//                      table per level (the partition point of the level's smallest keys), with
//                      SsTable::may_contain and SsTableIterator::seek_to_key in every table tried
//                      (tpz_seek_dev.h: the routines of bloom_kernel and seek_kernel), the
//                      equality test and the tombstone rule. The key is hashed at most once, before
//                      the walk and only when some table has a filter (hashed where the walk first
//                      needs it, the hash's registers add to the seek's: 94 VGPRs and 5 waves per
//                      SIMD, against 58 and 8). Like the seek it is a chain of dependent loads;
//                      the query count supplies the parallelism. Every lane of a wave takes
//                      the walk's steps in the same order (step s < |L0| is L0 table |L0|-1-s for
//                      all of them, so those descriptor reads are one address per wave); a lane
//                      whose get has ended sits the rest out. Table descriptors are read from the
//                      array in HBM field by field where the seek uses them, never copied.
//   (scan)             The value lengths become d_val_pos with launch_scan_u64 (tpz_flat.hip).
//   get_gather_kernel  The value of every FOUND query, located in its block's slot or spill record
//                      as the seek locates keys, copied to d_vals in 16-byte pieces of the
//                      destination (tpz_copy.h, as merge_gather_kernel): by its own lane up to
//                      kLaneCopyMax bytes, longer ones by the whole wave.
//   (lsm_get_walk_kernel   is tpz_mem.hip's, launched from here: compiled next to get_walk_kernel
//                          its code comes out different, so it stayed in its file.)
//   lsm_get_gather_kernel  get_gather_kernel with a second source: a hit whose table carries
//                          TPZ_HIT_MEM is entry d_entry of that run, checked against the run
//                          descriptors; copies are clipped to val_cap.
//
// Nothing here trusts the level order or the positions it is handed: the bisections are bounded
// by the table counts, and the gather checks table, block and entry against the descriptors and
// clips every copy to val_cap.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_get_dev.h"
#include "tpz_internal.h"
#include "tpz_mem_dev.h"

namespace tpz {

namespace {

using getdev::GatherParams;
using getdev::kNone;
using getdev::WalkParams;
using seekdev::u32;
using seekdev::u64;

// The walk and the value's location are tpz_get_dev.h's (tpz_mem.hip runs the same walk after the
// memtable runs).
__global__ __launch_bounds__(256, 8) void get_walk_kernel(WalkParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool any_filter = getdev::any_filter(p);
  if (i >= p.n_q) return;
  const u64 qa = p.q_pos[i];
  getdev::WalkOut o{TPZ_GET_ABSENT, TPZ_BLOCK_OK, getdev::kNone, getdev::kNone, getdev::kNone, 0};
  getdev::walk(p, p.q + qa, p.q_pos[i + 1] - qa, any_filter, o);
  getdev::store(p, i, o);
}

__global__ __launch_bounds__(256) void get_gather_kernel(GatherParams p) {
  const u32 lane = copydev::lane_id();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 queries are consecutive)
  const uint8_t* src = nullptr;
  u64 len = 0, d = 0;
  if (i < p.n_q && p.result[i] == TPZ_GET_FOUND) {
    src = getdev::table_value(p.tabs, p.n_tables, p.table[i], p.block[i], p.entry[i], len);
    if (src) {
      d = p.val_pos[i];
      const u64 room = p.val_pos[i + 1] - d;      // the range tpz_get_keys gave this value
      if (len > room) len = room;
    }
  }
  getdev::copy_values(p.vals, p.val_cap, d, src, len, lane);
}

struct LsmGatherParams {
  getdev::GatherParams g;
  const tpz_mem_run* runs;
  u32 n_runs;
};

__global__ __launch_bounds__(256) void lsm_get_gather_kernel(LsmGatherParams p) {
  const u32 lane = copydev::lane_id();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 queries are consecutive)
  const uint8_t* src = nullptr;
  u64 len = 0, d = 0;
  if (i < p.g.n_q && p.g.result[i] == TPZ_GET_FOUND) {
    const u32 t = p.g.table[i], j = p.g.entry[i];
    if (t != kNone && (t & TPZ_HIT_MEM)) {
      const u32 r = t & ~TPZ_HIT_MEM;
      if (r < p.n_runs && j < p.runs[r].entries.n_entries)
        src = memdev::run_value(p.runs[r].entries, j, len);
    } else {
      src = getdev::table_value(p.g.tabs, p.g.n_tables, t, p.g.block[i], j, len);
    }
    if (src) {
      d = p.g.val_pos[i];
      const u64 room = p.g.val_pos[i + 1] - d;     // the range tpz_lsm_get_keys gave this value
      if (len > room) len = room;
    } else {
      len = 0;
    }
  }
  getdev::copy_values(p.g.vals, p.g.val_cap, d, src, len, lane);
}

}  // namespace

void launch_get_walk(const GetLaunch& a, hipStream_t stream) {
  if (a.kind == TableKind::kRaw) return launch_raw_get_walk(a, stream);   // tpz_raw.hip
  WalkParams p{};
  p.tabs = static_cast<const tpz_get_table*>(a.tabs);
  p.n_tables = a.n_tables;
  p.n_levels = a.n_levels;
  for (u32 l = 0; l <= TPZ_GET_MAX_LEVELS; l++)
    p.level_first[l] = a.n_levels ? a.level_first[l < a.n_levels ? l : a.n_levels] : 0u;
  p.q = a.q;
  p.q_pos = a.q_pos;
  p.n_q = a.n_q;
  p.result = a.result;
  p.status = a.status;
  p.table = a.table;
  p.block = a.block;
  p.entry = a.entry;
  p.val_len = a.val_pos;
  const dim3 grid((a.n_q + 255) / 256);
  if (a.flavour == Flavour::kLsm)
    getdev::launch_lsm_walk_kernel(p, a.runs, a.n_runs, grid, stream);
  else
    hipLaunchKernelGGL(get_walk_kernel, grid, dim3(256), 0, stream, p);
  launch_scan_u64(a.val_pos, a.n_q, a.part, stream);
}

void launch_get_gather(const GetGatherLaunch& a, hipStream_t stream) {
  if (a.kind == TableKind::kRaw) return launch_raw_get_gather(a, stream);   // tpz_raw.hip
  const GatherParams p{static_cast<const tpz_get_table*>(a.tabs), a.n_tables, a.n_q, a.result, a.table, a.block, a.entry, a.val_pos,
                       a.vals, a.val_cap};
  const dim3 grid((a.n_q + 255) / 256);
  if (a.flavour == Flavour::kLsm) {
    const LsmGatherParams lp{p, a.runs, a.n_runs};
    hipLaunchKernelGGL(lsm_get_gather_kernel, grid, dim3(256), 0, stream, lp);
  } else {
    hipLaunchKernelGGL(get_gather_kernel, grid, dim3(256), 0, stream, p);
  }
}

}  // namespace tpz

// tpz_mem.hip — gfx950 kernels over memtable runs resident in HBM (tpz_mem_run: one memtable's
// sorted snapshot; include/tpz_gpu.h): tpz_mem_prefix, the batched LsmStorage::get
// (src/lsm_storage.rs:198-213) over runs plus tables (tpz_lsm_get_keys, tpz_lsm_get_values) and
// the batched LsmStorage::scan, whole (:335-374; tpz_lsm_scan_ranges, tpz_lsm_scan_entries).
//
//   mem_prefix_kernel      One thread per entry: the key's first 8 bytes, big-endian, zero padded
//                          (tpz_mem_dev.h key_prefix): the column the bisections of a run read.
//   lsm_get_walk_kernel    One thread per query. The memtables first, newest first (the runs from
//                          n_runs - 1 down to 0, MemTable::get = an exact match: tpz_mem_dev.h
//                          run_find), every lane of a wave taking the runs in the same order, so
//                          the descriptor reads are one address per wave; a lane that has its
//                          answer sits the rest out. A query no run answers takes get_walk_kernel's
//                          walk (tpz_get_dev.h), in the same launch. An empty key is the
//                          reference's assert (lsm_storage.rs:199).
//   (scan)                 The value lengths become d_val_pos with launch_scan_u64 (tpz_flat.hip).
//   lsm_get_gather_kernel  get_gather_kernel with a second source: a hit whose table carries
//                          TPZ_HIT_MEM is entry d_entry of that run, checked against the run
//                          descriptors; copies are clipped to val_cap.
//   lsm_scan_*_kernel      The scan's three kernels (tpz_scan.hip) with the memtable side, from the
//                          same bodies (tpz_scan_dev.h, kMem): the seek pass also bisects every
//                          run twice per scan (map.range's two ends), the merge gives lanes
//                          0 .. n_runs - 1 to the runs, newest first, and takes TwoMergeIterator's
//                          eager step (the SST cursors leave a key a run holds before that key is
//                          looked at), and the gather reads run entries too.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_get_dev.h"
#include "tpz_internal.h"
#include "tpz_mem_dev.h"
#include "tpz_scan_dev.h"

namespace tpz {

namespace {

using getdev::kNone;
using seekdev::u32;
using seekdev::u64;

__global__ __launch_bounds__(256) void mem_prefix_kernel(tpz_entries e, u64* prefix) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= e.n_entries) return;
  u64 kl;
  const uint8_t* k = memdev::run_key(e, i, kl);
  prefix[i] = memdev::key_prefix(k, kl);
}

struct LsmWalkParams {
  getdev::WalkParams w;
  const tpz_mem_run* runs;
  u32 n_runs;
};

__global__ __launch_bounds__(256, 8) void lsm_get_walk_kernel(LsmWalkParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool any_filter = getdev::any_filter(p.w);
  if (i >= p.w.n_q) return;
  const u64 qa = p.w.q_pos[i];
  const uint8_t* qk = p.w.q + qa;
  const u64 ql = p.w.q_pos[i + 1] - qa;
  getdev::WalkOut o{TPZ_GET_ABSENT, TPZ_BLOCK_OK, kNone, kNone, kNone, 0};
  if (ql == 0) {                                 // assert!(!key.is_empty()) (lsm_storage.rs:199)
    o.res = TPZ_GET_ERROR;
    o.st = TPZ_BLOCK_MALFORMED;
  } else {
    const u64 qp = memdev::key_prefix(qk, ql);
    for (u32 r = p.n_runs; r-- > 0;) {           // view().iter().rev(): the mutable one first
      const tpz_mem_run& run = p.runs[r];
      const u32 j = memdev::run_find(run, qk, ql, qp);
      if (j == kNone) continue;
      memdev::run_value(run.entries, j, o.vlen);
      o.res = o.vlen ? TPZ_GET_FOUND : TPZ_GET_DELETED;   // :203-208: an empty value is deleted
      o.tb = TPZ_HIT_MEM | r;
      o.blk = 0;
      o.ent = j;
      break;
    }
    if (o.tb == kNone) getdev::walk(p.w, qk, ql, any_filter, o);
  }
  getdev::store(p.w, i, o);
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

// LsmStorage::scan whole: the scan's bodies (tpz_scan_dev.h) with the memtable side.
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

void launch_mem_prefix(const tpz_entries& e, uint64_t* prefix, hipStream_t stream) {
  hipLaunchKernelGGL(mem_prefix_kernel, dim3((e.n_entries + 255) / 256), dim3(256), 0, stream, e,
                     prefix);
}

void launch_lsm_get_walk(const LsmGetLaunch& l, hipStream_t stream) {
  const GetLaunch& a = l.get;
  LsmWalkParams p{};
  p.w.tabs = a.tabs;
  p.w.n_tables = a.n_tables;
  p.w.n_levels = a.n_levels;
  for (u32 lv = 0; lv <= TPZ_GET_MAX_LEVELS; lv++)
    p.w.level_first[lv] = a.n_levels ? a.level_first[lv < a.n_levels ? lv : a.n_levels] : 0u;
  p.w.q = a.q;
  p.w.q_pos = a.q_pos;
  p.w.n_q = a.n_q;
  p.w.result = a.result;
  p.w.status = a.status;
  p.w.table = a.table;
  p.w.block = a.block;
  p.w.entry = a.entry;
  p.w.val_len = a.val_pos;
  p.runs = l.runs;
  p.n_runs = l.n_runs;
  hipLaunchKernelGGL(lsm_get_walk_kernel, dim3((a.n_q + 255) / 256), dim3(256), 0, stream, p);
  launch_scan_u64(a.val_pos, a.n_q, a.part, stream);
}

void launch_lsm_get_gather(const LsmGetGatherLaunch& l, hipStream_t stream) {
  const GetGatherLaunch& a = l.get;
  LsmGatherParams p{{a.tabs, a.n_tables, a.n_q, a.result, a.table, a.block, a.entry, a.val_pos,
                     a.vals, a.val_cap}, l.runs, l.n_runs};
  hipLaunchKernelGGL(lsm_get_gather_kernel, dim3((a.n_q + 255) / 256), dim3(256), 0, stream, p);
}

void launch_lsm_scan_ranges(const LsmScanLaunch& l, hipStream_t stream) {
  const ScanLaunch& a = l.scan;
  const u32 n_cur = a.n_tables + l.n_runs;
  const uint64_t cells = (uint64_t)a.n_scans * n_cur;
  u32* cur = static_cast<u32*>(a.work);
  uint8_t* cst = reinterpret_cast<uint8_t*>(cur + 2 * cells);
  u64* part = reinterpret_cast<u64*>(cst + ((cells + 7) & ~7ull));
  const scandev::Runs m{l.runs, l.n_runs};
  if (cells) {
    LsmSeekParams s{{a.tabs, a.n_tables, a.l0, a.lo, a.lo_pos, a.lo_kind, a.hi, a.hi_pos,
                     a.hi_kind, a.n_scans, cur, cst}, m};
    hipLaunchKernelGGL(lsm_scan_seek_kernel, dim3((u32)((cells + 255) / 256)), dim3(256), 0, stream,
                       s);
  }
  LsmMergeParams mp{{a.tabs, a.n_tables, a.l0, a.hi, a.hi_pos, a.lo_kind, a.hi_kind, a.n_scans,
                     a.limit, cur, cst, a.result, a.status, a.where, a.hit_table, a.hit_block,
                     a.hit_entry, a.first, a.key_first, a.val_first}, m};
  hipLaunchKernelGGL(lsm_scan_merge_kernel,
                     dim3((a.n_scans + scandev::kWaves - 1) / scandev::kWaves), dim3(256), 0, stream,
                     mp);
  launch_scan_totals(a, part, stream);
}

void launch_lsm_scan_entries(const LsmScanEntriesLaunch& l, hipStream_t stream) {
  const ScanEntriesLaunch& a = l.scan;
  u64* kbase = static_cast<u64*>(a.work);
  u64* vbase = kbase + a.n_scans + 1;
  u64* part = vbase + a.n_scans + 1;
  LsmEntriesParams p{{a.tabs, a.n_tables, a.n_scans, a.limit, a.hit_table, a.hit_block,
                      a.hit_entry, a.first, kbase, vbase, a.keys, a.key_cap, a.kpos, a.vals,
                      a.val_cap, a.vpos}, {l.runs, l.n_runs}};
  const dim3 grid((a.n_scans + scandev::kWaves - 1) / scandev::kWaves);
  hipLaunchKernelGGL(lsm_scan_entries_kernel<false>, grid, dim3(256), 0, stream, p);
  launch_scan_u64(kbase, a.n_scans, part, stream);
  launch_scan_u64(vbase, a.n_scans, part, stream);
  hipLaunchKernelGGL(lsm_scan_entries_kernel<true>, grid, dim3(256), 0, stream, p);
}

}  // namespace tpz

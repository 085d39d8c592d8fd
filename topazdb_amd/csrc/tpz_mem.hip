// tpz_mem.hip — gfx950 kernels over memtable runs resident in HBM (tpz_mem_run: one memtable's
// sorted snapshot; include/tpz_gpu.h): tpz_mem_prefix, and the walk of the batched
// LsmStorage::get (src/lsm_storage.rs:198-213) over runs plus tables (tpz_lsm_get_keys). The rest
// of the queries over runs plus tables is with the tables' kernels: the get's gather and its
// launcher in tpz_get.hip, LsmStorage::scan in tpz_scan.hip.
//
//   mem_prefix_kernel      One thread per entry: the key's first 8 bytes, big-endian, zero padded
//                          (tpz_mem_dev.h key_prefix): the column the bisections of a run read.
//   lsm_get_walk_kernel    One thread per query. The memtables first, newest first (the runs from
//                          n_runs - 1 down to 0, MemTable::get = an exact match: tpz_mem_dev.h
//                          run_find), every lane of a wave taking the runs in the same order, so
//                          the descriptor reads are one address per wave; a lane that has its
//                          answer sits the rest out. A query no run answers takes get_walk_kernel's
//                          walk (tpz_get_dev.h), in the same launch. An empty key is the
//                          reference's assert (lsm_storage.rs:199). launch_get_walk (tpz_get.hip)
//                          launches it; the kernel stays in this file because its generated code
//                          changes when it is compiled next to get_walk_kernel.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_get_dev.h"
#include "tpz_internal.h"
#include "tpz_mem_dev.h"

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

}  // namespace

void launch_mem_prefix(const tpz_entries& e, uint64_t* prefix, hipStream_t stream) {
  hipLaunchKernelGGL(mem_prefix_kernel, dim3((e.n_entries + 255) / 256), dim3(256), 0, stream, e,
                     prefix);
}

void getdev::launch_lsm_walk_kernel(const WalkParams& w, const tpz_mem_run* runs, u32 n_runs,
                                    dim3 grid, hipStream_t stream) {
  const LsmWalkParams p{w, runs, n_runs};
  hipLaunchKernelGGL(lsm_get_walk_kernel, grid, dim3(256), 0, stream, p);
}

}  // namespace tpz

// tpz_raw.hip — gfx950 kernels over in-place tables (tpz_raw_table; include/tpz_gpu.h): resident
// tables whose encoded blocks are read where they lie in HBM, with no decoded columns.
// tpz_raw_verify, tpz_raw_seek_keys, tpz_raw_get_keys / tpz_raw_get_values and
// tpz_raw_lsm_get_keys / tpz_raw_lsm_get_values.
//
//   raw_verify_kernel      One thread per block, after the range CRC of tpz_crc.hip ran over the
//                          batch with trailer 5 (the payload's CRC, compared with the BE u32 behind
//                          it): the rest of what Block::decode checks before any entry is read
//                          (src/block/compress.rs:95-113: empty data, the tag; src/block.rs:49-59:
//                          the CRC split, n, the n offsets), in tpz_decode_blocks' order and with
//                          its d_crc conventions. A few byte loads per block.
//   raw_seek_kernel        seek_kernel (tpz_seek.hip) over a tpz_raw_table.
//   raw_get_walk_kernel    get_walk_kernel (tpz_get.hip), raw_lsm_get_walk_kernel its lsm flavour
//   raw_get_gather_kernel  (tpz_mem.hip's runs in front), and the two gathers. One lane per query.
//                          The routines are the decoded route's, instantiated for the in-place view
//                          (tpz_raw_dev.h): seekdev::seek_table, getdev::walk, level_table,
//                          table_value and copy_values; only the block view differs. A bisection
//                          step is offsets[mid] (2 byte loads), then klen (2 byte loads) with the
//                          key behind it, against the decoded view's {kend, vend} pair and the
//                          key; the value read adds vlen behind the key.
//
// They live in their own file: neighbours in a translation unit change each other's register
// allocation (lsm_get_walk_kernel, tpz_mem.hip). Resources (hipcc -O3, gfx950, from
// -Rpass-analysis=kernel-resource-usage; no kernel uses scratch; the gathers' 8 KiB of LDS are
// tpz_copy.h's wave_copy staging, as in get_gather_kernel), all at 8 waves per SIMD:
//   raw_get_walk_kernel        62 VGPRs (get_walk_kernel: 58)
//   raw_lsm_get_walk_kernel    62 VGPRs (lsm_get_walk_kernel: 64)
//   raw_seek_kernel            39 VGPRs (seek_kernel: 32)
//   raw_get_gather_kernel      32 VGPRs
//   raw_lsm_get_gather_kernel  34 VGPRs
//   raw_verify_kernel          10 VGPRs
// (profiles/rawget/resource_usage.txt)
//
// As in tpz_get.hip nothing trusts the level order or the positions handed in: bisections are
// bounded by the table, block and entry counts, the gathers check table, block and entry against
// the descriptors and clip every copy to val_cap, and the view reads no byte outside its block's
// extent.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_get_dev.h"
#include "tpz_internal.h"
#include "tpz_mem_dev.h"
#include "tpz_raw_dev.h"

namespace tpz {

namespace {

using getdev::kNone;
using getdev::RawGatherParams;
using getdev::RawWalkParams;
using seekdev::u32;
using seekdev::u64;

struct RawVerifyParams {
  const uint8_t* src;
  const u64* ext;
  u32 n_blocks;
  uint8_t* status;   // in: the range CRC's OK / CHECKSUM_MISMATCH / MALFORMED (len < 5)
  u32* crc;          // in: the payload's CRC (0 where len < 5)
};

__global__ __launch_bounds__(256) void raw_verify_kernel(RawVerifyParams p) {
  const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.n_blocks) return;
  const u64 e0 = p.ext[b], e1 = p.ext[b + 1];
  const u64 len = e1 > e0 ? e1 - e0 : 0;
  const uint8_t* blk = p.src + e0;
  const u32 tag = len ? blk[len - 1] : 0u;
  u32 st;
  if (len == 0) st = TPZ_BLOCK_EMPTY;                              // compress.rs:96-98
  else if (tag == 0 || tag > 3) st = TPZ_BLOCK_BAD_TAG;            // :44-53, :102
  else if (tag != 1) st = TPZ_BLOCK_UNSUPPORTED_CODEC;             // the codec step comes first
  else if (len - 1 < 4) st = TPZ_BLOCK_MALFORMED;                  // block.rs:49
  else {
    st = p.status[b];                                              // checksum.rs:17-21
    if (st != TPZ_BLOCK_CHECKSUM_MISMATCH) {
      const u64 P = len - 5;
      st = TPZ_BLOCK_OK;
      if (P < 2 || P < 2 + 2 * (u64)seekdev::raw_be16(blk)) st = TPZ_BLOCK_MALFORMED;   // :54-59
    }
    p.status[b] = (uint8_t)st;
    return;
  }
  p.status[b] = (uint8_t)st;
  p.crc[b] = 0;
}

struct RawSeekParams {
  tpz_raw_table t;
  const uint8_t* q;
  const u64* q_pos;
  u32 n_q;
  u32* out_block;
  u32* out_entry;
  uint8_t* out_status;
  uint8_t* out_valid;
};

__global__ __launch_bounds__(256) void raw_seek_kernel(RawSeekParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_q) return;
  const u64 a = p.q_pos[i];
  const seekdev::SeekPos r = seekdev::seek_table(p.t, p.q + a, p.q_pos[i + 1] - a);
  p.out_block[i] = r.block;
  p.out_entry[i] = r.entry;
  p.out_status[i] = (uint8_t)r.status;
  p.out_valid[i] = r.valid;
}

__global__ __launch_bounds__(256, 8) void raw_get_walk_kernel(RawWalkParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool any_filter = getdev::any_filter(p);
  if (i >= p.n_q) return;
  const u64 qa = p.q_pos[i];
  getdev::WalkOut o{TPZ_GET_ABSENT, TPZ_BLOCK_OK, kNone, kNone, kNone, 0};
  getdev::walk(p, p.q + qa, p.q_pos[i + 1] - qa, any_filter, o);
  getdev::store(p, i, o);
}

struct RawLsmWalkParams {
  RawWalkParams w;
  const tpz_mem_run* runs;
  u32 n_runs;
};

// lsm_get_walk_kernel (tpz_mem.hip): the memtable runs newest first, then the walk.
__global__ __launch_bounds__(256, 8) void raw_lsm_get_walk_kernel(RawLsmWalkParams p) {
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

__global__ __launch_bounds__(256) void raw_get_gather_kernel(RawGatherParams p) {
  const u32 lane = copydev::lane_id();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 queries are consecutive)
  const uint8_t* src = nullptr;
  u64 len = 0, d = 0;
  if (i < p.n_q && p.result[i] == TPZ_GET_FOUND) {
    src = getdev::table_value(p.tabs, p.n_tables, p.table[i], p.block[i], p.entry[i], len);
    if (src) {
      d = p.val_pos[i];
      const u64 room = p.val_pos[i + 1] - d;      // the range tpz_raw_get_keys gave this value
      if (len > room) len = room;
    }
  }
  getdev::copy_values(p.vals, p.val_cap, d, src, len, lane);
}

struct RawLsmGatherParams {
  RawGatherParams g;
  const tpz_mem_run* runs;
  u32 n_runs;
};

__global__ __launch_bounds__(256) void raw_lsm_get_gather_kernel(RawLsmGatherParams p) {
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
      const u64 room = p.g.val_pos[i + 1] - d;     // the range tpz_raw_lsm_get_keys gave this value
      if (len > room) len = room;
    } else {
      len = 0;
    }
  }
  getdev::copy_values(p.g.vals, p.g.val_cap, d, src, len, lane);
}

}  // namespace

void launch_raw_verify_headers(const uint8_t* src, const uint64_t* ext, uint32_t n_blocks,
                               uint8_t* status, uint32_t* crc, hipStream_t stream) {
  const RawVerifyParams p{src, ext, n_blocks, status, crc};
  hipLaunchKernelGGL(raw_verify_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, stream, p);
}

void launch_raw_seek(const RawSeekLaunch& a, hipStream_t stream) {
  const RawSeekParams p{a.t, a.q, a.q_pos, a.n_q, a.out_block, a.out_entry, a.out_status,
                        a.out_valid};
  hipLaunchKernelGGL(raw_seek_kernel, dim3((a.n_q + 255) / 256), dim3(256), 0, stream, p);
}

void launch_raw_get_walk(const GetLaunch& a, hipStream_t stream) {
  RawWalkParams p{};
  p.tabs = static_cast<const tpz_raw_table*>(a.tabs);
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
  if (a.flavour == Flavour::kLsm) {
    const RawLsmWalkParams lp{p, a.runs, a.n_runs};
    hipLaunchKernelGGL(raw_lsm_get_walk_kernel, grid, dim3(256), 0, stream, lp);
  } else {
    hipLaunchKernelGGL(raw_get_walk_kernel, grid, dim3(256), 0, stream, p);
  }
  launch_scan_u64(a.val_pos, a.n_q, a.part, stream);
}

void launch_raw_get_gather(const GetGatherLaunch& a, hipStream_t stream) {
  const RawGatherParams p{static_cast<const tpz_raw_table*>(a.tabs), a.n_tables, a.n_q, a.result,
                          a.table, a.block, a.entry, a.val_pos, a.vals, a.val_cap};
  const dim3 grid((a.n_q + 255) / 256);
  if (a.flavour == Flavour::kLsm) {
    const RawLsmGatherParams lp{p, a.runs, a.n_runs};
    hipLaunchKernelGGL(raw_lsm_get_gather_kernel, grid, dim3(256), 0, stream, lp);
  } else {
    hipLaunchKernelGGL(raw_get_gather_kernel, grid, dim3(256), 0, stream, p);
  }
}

}  // namespace tpz

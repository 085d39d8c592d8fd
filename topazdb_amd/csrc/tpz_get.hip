// tpz_get.hip — gfx950 kernels of the batched LevelController::get (src/level.rs:427-465) over
// tables resident in HBM (tpz_get_keys, tpz_get_values; include/tpz_gpu.h).
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
//
// Nothing here trusts the level order or the positions it is handed: the bisections are bounded
// by the table counts, and the gather checks table, block and entry against the descriptors and
// clips every copy to val_cap.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_internal.h"
#include "tpz_seek_dev.h"
#include "tpz_xxh3.h"

namespace tpz {

namespace {

using seekdev::u32;
using seekdev::u64;

constexpr u32 kNone = 0xFFFFFFFFu;
// Values up to this many bytes are copied by their own lane, longer ones by the whole wave (the
// merge gather's threshold, tpz_merge.hip).
constexpr u64 kLaneCopyMax = 256;

struct WalkParams {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 n_levels;
  u32 level_first[TPZ_GET_MAX_LEVELS + 1];   // padded with n_tables
  const uint8_t* q;         // query keys, packed
  const u64* q_pos;         // n_q + 1
  u32 n_q;
  uint8_t* result;
  uint8_t* status;
  u32* table;
  u32* block;
  u32* entry;
  u64* val_len;             // n_q + 1 (the scan fills the last one)
};

// tables[lo .. hi): partition_point(smallest_key <= key).saturating_sub(1) (level.rs:449-451);
// smallest_key = block_metas[0].first_key (table.rs:143-151). lo < hi.
__device__ __forceinline__ u32 level_table(const tpz_get_table* tabs, u32 lo, u32 hi,
                                           const uint8_t* qk, u64 ql) {
  const u32 first = lo;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const tpz_table& t = tabs[mid].table;
    u64 a = 0, len = 0;
    if (t.n_blocks) {           // (a table without blocks cannot be opened: its key reads empty)
      a = t.d_first_pos[0];
      len = t.d_first_pos[1] - a;
    }
    if (seekdev::key_cmp(t.d_first_keys + a, len, qk, ql) <= 0) lo = mid + 1; else hi = mid;
  }
  return lo > first ? lo - 1 : first;
}

__global__ __launch_bounds__(256, 8) void get_walk_kernel(WalkParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  // Does any table of the set have a filter? The whole wave looks, a lane per table, before the
  // lanes past the last query leave: the vote must not depend on how many lanes have a query (the
  // last wave of a launch may hold one).
  bool filters = false;
  for (u32 t = copydev::lane_id(); t < p.n_tables; t += 64) filters |= p.tabs[t].d_filter != nullptr;
  const bool any_filter = __any(filters);
  if (i >= p.n_q) return;
  const u64 qa = p.q_pos[i];
  const uint8_t* qk = p.q + qa;
  const u64 ql = p.q_pos[i + 1] - qa;
  const u32 l0 = p.n_levels ? p.level_first[1] : 0u;               // L0 = tables [0, l0)
  const u32 steps = p.n_levels ? l0 + (p.n_levels - 1) : 0u;       // L0's tables, then a level each
  u32 res = TPZ_GET_ABSENT, st = TPZ_BLOCK_OK, tb = kNone, blk = kNone, ent = kNone;
  u64 vlen = 0;
  const u64 h = any_filter ? xxh3::hash64(qk, ql) : 0;   // xxh3_64(key) for may_contain, once
  for (u32 s = 0; s < steps; s++) {
    u32 t;
    if (s < l0) {
      t = l0 - 1 - s;                           // level.rs:430: tables.iter().rev()
    } else {
      const u32 lv = s - l0 + 1;
      const u32 lo = p.level_first[lv], hi = p.level_first[lv + 1];
      if (lo >= hi) continue;                   // :446-448: an empty level
      t = level_table(p.tabs, lo, hi, qk, ql);
    }
    const tpz_get_table& g = p.tabs[t];
    const uint8_t* filter = g.d_filter;
    if (filter) {                               // may_contain (table.rs:114-119)
      const u32 pr = seekdev::bloom_probe(filter, g.filter_len, h);
      if (pr == 0) continue;
      if (pr == 2) {                            // Bloom::may_contain panics
        res = TPZ_GET_ERROR;
        st = TPZ_BLOCK_MALFORMED;
        tb = t;
        break;
      }
    }
    const seekdev::SeekPos r = seekdev::seek_table(g.table, qk, ql);
    if (r.status != TPZ_BLOCK_OK) {             // create_and_seek_to_key(..)? / its panics
      res = TPZ_GET_ERROR;
      st = r.status;
      tb = t;
      blk = r.block;
      ent = r.entry;
      break;
    }
    if (!r.valid) continue;
    // iter.key() == key (:435): the iterator is valid, so its block decoded and holds the entry
    const seekdev::BlockView v = seekdev::block_view(g.table, r.block, g.table.d_status[r.block]);
    u64 kl;
    const uint8_t* k = seekdev::entry_key(v, r.entry, kl);
    if (kl != ql || seekdev::key_cmp(k, kl, qk, ql) != 0) continue;
    seekdev::entry_value(v, g.table.d_count[r.block], r.entry, vlen);
    res = vlen ? TPZ_GET_FOUND : TPZ_GET_DELETED;   // :436-439: an empty value is a tombstone
    tb = t;
    blk = r.block;
    ent = r.entry;
    break;
  }
  p.result[i] = (uint8_t)res;
  p.status[i] = (uint8_t)st;
  p.table[i] = tb;
  p.block[i] = blk;
  p.entry[i] = ent;
  p.val_len[i] = vlen;
}

struct GatherParams {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 n_q;
  const uint8_t* result;
  const u32* table;
  const u32* block;
  const u32* entry;
  const u64* val_pos;
  uint8_t* vals;
  u64 val_cap;
};

__global__ __launch_bounds__(256) void get_gather_kernel(GatherParams p) {
  const u32 lane = copydev::lane_id();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 queries are consecutive)
  const uint8_t* src = nullptr;
  u64 len = 0, d = 0;
  if (i < p.n_q && p.result[i] == TPZ_GET_FOUND) {
    const u32 t = p.table[i], b = p.block[i], j = p.entry[i];
    if (t < p.n_tables) {
      const tpz_table& tab = p.tabs[t].table;
      if (b < tab.n_blocks) {
        const u32 st = tab.d_status[b];
        const u32 n = tab.d_count[b];
        if (block_decoded(st) && j < n) {
          const seekdev::BlockView v = seekdev::block_view(tab, b, st);
          src = seekdev::entry_value(v, n, j, len);
          d = p.val_pos[i];
          const u64 room = p.val_pos[i + 1] - d;      // the range tpz_get_keys gave this value
          if (len > room) len = room;
        }
      }
    }
  }
  if (len && len <= kLaneCopyMax) copydev::lane_copy(p.vals, p.val_cap, d, src, len);
  u64 mask = __ballot(len > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    copydev::wave_copy(p.vals, p.val_cap, __shfl(d, l, 64),
                       reinterpret_cast<const uint8_t*>(__shfl((u64)(uintptr_t)src, l, 64)),
                       __shfl(len, l, 64), lane);
  }
}

}  // namespace

void launch_get_walk(const GetLaunch& a, hipStream_t stream) {
  WalkParams p{};
  p.tabs = a.tabs;
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
  hipLaunchKernelGGL(get_walk_kernel, dim3((a.n_q + 255) / 256), dim3(256), 0, stream, p);
  launch_scan_u64(a.val_pos, a.n_q, a.part, stream);
}

void launch_get_gather(const GetGatherLaunch& a, hipStream_t stream) {
  GatherParams p{a.tabs, a.n_tables, a.n_q, a.result, a.table, a.block, a.entry, a.val_pos,
                 a.vals, a.val_cap};
  hipLaunchKernelGGL(get_gather_kernel, dim3((a.n_q + 255) / 256), dim3(256), 0, stream, p);
}

}  // namespace tpz

// tpz_get_dev.h — LevelController::get's walk for one query and the location of a hit's value,
// shared by the kernels of tpz_get.hip (tpz_get_keys, tpz_get_values) and tpz_mem.hip
// (tpz_lsm_get_keys, tpz_lsm_get_values: the same walk after the memtable runs).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "tpz_copy.h"
#include "tpz_internal.h"
#include "tpz_raw_dev.h"
#include "tpz_seek_dev.h"
#include "tpz_xxh3.h"

namespace tpz {
namespace getdev {

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

// Host side: lsm_get_walk_kernel lives in tpz_mem.hip, so launch_get_walk (tpz_get.hip), which
// fills `w` for both flavours, launches it through this.
void launch_lsm_walk_kernel(const WalkParams& w, const tpz_mem_run* runs, u32 n_runs, dim3 grid,
                            hipStream_t stream);

// What a query reports (tpz_get_keys' columns for it).
struct WalkOut {
  u32 res, st, tb, blk, ent;
  u64 vlen;
};

// tables[lo .. hi): partition_point(smallest_key <= key).saturating_sub(1) (level.rs:449-451);
// smallest_key = block_metas[0].first_key (table.rs:143-151). lo < hi.
template <class G>
__device__ __forceinline__ u32 level_table(const G* tabs, u32 lo, u32 hi, const uint8_t* qk,
                                           u64 ql) {
  const u32 first = lo;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const auto& t = table_of(tabs[mid]);
    u64 a = 0, len = 0;
    if (t.n_blocks) {           // (a table without blocks cannot be opened: its key reads empty)
      a = t.d_first_pos[0];
      len = t.d_first_pos[1] - a;
    }
    if (seekdev::key_cmp(t.d_first_keys + a, len, qk, ql) <= 0) lo = mid + 1; else hi = mid;
  }
  return lo > first ? lo - 1 : first;
}

// Does any table of the set have a filter? The whole wave looks, a lane per table, before the
// lanes past the last query leave: the vote must not depend on how many lanes have a query (the
// last wave of a launch may hold one).
template <class P>
__device__ __forceinline__ bool any_filter(const P& p) {
  bool filters = false;
  for (u32 t = copydev::lane_id(); t < p.n_tables; t += 64) filters |= p.tabs[t].d_filter != nullptr;
  return __any(filters);
}

// The walk over L0 and the levels for the key qk[0 .. ql); `o` holds ABSENT on entry. P is
// WalkParams, or RawWalkParams over in-place tables (tpz_raw_dev.h).
template <class P>
__device__ __forceinline__ void walk(const P& p, const uint8_t* qk, u64 ql, bool any_filter,
                                     WalkOut& o) {
  const u32 l0 = p.n_levels ? p.level_first[1] : 0u;               // L0 = tables [0, l0)
  const u32 steps = p.n_levels ? l0 + (p.n_levels - 1) : 0u;       // L0's tables, then a level each
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
    const auto& g = p.tabs[t];
    const uint8_t* filter = g.d_filter;
    if (filter) {                               // may_contain (table.rs:114-119)
      const u32 pr = seekdev::bloom_probe(filter, g.filter_len, h);
      if (pr == 0) continue;
      if (pr == 2) {                            // Bloom::may_contain panics
        o.res = TPZ_GET_ERROR;
        o.st = TPZ_BLOCK_MALFORMED;
        o.tb = t;
        break;
      }
    }
    const auto& tab = table_of(g);
    const seekdev::SeekPos r = seekdev::seek_table(tab, qk, ql);
    if (r.status != TPZ_BLOCK_OK) {             // create_and_seek_to_key(..)? / its panics
      o.res = TPZ_GET_ERROR;
      o.st = r.status;
      o.tb = t;
      o.blk = r.block;
      o.ent = r.entry;
      break;
    }
    if (!r.valid) continue;
    // iter.key() == key (:435): the iterator is valid, so its block decoded and holds the entry
    const auto v = seekdev::block_view(tab, r.block, tab.d_status[r.block]);
    u64 kl;
    const uint8_t* k = seekdev::entry_key(v, r.entry, kl);
    if (kl != ql || seekdev::key_cmp(k, kl, qk, ql) != 0) continue;
    seekdev::entry_value(v, seekdev::block_count(tab, r.block), r.entry, o.vlen);
    o.res = o.vlen ? TPZ_GET_FOUND : TPZ_GET_DELETED;   // :436-439: an empty value is a tombstone
    o.tb = t;
    o.blk = r.block;
    o.ent = r.entry;
    break;
  }
}

template <class P>
__device__ __forceinline__ void store(const P& p, u32 i, const WalkOut& o) {
  p.result[i] = (uint8_t)o.res;
  p.status[i] = (uint8_t)o.st;
  p.table[i] = o.tb;
  p.block[i] = o.blk;
  p.entry[i] = o.ent;
  p.val_len[i] = o.vlen;
}

// The value of entry j of block b of table t, each checked against the descriptors: null and
// len = 0 where one is out of range or the block did not decode.
template <class G>
__device__ __forceinline__ const uint8_t* table_value(const G* tabs, u32 n_tables, u32 t, u32 b,
                                                      u32 j, u64& len) {
  if (t < n_tables) {
    const auto& tab = table_of(tabs[t]);
    if (b < tab.n_blocks) {
      const u32 st = tab.d_status[b];
      // (the decoded count is read here, not through block_count: behind the call this load
      // comes out as a flat load in the gather kernels of tpz_get.hip)
      u32 n;
      if constexpr (std::is_same<G, tpz_get_table>::value) n = tab.d_count[b];
      else n = seekdev::block_count(tab, b);
      if (block_decoded(st) && j < n) {
        const auto v = seekdev::block_view(tab, b, st);
        return seekdev::entry_value(v, n, j, len);
      }
    }
  }
  return nullptr;
}

// The gather's copies for a wave: every lane's value (src, len) to vals[d ..), by its own lane up
// to kLaneCopyMax bytes, longer ones by the whole wave; nothing at or past val_cap.
__device__ __forceinline__ void copy_values(uint8_t* vals, u64 val_cap, u64 d, const uint8_t* src,
                                            u64 len, u32 lane) {
  if (len && len <= kLaneCopyMax) copydev::lane_copy(vals, val_cap, d, src, len);
  u64 mask = __ballot(len > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    copydev::wave_copy(vals, val_cap, __shfl(d, l, 64),
                       reinterpret_cast<const uint8_t*>(__shfl((u64)(uintptr_t)src, l, 64)),
                       __shfl(len, l, 64), lane);
  }
}

}  // namespace getdev
}  // namespace tpz

// tpz_seek_dev.h — the per-query device routines of the point-get side, shared by the kernels
// of tpz_seek.hip (tpz_seek_keys, tpz_bloom_may_contain) and tpz_get.hip (tpz_get_keys,
// tpz_get_values): SsTableIterator::seek_to_key over one resident table, the Bloom probe of a
// hashed key, and the view of a decoded block (its slot or its spill record).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"
#include "tpz_raw_dev.h"   // the in-place view's overloads, ahead of the templates below

namespace tpz {
namespace seekdev {

typedef uint32_t u32;
typedef uint64_t u64;

// memcmp then length, as Rust's Ord for [u8]
__device__ __forceinline__ int key_cmp(const uint8_t* a, u64 al, const uint8_t* b, u64 bl) {
  const u64 n = al < bl ? al : bl;
  for (u64 i = 0; i < n; i++) {
    const u32 x = a[i], y = b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return al < bl ? -1 : (al > bl ? 1 : 0);
}

// A decoded block's ends and stream: its slot, or its spill record (include/tpz_gpu.h); the
// entry classes of a BAD_ENTRY block (null otherwise: every entry reads whole).
struct BlockView {
  const u32* ends;
  const uint8_t* stream;
  const uint8_t* cls;
  // seek_to(j) / the bisection's key read panic on entry j (iterator.rs:74-82, :95-98)
  __device__ __forceinline__ bool seek_panics(u32 j) const { return cls && cls[j] != TPZ_ENTRY_OK; }
  __device__ __forceinline__ bool key_panics(u32 j) const { return cls && cls[j] == TPZ_ENTRY_BAD_KEY; }
};
// `t` may live in the kernel's arguments (tpz_seek_keys) or in HBM (tpz_get_keys' descriptor
// array): its fields are read where they are used.
__device__ __forceinline__ BlockView block_view(const tpz_table& t, u32 b, u32 st) {
  if (block_in_spill(st)) {
    const u32 n = t.d_count[b];
    const uint8_t* r = t.d_spill + t.d_spill_off[b];
    const u32* e = reinterpret_cast<const u32*>(r);
    const uint8_t* cls = (st == TPZ_BLOCK_BAD_ENTRY && n)
                             ? r + spill_classes(n, e[2 * (n - 1)], e[2 * (n - 1) + 1]) : nullptr;
    return BlockView{e, r + spill_stream(n), cls};
  }
  const u64 e0 = t.d_ext[b];
  return BlockView{t.d_ends + 2 * ends_base(t.d_entry_first, e0, b), t.d_data + slot_base(e0, b),
                   nullptr};
}
__device__ __forceinline__ u32 block_count(const tpz_table& t, u32 b) { return t.d_count[b]; }
// Entry j's key: its bytes and length.
__device__ __forceinline__ const uint8_t* entry_key(const BlockView& v, u32 j, u64& len) {
  const u32 lo = j ? v.ends[2 * (j - 1)] : 0u, hi = v.ends[2 * j];
  len = hi - lo;
  return v.stream + lo;
}
// Entry j's value in a block of n entries: the values start value_start(K) into the stream, K =
// the block's key bytes (its last kend).
__device__ __forceinline__ const uint8_t* entry_value(const BlockView& v, u32 n, u32 j, u64& len) {
  const u32 lo = j ? v.ends[2 * (j - 1) + 1] : 0u, hi = v.ends[2 * j + 1];
  len = hi - lo;
  return v.stream + value_start(v.ends[2 * (n - 1)]) + lo;
}

// Where SsTableIterator::seek_to_key ends (tpz_seek_keys' four outputs for one query).
struct SeekPos {
  u32 block;
  u32 entry;
  u32 status;   // TPZ_BLOCK_OK, the Err status of the last block read, or MALFORMED (a panic)
  bool valid;   // is_valid(): the current key is non-empty
};

// SsTableIterator::seek_to_key (src/table/iterator.rs:44-72) for the key qk[0 .. ql), over a
// decoded table (tpz_table) or an in-place one (tpz_raw_table, tpz_raw_dev.h).
template <class Table>
__device__ __forceinline__ SeekPos seek_table(const Table& t, const uint8_t* qk, u64 ql) {
  const u32 n_blocks = t.n_blocks;
  if (n_blocks == 0)                          // block_metas[0]: the reference panics
    return SeekPos{0, 0, TPZ_BLOCK_MALFORMED, false};
  // find_block_idx: partition_point(first_key <= key) (the lower-bound bisection), minus one
  u32 lo = 0, hi = n_blocks;
  {
    const uint8_t* fk = t.d_first_keys;
    const u64* fk_pos = t.d_first_pos;
    while (lo < hi) {
      const u32 mid = lo + (hi - lo) / 2;
      const u64 a = fk_pos[mid];
      if (key_cmp(fk + a, fk_pos[mid + 1] - a, qk, ql) <= 0) lo = mid + 1; else hi = mid;
    }
  }
  u32 b = lo ? lo - 1 : 0;
  u32 st = t.d_status[b], pos = 0;
  bool valid = false, panic = false;
  if (block_decoded(st)) {
    // BlockIterator::seek_to_key
    const auto v = block_view(t, b, st);
    const u32 n = block_count(t, b);
    u32 l = 0, r = n;
    pos = n;
    bool found = false;
    while (l < r) {
      const u32 mid = (r - l) / 2 + l;
      if (v.key_panics(mid)) { pos = mid; panic = true; break; }   // iterator.rs:95-98
      u64 kl;
      const uint8_t* k = entry_key(v, mid, kl);
      const int c = key_cmp(k, kl, qk, ql);
      if (c > 0) r = mid;
      else if (c < 0) l = mid + 1;
      else { pos = mid; found = true; break; }
    }
    if (!found && !panic) pos = l;
    if (!panic && pos < n && v.seek_panics(pos)) panic = true;      // seek_to, :74-82
    u64 kl = 0;
    if (pos < n) entry_key(v, pos, kl);
    valid = !panic && pos < n && kl > 0;      // is_valid: the current key is non-empty
    if (!panic && !valid && b + 1 < n_blocks) {     // the next block, from its first entry
      b++;
      st = t.d_status[b];
      pos = 0;
      valid = false;
      if (block_decoded(st) && block_count(t, b) > 0) {
        const auto w = block_view(t, b, st);
        panic = w.seek_panics(0);
        entry_key(w, 0, kl);
        valid = !panic && kl > 0;
      }
    }
  }
  const bool dec = block_decoded(st);
  return SeekPos{b, pos, panic ? (u32)TPZ_BLOCK_MALFORMED : dec ? (u32)TPZ_BLOCK_OK : st,
                 dec && valid};
}

// Bloom::may_contain (src/bloom.rs:72-84) of the hash h = xxh3_64(key) in `filter` (Bloom::encode:
// the bit array, then k in the last byte): 1 (may contain), 0 (absent), 2 (the reference panics:
// an empty filter, filter.last().unwrap(); or no bit array with k > 0, `% 0`).
__device__ __forceinline__ u32 bloom_probe(const uint8_t* filter, u64 filter_len, u64 h) {
  if (filter_len == 0) return 2;
  const u64 delta = (h >> 34) | (h << 30);
  const u32 k = filter[filter_len - 1];
  const u64 limit = (filter_len - 1) * 8;
  if (limit == 0) return k ? 2 : 1;
  for (u32 j = 0; j < k; j++) {
    const u64 bit = h % limit;
    if (!(filter[bit >> 3] & (1u << (bit & 7)))) return 0;
    h += delta;
  }
  return 1;
}

}  // namespace seekdev
}  // namespace tpz

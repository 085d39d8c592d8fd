// tpz_raw_dev.h — the view of an encoded block where it lies in HBM (an in-place table,
// tpz_raw_table; include/tpz_gpu.h), with the interface the point-get routines use from the
// decoded view (tpz_seek_dev.h BlockView): block_view, block_count, entry_key, entry_value,
// key_panics, seek_panics. tpz_seek_dev.h includes it ahead of its templates (seek_table) and
// tpz_get_dev.h ahead of the walk, so both resolve these overloads for a tpz_raw_table; the
// kernels over in-place tables are tpz_raw.hip's.
//
// An Uncompress block is [n u16 BE][n offsets u16 BE][data][crc u32 BE][tag 1] (src/block.rs:31-44,
// src/block/compress.rs:85-89). The view reads what BlockIterator reads (src/block/iterator.rs):
//   n            the BE u16 at the block start (block.rs:54)
//   off(j)       offsets[j], the BE u16 at 2 + 2j (:56-59)
//   data         the dl = len - 5 - 2 - 2n bytes after the header
//   entry j      klen = BE u16 at data[off], the key, vlen = BE u16 behind it, the value (:74-82)
//   key_panics   off + 2 > dl or off + 2 + klen > dl: `data[offset..]`, get_u16 or `buf[..klen]`
//                panics (:97-100; the spill path's TPZ_ENTRY_BAD_KEY)
//   seek_panics  that, or off + 4 + klen > dl or off + 4 + klen + vlen > dl (:74-82; BAD_KEY or
//                TPZ_ENTRY_BAD_VALUE)
// Blocks start at any byte offset, so every field is assembled from byte loads, zero-extended:
// offsets and lengths reach 65,535 and extents pass 2^32 (all positions are u64). Nothing is read
// outside [ext[b], ext[b + 1]): a block whose bytes no longer hold the header its status promises
// (7 + 2n > len) reads as n = 0, and an entry that panics reads as an empty key and value.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"

namespace tpz {
namespace seekdev {

typedef uint32_t u32;
typedef uint64_t u64;

__device__ __forceinline__ u32 raw_be16(const uint8_t* p) { return (u32)p[0] << 8 | (u32)p[1]; }

struct RawView {
  const uint8_t* blk;    // the block's first byte (n, then the offsets)
  const uint8_t* data;   // blk + 2 + 2n
  u64 dl;                // data.len()
  u32 n;
  // Entry j's key: false where reading it panics; o = offsets[j], kl = klen otherwise.
  __device__ __forceinline__ bool key_at(u32 j, u64& o, u64& kl) const {
    o = raw_be16(blk + 2 + 2 * (u64)j);
    kl = 0;
    if (o + 2 > dl) return false;
    kl = raw_be16(data + o);
    return o + 2 + kl <= dl;
  }
  __device__ __forceinline__ bool key_panics(u32 j) const {
    u64 o, kl;
    return !key_at(j, o, kl);
  }
  __device__ __forceinline__ bool seek_panics(u32 j) const {
    u64 o, kl;
    if (!key_at(j, o, kl)) return true;
    const u64 v = o + 2 + kl;
    if (v + 2 > dl) return true;
    return v + 2 + raw_be16(data + v) > dl;
  }
};

// The status of a raw table's block is tpz_raw_verify's: OK promises n and the n offsets readable.
__device__ __forceinline__ RawView block_view(const tpz_raw_table& t, u32 b, u32 /*st*/) {
  const u64 e0 = t.d_ext[b], e1 = t.d_ext[b + 1];
  const u64 len = e1 > e0 ? e1 - e0 : 0;
  const uint8_t* blk = t.d_src + e0;
  u32 n = len >= 7 ? raw_be16(blk) : 0u;
  if (7 + 2 * (u64)n > len) n = 0;
  const u64 db = 2 + 2 * (u64)n;
  return RawView{blk, blk + db, len >= 7 ? len - 5 - db : 0, n};
}
__device__ __forceinline__ u32 block_count(const tpz_raw_table& t, u32 b) {
  return block_view(t, b, TPZ_BLOCK_OK).n;
}
// Entry j's key: its bytes and length (empty where key_panics(j)).
__device__ __forceinline__ const uint8_t* entry_key(const RawView& v, u32 j, u64& len) {
  u64 o;
  if (!v.key_at(j, o, len)) {
    len = 0;
    return v.data;
  }
  return v.data + o + 2;
}
// Entry j's value (empty where seek_panics(j)).
__device__ __forceinline__ const uint8_t* entry_value(const RawView& v, u32 /*n*/, u32 j, u64& len) {
  u64 o, kl;
  len = 0;
  if (!v.key_at(j, o, kl)) return v.data;
  const u64 p = o + 2 + kl;
  if (p + 2 > v.dl) return v.data;
  const u64 vl = raw_be16(v.data + p);
  if (p + 2 + vl > v.dl) return v.data;
  len = vl;
  return v.data + p + 2;
}

}  // namespace seekdev

namespace getdev {

using seekdev::u32;
using seekdev::u64;

// tpz_get_dev.h's WalkParams / GatherParams over in-place tables (the same fields, so the walk,
// the store and the gather read either).
struct RawWalkParams {
  const tpz_raw_table* tabs;
  u32 n_tables;
  u32 n_levels;
  u32 level_first[TPZ_GET_MAX_LEVELS + 1];   // padded with n_tables
  const uint8_t* q;
  const u64* q_pos;
  u32 n_q;
  uint8_t* result;
  uint8_t* status;
  u32* table;
  u32* block;
  u32* entry;
  u64* val_len;
};

struct RawGatherParams {
  const tpz_raw_table* tabs;
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

// The table of a descriptor: a tpz_get_table wraps it, a tpz_raw_table is it.
__device__ __forceinline__ const tpz_table& table_of(const tpz_get_table& g) { return g.table; }
__device__ __forceinline__ const tpz_raw_table& table_of(const tpz_raw_table& g) { return g; }

}  // namespace getdev
}  // namespace tpz

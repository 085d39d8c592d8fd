// tpz_mem_dev.h — the device routines over a memtable run (tpz_mem_run, include/tpz_gpu.h): the
// 8-byte key prefix and the comparison of keys whose prefixes tie (shared with the scan's merge,
// tpz_scan.hip), and the bisection of a run's sorted keys, over its prefix column where it has one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"
#include "tpz_seek_dev.h"

namespace tpz {
namespace memdev {

using seekdev::u32;
using seekdev::u64;

// The first 8 bytes of a key, big-endian, zero-padded: orders keys as memcmp does wherever two
// prefixes differ.
__device__ __forceinline__ u64 key_prefix(const uint8_t* k, u64 len) {
  u64 x = 0;
  const u32 n = len < 8 ? (u32)len : 8u;
  for (u32 j = 0; j < n; j++) x |= (u64)k[j] << (56 - 8 * j);
  return x;
}
// key_cmp for two keys whose key_prefix is equal: with a key of at most 8 bytes the shorter one
// is a prefix of the other (`a` against `a\0`: the padding is not part of the key), else the
// bytes after the eighth decide.
__device__ __forceinline__ int cmp_tied(const uint8_t* a, u64 al, const uint8_t* b, u64 bl) {
  if (al <= 8 || bl <= 8) return al < bl ? -1 : (al > bl ? 1 : 0);
  return seekdev::key_cmp(a + 8, al - 8, b + 8, bl - 8);
}

// Entry j's key / value in a run (j < n_entries). A position past the column's bytes is clamped:
// the bytes read lie inside [d_keys, d_keys + key_bytes) whatever d_kpos holds.
__device__ __forceinline__ const uint8_t* run_key(const tpz_entries& e, u32 j, u64& len) {
  const u64 cap = e.key_bytes;
  u64 a = e.d_kpos[j], b = e.d_kpos[j + 1];
  a = a < cap ? a : cap;
  b = b < cap ? b : cap;
  len = b > a ? b - a : 0;
  return e.d_keys + a;
}
__device__ __forceinline__ const uint8_t* run_value(const tpz_entries& e, u32 j, u64& len) {
  const u64 cap = e.val_bytes;
  u64 a = e.d_vpos[j], b = e.d_vpos[j + 1];
  a = a < cap ? a : cap;
  b = b < cap ? b : cap;
  len = b > a ? b - a : 0;
  return e.d_vals + a;
}

// One step's comparison of entry `mid` with the probe (qk, ql; qp = its key_prefix): by the
// prefix column alone where the prefixes differ (one 8-byte load), else by the key bytes.
__device__ __forceinline__ int run_cmp(const tpz_mem_run& r, u32 mid, const uint8_t* qk, u64 ql,
                                       u64 qp) {
  const u64* pfx = r.d_prefix;
  if (pfx) {
    const u64 x = pfx[mid];
    if (x != qp) return x < qp ? -1 : 1;
  }
  u64 kl;
  const uint8_t* k = run_key(r.entries, mid, kl);
  return pfx ? cmp_tied(k, kl, qk, ql) : seekdev::key_cmp(k, kl, qk, ql);
}

// The number of the run's entries whose key is < the probe (or <= it with `incl`): the start of
// map.range((Included(q), ..)) / of ((Excluded(q), ..)). `r` lives in HBM: its fields are read
// where they are used. The loop halves [lo, hi) and so ends whatever the keys' order.
__device__ __forceinline__ u32 run_bound(const tpz_mem_run& r, const uint8_t* qk, u64 ql, u64 qp,
                                         bool incl) {
  u32 lo = 0, hi = r.entries.n_entries;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const int c = run_cmp(r, mid, qk, ql, qp);
    if (c < 0 || (incl && c == 0)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// SkipMap::get(key) (MemTable::get, src/mem_table.rs:150-152): the index of the entry with an
// equal key, or 0xFFFFFFFF. A run's keys are strictly increasing, so at most one is equal.
__device__ __forceinline__ u32 run_find(const tpz_mem_run& r, const uint8_t* qk, u64 ql, u64 qp) {
  u32 lo = 0, hi = r.entries.n_entries;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const int c = run_cmp(r, mid, qk, ql, qp);
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1; else hi = mid;
  }
  return 0xFFFFFFFFu;
}

}  // namespace memdev
}  // namespace tpz

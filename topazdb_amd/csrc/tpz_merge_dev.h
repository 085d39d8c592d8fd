// tpz_merge_dev.h — the device bodies of a merge pass over lists of u32 entry ids (key bytes
// never move): the key compare on {8-byte prefix, tail bytes, lengths}, the merge-path partition
// and the LDS tile merge. Two users instantiate them: tpz_merge.hip (tpz_merge_runs: the lists of
// a level are groups of the caller's sorted runs, ties take the lower run: a stable merge) and
// tpz_membuild.hip (tpz_mem_build: the lists are equal-length sorted pieces of one unsorted batch,
// ties are broken by the entry id: a total order).
//
// A params type P carries the columns (keys, kpos, key_bytes, n, pref) and three members:
//   Pair pair_of(lvl, q)                      pair q of level lvl as entry ranges A, B
//   bool find_pair(lvl, npairs, t, extra, q, k, tile0)
//                                             the pair holding index t when every pair takes its
//                                             tiles plus `extra` slots
//   bool less(a, pa, b, pb)                   entry a (prefix pa) goes strictly before entry b
// Every bisection is a bounded loop over a clamped range, every id read from a list is clamped to
// n - 1 and every entry span to its byte column: lists that are not sorted leave the output
// unspecified but in bounds.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"

namespace tpz {
namespace mergedev {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kMgThreads = 256;
constexpr u32 kMgPer = kMergeTile / kMgThreads;   // items per thread
static_assert(kMgPer * kMgThreads == kMergeTile, "tile = threads x items");

__device__ __forceinline__ u64 min64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 max64(u64 a, u64 b) { return a > b ? a : b; }

// Entry e's bytes in a column of `cap` bytes: [at, at + len), clamped to the column.
__device__ __forceinline__ void span(const u64* pos, u64 cap, u32 e, u64& at, u64& len) {
  const u64 a = min64(pos[e], cap);
  const u64 b = min64(max64(pos[e + 1], a), cap);
  at = a;
  len = b - a;
}

__device__ __forceinline__ u64 load_be64(const uint8_t* p) {
  u64 x;
  __builtin_memcpy(&x, p, 8);
  return __builtin_bswap64(x);
}

// Order of two keys whose 8-byte prefixes are equal: the bytes from offset 8, then the lengths.
template <class P>
__device__ inline int tail_cmp(const P& p, u32 a, u32 b) {
  u64 sa, la, sb, lb;
  span(p.kpos, p.key_bytes, a, sa, la);
  span(p.kpos, p.key_bytes, b, sb, lb);
  const u64 m = min64(la, lb);
  u64 i = 8;
  for (; i + 8 <= m; i += 8) {
    const u64 x = load_be64(p.keys + sa + i), y = load_be64(p.keys + sb + i);
    if (x != y) return x < y ? -1 : 1;
  }
  for (; i < m; i++) {
    const u32 x = p.keys[sa + i], y = p.keys[sb + i];
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

__device__ __forceinline__ u32 clamp_id(u32 id, u32 n) { return id < n ? id : n - 1; }

struct Pair {
  u32 a0, a1, b1;   // A = entries [a0, a1), B = [a1, b1)
};
__device__ __forceinline__ u32 tiles_of(const Pair& x) { return (x.b1 - x.a0 + kMergeTile - 1) / kMergeTile; }

// part[tile0 + q + k] = how many of the first min(k * kMergeTile, total) merged entries of pair q
// come from A (the merge path's diagonal; A goes first unless B is strictly less).
template <class P>
__device__ __forceinline__ void partition_body(const P& p, u32 lvl, u32 npairs, u32 nslots,
                                               const u32* in, u32* part) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nslots) return;
  u32 q, k, tile0;
  if (!p.find_pair(lvl, npairs, t, 1, q, k, tile0)) return;
  const Pair x = p.pair_of(lvl, q);
  const u32 la = x.a1 - x.a0, lb = x.b1 - x.a1;
  const u64 d64 = (u64)k * kMergeTile;
  const u32 d = d64 < (u64)la + lb ? (u32)d64 : la + lb;
  u32 lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  for (int it = 0; it < 33 && lo < hi; it++) {
    const u32 mid = lo + (hi - lo) / 2;
    const u32 ia = clamp_id(in[x.a0 + mid], p.n), ib = clamp_id(in[x.a1 + (d - 1 - mid)], p.n);
    if (!p.less(ib, p.pref[ib], ia, p.pref[ia])) lo = mid + 1;   // A[mid] goes first
    else hi = mid;
  }
  part[tile0 + q + k] = lo;
}

// One workgroup of kMgThreads merges one tile of <= kMergeTile entries of its pair in LDS
// (s_pref: kMergeTile u64, s_id: kMergeTile u32).
template <class P>
__device__ __forceinline__ void tile_body(const P& p, u32 lvl, u32 npairs, const u32* in,
                                          const u32* part, u32* out, u64* s_pref, u32* s_id) {
  u32 q, k, tile0;
  if (!p.find_pair(lvl, npairs, blockIdx.x, 0, q, k, tile0)) return;
  const Pair x = p.pair_of(lvl, q);
  const u32 la = x.a1 - x.a0, lb = x.b1 - x.a1;
  const u32 d0 = k * kMergeTile;                       // (k < tiles_of(x): no overflow)
  const u32 d1 = la + lb - d0 < kMergeTile ? la + lb : d0 + kMergeTile;
  // the tile's share of A and B; sorted lists give s0 <= s1 and exact counts, anything else is
  // cut to the lists
  const u32 s0 = part[tile0 + q + k];
  u32 s1 = part[tile0 + q + k + 1];
  if (s1 < s0) s1 = s0;
  u32 na = s1 - s0;
  if (na > d1 - d0) na = d1 - d0;
  const u32 bs = d0 - s0;
  u32 nb = d1 - d0 - na;
  if (nb > lb - bs) nb = lb - bs;
  const u32 cnt = na + nb;
  const u32 tid = threadIdx.x;
  for (u32 i = tid; i < cnt; i += kMgThreads) {
    const u32 id = clamp_id(i < na ? in[x.a0 + s0 + i] : in[x.a1 + bs + (i - na)], p.n);
    s_id[i] = id;
    s_pref[i] = p.pref[id];
  }
  __syncthreads();
  const u32 dt = tid * kMgPer < cnt ? tid * kMgPer : cnt;
  u32 lo = dt > nb ? dt - nb : 0, hi = dt < na ? dt : na;
  for (int it = 0; it < 12 && lo < hi; it++) {
    const u32 mid = lo + (hi - lo) / 2;
    const u32 jb = na + (dt - 1 - mid);
    if (!p.less(s_id[jb], s_pref[jb], s_id[mid], s_pref[mid])) lo = mid + 1;
    else hi = mid;
  }
  u32 i = lo, j = dt - lo;   // next item of A / of B
  u32 r[kMgPer];
#pragma unroll
  for (u32 t = 0; t < kMgPer; t++) {
    r[t] = 0;
    if (dt + t < cnt && (i < na || j < nb)) {
      bool take_a = j >= nb;
      if (!take_a && i < na)
        take_a = !p.less(s_id[na + j], s_pref[na + j], s_id[i], s_pref[i]);
      r[t] = take_a ? s_id[i] : s_id[na + j];
      if (take_a) i++;
      else j++;
    }
  }
  __syncthreads();
#pragma unroll
  for (u32 t = 0; t < kMgPer; t++)
    if (tid * kMgPer + t < cnt) s_id[tid * kMgPer + t] = r[t];
  __syncthreads();
  for (u32 o = tid; o < cnt; o += kMgThreads) out[x.a0 + d0 + o] = s_id[o];
}

}  // namespace mergedev
}  // namespace tpz

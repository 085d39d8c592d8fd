// tpz_copy.h — byte-range copies between columns in HBM for the gather kernels (tpz_merge.hip
// merge_gather_kernel, tpz_get.hip get_gather_kernel): whole 16-byte pieces of the destination
// as vector stores, the pieces a range shares with its neighbours byte by byte.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpz {
namespace copydev {

typedef uint32_t u32;
typedef uint64_t u64;

__device__ __forceinline__ u32 lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// The whole wave copies src[0 .. len) to dst[d .. d + len) (dst 16-byte aligned, cap bytes): a lane
// per 16-byte piece of dst, the pieces the range only partly covers byte by byte.
__device__ __forceinline__ void wave_copy(uint8_t* dst, u64 cap, u64 d, const uint8_t* src, u64 len,
                                          u32 lane) {
  if (d >= cap) return;
  if (len > cap - d) len = cap - d;
  const u64 c0 = d & ~15ull, end = d + len;
  const u64 pieces = (((end + 15) & ~15ull) - c0) >> 4;
  for (u64 c = lane; c < pieces; c += 64) {
    const u64 cb = c0 + 16 * c;
    const u64 lo = (cb > d ? cb : d), hi = (cb + 16 < end ? cb + 16 : end);
    if (hi - lo == 16) {
      uint4 v;
      __builtin_memcpy(&v, src + (cb - d), 16);
      *reinterpret_cast<uint4*>(dst + cb) = v;
    } else {
      for (u64 x = lo; x < hi; x++) dst[x] = src[x - d];
    }
  }
}

// Byte b (0..15) of a 16-byte register value, without indexing it in memory.
__device__ __forceinline__ u32 byte_of(const uint4& v, u32 b) {
  const u32 w = b < 8 ? (b < 4 ? v.x : v.y) : (b < 12 ? v.z : v.w);
  return (w >> (8 * (b & 3))) & 0xFFu;
}

// One lane copies src[0 .. len) to dst[d .. d + len): whole 16-byte pieces of dst between a head
// and a tail that are stored byte by byte out of one 16-byte load each (the stores do not wait for
// one another; a byte loop that loads would pay a load latency per byte).
__device__ __forceinline__ void lane_copy(uint8_t* dst, u64 cap, u64 d, const uint8_t* src, u64 len) {
  if (d >= cap) return;
  if (len > cap - d) len = cap - d;
  if (len < 16) {
    for (u64 x = 0; x < len; x++) dst[d + x] = src[x];
    return;
  }
  const u64 end = d + len;
  const u64 c1 = (d + 15) & ~15ull, c2 = end & ~15ull;   // d <= c1 <= c2 <= end
  uint4 h, t;
  __builtin_memcpy(&h, src, 16);
  __builtin_memcpy(&t, src + (len - 16), 16);
  const u32 hn = (u32)(c1 - d), tn = (u32)(end - c2);
  for (u32 b = 0; b < hn; b++) dst[d + b] = (uint8_t)byte_of(h, b);
  for (u64 c = c1; c < c2; c += 16) {
    uint4 v;
    __builtin_memcpy(&v, src + (c - d), 16);
    *reinterpret_cast<uint4*>(dst + c) = v;
  }
  for (u32 b = 0; b < tn; b++) dst[c2 + b] = (uint8_t)byte_of(t, 16 - tn + b);
}

}  // namespace copydev
}  // namespace tpz

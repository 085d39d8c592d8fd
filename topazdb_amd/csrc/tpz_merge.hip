// tpz_merge.hip — tpz_merge_runs: compaction's MergeIterator over sorted runs of entries in HBM
// (src/iterators/merge_iterator.rs:41-106 as sub_compact drives it, src/level.rs:188-212).
//
// What the iterator yields, for runs r = 0..R-1 each sorted non-decreasing by key (create()
// numbers the non-empty iterators in the caller's order, :48-53; the heap's top is the smallest
// (key, index), :21-29; next() steps every other iterator past the current key, :76-88, then the
// current one, and keeps it current while no other (key, index) is smaller, :90-103):
//   entry (r, j) is yielded iff no run with a lower index holds an equal key, in (key, r, j) order
// (tests/_merge_model.py restates create/next line by line and checks this rule against it).
// Entries are numbered run after run, so (key, r, j) order is (key, entry id) order: a STABLE
// merge of the runs by key, followed by dropping every entry whose run is not the run of the
// first entry of its equal-key group.
//
// Passes (nothing waits between workgroups; every launch runs to completion on its own):
//   prefix     one thread per entry: its first 8 key bytes as a big-endian u64, zero padded, the
//              identity id list, and the first empty key (info[3])
//   ceil(log2 R) x { partition, tile merge }: lists of 2^l runs are merged pairwise from a ping
//              into a pong array of u32 entry ids (key bytes never move); an odd last list is
//              copied through. partition: one thread per tile boundary bisects the merge path
//              diagonal in global memory; tile merge: a workgroup stages its <= kMergeTile ids and
//              prefixes in LDS, every thread bisects its own diagonal there and merges 4 items.
//              (Both bodies are tpz_merge_dev.h's, which tpz_membuild.hip instantiates too.)
//   drop       one thread per merged position: the head of its equal-key group by a galloping
//              bisection backwards (O(log group) compares, not a walk), keep = same run as the head;
//              writes {keep, kept key bytes, kept value bytes} for the scans
//   scan       the flat layout's three-array scan (tpz_flat.hip)
//   gather     a thread per merged position: positions, source ids, then the kept entry's key and
//              value copied in 16-byte pieces of the DESTINATION (the pieces an entry shares with
//              its neighbours are written byte by byte): by its own lane up to kLaneCopyMax bytes,
//              by the whole wave, a lane per piece, past that (the first version copied every
//              entry with the whole wave, one entry after the other: 1.4-2.1 ms of the 2.3 ms a
//              2^22-entry merge took, against 0.35 ms for every other pass together)
// A compare reads the two prefixes first; key bytes only when they are equal, then from offset 8
// on, then the lengths (the zero padding cannot tell "a" from "a\0").
//
// Unsorted runs (a precondition violation) leave the outputs unspecified but in bounds: every
// bisection is a bounded loop over a clamped range, every id read from a list is clamped to
// n - 1, every entry span is clamped to the byte columns, and the gather cuts what would pass the
// output capacities (an id list with repeats could otherwise sum to more bytes than the input).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_internal.h"
#include "tpz_merge_dev.h"

namespace tpz {
namespace {

using mergedev::clamp_id;
using mergedev::kMgThreads;
using mergedev::Pair;
using mergedev::span;
using mergedev::tiles_of;
using mergedev::u32;
using mergedev::u64;

struct MergeParams {
  const uint8_t* keys;
  const u64* kpos;
  u64 key_bytes;
  const uint8_t* vals;
  const u64* vpos;
  u64 val_bytes;
  u32 n;
  u32 n_runs;
  const u64* pref;
  u32 run_first[TPZ_MERGE_MAX_RUNS + 1];

  // Lists of a level: list k = runs [k << lvl, (k + 1) << lvl); pair q merges lists 2q (A) and
  // 2q + 1 (B) into the entry range both cover.
  __device__ __forceinline__ Pair pair_of(u32 lvl, u32 q) const {
    const u32 R = n_runs;
    const u64 w = 1ull << lvl;
    const u64 r0 = 2 * q * w, r1 = r0 + w, r2 = r1 + w;
    Pair x;
    x.a0 = run_first[r0 < R ? r0 : R];
    x.a1 = run_first[r1 < R ? r1 : R];
    x.b1 = run_first[r2 < R ? r2 : R];
    return x;
  }
  // The pair that holds index t when every pair takes its tiles plus `extra` slots; k = the index
  // within the pair, tile0 = the tiles of the pairs before it. False past the last pair.
  __device__ __forceinline__ bool find_pair(u32 lvl, u32 npairs, u32 t, u32 extra, u32& q, u32& k,
                                            u32& tile0) const {
    u32 base = 0;
    for (u32 i = 0; i < npairs; i++) {
      const u32 tp = tiles_of(pair_of(lvl, i));
      if (t < tp + extra) {
        q = i;
        k = t;
        tile0 = base;
        return true;
      }
      t -= tp + extra;
      base += tp;
    }
    return false;
  }
  // By key alone: entries are numbered run after run, so "A first on a tie" is the stable merge.
  __device__ __forceinline__ bool less(u32 a, u64 pa, u32 b, u64 pb) const {
    if (pa != pb) return pa < pb;
    return mergedev::tail_cmp(*this, a, b) < 0;
  }
};

__device__ __forceinline__ int tail_cmp(const MergeParams& p, u32 a, u32 b) {
  return mergedev::tail_cmp(p, a, b);
}

__global__ __launch_bounds__(256) void merge_prefix_kernel(const uint8_t* keys, const u64* kpos,
                                                            u64 key_bytes, u32 n, u64* pref, u32* ids,
                                                            u64* info) {
  const u64 e64 = (u64)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= n) return;
  const u32 e = (u32)e64;
  u64 at, len;
  span(kpos, key_bytes, e, at, len);
  u64 x = 0;
  for (u32 i = 0; i < 8; i++) x = (x << 8) | (i < len ? keys[at + i] : 0u);
  pref[e] = x;
  ids[e] = e;
  if (len == 0) atomicMin(reinterpret_cast<unsigned long long*>(info + 3), (unsigned long long)e);
}

// The partition and the tile merge of a level (tpz_merge_dev.h).
__global__ __launch_bounds__(256) void merge_partition_kernel(MergeParams p, u32 lvl, u32 npairs,
                                                               u32 nslots, const u32* in, u32* part) {
  mergedev::partition_body(p, lvl, npairs, nslots, in, part);
}

__global__ __launch_bounds__(kMgThreads) void merge_tile_kernel(MergeParams p, u32 lvl, u32 npairs,
                                                                 const u32* in, const u32* part,
                                                                 u32* out) {
  __shared__ u64 s_pref[kMergeTile];
  __shared__ u32 s_id[kMergeTile];
  mergedev::tile_body(p, lvl, npairs, in, part, out, s_pref, s_id);
}

// The run that holds entry id: the largest r with run_first[r] <= id (empty runs share a start
// with the run after them and are passed over).
__device__ __forceinline__ u32 run_of(const MergeParams& p, u32 id) {
  u32 lo = 0, hi = p.n_runs;   // run_first[lo] <= id < run_first[hi]
  for (int it = 0; it < 10 && lo + 1 < hi; it++) {
    const u32 mid = (lo + hi) / 2;
    if (p.run_first[mid] <= id) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool key_equal(const MergeParams& p, u32 a, u64 pa, u32 b) {
  return p.pref[b] == pa && tail_cmp(p, a, b) == 0;
}

// scan[0][i] = keep, scan[1][i] = its key bytes if kept, scan[2][i] = its value bytes if kept.
__global__ __launch_bounds__(256) void merge_drop_kernel(MergeParams p, const u32* m, u64* scan) {
  const u64 i64 = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= p.n) return;
  const u32 i = (u32)i64;
  const u32 id = clamp_id(m[i], p.n);
  const u64 pf = p.pref[id];
  // the head of the equal-key group: the smallest h with key(m[h]) == key(m[i]), found by
  // doubling steps back from i and a bisection between the last unequal and the first equal probe
  u32 good = i;
  bool have_bad = false;
  u32 bad = 0;
  u32 step = 1;
  for (int it = 0; it < 33 && good > 0; it++) {
    const u32 probe = good > step ? good - step : 0;
    if (key_equal(p, id, pf, clamp_id(m[probe], p.n))) {
      good = probe;
      step <<= 1;
    } else {
      bad = probe;
      have_bad = true;
      break;
    }
  }
  if (have_bad) {
    for (int it = 0; it < 33 && bad + 1 < good; it++) {
      const u32 mid = bad + (good - bad) / 2;
      if (key_equal(p, id, pf, clamp_id(m[mid], p.n))) good = mid;
      else bad = mid;
    }
  }
  const bool keep = run_of(p, clamp_id(m[good], p.n)) == run_of(p, id);
  u64 at, kl, vl;
  span(p.kpos, p.key_bytes, id, at, kl);
  span(p.vpos, p.val_bytes, id, at, vl);
  const u64 st = (u64)p.n + 1;
  scan[i] = keep ? 1 : 0;
  scan[st + i] = keep ? kl : 0;
  scan[2 * st + i] = keep ? vl : 0;
}

using copydev::lane_copy;
using copydev::lane_id;
using copydev::wave_copy;

// Keys / values up to this many bytes are copied by their own lane (64 entries at a time); longer
// ones by the whole wave, one entry at a time (at least a quarter of the lanes then have a piece).
constexpr u64 kLaneCopyMax = 256;

struct GatherOut {
  uint8_t* keys;
  u64* kpos;
  uint8_t* vals;
  u64* vpos;
  u32* src_entry;
  u64* info;
};

__global__ __launch_bounds__(256) void merge_gather_kernel(MergeParams p, const u32* m, const u64* scan,
                                                            GatherOut o) {
  const u32 lane = lane_id();
  const u64 st = (u64)p.n + 1;
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 positions are consecutive)
  if (i == 0) {
    const u64 n_out = scan[p.n], kb = scan[st + p.n], vb = scan[2 * st + p.n];
    o.info[0] = n_out;
    o.info[1] = kb;
    o.info[2] = vb;
    o.kpos[n_out] = kb;
    o.vpos[n_out] = vb;
  }
  bool keep = false;
  u64 ks = 0, kl = 0, kd = 0, vs = 0, vl = 0, vd = 0;
  if (i < p.n) {
    const u64 out = scan[i];
    keep = scan[i + 1] != out;
    if (keep) {
      const u32 id = clamp_id(m[i], p.n);
      span(p.kpos, p.key_bytes, id, ks, kl);
      span(p.vpos, p.val_bytes, id, vs, vl);
      kd = scan[st + i];
      vd = scan[2 * st + i];
      o.kpos[out] = kd;
      o.vpos[out] = vd;
      if (o.src_entry) o.src_entry[out] = id;
    }
  }
  if (keep && kl <= kLaneCopyMax) lane_copy(o.keys, p.key_bytes, kd, p.keys + ks, kl);
  if (keep && vl <= kLaneCopyMax) lane_copy(o.vals, p.val_bytes, vd, p.vals + vs, vl);
  u64 mask = __ballot(keep && kl > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    wave_copy(o.keys, p.key_bytes, __shfl(kd, l, 64), p.keys + __shfl(ks, l, 64), __shfl(kl, l, 64), lane);
  }
  mask = __ballot(keep && vl > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    wave_copy(o.vals, p.val_bytes, __shfl(vd, l, 64), p.vals + __shfl(vs, l, 64), __shfl(vl, l, 64), lane);
  }
}

struct Work {
  u64* pref;
  u64* scan;
  u64* parts;
  u32* ida;
  u32* idb;
  u32* mpart;
  u64 bytes;
};
// The workspace's parts, 16-byte aligned, from `base` (0: only the size is wanted).
Work work_layout(uintptr_t base, u32 n, u32 n_runs) {
  Work w;
  u64 off = 0;
  auto take = [&](u64 bytes) {
    const uintptr_t r = base + off;
    off += (bytes + 15) & ~15ull;
    return r;
  };
  w.pref = reinterpret_cast<u64*>(take(8ull * n));
  w.scan = reinterpret_cast<u64*>(take(24ull * ((u64)n + 1)));
  w.parts = reinterpret_cast<u64*>(take(8 * flat_scan_parts_words(n)));
  w.ida = reinterpret_cast<u32*>(take(4ull * n));
  w.idb = reinterpret_cast<u32*>(take(4ull * n));
  // a level has at most n / kMergeTile + (pairs) tiles and one more slot per pair
  w.mpart = reinterpret_cast<u32*>(take(4ull * ((u64)n / kMergeTile + 2ull * n_runs + 2)));
  w.bytes = off;
  return w;
}

}  // namespace

uint64_t merge_work_bytes(uint32_t n, uint32_t n_runs) { return work_layout(0, n, n_runs).bytes; }

hipError_t launch_merge(const MergeLaunch& a, hipStream_t stream) {
  const u32 n = a.n, R = a.n_runs;
  const Work w = work_layout(reinterpret_cast<uintptr_t>(a.work), n, R);
  MergeParams p{};
  p.keys = a.keys;
  p.kpos = a.kpos;
  p.key_bytes = a.key_bytes;
  p.vals = a.vals;
  p.vpos = a.vpos;
  p.val_bytes = a.val_bytes;
  p.n = n;
  p.n_runs = R;
  p.pref = w.pref;
  for (u32 r = 0; r <= TPZ_MERGE_MAX_RUNS; r++) p.run_first[r] = a.run_first[r < R ? r : R];
  hipError_t e = hipMemsetAsync(a.info, 0xFF, 32, stream);   // info[3] = UINT64_MAX: no empty key
  if (e != hipSuccess) return e;
  const u32 grid_n = (n + 255) / 256;
  hipLaunchKernelGGL(merge_prefix_kernel, dim3(grid_n), dim3(256), 0, stream, a.keys, a.kpos,
                     a.key_bytes, n, w.pref, w.ida, a.info);
  u32* in = w.ida;
  u32* out = w.idb;
  for (u32 lvl = 0; (1u << lvl) < R; lvl++) {
    const u32 wd = 1u << lvl;
    const u32 nlists = (R + wd - 1) / wd, npairs = nlists / 2;
    u32 tiles = 0;
    for (u32 q = 0; q < npairs; q++) {
      const u32 r0 = 2 * q * wd, r2 = r0 + 2 * wd;
      tiles += (a.run_first[r2 < R ? r2 : R] - a.run_first[r0] + kMergeTile - 1) / kMergeTile;
    }
    const u32 nslots = tiles + npairs;
    hipLaunchKernelGGL(merge_partition_kernel, dim3((nslots + 255) / 256), dim3(256), 0, stream, p, lvl,
                       npairs, nslots, in, w.mpart);
    if (tiles)
      hipLaunchKernelGGL(merge_tile_kernel, dim3(tiles), dim3(kMgThreads), 0, stream, p, lvl, npairs, in,
                         w.mpart, out);
    if (nlists & 1) {   // the odd last list passes through
      const u32 x0 = a.run_first[(nlists - 1) * wd];
      if (n > x0) {
        e = hipMemcpyAsync(out + x0, in + x0, 4ull * (n - x0), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
      }
    }
    u32* t = in;
    in = out;
    out = t;
  }
  hipLaunchKernelGGL(merge_drop_kernel, dim3(grid_n), dim3(256), 0, stream, p, in, w.scan);
  launch_scan3_u64(w.scan, n, w.parts, stream);
  GatherOut o{a.out_keys, a.out_kpos, a.out_vals, a.out_vpos, a.src_entry, a.info};
  hipLaunchKernelGGL(merge_gather_kernel, dim3(grid_n), dim3(256), 0, stream, p, in, w.scan, o);
  return hipGetLastError();
}

}  // namespace tpz

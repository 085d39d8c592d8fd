// tpz_membuild.hip — tpz_mem_build: a memtable run built on the device from entries in arrival
// order (a write batch, or the records of a WAL image), and tpz_wal_entries, which splits a WAL
// image in HBM into those entries.
//
// The reference has two rules (src/mem_table.rs):
//   REPLAY  MemTable::open (:119-143) over WalIterator (src/wal/iterator.rs): records are read
//           while the key is non-empty (:125, iterator.rs:30-32): the first empty key ends the
//           replay. map.insert (:129) replaces: the LAST record of a key wins. size (:128) adds
//           klen + vlen of every record read.
//   PUT     do_mem_put (:169-196) per entry with the version of its WAL append (:156, :162: one
//           version per put_entries batch). compare_insert(.., |x| x.version < version) (:179-181)
//           replaces only on a strictly greater version, so the entry the map holds for a key is
//           the FIRST one, in arrival order, of the key's highest version. The size update
//           (:185-195) runs whenever the entry the map then holds has this entry's version: for the
//           entry that inserted or replaced, and also for a later entry of the same key and the
//           same version, which compare_insert turned away (it returns the entry it kept, whose
//           version equals this one's, :185). old_size (:170-174) is klen + the value length of the
//           entry the map held before the call:
//             no such entry                      size += klen + vlen
//             klen + vlen >= old_size (:189)     size += vlen - vlen_held
//             otherwise (:193)                   size -= old_size - klen + vlen = vlen_held + vlen
//           (the reference's operator precedence, kept), wrapping as usize does.
// With versions non-decreasing in arrival order (a precondition: they are WAL append counters; what
// the passes below rely on is only that the entries of one key have them non-decreasing) the entry
// held before entry e is the first entry of e's own version if e is not that entry, else the
// first entry of the key's previous version. Every term depends on e and that one entry, and the
// wrapping sum does not depend on the order: a parallel reduction.
//
// Passes (no launch waits on another workgroup; every launch runs to completion on its own):
//   tile sort  a workgroup per kMergeTile entries: prefixes (the key's first 8 bytes, big-endian,
//              zero padded) and ids into LDS (12 KiB), the first empty key into info[3], a bitonic
//              sort there by {prefix, key bytes past the eighth, lengths, entry id}: a total order,
//              so no stability question arises. Key bytes are read from HBM only on prefix ties.
//   ceil(log2 tiles) x { partition, tile merge }: tpz_merge.hip's passes (tpz_merge_dev.h) over
//              lists of kMergeTile << level entries; an odd last list is copied through.
//   pick       one thread per sorted position. Equal keys are adjacent, in arrival order. REPLAY:
//              an entry is live iff its id is below info[3]; the winner is the live entry whose
//              successor is dead or another key. PUT: the heads of the version subgroups are found
//              from the predecessor; the entry held before this one and, for a head, the end of
//              its subgroup by galloping bisections (O(log group) compares, never a walk). Writes
//              {keep, kept key bytes, kept value bytes} for the scans and adds the size terms:
//              wave and workgroup reduction, one atomic per workgroup into info[4].
//   scan       the flat layout's three-array scan (tpz_flat.hip)
//   gather     a thread per sorted position: positions, source ids, prefixes, versions, then the
//              kept entry's key and value (tpz_copy.h: its own lane up to kLaneCopyMax bytes, the
//              whole wave past that).
// Versions that decrease or positions that are not monotone leave the outputs unspecified but in
// bounds: every loop is bounded, every id is clamped to n - 1, every span to its column, and the
// gather cuts what would pass the output capacities.
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
using mergedev::u32;
using mergedev::u64;

constexpr u32 kPad = 0xFFFFFFFFu;   // a tile's filler past n: after every entry

struct SortParams {
  const uint8_t* keys;
  const u64* kpos;
  u64 key_bytes;
  const uint8_t* vals;
  const u64* vpos;
  u64 val_bytes;
  u32 n;
  u64* pref;

  // Lists of a level are kMergeTile << lvl entries long (the last one shorter).
  __device__ __forceinline__ Pair pair_of(u32 lvl, u32 q) const {
    const u64 len = (u64)kMergeTile << lvl;
    const u64 a = 2 * q * len;
    Pair x;
    x.a0 = (u32)mergedev::min64(a, n);
    x.a1 = (u32)mergedev::min64(a + len, n);
    x.b1 = (u32)mergedev::min64(a + 2 * len, n);
    return x;
  }
  // Every pair but the last has 2 << lvl tiles: the pair of index t in closed form.
  __device__ __forceinline__ bool find_pair(u32 lvl, u32 npairs, u32 t, u32 extra, u32& q, u32& k,
                                            u32& tile0) const {
    const u32 tp = 2u << lvl;
    q = t / (tp + extra);
    if (q >= npairs) return false;
    k = t - q * (tp + extra);
    tile0 = q * tp;
    return k < mergedev::tiles_of(pair_of(lvl, q)) + extra;
  }
  // {key, entry id}: a total order.
  __device__ __forceinline__ bool less(u32 a, u64 pa, u32 b, u64 pb) const {
    if (pa != pb) return pa < pb;
    const int c = mergedev::tail_cmp(*this, a, b);
    return c ? c < 0 : a < b;
  }
  __device__ __forceinline__ bool key_equal(u32 a, u64 pa, u32 b) const {
    return pref[b] == pa && mergedev::tail_cmp(*this, a, b) == 0;
  }
};

__device__ __forceinline__ bool pad_less(const SortParams& p, u32 a, u64 pa, u32 b, u64 pb) {
  if (a == kPad) return false;
  if (b == kPad) return true;
  return p.less(a, pa, b, pb);
}

__global__ __launch_bounds__(kMgThreads) void mb_tile_sort_kernel(SortParams p, u32* out, u64* info) {
  __shared__ u64 s_pref[kMergeTile];
  __shared__ u32 s_id[kMergeTile];
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x * kMergeTile;
  for (u32 i = tid; i < kMergeTile; i += kMgThreads) {
    const u64 e64 = base + i;
    u32 id = kPad;
    u64 x = 0;
    if (e64 < p.n) {
      id = (u32)e64;
      u64 at, len;
      span(p.kpos, p.key_bytes, id, at, len);
      for (u32 b = 0; b < 8; b++) x = (x << 8) | (b < len ? p.keys[at + b] : 0u);
      p.pref[id] = x;
      if (len == 0) atomicMin(reinterpret_cast<unsigned long long*>(info + 3), (unsigned long long)id);
    }
    s_id[i] = id;
    s_pref[i] = x;
  }
  __syncthreads();
  for (u32 k = 2; k <= kMergeTile; k <<= 1) {
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      for (u32 t = tid; t < kMergeTile / 2; t += kMgThreads) {
        const u32 lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const u32 a = s_id[lo], b = s_id[hi];
        const u64 pa = s_pref[lo], pb = s_pref[hi];
        const bool up = (lo & k) == 0;
        // swap iff the pair is out of order for its direction
        if (up ? pad_less(p, b, pb, a, pa) : pad_less(p, a, pa, b, pb)) {
          s_id[lo] = b;
          s_pref[lo] = pb;
          s_id[hi] = a;
          s_pref[hi] = pa;
        }
      }
      __syncthreads();
    }
  }
  for (u32 i = tid; i < kMergeTile; i += kMgThreads)
    if (base + i < p.n) out[base + i] = s_id[i];   // (the pads are last: these are all entries)
}

__global__ __launch_bounds__(256) void mb_partition_kernel(SortParams p, u32 lvl, u32 npairs,
                                                            u32 nslots, const u32* in, u32* part) {
  mergedev::partition_body(p, lvl, npairs, nslots, in, part);
}

__global__ __launch_bounds__(kMgThreads) void mb_tile_merge_kernel(SortParams p, u32 lvl, u32 npairs,
                                                                    const u32* in, const u32* part,
                                                                    u32* out) {
  __shared__ u64 s_pref[kMergeTile];
  __shared__ u32 s_id[kMergeTile];
  mergedev::tile_body(p, lvl, npairs, in, part, out, s_pref, s_id);
}

// The smallest h <= start with ok(h), where ok(start) holds and ok is true on a range ending at
// start: doubling steps back, then a bisection between the last bad and the first good probe.
template <class Ok>
__device__ __forceinline__ u32 gallop_back(u32 start, Ok ok) {
  u32 good = start, bad = 0, step = 1;
  bool have_bad = false;
  for (int it = 0; it < 33 && good > 0; it++) {
    const u32 probe = good > step ? good - step : 0;
    if (ok(probe)) {
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
      if (ok(mid)) good = mid;
      else bad = mid;
    }
  }
  return good;
}

// The largest e >= start, e < n, with ok(e), ok true on a range starting at start.
template <class Ok>
__device__ __forceinline__ u32 gallop_fwd(u32 start, u32 n, Ok ok) {
  u32 good = start, bad = n, step = 1;   // (bad = n: past the end)
  for (int it = 0; it < 33 && good + 1 < n; it++) {
    const u32 probe = n - 1 - good > step ? good + step : n - 1;
    if (ok(probe)) {
      good = probe;
      step <<= 1;
    } else {
      bad = probe;
      break;
    }
  }
  for (int it = 0; it < 33 && good + 1 < bad; it++) {
    const u32 mid = good + (bad - good) / 2;
    if (ok(mid)) good = mid;
    else bad = mid;
  }
  return good;
}

// scan[0][i] = keep, scan[1][i] = its key bytes if kept, scan[2][i] = its value bytes if kept;
// info[4] += the size terms.
__global__ __launch_bounds__(256) void mb_pick_kernel(SortParams p, u32 mode, const u64* ver,
                                                       const u32* m, u64* scan, u64* info) {
  const u64 i64 = (u64)blockIdx.x * 256 + threadIdx.x;
  u64 term = 0;
  if (i64 < p.n) {
    const u32 i = (u32)i64;
    const u32 id = clamp_id(m[i], p.n);
    const u64 pf = p.pref[id];
    u64 at, kl, vl;
    span(p.kpos, p.key_bytes, id, at, kl);
    span(p.vpos, p.val_bytes, id, at, vl);
    bool keep;
    if (mode == TPZ_MEM_REPLAY) {
      const u64 stop = info[3];                      // the first empty key ends the replay
      const bool live = id < stop;
      keep = live;
      if (live && i + 1 < p.n) {
        const u32 nx = clamp_id(m[i + 1], p.n);
        if (nx < stop && p.key_equal(id, pf, nx)) keep = false;   // a later record replaces it
      }
      term = live ? kl + vl : 0;
    } else {
      const u64 v = ver[id];
      const bool has_prev = i > 0 && p.key_equal(id, pf, clamp_id(m[i - 1], p.n));
      const bool head = !has_prev || ver[clamp_id(m[i - 1], p.n)] != v;   // of its version subgroup
      if (!has_prev) {
        term = kl + vl;
      } else {
        // the entry the map held: the head of this subgroup, or of the one before it
        const u32 from = head ? i - 1 : i;
        const u64 hv = head ? ver[clamp_id(m[from], p.n)] : v;
        const u32 h = gallop_back(from, [&](u32 j) {
          const u32 e = clamp_id(m[j], p.n);
          return p.key_equal(id, pf, e) && ver[e] == hv;
        });
        u64 hl;
        span(p.vpos, p.val_bytes, clamp_id(m[h], p.n), at, hl);
        term = vl >= hl ? vl - hl : 0 - (hl + vl);
      }
      keep = false;
      if (head) {   // the winner iff no entry of the key has a later version
        const u32 e = gallop_fwd(i, p.n, [&](u32 j) {
          const u32 x = clamp_id(m[j], p.n);
          return p.key_equal(id, pf, x) && ver[x] == v;
        });
        keep = !(e + 1 < p.n && p.key_equal(id, pf, clamp_id(m[e + 1], p.n)));
      }
    }
    const u64 st = (u64)p.n + 1;
    scan[i] = keep ? 1 : 0;
    scan[st + i] = keep ? kl : 0;
    scan[2 * st + i] = keep ? vl : 0;
  }
  // one atomic per workgroup (they all hit one address): waves first, then their four sums
  __shared__ u64 s_term[256 / 64];
  for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
  if (copydev::lane_id() == 0) s_term[threadIdx.x / 64] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 sum = s_term[0] + s_term[1] + s_term[2] + s_term[3];
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(info + 4), (unsigned long long)sum);
  }
}

using copydev::lane_copy;
using copydev::lane_id;
using copydev::wave_copy;

constexpr u64 kLaneCopyMax = 256;   // as tpz_merge.hip's gather

struct BuildOut {
  uint8_t* keys;
  u64* kpos;
  uint8_t* vals;
  u64* vpos;
  u64* prefix;      // or null
  u32* src_entry;   // or null
  u64* version;     // or null
  u64* info;
};

__global__ __launch_bounds__(256) void mb_gather_kernel(SortParams p, u32 mode, const u64* ver,
                                                         const u32* m, const u64* scan, BuildOut o) {
  const u32 lane = lane_id();
  const u64 st = (u64)p.n + 1;
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;   // (a wave's 64 positions are consecutive)
  if (i == 0) {
    const u64 n_out = scan[p.n], kb = scan[st + p.n], vb = scan[2 * st + p.n];
    o.info[0] = n_out;
    o.info[1] = kb;
    o.info[2] = vb;
    o.info[5] = mode == TPZ_MEM_REPLAY ? mergedev::min64(o.info[3], p.n) : p.n;
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
      if (o.prefix) o.prefix[out] = p.pref[id];
      if (o.src_entry) o.src_entry[out] = id;
      if (o.version) o.version[out] = mode == TPZ_MEM_PUT ? ver[id] : 0;   // open(): version 0 (:133)
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
// The workspace's parts, 16-byte aligned, from `base` (0: only the size is wanted): 40 bytes per
// entry plus the scan's partial sums and a partition slot per tile and pair.
Work work_layout(uintptr_t base, u32 n) {
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
  // a level has at most ceil(n / kMergeTile) tiles and one more slot per pair (<= tiles / 2 + 1)
  w.mpart = reinterpret_cast<u32*>(take(4ull * (2ull * ((u64)n / kMergeTile) + 8)));
  w.bytes = off;
  return w;
}

// ---- tpz_wal_entries ---------------------------------------------------------------------------
// A record is BE u16 klen | key | BE u16 vlen | value (Entry::encode, src/block/builder.rs:72-81;
// WalIterator::next reads it back, src/wal/iterator.rs:39-44).
struct WalParams {
  const uint8_t* img;
  u64 img_bytes;
  const u64* rec;   // n + 1 record starts
  u32 n;
  uint8_t* keys;
  u64* kpos;
  uint8_t* vals;
  u64* vpos;
  u64* info;
};

// Record i's key and value lengths, re-read from the image and checked against the record starts:
// false (and empty spans) unless rec[i] + 4 + klen + vlen == rec[i + 1] inside the image.
__device__ __forceinline__ bool wal_record(const WalParams& p, u32 i, u64& r0, u64& kl, u64& vl) {
  r0 = p.rec[i];
  const u64 r1 = p.rec[i + 1];
  kl = vl = 0;
  if (r1 > p.img_bytes || r0 > r1 || r1 - r0 < 4) return false;
  const u64 k = ((u64)p.img[r0] << 8) | p.img[r0 + 1];
  if (k > r1 - r0 - 4) return false;
  const u64 v = ((u64)p.img[r0 + 2 + k] << 8) | p.img[r0 + 3 + k];
  if (r0 + 4 + k + v != r1) return false;
  kl = k;
  vl = v;
  return true;
}

__global__ __launch_bounds__(256) void wal_len_kernel(WalParams p) {
  const u64 i64 = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= p.n) return;
  const u32 i = (u32)i64;
  u64 r0, kl, vl;
  if (!wal_record(p, i, r0, kl, vl))
    atomicMin(reinterpret_cast<unsigned long long*>(p.info + 3), (unsigned long long)i);
  p.kpos[i] = kl;
  p.vpos[i] = vl;
}

__global__ __launch_bounds__(256) void wal_copy_kernel(WalParams p) {
  const u32 lane = lane_id();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    p.info[0] = p.n;
    p.info[1] = p.kpos[p.n];
    p.info[2] = p.vpos[p.n];
  }
  u64 r0 = 0, kl = 0, vl = 0, kd = 0, vd = 0;
  if (i < p.n) {
    if (!wal_record(p, (u32)i, r0, kl, vl)) r0 = 0;
    kd = p.kpos[i];
    vd = p.vpos[i];
  }
  const uint8_t* ks = p.img + r0 + 2;        // (read only for kl, vl > 0: a checked record)
  const uint8_t* vs = p.img + r0 + 4 + kl;
  if (kl && kl <= kLaneCopyMax) lane_copy(p.keys, p.img_bytes, kd, ks, kl);
  if (vl && vl <= kLaneCopyMax) lane_copy(p.vals, p.img_bytes, vd, vs, vl);
  u64 mask = __ballot(kl > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    wave_copy(p.keys, p.img_bytes, __shfl(kd, l, 64), p.img + __shfl(r0, l, 64) + 2, __shfl(kl, l, 64), lane);
  }
  mask = __ballot(vl > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    const u64 r = __shfl(r0, l, 64), k = __shfl(kl, l, 64);
    wave_copy(p.vals, p.img_bytes, __shfl(vd, l, 64), p.img + r + 4 + k, __shfl(vl, l, 64), lane);
  }
}

}  // namespace

uint64_t membuild_work_bytes(uint32_t n) { return work_layout(0, n).bytes; }

hipError_t launch_membuild(const MemBuildLaunch& a, hipStream_t stream) {
  const u32 n = a.n;
  const Work w = work_layout(reinterpret_cast<uintptr_t>(a.work), n);
  SortParams p{a.keys, a.kpos, a.key_bytes, a.vals, a.vpos, a.val_bytes, n, w.pref};
  hipError_t e = hipMemsetAsync(a.info, 0, 64, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.info + 3, 0xFF, 8, stream);   // info[3] = UINT64_MAX: no empty key
  if (e != hipSuccess) return e;
  const u32 tiles = (u32)(((u64)n + kMergeTile - 1) / kMergeTile);
  u32* in = w.ida;
  u32* out = w.idb;
  hipLaunchKernelGGL(mb_tile_sort_kernel, dim3(tiles), dim3(kMgThreads), 0, stream, p, in, a.info);
  for (u32 lvl = 0; ((u64)kMergeTile << lvl) < n; lvl++) {
    const u64 len = (u64)kMergeTile << lvl;
    const u32 nlists = (u32)((n + len - 1) / len), npairs = nlists / 2;
    // every pair but the last has 2 << lvl tiles; the last covers what is left of its range
    const u64 last0 = 2 * (u64)(npairs - 1) * len;
    const u64 last1 = last0 + 2 * len < n ? last0 + 2 * len : n;
    const u32 mtiles = (npairs - 1) * (2u << lvl) + (u32)((last1 - last0 + kMergeTile - 1) / kMergeTile);
    const u32 nslots = mtiles + npairs;
    hipLaunchKernelGGL(mb_partition_kernel, dim3((nslots + 255) / 256), dim3(256), 0, stream, p, lvl,
                       npairs, nslots, in, w.mpart);
    hipLaunchKernelGGL(mb_tile_merge_kernel, dim3(mtiles), dim3(kMgThreads), 0, stream, p, lvl, npairs,
                       in, w.mpart, out);
    if (nlists & 1) {   // the odd last list passes through
      const u64 x0 = (u64)(nlists - 1) * len;
      e = hipMemcpyAsync(out + x0, in + x0, 4ull * (n - x0), hipMemcpyDeviceToDevice, stream);
      if (e != hipSuccess) return e;
    }
    u32* t = in;
    in = out;
    out = t;
  }
  if (a.stop_after == 1) return hipGetLastError();
  const u32 grid_n = (n + 255) / 256;
  hipLaunchKernelGGL(mb_pick_kernel, dim3(grid_n), dim3(256), 0, stream, p, a.mode, a.version, in,
                     w.scan, a.info);
  launch_scan3_u64(w.scan, n, w.parts, stream);
  if (a.stop_after == 2) return hipGetLastError();
  BuildOut o{a.out_keys, a.out_kpos, a.out_vals, a.out_vpos, a.out_prefix, a.src_entry,
             a.out_version, a.info};
  hipLaunchKernelGGL(mb_gather_kernel, dim3(grid_n), dim3(256), 0, stream, p, a.mode, a.version, in,
                     w.scan, o);
  return hipGetLastError();
}

uint64_t wal_entries_work_bytes(uint32_t n) { return 8 * (flat_scan_parts_words(n) / 3); }

hipError_t launch_wal_entries(const WalEntriesLaunch& a, hipStream_t stream) {
  WalParams p{a.img, a.img_bytes, a.rec, a.n, a.keys, a.kpos, a.vals, a.vpos, a.info};
  hipError_t e = hipMemsetAsync(a.info, 0, 24, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.info + 3, 0xFF, 8, stream);   // info[3] = UINT64_MAX: every record checks
  if (e != hipSuccess) return e;
  const u32 grid_n = (a.n + 255) / 256;
  hipLaunchKernelGGL(wal_len_kernel, dim3(grid_n), dim3(256), 0, stream, p);
  launch_scan_u64(a.kpos, a.n, static_cast<u64*>(a.work), stream);
  launch_scan_u64(a.vpos, a.n, static_cast<u64*>(a.work), stream);
  hipLaunchKernelGGL(wal_copy_kernel, dim3(grid_n), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace tpz

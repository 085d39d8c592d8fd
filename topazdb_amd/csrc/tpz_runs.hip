// tpz_runs.hip — tpz_table_runs_layout / tpz_table_runs_entries (include/tpz_gpu.h): the device's
// SsTableIterator (src/table/iterator.rs:10-96) over tables that are resident in HBM. For a list of
// tpz_table descriptors in priority order (sub_compact's this_tables + next_tables,
// src/level.rs:184-197) the entries of every table, block after block, become one run of a
// tpz_entries: dense key and value columns plus absolute entry positions, what tpz_merge_runs and
// the write side take.
//
// In the slotted layout a block's keys are one contiguous range of its slot and its values another
// (a spill record has the same shape, tpz_seek_dev.h block_view), so the gather moves two byte
// ranges per block and is not entry-driven:
//   runs_sizes_kernel   a thread per (run, block): {n, K, V} from the block's status, count and last
//                       {kend, vend} pair; the first block that is not OK / OK_SPILLED
//   launch_scan3_u64    the three exclusive scans in run order (tpz_flat.hip)
//   runs_finish_kernel  the run table (entries before every run) and the totals
//   runs_gather_kernel  a wave per block: the entry positions as coalesced u64 stores, then the two
//                       ranges with copydev::wave_copy. The destinations have any alignment: a
//                       lane takes one 16-byte-aligned piece of the destination and stores 16
//                       bytes; the first and last piece of a range also hold the neighbouring
//                       blocks' bytes and are stored byte by byte, so no two blocks store the same
//                       byte and no block waits for another.
// The kernel has a second form (kAligned, behind the diagnostic export tpz_debug_table_runs_entries):
// instead of wave_copy's one unaligned 16-byte load per piece, a lane loads the one or two ALIGNED
// 16-byte source words that hold its bytes and shifts them by the range's uniform misalignment
// (v_alignbyte). It measured slower (0.277 against 0.244 ms for 487 MB, DESIGN.md §3.18: two loads
// and 84 VGPRs per lane against one and 28), so the product call takes the simpler form.
//
// Every index read from device memory is clamped: a block past the descriptor's n_blocks holds
// nothing, n is at most the block's reserved pairs (65535 for a spill record), K and V stay inside
// the slot, an entry's end is at most K / V, and the gather never takes more than the layout
// reserved for the block. All positions are u64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_internal.h"

namespace tpz {
namespace {

typedef uint32_t u32;
typedef uint64_t u64;

constexpr int kRnWaves = 4;   // blocks per gather workgroup (one per wave)

struct RunsParams {
  const tpz_table* tabs;
  u32 n_runs;
  u32 nb;                                      // block_first[n_runs]
  u32 block_first[TPZ_MERGE_MAX_RUNS + 1];
};

// The run that holds block g: the largest r with block_first[r] <= g (tables without blocks share
// a start with the run after them and are passed over).
__device__ __forceinline__ u32 run_of(const RunsParams& p, u32 g) {
  u32 lo = 0, hi = p.n_runs;   // block_first[lo] <= g < block_first[hi]
  for (int it = 0; it < 10 && lo + 1 < hi; it++) {
    const u32 mid = (lo + hi) / 2;
    if (p.block_first[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What block b of table t gives a run: its entries, key bytes and value bytes, its {kend, vend}
// pairs and its stream (keys from 0, values from value_start(K)).
struct Shape {
  bool ok;       // OK or OK_SPILLED, inside the table
  u32 n, k, v;
  const u32* ends;
  const uint8_t* stream;
};
__device__ __forceinline__ Shape block_shape(const tpz_table& t, u32 b) {
  Shape s{false, 0, 0, 0, nullptr, nullptr};
  if (b >= t.n_blocks) return s;
  const u32 st = t.d_status[b];
  if (st == TPZ_BLOCK_OK) {
    const u64 e0 = t.d_ext[b], e1 = t.d_ext[b + 1];
    if (e1 < e0) return s;
    const u64 sb = slot_base(e0, b), slot = slot_base(e1, (u64)b + 1) - sb;
    const u64* ef = t.d_entry_first;
    const u64 p0 = ends_base(ef, e0, b), p1 = ends_base(ef, e1, (u64)b + 1);
    u64 n = t.d_count[b];
    if (n > 65535u) n = 65535u;
    if (n > (p1 > p0 ? p1 - p0 : 0)) n = p1 > p0 ? p1 - p0 : 0;
    s.ok = true;
    s.n = (u32)n;
    s.ends = t.d_ends + 2 * p0;
    s.stream = t.d_data + sb;
    if (n) {
      u64 k = s.ends[2 * (n - 1)], v = s.ends[2 * (n - 1) + 1];
      if (k > slot) k = slot;
      const u64 room = slot > value_start(k) ? slot - value_start(k) : 0;
      if (v > room) v = room;
      s.k = (u32)k;
      s.v = (u32)v;
    }
  } else if (st == TPZ_BLOCK_OK_SPILLED && t.d_spill) {
    const uint8_t* r = t.d_spill + t.d_spill_off[b];
    u32 n = t.d_count[b];
    if (n > 65535u) n = 65535u;
    s.ok = true;
    s.n = n;
    s.ends = reinterpret_cast<const u32*>(r);
    s.stream = r + spill_stream(n);
    if (n) {
      const u32 lim = 65535u * 65535u;
      const u32 k = s.ends[2 * (n - 1)], v = s.ends[2 * (n - 1) + 1];
      s.k = k < lim ? k : lim;
      s.v = v < lim ? v : lim;
    }
  }
  return s;
}

__global__ __launch_bounds__(256) void runs_sizes_kernel(RunsParams p, u64* first, u64* info) {
  const u64 g64 = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g64 >= p.nb) return;
  const u32 g = (u32)g64;
  const u32 r = run_of(p, g), b = g - p.block_first[r];
  const Shape s = block_shape(p.tabs[r], b);
  const u64 st = (u64)p.nb + 1;
  first[g] = s.n;
  first[st + g] = s.k;
  first[2 * st + g] = s.v;
  if (!s.ok)
    atomicMin(reinterpret_cast<unsigned long long*>(info + 3), ((unsigned long long)r << 32) | b);
}

__global__ __launch_bounds__(512) void runs_finish_kernel(RunsParams p, const u64* first,
                                                          u32* run_first, u64* info) {
  const u32 r = threadIdx.x;
  const u64 st = (u64)p.nb + 1;
  if (r <= p.n_runs) {
    const u64 e = first[p.block_first[r < p.n_runs ? r : p.n_runs]];
    run_first[r] = e < 0xFFFFFFFFull ? (u32)e : 0xFFFFFFFFu;
  }
  if (r < 3) info[r] = first[r * st + p.nb];
}

// Sixteen bytes held as four words by value: the funnel shift and the byte picks below are selects
// between registers. (Through a uint4 reference the selects become selects between addresses of a
// private copy, which the compiler keeps in LDS; so does a switch over the four word offsets.)
struct Words {
  u32 x, y, z, w;
};
// {b : a} (a = the low 16 bytes) shifted right by sh bytes (0..15, uniform), the low 16 bytes: by 8
// bytes, then by 4, as selects on the uniform shift, then by bytes (v_alignbyte).
__device__ __forceinline__ Words funnel(Words a, Words b, u32 sh) {
  const bool s8 = (sh & 8u) != 0, s4 = (sh & 4u) != 0;
  const u32 z0 = s8 ? a.z : a.x, z1 = s8 ? a.w : a.y, z2 = s8 ? b.x : a.z, z3 = s8 ? b.y : a.w,
            z4 = s8 ? b.z : b.x, z5 = s8 ? b.w : b.y;
  const u32 y0 = s4 ? z1 : z0, y1 = s4 ? z2 : z1, y2 = s4 ? z3 : z2, y3 = s4 ? z4 : z3,
            y4 = s4 ? z5 : z4;
  const u32 s = sh & 3u;
  return Words{__builtin_amdgcn_alignbyte(y1, y0, s), __builtin_amdgcn_alignbyte(y2, y1, s),
               __builtin_amdgcn_alignbyte(y3, y2, s), __builtin_amdgcn_alignbyte(y4, y3, s)};
}
// Byte i (0..15) of v.
__device__ __forceinline__ u32 byte_at(Words v, u32 i) {
  const u32 q = i >> 2;
  const u32 lo = q == 0 ? v.x : v.y, hi = q == 2 ? v.z : v.w;
  return ((q < 2 ? lo : hi) >> (8 * (i & 3u))) & 0xFFu;
}

// copydev::wave_copy with aligned loads (the diagnostic form): the whole wave copies src[0 .. len) to dst[d .. d + len)
// (dst 16-byte aligned, cap bytes). The source byte of dst byte x lies at P + x, P = src - d, so
// every 16-byte piece of dst reads the aligned source words w and w + 16 shifted by sh = P & 15,
// the same for all pieces. A word is loaded only when the piece takes a byte of it: no load
// reaches past the aligned 16 bytes that hold the range's first and last byte.
__device__ __forceinline__ void wave_copy_aligned(uint8_t* dst, u64 cap, u64 d, const uint8_t* src,
                                                  u64 len, u32 lane) {
  if (d >= cap) return;
  if (len > cap - d) len = cap - d;
  if (len == 0) return;
  const u64 c0 = d & ~15ull, end = d + len;
  const u64 pieces = (((end + 15) & ~15ull) - c0) >> 4;
  const u64 p0 = (u64)reinterpret_cast<uintptr_t>(src) + c0 - d;   // source of dst byte c0
  const u32 sh = __builtin_amdgcn_readfirstlane((u32)(p0 & 15u));
  const u64 w0 = p0 & ~15ull;
  for (u64 c = lane; c < pieces; c += 64) {
    const u64 cb = c0 + 16 * c;
    const u64 lo = (cb > d ? cb : d), hi = (cb + 16 < end ? cb + 16 : end);
    const u32 i0 = (u32)(lo - cb), i1 = (u32)(hi - cb);            // the piece's bytes [i0, i1)
    const uint4* w = reinterpret_cast<const uint4*>(static_cast<uintptr_t>(w0 + 16 * c));
    Words a{0, 0, 0, 0}, b{0, 0, 0, 0};
    if (i0 < 16u - sh) {
      const uint4 t = w[0];
      a = Words{t.x, t.y, t.z, t.w};
    }
    if (sh && i1 > 16u - sh) {
      const uint4 t = w[1];
      b = Words{t.x, t.y, t.z, t.w};
    }
    const Words v = funnel(a, b, sh);
    if (i1 - i0 == 16) {
      *reinterpret_cast<uint4*>(dst + cb) = make_uint4(v.x, v.y, v.z, v.w);
    } else {
      for (u32 x = i0; x < i1; x++) dst[cb + x] = (uint8_t)byte_at(v, x);
    }
  }
}

template <bool kAligned>
__device__ __forceinline__ void copy_range(uint8_t* dst, u64 cap, u64 d, const uint8_t* src, u64 len,
                                           u32 lane) {
  if (kAligned) wave_copy_aligned(dst, cap, d, src, len, lane);
  else copydev::wave_copy(dst, cap, d, src, len, lane);
}

template <bool kAligned>
__global__ __launch_bounds__(256) void runs_gather_kernel(RunsParams p, const u64* first,
                                                          uint8_t* keys, u64 key_cap, u64* kpos,
                                                          uint8_t* vals, u64 val_cap, u64* vpos,
                                                          u64 entry_cap) {
  const u32 lane = copydev::lane_id(), wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u64 g64 = (u64)blockIdx.x * kRnWaves + wid;
  if (g64 >= p.nb) return;
  const u32 g = (u32)g64;
  const u32 r = run_of(p, g), b = g - p.block_first[r];
  const Shape s = block_shape(p.tabs[r], b);
  const u64 st = (u64)p.nb + 1;
  const u64 e0 = first[g], kb = first[st + g], vb = first[2 * st + g];
  // never more than the layout reserved for this block, whatever the columns hold by now
  const u64 er = first[g + 1] - e0, kr = first[st + g + 1] - kb, vr = first[2 * st + g + 1] - vb;
  const u64 n = s.n < er ? s.n : er;
  const u64 K = s.k < kr ? s.k : kr, V = s.v < vr ? s.v : vr;
  for (u64 j = lane; j < n; j += 64) {
    const u64 e = e0 + j;
    u64 k = 0, v = 0;
    if (j) {
      k = s.ends[2 * (j - 1)];
      v = s.ends[2 * (j - 1) + 1];
      if (k > K) k = K;
      if (v > V) v = V;
    }
    if (e <= entry_cap) {
      kpos[e] = kb + k;
      vpos[e] = vb + v;
    }
  }
  if (g == p.nb - 1 && lane == 0) {
    const u64 total = first[p.nb];
    if (total <= entry_cap) {
      kpos[total] = first[st + p.nb];
      vpos[total] = first[2 * st + p.nb];
    }
  }
  if (K) copy_range<kAligned>(keys, key_cap, kb, s.stream, K, lane);
  if (V) copy_range<kAligned>(vals, val_cap, vb, s.stream + value_start(s.k), V, lane);
}

RunsParams make_params(const tpz_table* tabs, u32 n_runs, const u32* h_block_first) {
  RunsParams p;
  p.tabs = tabs;
  p.n_runs = n_runs;
  p.nb = h_block_first[n_runs];
  for (u32 r = 0; r <= TPZ_MERGE_MAX_RUNS; r++)
    p.block_first[r] = h_block_first[r < n_runs ? r : n_runs];
  return p;
}

}  // namespace

void launch_table_runs_layout(const tpz_table* tabs, u32 n_runs, const u32* h_block_first, u64* first,
                              u32* run_first, u64* info, u64* part, hipStream_t stream) {
  const RunsParams p = make_params(tabs, n_runs, h_block_first);
  (void)hipMemsetAsync(info, 0, 24, stream);
  (void)hipMemsetAsync(info + 3, 0xFF, 8, stream);
  if (p.nb == 0) {
    (void)hipMemsetAsync(first, 0, 3 * 8, stream);
    (void)hipMemsetAsync(run_first, 0, 4 * ((size_t)n_runs + 1), stream);
    return;
  }
  hipLaunchKernelGGL(runs_sizes_kernel, dim3((p.nb + 255) / 256), dim3(256), 0, stream, p, first, info);
  launch_scan3_u64(first, p.nb, part, stream);
  hipLaunchKernelGGL(runs_finish_kernel, dim3(1), dim3(512), 0, stream, p, first, run_first, info);
}

void launch_table_runs_entries(const tpz_table* tabs, u32 n_runs, const u32* h_block_first,
                               const u64* first, uint8_t* keys, u64 key_cap, u64* kpos, uint8_t* vals,
                               u64 val_cap, u64* vpos, u64 entry_cap, bool aligned,
                               hipStream_t stream) {
  const RunsParams p = make_params(tabs, n_runs, h_block_first);
  if (p.nb == 0) {
    (void)hipMemsetAsync(kpos, 0, 8, stream);
    (void)hipMemsetAsync(vpos, 0, 8, stream);
    return;
  }
  const dim3 grid((u32)(((u64)p.nb + kRnWaves - 1) / kRnWaves));
  if (aligned)
    hipLaunchKernelGGL(runs_gather_kernel<true>, grid, dim3(256), 0, stream, p, first, keys, key_cap,
                       kpos, vals, val_cap, vpos, entry_cap);
  else
    hipLaunchKernelGGL(runs_gather_kernel<false>, grid, dim3(256), 0, stream, p, first, keys, key_cap,
                       kpos, vals, val_cap, vpos, entry_cap);
}

}  // namespace tpz

// tpz_tables.hip — gfx950 kernels around a whole compaction task's output (do_compact,
// src/level.rs:133-222): the key ranges of its sub-compactions, SsTableBuilder's table cuts and the
// bytes of every output file (tpz_entries_bound, tpz_table_cut, tpz_sst_finish; include/tpz_gpu.h).
//
//   entries_bound_kernel  One thread per probe key: a bisection over the merged entries for the
//                         number of keys below (or at) the probe. A handful of probes per task
//                         (two per sub-compaction): a chain of dependent loads each, nothing to
//                         spread.
//   table_cut_kernel      One workgroup per call. Thread 0 bisects the window's stored extents for
//                         the cut (they are non-decreasing, so `ext[k + 1] + 2 (k + 1) >= capacity`
//                         is monotone in k), patches the plan so that the block after the cut holds
//                         one entry, and bisects the entries' raw bytes for the next window's end;
//                         the workgroup then sums the table's first-key lengths (what the image's
//                         meta block will take).
//   sst_klen_kernel       Per image and 1,024 blocks: the sum of the blocks' first-key lengths.
//   sst_layout_kernel     One workgroup walks the images in order: the exclusive scan of every
//                         image's partial sums, its offsets (meta, bloom, size), the big-endian
//                         offset fields, and the CRC's ranges: image i is range 2i, the bytes up to
//                         the next image range 2i + 1, over the span as one batch, so that the
//                         whole-range CRC kernels (tpz_crc.hip) take every image in one launch. The
//                         walk is sequential because an image is checked against the end of the one
//                         before it.
//   sst_meta_kernel       Per image and 1,024 blocks: a scan of the key lengths in LDS gives every
//                         block's meta its place; a thread writes its block's 6 header bytes and
//                         gathers the key. Destinations have no alignment, so bytes are stored one
//                         by one (a first key per block: 1/34 of the keys on the 4k shape).
//   sst_bloom_kernel      The filter from its 4-byte aligned scratch (tpz_bloom_build's output
//                         rule) to its place in the image: aligned u32 loads, byte stores.
//   sst_crc_kernel        The four big-endian CRC bytes of every image.
//
// Nothing here trusts the sort order or the descriptors: bisections are bounded by the counts,
// entry indices and key positions are clamped to the columns, a descriptor that leaves the span or
// overlaps its predecessor is skipped.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"

namespace tpz {

namespace {

using u32 = uint32_t;
using u64 = uint64_t;

__device__ __forceinline__ u64 min64(u64 a, u64 b) { return a < b ? a : b; }

// ------------------------------------------------------------------ bound search
struct BoundParams {
  const uint8_t* keys;
  const u64* kpos;
  u64 key_bytes;
  u32 n;
  const uint8_t* q;
  const u64* q_pos;
  const uint8_t* incl;
  u32 n_q;
  u32* out;
};

__global__ __launch_bounds__(64) void entries_bound_kernel(BoundParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_q) return;
  const u64 q0 = p.q_pos[i], q1 = p.q_pos[i + 1];
  const u64 ql = q1 > q0 ? q1 - q0 : 0;
  const uint8_t* qk = p.q + q0;
  const bool incl = p.incl[i] != 0;
  u32 lo = 0, hi = p.n;
  for (int it = 0; it < 33 && lo < hi; it++) {
    const u32 mid = lo + (hi - lo) / 2;
    const u64 a = min64(p.kpos[mid], p.key_bytes);
    u64 b = min64(p.kpos[mid + 1], p.key_bytes);
    if (b < a) b = a;
    const u64 kl = b - a;
    const u64 m = min64(kl, ql);
    const uint8_t* k = p.keys + a;
    int c = 0;                       // sign of key - probe over the common prefix
    for (u64 j = 0; j < m; j++) {
      const int x = (int)k[j] - (int)qk[j];
      if (x != 0) {
        c = x;
        break;
      }
    }
    if (c == 0) c = kl < ql ? -1 : (kl > ql ? 1 : 0);
    if (c < 0 || (c == 0 && incl)) lo = mid + 1; else hi = mid;
  }
  p.out[i] = lo;
}

// ------------------------------------------------------------------ table cut
struct CutParams {
  const u64* kpos;
  const u64* vpos;
  u32 start;
  u32 win;
  u32 seg_end;
  u32* first;
  u64* ext;
  const u64* cut_ext;
  u32* info;
  u32 block_size;
  u64 capacity;
  u64* cut;
};

// Entry bytes before entry i (4 + key + value each; DESIGN.md §3.8's S up to a constant).
__device__ __forceinline__ u64 raw_at(const CutParams& p, u32 i) {
  return 4ull * i + p.kpos[i] + p.vpos[i];
}

__global__ __launch_bounds__(256) void table_cut_kernel(CutParams p) {
  __shared__ u32 s_nb;
  __shared__ u64 s_sum[4];
  if (threadIdx.x == 0) {
    u32 nb = 0, status = TPZ_CUT_NONE;
    u64 k = 0, n_ent = p.win, data = 0;
    if (p.win) {
      const u32 bad = p.info[1];
      nb = p.info[2];
      if (nb > p.win) nb = p.win;            // at most a block per entry
      if (bad != 0xFFFFFFFFu) {
        status = TPZ_CUT_BAD_ENTRY;
        k = (u64)p.start + bad;
        nb = 0;
      } else if (nb >= 2) {
        // smallest j in [0, nb - 2] with cut_ext[j + 1] + 2 (j + 1) >= capacity
        u32 lo = 0, hi = nb - 1;
        for (int it = 0; it < 33 && lo < hi; it++) {
          const u32 mid = lo + (hi - lo) / 2;
          if (p.cut_ext[mid + 1] + 2ull * (mid + 1) >= p.capacity) hi = mid; else lo = mid + 1;
        }
        if (lo < nb - 1) {
          status = TPZ_CUT_FOUND;
          k = lo;
          u32 e = p.first[lo + 1];           // the entry that built block k: alone in block k + 1
          if (e >= p.win) e = p.win - 1;
          const u32 f2 = e + 1;
          const u64 s = raw_at(p, p.start + f2) - raw_at(p, p.start);
          p.first[lo + 2] = f2;
          p.ext[lo + 2] = s + 2ull * f2 + 7ull * (lo + 2);
          p.info[2] = lo + 2;
          nb = lo + 2;
          n_ent = f2;
        }
      }
      if (status != TPZ_CUT_BAD_ENTRY) data = p.ext[nb];
    }
    // the next window: from the next table (or from `start` again) until its raw bytes reach
    // capacity + block_size, plus twice the bytes of a window that held no cut
    const u32 from = status == TPZ_CUT_FOUND ? p.start + (u32)n_ent : p.start;
    u64 need = p.capacity < (1ull << 62) ? p.capacity + p.block_size : (1ull << 62);
    if (status == TPZ_CUT_NONE && p.win)
      need += 2 * (raw_at(p, p.start + p.win) - raw_at(p, p.start));
    const u64 r0 = raw_at(p, from);
    u32 lo = from, hi = p.seg_end;           // smallest w with raw(w) - raw(from) >= need
    for (int it = 0; it < 33 && lo < hi; it++) {
      const u32 mid = lo + (hi - lo) / 2;
      if (raw_at(p, mid) - r0 >= need) hi = mid; else lo = mid + 1;
    }
    p.cut[0] = status;
    p.cut[1] = k;
    p.cut[2] = nb;
    p.cut[3] = status == TPZ_CUT_BAD_ENTRY ? 0 : n_ent;
    p.cut[4] = data;
    p.cut[6] = from;
    p.cut[7] = lo;
    s_nb = nb;
  }
  __syncthreads();   // (thread 0's stores to first[] are its own: the workgroup sees them after this)
  const u32 nb = s_nb;
  u64 sum = 0;
  for (u32 b = threadIdx.x; b < nb; b += blockDim.x) {
    u32 e = p.first[b];
    if (e >= p.win) e = p.win - 1;
    const u64 a = p.kpos[p.start + e], z = p.kpos[p.start + e + 1];
    sum += z > a ? z - a : 0;
  }
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) p.cut[5] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// ------------------------------------------------------------------ image finish
constexpr u32 kFinThreads = 256;
constexpr u32 kFinPer = 4;                          // blocks per thread
constexpr u32 kFinChunk = kFinThreads * kFinPer;    // blocks per workgroup
constexpr u32 kBloomWgs = 64;                       // workgroups per image copying its filter

struct FinParams {
  const uint8_t* keys;
  const u64* kpos;
  u64 key_bytes;
  u32 n_entries;
  const tpz_sst_image* img;
  u32 n_images;
  u32 max_blocks;
  u32 P;                 // partial sums per image: ceil(max_blocks / kFinChunk), >= 1
  uint8_t* base;
  u64 span;
  u64* part;             // n_images x P
  u64* crc_ext;          // 2 n_images + 1
  const u32* crc;        // 2 n_images
  u64* info;             // 4 per image
};

__device__ __forceinline__ u32 img_blocks(const FinParams& p, const tpz_sst_image& im) {
  return im.n_blocks < p.max_blocks ? im.n_blocks : p.max_blocks;
}

// Block b's first key: its start in the key column and its length (clamped to the column; the
// meta's length field is a u16, and so is every key a block can hold).
__device__ __forceinline__ u64 first_key(const FinParams& p, const tpz_sst_image& im, u32 b,
                                         u32* len) {
  u64 e = (u64)im.entry_base + im.d_first[b];
  if (e >= p.n_entries) {
    *len = 0;
    return 0;
  }
  const u64 a = min64(p.kpos[e], p.key_bytes);
  u64 z = min64(p.kpos[e + 1], p.key_bytes);
  if (z < a) z = a;
  *len = (u32)min64(z - a, 0xFFFFu);
  return a;
}

__device__ __forceinline__ void put_be32(uint8_t* d, u32 v) {
  d[0] = (uint8_t)(v >> 24);
  d[1] = (uint8_t)(v >> 16);
  d[2] = (uint8_t)(v >> 8);
  d[3] = (uint8_t)v;
}

__global__ __launch_bounds__(kFinThreads) void sst_klen_kernel(FinParams p) {
  __shared__ u64 s_sum[kFinThreads / 64];
  const tpz_sst_image& im = p.img[blockIdx.y];
  const u32 nb = img_blocks(p, im);
  u64 sum = 0;
#pragma unroll
  for (u32 r = 0; r < kFinPer; r++) {
    const u32 b = blockIdx.x * kFinChunk + r * kFinThreads + threadIdx.x;
    if (b < nb) {
      u32 len;
      (void)first_key(p, im, b, &len);
      sum += len;
    }
  }
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0)
    p.part[(u64)blockIdx.y * p.P + blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

__global__ __launch_bounds__(kFinThreads) void sst_layout_kernel(FinParams p) {
  __shared__ u64 s_wave[kFinThreads / 64];
  __shared__ u64 s_carry;
  u64 prev_end = 0;      // thread 0: where the image before this one ended, relative to base
  for (u32 i = 0; i < p.n_images; i++) {
    const tpz_sst_image& im = p.img[i];
    u64* part = p.part + (u64)i * p.P;
    // exclusive scan of the image's P partial sums, kFinThreads at a time
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u32 c0 = 0; c0 < p.P; c0 += kFinThreads) {
      const u32 j = c0 + threadIdx.x;
      const u64 v = j < p.P ? part[j] : 0;
      u64 x = v;
      for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o);
        if ((threadIdx.x & 63) >= (u32)o) x += y;
      }
      if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = x;
      __syncthreads();
      u64 before = s_carry;
      for (u32 w = 0; w < (threadIdx.x >> 6); w++) before += s_wave[w];
      if (j < p.P) part[j] = before + x - v;
      __syncthreads();
      if (threadIdx.x == kFinThreads - 1) s_carry = before + x;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const u32 nb = img_blocks(p, im);
      const u64 kb = s_carry;
      const u64 meta_off = im.data_bytes;
      const u64 after_meta = meta_off + 6ull * nb + kb + 4;       // metas, then the meta offset
      const bool bloom = im.d_filter != nullptr;
      const u64 bloom_off = after_meta;
      const u64 size = after_meta + (bloom ? im.filter_len + 4 : 0) + 4;
      const u64 at = (u64)(im.d_image - p.base);
      bool ok = im.d_image >= p.base && at >= prev_end && at <= p.span && size <= p.span - at &&
                im.data_bytes <= p.span && (!bloom || im.filter_len <= p.span) &&
                im.n_blocks <= p.max_blocks && (nb == 0 || (im.d_first && im.d_ext));
      if (ok) {
        put_be32(im.d_image + after_meta - 4, (u32)meta_off);          // builder.rs:108
        if (bloom) put_be32(im.d_image + bloom_off + im.filter_len, (u32)bloom_off);   // :139
      }
      p.info[4 * i + 0] = ok ? size : 0;
      p.info[4 * i + 1] = meta_off;
      p.info[4 * i + 2] = bloom ? bloom_off : ~0ull;
      p.info[4 * i + 3] = 0;
      // range 2i: the image (its last 4 bytes are the trailer the CRC leaves out); range 2i + 1:
      // the bytes up to the next image. A skipped image is two empty ranges.
      const u64 lo = ok ? at : prev_end;
      const u64 end = ok ? at + size : prev_end;
      p.crc_ext[2 * i] = lo;
      p.crc_ext[2 * i + 1] = end;
      if (i + 1 == p.n_images) p.crc_ext[2 * i + 2] = end;
      prev_end = end;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFinThreads) void sst_meta_kernel(FinParams p) {
  __shared__ u32 s_wave[kFinThreads / 64];
  const u32 i = blockIdx.y;
  if (p.info[4 * i] == 0) return;                       // skipped by the layout
  const tpz_sst_image& im = p.img[i];
  const u32 nb = img_blocks(p, im);
  const u32 b0 = blockIdx.x * kFinChunk + threadIdx.x * kFinPer;   // this thread's kFinPer blocks
  u32 len[kFinPer];
  u64 at[kFinPer];
  u32 mine = 0;
#pragma unroll
  for (u32 r = 0; r < kFinPer; r++) {
    len[r] = 0;
    at[r] = 0;
    if (b0 + r < nb) at[r] = first_key(p, im, b0 + r, &len[r]);
    mine += len[r];
  }
  u32 x = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const u32 y = __shfl_up(x, o);
    if ((threadIdx.x & 63) >= (u32)o) x += y;
  }
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = x;
  __syncthreads();
  u64 off = p.part[(u64)i * p.P + blockIdx.x] + x - mine;
  for (u32 w = 0; w < (threadIdx.x >> 6); w++) off += s_wave[w];
  uint8_t* meta = im.d_image + im.data_bytes;
#pragma unroll
  for (u32 r = 0; r < kFinPer; r++) {
    const u32 b = b0 + r;
    if (b < nb) {
      uint8_t* d = meta + 6ull * b + off;               // table.rs:33-46
      put_be32(d, (u32)im.d_ext[b]);
      d[4] = (uint8_t)(len[r] >> 8);
      d[5] = (uint8_t)len[r];
      const uint8_t* k = p.keys + at[r];
      for (u32 j = 0; j < len[r]; j++) d[6 + j] = k[j];
      off += len[r];
    }
  }
}

__global__ __launch_bounds__(kFinThreads) void sst_bloom_kernel(FinParams p) {
  const u32 i = blockIdx.y;
  if (p.info[4 * i] == 0) return;
  const tpz_sst_image& im = p.img[i];
  if (!im.d_filter) return;
  uint8_t* d = im.d_image + p.info[4 * i + 2];
  const u32* s = reinterpret_cast<const u32*>(im.d_filter);
  const u64 len = im.filter_len, words = len / 4;
  for (u64 w = (u64)blockIdx.x * kFinThreads + threadIdx.x; w < words;
       w += (u64)gridDim.x * kFinThreads) {
    const u32 v = s[w];
    d[4 * w] = (uint8_t)v;
    d[4 * w + 1] = (uint8_t)(v >> 8);
    d[4 * w + 2] = (uint8_t)(v >> 16);
    d[4 * w + 3] = (uint8_t)(v >> 24);
  }
  if (blockIdx.x == 0 && threadIdx.x < (len & 3)) d[4 * words + threadIdx.x] = im.d_filter[4 * words + threadIdx.x];
}

__global__ __launch_bounds__(256) void sst_crc_kernel(FinParams p) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n_images) return;
  const u64 size = p.info[4 * i];
  if (size == 0) return;
  const u32 crc = p.crc[2 * i];
  put_be32(p.img[i].d_image + size - 4, crc);           // file_object.rs:44-47
  p.info[4 * i + 3] = crc;
}

FinParams fin_params(const FinishLaunch& a) {
  FinParams p{};
  p.keys = a.keys;
  p.kpos = a.kpos;
  p.key_bytes = a.key_bytes;
  p.n_entries = a.n_entries;
  p.img = a.images;
  p.n_images = a.n_images;
  p.max_blocks = a.max_blocks;
  p.P = finish_parts(a.max_blocks);
  p.base = a.base;
  p.span = a.span;
  p.part = a.part;
  p.crc_ext = a.crc_ext;
  p.crc = a.crc;
  p.info = a.info;
  return p;
}

}  // namespace

void launch_entries_bound(const BoundLaunch& a, hipStream_t s) {
  BoundParams p{a.keys, a.kpos, a.key_bytes, a.n, a.q, a.q_pos, a.incl, a.n_q, a.out};
  entries_bound_kernel<<<(a.n_q + 63) / 64, 64, 0, s>>>(p);
}

void launch_table_cut(const CutLaunch& a, hipStream_t s) {
  CutParams p{a.kpos,    a.vpos, a.start,      a.win,      a.seg_end, a.first,
              a.ext,     a.cut_ext, a.info,    a.block_size, a.capacity, a.cut};
  table_cut_kernel<<<1, 256, 0, s>>>(p);
}

u32 finish_parts(u32 max_blocks) {
  const u32 p = (u32)(((u64)max_blocks + kFinChunk - 1) / kFinChunk);
  return p ? p : 1;
}

void launch_finish_layout(const FinishLaunch& a, hipStream_t s) {
  const FinParams p = fin_params(a);
  sst_klen_kernel<<<dim3(p.P, a.n_images), kFinThreads, 0, s>>>(p);
  sst_layout_kernel<<<1, kFinThreads, 0, s>>>(p);
  sst_meta_kernel<<<dim3(p.P, a.n_images), kFinThreads, 0, s>>>(p);
  sst_bloom_kernel<<<dim3(kBloomWgs, a.n_images), kFinThreads, 0, s>>>(p);
}

void launch_finish_crc(const FinishLaunch& a, hipStream_t s) {
  const FinParams p = fin_params(a);
  sst_crc_kernel<<<(a.n_images + 255) / 256, 256, 0, s>>>(p);
}

}  // namespace tpz

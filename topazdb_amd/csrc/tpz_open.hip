// tpz_open.hip — gfx950 kernels of SsTable::open's parse (src/table.rs:75-112: read_bloom, the meta
// offset, BlockMeta::decode_block_meta) over whole SST file images that are resident in HBM
// (tpz_open_index, tpz_open_metas; include/tpz_gpu.h).
//
// The meta section is a serial length chain (a record = BE u32 offset, BE u16 key length, key), so
// it is walked once out of LDS, and that walk leaves a checkpoint per tile from which the second
// call runs fully in parallel. A tile is kOpenTile = TPZ_OPEN_TILE bytes of the section, counted
// from the 16-byte aligned address at or below its first byte, so that every staging load is an
// aligned 16-byte load whatever the meta offset is. A position "in tile coordinates" is a distance
// from that aligned address.
//
//   open_index_kernel  One workgroup per file. Thread 0 reads the footer (bloom offset, meta
//                      offset: two dependent loads after the span) and runs SsTable::open's range
//                      checks in the reference's order. The workgroup then stages the section
//                      through a ring of two tiles in LDS, a 16-byte load per thread and tile;
//                      tile t + 2 is in flight in registers while thread 0 walks the records that
//                      start in tile t (a header may reach up to 5 bytes into tile t + 1, which is
//                      resident; a key may skip any number of tiles). The walk counts records and
//                      key bytes, checks the offsets' order, and writes tile t's checkpoint:
//                        u64 a = key bytes before the record | its start within the tile << 40
//                        u64 b = the record's index | the file << 32
//                      for the first record that starts in the tile; a tile no record starts in
//                      keeps the 0xFF fill (a == UINT64_MAX). File f's tiles are checkpoints
//                      start / kOpenTile + 2 f onwards: disjoint for disjoint spans in address
//                      order, without a pass over the files.
//   open_scan_kernel   One workgroup: the exclusive prefix sums of the files' block counts and
//                      first-key bytes, in place.
//   open_metas_kernel  One wave per checkpoint. It stages its tile (plus the 16 bytes a header may
//                      reach into) in LDS, walks the at most kOpenTile / 6 + 1 records that start
//                      there for their positions and key prefixes, and then works per record in
//                      parallel: extent, first-key position, and the key bytes (a lane per key up
//                      to kLaneCopyMax bytes, the whole wave for a longer one). Sources and
//                      destinations have no alignment: plain byte stores.
//   open_flags_kernel  One thread per extent slot: the tag byte at ext[j + 1] - 1 (compress.rs:
//                      104-111); tag 2 / 3 ORs bit 0 into the file's flags.
//
// Nothing trusts the images, the spans or (in the second call) the checkpoints: every read is
// clamped to the file's span, every record is bounds-checked again before it is used, and every
// store is checked against the scratch size or the caller's capacities.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"

namespace tpz {

namespace {

using u32 = uint32_t;
using u64 = uint64_t;

constexpr u32 kOpenTile = TPZ_OPEN_TILE;
constexpr u32 kIdxThreads = kOpenTile / 16;      // a 16-byte chunk per thread and tile
constexpr u32 kRing = 2 * kOpenTile;
constexpr u32 kMaxRec = kOpenTile / 6 + 1;       // records that can start in one tile
constexpr u32 kLaneCopyMax = 64;                 // longer keys are copied by the whole wave
constexpr u64 kMaxLen = 1ull << 34;              // TPZ_OPEN_UNSUPPORTED past this
constexpr u64 kUnused = ~0ull;

static_assert(kIdxThreads == 256 && (kRing & (kRing - 1)) == 0, "tile geometry");

struct OpenParams {
  const uint8_t* src;
  u64 span_bytes;
  const u64* span;
  u32 n_files;
  u64* info;
  u64* file_block;
  u64* file_key;
  u64* ck;               // 2 u64 per checkpoint
  u64 n_ck;
  u64* ext;
  u64* first_pos;
  uint8_t* first_keys;
  u64 block_cap;
  u64 key_cap;
};

__device__ __forceinline__ u32 be32(const uint8_t* p) {
  return ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | (u32)p[3];
}

// The 16 bytes at the 16-byte aligned address g; only bytes inside the span [lo, hi) are read
// (the rest read as 0).
__device__ __forceinline__ uint4 load_chunk(const uint8_t* g, const uint8_t* lo, const uint8_t* hi) {
  const uintptr_t a = (uintptr_t)g, l = (uintptr_t)lo, h = (uintptr_t)hi;
  if (a >= l && a + 16 <= h) return *reinterpret_cast<const uint4*>(g);
  u32 w[4] = {0, 0, 0, 0};
#pragma unroll
  for (u32 i = 0; i < 16; i++)
    if (a + i >= l && a + i < h) w[i >> 2] |= (u32)g[i] << (8 * (i & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ bool span_ok(const OpenParams& p, u32 f, u64* start, u64* len) {
  const u64 s = p.span[2ull * f], l = p.span[2ull * f + 1];
  *start = s;
  *len = l;
  if (s > p.span_bytes || l > p.span_bytes - s) return false;
  if (f > 0) {
    const u64 ps = p.span[2ull * f - 2], pl = p.span[2ull * f - 1];
    if (pl > ~0ull - ps || s < ps + pl) return false;
  }
  return true;
}

__global__ __launch_bounds__(kIdxThreads) void open_index_kernel(OpenParams p) {
  __shared__ __align__(16) uint8_t s_ring[kRing];
  __shared__ u64 s_hdr[6];     // status, size, meta offset, meta bytes, bloom offset, filter_len
  __shared__ u32 s_stop;
  const u32 f = blockIdx.x;
  u64 start, len;
  const bool sp_ok = span_ok(p, f, &start, &len);
  if (threadIdx.x == 0) {
    u64 status = TPZ_OPEN_OK, meta_off = 0, meta_bytes = 0, bloom_off = ~0ull, flen = 0;
    const u64 size = len >= 4 ? len - 4 : 0;                     // FileObject::size()
    if (!sp_ok || len > kMaxLen) {
      status = TPZ_OPEN_UNSUPPORTED;
    } else if (len < 8) {
      status = TPZ_OPEN_SHORT;                                   // table.rs:78
    } else {
      const uint8_t* img = p.src + start;
      const u64 off = be32(img + size - 4);
      if (off + 4 > size) {
        status = TPZ_OPEN_BLOOM_RANGE;                           // :84
      } else {
        if (off + 4 != size) {                                   // :81-86
          bloom_off = off;
          flen = size - 4 - off;
        }
        if (off < 4) {
          status = TPZ_OPEN_META_RANGE;                          // :94
        } else {
          const u64 mo = be32(img + off - 4);
          if (mo > off - 4) {
            status = TPZ_OPEN_META_RANGE;                        // :97
          } else {
            meta_off = mo;
            meta_bytes = off - 4 - mo;
          }
        }
      }
    }
    s_hdr[0] = status;
    s_hdr[1] = size;
    s_hdr[2] = meta_off;
    s_hdr[3] = meta_bytes;
    s_hdr[4] = bloom_off;
    s_hdr[5] = flen;
    s_stop = 0;
  }
  __syncthreads();
  u64 status = s_hdr[0];
  const u64 meta_off = s_hdr[2], meta_bytes = s_hdr[3];
  // thread 0's walk: the next record's start (tile coordinates), records and key bytes so far,
  // the last offset seen, whether an offset decreased, whether a record ran past the section
  u64 q = 0, idx = 0, kb = 0, prev = 0;
  bool bad = false, trunc = false;
  if (status == TPZ_OPEN_OK && meta_bytes) {
    const uint8_t* lo = p.src + start;
    const uint8_t* hi = lo + len;
    const uint8_t* meta = lo + meta_off;
    const u32 A = (u32)((uintptr_t)meta & 15u);
    const uint8_t* base = meta - A;
    const u64 E = A + meta_bytes;                                // the section's end
    const u64 nt = (E + kOpenTile - 1) / kOpenTile;
    const u64 ck_base = start / kOpenTile + 2ull * f;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4* ring = reinterpret_cast<uint4*>(s_ring);
    ring[threadIdx.x] = load_chunk(base + 16 * threadIdx.x, lo, hi);
    ring[kIdxThreads + threadIdx.x] =
        nt > 1 ? load_chunk(base + kOpenTile + 16 * threadIdx.x, lo, hi) : zero;
    __syncthreads();
    q = A;
    for (u64 t = 0; t < nt; t++) {
      // tile t + 2 is in flight while tile t is walked
      const uint4 nx =
          t + 2 < nt ? load_chunk(base + (t + 2) * kOpenTile + 16 * threadIdx.x, lo, hi) : zero;
      if (threadIdx.x == 0) {
        const u64 t0 = t * kOpenTile;
        const u64 tend = t0 + kOpenTile < E ? t0 + kOpenTile : E;
        if (q < tend && ck_base + t < p.n_ck) {
          p.ck[2 * (ck_base + t)] = kb | ((q - t0) << 40);
          p.ck[2 * (ck_base + t) + 1] = idx | ((u64)f << 32);
        }
        while (q < tend) {
          if (q + 6 > E) {                                       // get_u32 / get_u16, :52-53
            trunc = true;
            break;
          }
          uint8_t h[6];
#pragma unroll
          for (u32 i = 0; i < 6; i++) h[i] = s_ring[(u32)(q + i) & (kRing - 1)];
          const u64 off = be32(h);
          const u64 kl = ((u32)h[4] << 8) | h[5];
          if (q + 6 + kl > E) {                                  // copy_to_bytes, :54
            trunc = true;
            break;
          }
          if (off < prev) bad = true;
          prev = off;
          idx++;
          kb += kl;
          q += 6 + kl;
        }
        if (trunc) s_stop = 1;
      }
      __syncthreads();
      if (s_stop) break;
      ring[(t & 1) * kIdxThreads + threadIdx.x] = nx;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    if (status == TPZ_OPEN_OK) {
      if (trunc) status = TPZ_OPEN_META_TRUNCATED;
      else if (idx == 0) status = TPZ_OPEN_NO_BLOCKS;            // block_metas[0], :144
      else if (bad || prev > meta_off) status = TPZ_OPEN_BAD_EXTENTS;   // end - offset, :161
    }
    const bool ok = status == TPZ_OPEN_OK;
    u64* in = p.info + 8ull * f;
    in[0] = status;
    in[1] = s_hdr[1];
    in[2] = ok ? meta_off : 0;
    in[3] = ok ? meta_bytes : 0;
    in[4] = ok ? s_hdr[4] : 0;
    in[5] = ok ? s_hdr[5] : 0;
    in[6] = ok ? idx : 0;
    in[7] = 0;
    p.file_block[f] = ok ? idx : 0;
    p.file_key[f] = ok ? kb : 0;
  }
}

__global__ __launch_bounds__(256) void open_scan_kernel(OpenParams p) {
  __shared__ u64 s_wave[2][4];
  __shared__ u64 s_carry[2];
  if (threadIdx.x == 0) s_carry[0] = s_carry[1] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (u64 c0 = 0; c0 < p.n_files; c0 += 256) {
    const u64 j = c0 + threadIdx.x;
    const u64 vb = j < p.n_files ? p.file_block[j] : 0;
    const u64 vk = j < p.n_files ? p.file_key[j] : 0;
    u64 xb = vb, xk = vk;
    for (int o = 1; o < 64; o <<= 1) {
      const u64 yb = __shfl_up(xb, o), yk = __shfl_up(xk, o);
      if (lane >= (u32)o) {
        xb += yb;
        xk += yk;
      }
    }
    if (lane == 63) {
      s_wave[0][w] = xb;
      s_wave[1][w] = xk;
    }
    __syncthreads();
    u64 bb = s_carry[0], bk = s_carry[1];
    for (u32 i = 0; i < w; i++) {
      bb += s_wave[0][i];
      bk += s_wave[1][i];
    }
    if (j < p.n_files) {
      p.file_block[j] = bb + xb - vb;
      p.file_key[j] = bk + xk - vk;
    }
    __syncthreads();
    if (threadIdx.x == 255) {
      s_carry[0] = bb + xb;
      s_carry[1] = bk + xk;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.file_block[p.n_files] = s_carry[0];
    p.file_key[p.n_files] = s_carry[1];
  }
}

__global__ __launch_bounds__(64) void open_metas_kernel(OpenParams p) {
  __shared__ __align__(16) uint8_t s_tile[kOpenTile + 16];
  __shared__ uint16_t s_rel[kMaxRec];    // a record's start within the tile
  __shared__ u32 s_kb[kMaxRec];          // key bytes of the tile's records before it
  const u32 lane = threadIdx.x;
  const u64 out_cap = p.block_cap + p.n_files;
  for (u64 s = blockIdx.x; s < p.n_ck; s += gridDim.x) {
    const u64 a = p.ck[2 * s], b = p.ck[2 * s + 1];
    if (a == kUnused) continue;
    const u32 f = (u32)(b >> 32);
    const u64 idx0 = b & 0xFFFFFFFFull, kb0 = a & ((1ull << 40) - 1), rel0 = a >> 40;
    if (f >= p.n_files || rel0 >= kOpenTile) continue;
    const u64* in = p.info + 8ull * f;
    if (in[0] != TPZ_OPEN_OK) continue;
    u64 start, len;
    if (!span_ok(p, f, &start, &len)) continue;
    const u64 meta_off = in[2], meta_bytes = in[3], n = in[6];
    if (meta_off > len || meta_bytes > len - meta_off) continue;
    const u64 ck_base = start / kOpenTile + 2ull * f;
    if (s < ck_base) continue;
    const uint8_t* lo = p.src + start;
    const uint8_t* hi = lo + len;
    const uint8_t* meta = lo + meta_off;
    const u32 A = (u32)((uintptr_t)meta & 15u);
    const uint8_t* base = meta - A;
    const u64 E = A + meta_bytes;
    const u64 t0 = (s - ck_base) * kOpenTile;
    if (t0 >= E) continue;
    const u64 tend = t0 + kOpenTile < E ? t0 + kOpenTile : E;
    for (u32 c = lane; c < kOpenTile / 16 + 1; c += 64)
      reinterpret_cast<uint4*>(s_tile)[c] = load_chunk(base + t0 + 16 * c, lo, hi);
    __syncthreads();
    // every lane walks the same records (the LDS reads broadcast); lane 0 keeps the positions
    u64 q = t0 + rel0;
    u32 cnt = 0, kb = 0;
    while (q < tend && cnt < kMaxRec) {
      if (q + 6 > E) break;
      const u32 r = (u32)(q - t0);
      const u32 kl = ((u32)s_tile[r + 4] << 8) | s_tile[r + 5];
      if (q + 6 + kl > E) break;
      if (lane == 0) {
        s_rel[cnt] = (uint16_t)r;
        s_kb[cnt] = kb;
      }
      cnt++;
      kb += kl;
      q += 6 + kl;
    }
    __syncthreads();
    const u64 fb = p.file_block[f] + f, fk = p.file_key[f];
    for (u32 j = lane; j < cnt; j += 64) {
      const u64 g = idx0 + j;
      if (g >= n) continue;
      const u32 r = s_rel[j];
      const u32 off = be32(s_tile + r);
      const u32 kl = ((u32)s_tile[r + 4] << 8) | s_tile[r + 5];
      const u64 slot = fb + g, pos = kb0 + s_kb[j];
      if (slot < out_cap) {
        p.ext[slot] = off;
        p.first_pos[slot] = pos;
      }
      if (g + 1 == n && slot + 1 < out_cap) {      // the table's last block ends at the meta offset
        p.ext[slot + 1] = meta_off;
        p.first_pos[slot + 1] = pos + kl;
      }
      if (kl <= kLaneCopyMax && fk + pos + kl <= p.key_cap) {
        const uint8_t* k = base + t0 + r + 6;
        uint8_t* d = p.first_keys + fk + pos;
        for (u32 i = 0; i < kl; i++) d[i] = k[i];
      }
    }
    for (u32 j = 0; j < cnt && idx0 + j < n; j++) {
      const u32 r = s_rel[j];
      const u32 kl = ((u32)s_tile[r + 4] << 8) | s_tile[r + 5];
      if (kl <= kLaneCopyMax) continue;
      const u64 pos = kb0 + s_kb[j];
      if (fk + pos + kl > p.key_cap) continue;
      const uint8_t* k = base + t0 + r + 6;
      uint8_t* d = p.first_keys + fk + pos;
      for (u32 i = lane; i < kl; i += 64) d[i] = k[i];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void open_flags_kernel(OpenParams p) {
  const u64 out_cap = p.block_cap + p.n_files;
  for (u64 s = (u64)blockIdx.x * 256 + threadIdx.x; s + 1 < out_cap; s += (u64)gridDim.x * 256) {
    // the file whose slots hold s: the last f with file_block[f] + f <= s
    u32 lo = 0, hi = p.n_files;
    for (int it = 0; it < 33 && hi - lo > 1; it++) {
      const u32 mid = lo + (hi - lo) / 2;
      if (p.file_block[mid] + mid <= s) lo = mid; else hi = mid;
    }
    const u32 f = lo;
    u64* in = p.info + 8ull * f;
    const u64 fb = p.file_block[f] + f;
    if (in[0] != TPZ_OPEN_OK || s < fb || s - fb >= in[6]) continue;
    u64 start, len;
    if (!span_ok(p, f, &start, &len)) continue;
    const u64 b0 = p.ext[s], b1 = p.ext[s + 1];
    if (b1 <= b0 || b1 > in[2] || b1 > len) continue;
    const uint8_t tag = p.src[start + b1 - 1];
    if (tag == 2 || tag == 3) atomicOr(reinterpret_cast<unsigned long long*>(in + 7), 1ull);
  }
}

OpenParams open_params(const OpenIndexLaunch& a) {
  OpenParams p{};
  p.src = a.src;
  p.span_bytes = a.span_bytes;
  p.span = a.span;
  p.n_files = a.n_files;
  p.info = a.info;
  p.file_block = a.file_block;
  p.file_key = a.file_key;
  p.ck = a.ck;
  p.n_ck = a.n_ck;
  p.ext = a.ext;
  p.first_pos = a.first_pos;
  p.first_keys = a.first_keys;
  p.block_cap = a.block_cap;
  p.key_cap = a.key_cap;
  return p;
}

u32 capped_grid(u64 n) { return (u32)(n < (1u << 20) ? (n ? n : 1) : (1u << 20)); }

}  // namespace

void launch_open_index(const OpenIndexLaunch& a, hipStream_t s) {
  const OpenParams p = open_params(a);
  open_index_kernel<<<a.n_files, kIdxThreads, 0, s>>>(p);
  open_scan_kernel<<<1, 256, 0, s>>>(p);
}

void launch_open_metas(const OpenIndexLaunch& a, hipStream_t s) {
  const OpenParams p = open_params(a);
  open_metas_kernel<<<capped_grid(a.n_ck), 64, 0, s>>>(p);
  open_flags_kernel<<<capped_grid((a.block_cap + a.n_files + 255) / 256), 256, 0, s>>>(p);
}

}  // namespace tpz

// tpz_decode.hip — gfx950 kernels for topazdb's SSTable block decode + CRC-32 verify.
//
// Restates, on the device, for every block of a batch:
//   compress::decode tag dispatch          src/block/compress.rs:95-113
//   Block::decode (crc split, n, offsets)  src/block.rs:46-65
//   checksum::verify_checksum (crc32fast)  src/checksum.rs:6-21
//   BlockIterator::seek_to for every entry src/block/iterator.rs:63-83
// into the slotted column layout of include/tpz_gpu.h.
//
// Execution model:
//  * wave path  — one 64-lane wave owns one block at a time; 16 waves per 1024-thread
//    workgroup, one workgroup per CU, persistent over the batch. The NEXT block's bytes are
//    prefetched into VGPRs (5 x dwordx4 per lane = 5 KiB per wave) while the current block is
//    processed out of the wave's LDS slot, so HBM reads stay in flight during the decode.
//  * big path   — blocks that do not fit a wave slot (len > 4336 B or n > 255) are appended to
//    a device worklist by the wave path and decoded by a second kernel, one 16-wave workgroup
//    per block with a 92 KiB LDS window (TPZ_LDS_BLOCK_BYTES: every block a 64 KiB-target
//    BlockBuilder can emit).
//  * spill path — blocks longer than TPZ_LDS_BLOCK_BYTES, and blocks whose entries overlap or
//    repeat so that their decoded bytes do not fit the slot (the reference iterator accepts any
//    offsets, src/block/iterator.rs:63-83), are appended to the spill worklist by either path and
//    decoded by tpz_spill.hip into the caller's spill arena.
//  CRC-32: the payload is cut into 80-byte runs aligned to its END; lane l folds run l with
//  five slice-by-16 steps (fused with the copy's windows on the wave path), then a lane tree
//  (exec-masked shift-by-80*2^k lookups, DPP row shifts, readlane across rows) combines them.
//  All operators are byte-sliced lookup tables in LDS (41 KiB).
//  Decode: lanes parse 64 entries at a time (n, offsets, klen, vlen, bounds checks that mirror
//  the reference's panics), DPP wave prefix sums give packed output positions in the block's
//  output stream (key bytes, then value bytes from the next 16-byte boundary), and every
//  non-empty key and value goes into one entry table plus a chunk->entry map. The copy is
//  output-driven over that single stream: lane c assembles output chunk c from the (usually
//  one) source segment(s) covering it, then one coalesced dwordx4 store (1 KiB per wave
//  instruction). A regular block (every entry one key length and one value length, both >= 16,
//  back to back) skips the table and the map on the slotted wave path: its ends and the copy's
//  chunk -> entry index are closed forms of (n, KL, VL) (decode_block, copy_crc_piped<.., REG>);
//  a wave computes that index once per (n, KL, VL) and keeps it, packed, in its idle entry table
//  (lengths that are multiples of 4: as four source offsets per chunk, one per output dword).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"
// the tail kernel's spill phase (namespace tpz::sp), compiled into this unit
#include "tpz_spill.hip"

namespace tpz {

typedef uint32_t u32;
typedef uint64_t u64;

// ------------------------------------------------------------------ LDS geometry
constexpr int kWave = 64;
#ifdef TPZ_ABL_W20
// timing build (wrong CRCs: the shift and inverse tables alias T_0..T_15): two workgroups of 10
// waves per CU (20 waves), 16 KiB of tables per workgroup, 64-entry tables, VGPRs capped at 96
// (the compiler spills what does not fit); prices VERDICT r5's 18-20-wave shape
#ifdef TPZ_ABL_W8
constexpr int kWavesPerWG = 8;    // (two workgroups of 8: the co-residency check of DESIGN §4f)
#else
constexpr int kWavesPerWG = 10;
#endif
#else
constexpr int kWavesPerWG = 16;
#endif
constexpr int kWGThreads = kWave * kWavesPerWG;
// Blocks a wave of the wave path claims at a time (decode_wave_kernel): 2^chunk_shift, chosen
// per launch (launch_decode); TPZ_WAVE_CHUNK forces one (diagnostic builds).
// rows of 16 blocks (the claim unit of the wave path; chunks of 2^k blocks tile a row)
constexpr u32 kRowShift = 4, kRowBlocks = 1u << kRowShift;
// wave path: a workgroup's rows are claimed kRowAhead row slots ahead, into a ring of kRowRing
// (2^20 4k blocks: 2 slots 1.902 ms, 3 1.853-1.866, 4 1.859-1.878, 6 1.887; zipf 2.028 / 1.983-1.997
// / 1.985-1.996 / 2.001: profiles/r5/row_ahead/)
#ifndef TPZ_ROW_AHEAD
#define TPZ_ROW_AHEAD 3
#endif
constexpr u32 kRowAhead = TPZ_ROW_AHEAD, kRowRing = 16;
constexpr u32 kRowExit = 0xFFFFFFFFu;   // a slot that gets no row: the workgroup's rows are done
constexpr int kTableBytes = kNumCrcTables * 256 * 4;  // 41 KiB
constexpr int kGuard = 96;  // zeroed: the CRC's front lane reads up to 79+15 B before the payload

// wave path slot: [guard 96][window 4352][pad 32][entry table 512 x u32][map 288 x u16]
// The window holds any block of a block_size <= 4 KiB builder (<= 4101 B; topazdb's default,
// src/opt.rs:39); longer blocks take the big path.
constexpr int kWinRounds = 5;                       // prefetch: 5 x 1 KiB loads, the 5th partial
constexpr int kWinBytes = 4352;
constexpr u32 kWaveMaxLen = kWinBytes - 16;         // a0 (<=15) + len must fit the window
// The wave path's CRC tables in LDS: the decode tables, ids 0..40 (tpz_internal.h).
#ifdef TPZ_ABL_W20
constexpr int kWaveTabBytes = 16 * 1024;
constexpr u32 kWaveMaxN = 63;
constexpr int kWaveTabSlots = 128;
#else
constexpr int kWaveTabBytes = kTableBytes;
constexpr u32 kWaveMaxN = 255;                      // the table holds 2n + 1 <= 511 entries
constexpr int kWaveTabSlots = 512;
#endif
constexpr int kWaveMapLen = 288;                    // >= (kWaveMaxLen + 2) / 16 + 3 map slots
constexpr int kSlotBytes = kGuard + kWinBytes + 32 + kWaveTabSlots * 4 + 2 * kWaveMapLen;
static_assert(kSlotBytes % 16 == 0 && kWaveMapLen % 8 == 0, "slot alignment");
static_assert(2 * kWaveMaxN + 1 <= (u32)kWaveTabSlots, "entry table");
// (the regular path's copy index, 16 bytes per lane, lies at the head of the entry table, in the
// timing build with the short table in the map too: a regular block uses neither, and the
// general parse, which writes both, invalidates it)
static_assert(kWaveTabSlots * 4 + 2 * kWaveMapLen >= kWave * 16, "index cache");
// (the dword index of a geometry with 4-byte-multiple lengths takes 32 bytes per lane: the whole
// entry table, no LDS added; the timing build's short table has no room and never holds one)
constexpr bool kRegDwordFits = kWaveTabSlots * 4 >= kWave * 32;
#ifndef TPZ_ABL_W20
static_assert(kRegDwordFits && kWaveTabSlots * 4 == kWave * 32, "dword index cache");
#endif
constexpr int kWaveLds = kWaveTabBytes + kWavesPerWG * kSlotBytes;
static_assert(kWaveLds <= 163840, "wave path LDS");

// big path (one 16-wave workgroup per block): [tables][guard 96][window 92 KiB][pad 32]
// [map u16][group sums u64][window maxima u32][wave CRCs u32][entry table u64]; blocks whose
// entry table does not fit the LDS one (2n + 1 > kBigLdsSlots) use global scratch
constexpr int kBigWaves = 16;
constexpr int kBigThreads = kBigWaves * kWave;
constexpr int kBigWinBytes = 94208;
constexpr u32 kBigMaxLen = TPZ_LDS_BLOCK_BYTES;     // 94192 (a0 + len <= window)
constexpr int kBigMapLen = 5904;                    // >= (kBigMaxLen + 2) / 16 + 3
constexpr int kBigStage = (kBigWinBytes + 16 * kBigThreads - 1) / (16 * kBigThreads);  // 6
constexpr int kBigMaxGroups = 736;                  // n <= (P - 2) / 2 < 47096 entries / 64
constexpr int kBigMaxWin = 96;                      // copy windows: npad / 64 <= 92
constexpr int kBigLdsSlots = 960;                   // u64 entries of the LDS entry table
constexpr int kBigSuper = 20;                       // CRC super-rounds: ceil(94208 / 5120) <= 19
constexpr int kBigLds = kTableBytes + kGuard + kBigWinBytes + 32 + kBigMapLen * 2 +
                        kBigMaxGroups * 10 + kBigMaxWin * 4 + kBigWaves * 4 + kBigLdsSlots * 8;
static_assert(kBigMaxLen + 16 <= kBigWinBytes, "big window");
static_assert(kBigMapLen % 8 == 0 && (kWaveMaxLen + 2) / 16 + 3 <= (u32)kWaveMapLen &&
              (kBigMaxLen + 2) / 16 + 3 <= (u32)kBigMapLen, "map sizes");
static_assert(kBigLds <= 163840, "big path LDS");
static_assert((kTableBytes + kGuard + kBigWinBytes + 32 + kBigMapLen * 2 + kBigMaxWin * 4 +
               kBigWaves * 4) % 8 == 0, "big path entry table alignment");

// ------------------------------------------------------------------ small helpers
// The lane id, laundered: masks and offsets derived from it are recomputed where they are used
// (one or two VALU) instead of being hoisted out of the block loop into SGPR pairs, which spill
// (the loop is at its SGPR and VGPR limits).
__device__ __forceinline__ u32 lane_id() {
  u32 l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  asm volatile("" : "+v"(l));
  return l;
}
__device__ __forceinline__ u32 uni(u32 x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ u64 uni64(u64 x) {
  u32 lo = __builtin_amdgcn_readfirstlane((u32)x), hi = __builtin_amdgcn_readfirstlane((u32)(x >> 32));
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u32 readlane(u32 x, int l) { return __builtin_amdgcn_readlane(x, l); }
// DPP row op with bound_ctrl: lanes whose source is outside their row of 16 read 0.
template <int CTRL>
__device__ __forceinline__ u32 dpp(u32 x) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
constexpr int kRowShr = 0x110;  // row_shr:n = 0x110 + n (lane l reads l-n)
constexpr int kRowShl = 0x100;  // row_shl:n = 0x100 + n (lane l reads l+n)

// Unaligned little-endian u32 from LDS at byte offset a (>= 0) of an LDS byte array whose base
// is 4-byte aligned: two ds_read_b32 + v_alignbyte.
__device__ __forceinline__ u32 lds_u32(const uint8_t* base, u32 a) {
  const u32* p = reinterpret_cast<const u32*>(base + (a & ~3u));
  return __builtin_amdgcn_alignbyte(p[1], p[0], a & 3u);
}
// Big-endian u16 at byte offset a (bytes::Buf::get_u16).
__device__ __forceinline__ u32 lds_be16(const uint8_t* base, u32 a) {
  u32 w = lds_u32(base, a);
  return ((w & 0xFFu) << 8) | ((w >> 8) & 0xFFu);
}
__device__ __forceinline__ u32 bswap32(u32 w) { return __builtin_bswap32(w); }

// 16 bytes starting at LDS byte offset x (relative to base, base 16-aligned). Default: three
// 8-byte-aligned ds_read_b64 + a one-bit dword select + alignbyte (9 VALU). Diagnostic variants:
// one ds_read_b128 at the byte address (TPZ_ABL_U128; gfx950 replays it: 64 LDS cycles), two
// aligned ds_read_b128 + a two-bit select (16 VALU).
__device__ __forceinline__ uint4 lds_window16(const uint8_t* base, int x) {
       // unaligned ds_read_b128 replay) + a one-bit dword select + alignbyte
  typedef u32 u32x2 __attribute__((ext_vector_type(2)));
  const u32x2* p = reinterpret_cast<const u32x2*>(base + (x & ~7));
  u32x2 a = p[0], b = p[1], c = p[2];
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
  const u32 s = (u32)x & 3u;
  const bool h = ((u32)x & 4u) != 0;
  const u32 s0 = h ? a.y : a.x, s1 = h ? b.x : a.y, s2 = h ? b.y : b.x, s3 = h ? c.x : b.y,
            s4 = h ? c.y : c.x;
  return make_uint4(__builtin_amdgcn_alignbyte(s1, s0, s), __builtin_amdgcn_alignbyte(s2, s1, s),
                    __builtin_amdgcn_alignbyte(s3, s2, s), __builtin_amdgcn_alignbyte(s4, s3, s));
}

// ------------------------------------------------------------------ CRC-32 (table driven)
// tab = kNumCrcTables x 256 u32 in LDS. T_k[b] = R0(b || 0^k): raw CRC (init 0, no xorout).
// ids 0..15: T_0..T_15 (slice-by-16); ids 16+4j+i: T_{n_j-1-i}, n_j = kCrcShiftBytes[j].
#ifdef TPZ_ABL_NOCF
// timing build (wrong CRCs): every lookup of a half-wave hits its own bank (lane l reads word l %
// 32 of the table), with the dependence on the byte kept; prices the bank conflicts of the CRC
__device__ __forceinline__ u32 tlook(const u32* tab, int id, u32 byte) {
  u32 z = byte;
  asm volatile("" : "+v"(z));
  return tab[id * 256 + (((z & 0x10000u) + __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31u)];
}
#elif defined(TPZ_ABL_W20)
__device__ __forceinline__ u32 tlook(const u32* tab, int id, u32 byte) { return tab[(id & 15) * 256 + byte]; }
#else
__device__ __forceinline__ u32 tlook(const u32* tab, int id, u32 byte) { return tab[id * 256 + byte]; }
#endif

// a ^ b ^ c in one v_bitop3_b32.
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// R0 of one 16-byte chunk (little-endian dwords w0..w3): XOR_i T_{15-i}[c_i].
__device__ __forceinline__ u32 slice16(const u32* tab, u32 w0, u32 w1, u32 w2, u32 w3) {
  u32 c = xor3(tlook(tab, 15, w0 & 0xFF), tlook(tab, 14, (w0 >> 8) & 0xFF), tlook(tab, 13, (w0 >> 16) & 0xFF));
  c = xor3(c, tlook(tab, 12, w0 >> 24), tlook(tab, 11, w1 & 0xFF));
  c = xor3(c, tlook(tab, 10, (w1 >> 8) & 0xFF), tlook(tab, 9, (w1 >> 16) & 0xFF));
  c = xor3(c, tlook(tab, 8, w1 >> 24), tlook(tab, 7, w2 & 0xFF));
  c = xor3(c, tlook(tab, 6, (w2 >> 8) & 0xFF), tlook(tab, 5, (w2 >> 16) & 0xFF));
  c = xor3(c, tlook(tab, 4, w2 >> 24), tlook(tab, 3, w3 & 0xFF));
  c = xor3(c, tlook(tab, 2, (w3 >> 8) & 0xFF), tlook(tab, 1, (w3 >> 16) & 0xFF));
  return c ^ tlook(tab, 0, w3 >> 24);
}

// shift_k(A) = R_A(0^k) for a wave-uniform k in 0..15, from the slice tables T_0..T_15.
__device__ __forceinline__ u32 crc_shift_small(const u32* tab, u32 a, u32 k) {
  u32 r = k >= 4 ? 0u : (a >> (8 * k));
  for (u32 i = 0; i < 4 && i < k; i++) r ^= tlook(tab, (int)(k - 1 - i), (a >> (8 * i)) & 0xFF);
  return r;
}

// Inverse of shift_k: un-feed k zero bytes (crc' = (crc >> 8) ^ T_0[crc & 0xFF] is invertible
// because the top byte of T_0[b] determines b). Only used to report a mismatching CRC.
__device__ __forceinline__ u32 crc_unshift_small(const u32* tab, u32 r, u32 k) {
#ifdef TPZ_ABL_W20
  return r;   // (timing build: its CRCs mismatch by construction; no un-shift chain per block)
#endif
  for (u32 i = 0; i < k; i++) {
    const u32 b = tlook(tab, kCrcInvTable, r >> 24);
    r = ((r ^ tlook(tab, 0, b)) << 8) | b;
  }
  return r;
}

// a * b mod P in the reflected domain (bit 31 = x^0): R0(M || 0^n) = gf_mul(x^(8n) mod P,
// R0(M)). Table-free (32 VALU steps): the big path shifts each wave's CRC by its distance to the
// block end with it, once per wave and block.
__device__ __forceinline__ u32 gf_mul(u32 a, u32 b) {
  u32 p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    p ^= (a & (0x80000000u >> i)) ? b : 0u;
    b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
  }
  return p;
}

// a * b mod P with a per-lane multiplier a (bit 31 = x^0): 5 VALU per bit, no tables.
__device__ __forceinline__ u32 gf_mul_lane(u32 a, u32 b) {
  u32 p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const u32 m = (u32)((int)(a << i) >> 31);            // all ones iff a holds x^i
    p ^= b & m;
    b = (b >> 1) ^ (0xEDB88320u & (u32)(-(int)(b & 1u)));
  }
  return p;
}

// XOR of x over the wave (uniform result): DPP row shifts, then the four row totals.
__device__ __forceinline__ u32 wave_xor(u32 x) {
  x ^= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + 1, 0xF, 0xF, true);
  x ^= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + 2, 0xF, 0xF, true);
  x ^= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + 4, 0xF, 0xF, true);
  x ^= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x100 + 8, 0xF, 0xF, true);
  return __builtin_amdgcn_readlane(x, 0) ^ __builtin_amdgcn_readlane(x, 16) ^
         __builtin_amdgcn_readlane(x, 32) ^ __builtin_amdgcn_readlane(x, 48);
}

// shift_n(A) = R_A(0^n) = XOR_i T_{n-1-i}[byte_i(A)], n = kCrcShiftBytes[J].
template <int J>
__device__ __forceinline__ u32 crc_shift(const u32* tab, u32 a) {
  constexpr int b0 = 16 + 4 * J;
  return xor3(tlook(tab, b0, a & 0xFF), tlook(tab, b0 + 1, (a >> 8) & 0xFF),
              tlook(tab, b0 + 2, (a >> 16) & 0xFF)) ^ tlook(tab, b0 + 3, a >> 24);
}

// Keep the first k bytes of a 16-byte piece and zero the rest (k in 0..16): the stream's last
// chunk, whose bytes past the stream would otherwise be whatever LDS held (unspecified, but it
// made the output differ from run to run).
__device__ __forceinline__ uint4 keep_head(uint4 v, u32 k) {
  const u64 lo = (u64)v.y << 32 | v.x, hi = (u64)v.w << 32 | v.z;
  const u64 mlo = k >= 8 ? ~0ull : ((1ull << (8 * k)) - 1);
  const u64 mhi = k >= 16 ? ~0ull : (k <= 8 ? 0ull : ((1ull << (8 * (k - 8))) - 1));
  const u64 a = lo & mlo, b = hi & mhi;
  return make_uint4((u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
}

// Zero the first k bytes of a 16-byte piece (k in 0..15).
__device__ __forceinline__ uint4 zero_head(uint4 v, u32 k) {
  const u64 lo = (u64)v.y << 32 | v.x, hi = (u64)v.w << 32 | v.z;
  const u64 mlo = k >= 8 ? 0ull : (~0ull << (8 * k));
  const u64 mhi = k <= 8 ? ~0ull : (~0ull << (8 * (k - 8)));
  const u64 a = lo & mlo, b = hi & mhi;
  return make_uint4((u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
}

// Combine the lanes' run CRCs (lane l's run ends 80*l bytes before the end) into R0 of the whole
// range, as a tree: at level k the lanes l = 2^k (mod 2^(k+1)) shift their value by 80 * 2^k
// (exec-masked lookups: only those lanes touch LDS, so the random-index bank conflicts shrink
// with every level) and DPP hands it to lane l - 2^k, which XORs it in. Rows of 16 lanes finish
// in lanes 0, 16, 32, 48; those are shifted by 1280 / 2560 B and read out.
__device__ __forceinline__ u32 crc_combine(const u32* tab, u32 A) {
  // (the lane id is laundered so that the six lane masks are recomputed here, one v_cmp each,
  // instead of being hoisted out of the block loop into SGPR pairs that spill)
  u32 lane = lane_id();
  asm volatile("" : "+v"(lane));
  if ((lane & 1u) == 1u) A = crc_shift<0>(tab, A);
  A ^= dpp<kRowShl + 1>(A);
  if ((lane & 3u) == 2u) A = crc_shift<1>(tab, A);
  A ^= dpp<kRowShl + 2>(A);
  if ((lane & 7u) == 4u) A = crc_shift<2>(tab, A);
  A ^= dpp<kRowShl + 4>(A);
  if ((lane & 15u) == 8u) A = crc_shift<3>(tab, A);
  A ^= dpp<kRowShl + 8>(A);
  if ((lane & 31u) == 16u) A = crc_shift<4>(tab, A);
  if ((lane & 47u) == 32u) A = crc_shift<5>(tab, A);  // lanes 32 and 48
  return readlane(A, 0) ^ readlane(A, 16) ^ readlane(A, 32) ^ readlane(A, 48);
}

// Raw CRC R0 of the LDS bytes [pb, pb + Pa), where pb + Pa is 16-byte aligned: the payload
// (first four bytes already complemented: init 0xFFFFFFFF folded into the message) followed by
// the zero bytes that pad it to the 16-byte boundary (the caller compares in that shifted domain).
// The range is cut into 80-byte runs aligned to its END (leading zero padding leaves a raw CRC
// unchanged), so every LDS read is an aligned ds_read_b128 (80-byte lane stride: conflict-free
// per 16 lanes); lane l folds run l (counted from the end) with five chained slice-by-16 steps;
// super-rounds of 64 runs (5120 B, long blocks only) are chained with two shift-by-2560 steps.
// Run l then sits 80*l bytes before the end; crc_combine merges the lanes' values as a tree
// (shift-by-80*2^k at level k, DPP, readlane). Returns R0 (wave-uniform).
__device__ __forceinline__ u32 wave_crc(const u32* tab, const uint8_t* win, int pb, u32 Pa) {
  typedef u32 u32x4 __attribute__((ext_vector_type(4)));
  const u32 lane = lane_id();
  const u32 S = (Pa + 5119) / 5120;      // super-rounds, end-aligned
  u32 A = 0;
  for (u32 r = S; r-- > 0;) {
    const int seg = (int)Pa - 5120 * (int)r - kCrcLaneBytes * (int)(lane + 1);
    u32 c = 0;
    if (seg + kCrcLaneBytes > 0) {
#pragma unroll
      for (int t = 0; t < kCrcLaneBytes / 16; t++) {
        // bytes before the payload read as zero: the zeroed guard, and the window's leading
        // bytes (another block's tail) are zeroed when the window is staged
        const u32x4 w = *reinterpret_cast<const u32x4*>(win + pb + seg + 16 * t);
        c = slice16(tab, w.x ^ c, w.y, w.z, w.w);
      }
    }
    A = (r + 1 == S) ? c : (crc_shift<5>(tab, crc_shift<5>(tab, A)) ^ c);
  }
  return crc_combine(tab, A);
}

// ------------------------------------------------------------------ entry tables
// The NON-EMPTY keys in order, then the non-empty values in order (one table for the block's
// output stream): end = exclusive end offset of the segment's bytes in the stream, delta = (LDS
// offset of its first byte) - (its start offset in the stream), so byte x of the stream inside
// that segment sits at LDS offset x + delta.
// Wave path: one u32 per segment, (end << 16) | (u16)delta (block <= 4336 B).
struct ColSmall {
  u32* t;
  __device__ __forceinline__ void put(u32 k, u32 end, int delta) const {
    t[k] = (end << 16) | ((u32)delta & 0xFFFFu);
  }
  __device__ __forceinline__ u32 end(u32 k) const { return t[k] >> 16; }
  __device__ __forceinline__ void get(u32 k, u32& end, int& delta) const {
    const u32 v = t[k];
    end = v >> 16;
    delta = (int)(short)(v & 0xFFFFu);
  }
  // entries k and k + 1 in one ds_read2_b32 (k + 1 may be one past the last entry: the table has
  // room for it and the caller ignores it)
  __device__ __forceinline__ void get2(u32 k, u32& e0, int& d0, u32& e1, int& d1) const {
    const u32 a = t[k], b = t[k + 1];
    e0 = a >> 16;
    d0 = (int)(short)(a & 0xFFFFu);
    e1 = b >> 16;
    d1 = (int)(short)(b & 0xFFFFu);
  }
};
// Big path: one u64 per entry, {end, delta}, in this workgroup's global scratch. Written and
// read back by the same wave: stores are drained (s_waitcnt vmcnt(0)) before the copy phase and
// reads use sc1 (L2-served) loads, so no stale L1 line of a previous block can be returned.
struct ColBig {
  u64* t;
  __device__ __forceinline__ void put(u32 k, u32 end, int delta) const {
    t[k] = ((u64)(u32)delta << 32) | end;
  }
  __device__ __forceinline__ u64 ld(u32 k) const {
    return __hip_atomic_load(t + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ u32 end(u32 k) const { return (u32)ld(k); }
  __device__ __forceinline__ void get(u32 k, u32& end, int& delta) const {
    const u64 v = ld(k);
    end = (u32)v;
    delta = (int)(u32)(v >> 32);
  }
  __device__ __forceinline__ void get2(u32 k, u32& e0, int& d0, u32& e1, int& d1) const {
    get(k, e0, d0);
    get(k + 1, e1, d1);
  }
};
// Big path, blocks with 2n + 1 <= kBigLdsSlots: the same {end, delta} entries in LDS.
struct ColLds {
  u64* t;
  __device__ __forceinline__ void put(u32 k, u32 end, int delta) const {
    t[k] = ((u64)(u32)delta << 32) | end;
  }
  __device__ __forceinline__ u32 end(u32 k) const { return (u32)t[k]; }
  __device__ __forceinline__ void get(u32 k, u32& end, int& delta) const {
    const u64 v = t[k];
    end = (u32)v;
    delta = (int)(u32)(v >> 32);
  }
  __device__ __forceinline__ void get2(u32 k, u32& e0, int& d0, u32& e1, int& d1) const {
    get(k, e0, d0);
    get(k + 1, e1, d1);
  }
};

// Wave-inclusive prefix sum / max over 64 lanes: DPP row shifts, then row_bcast:15 / :31
// (GFX9 DPP) carry each row's last lane into the following rows. Six DPP ops, no readlane.
constexpr int kRowBcast15 = 0x142, kRowBcast31 = 0x143;
__device__ __forceinline__ u32 wave_scan_incl(u32 x) {
  x += dpp<kRowShr + 1>(x);
  x += dpp<kRowShr + 2>(x);
  x += dpp<kRowShr + 4>(x);
  x += dpp<kRowShr + 8>(x);
  x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, kRowBcast15, 0xA, 0xF, false);
  x += (u32)__builtin_amdgcn_update_dpp(0, (int)x, kRowBcast31, 0xC, 0xF, false);
  return x;
}
__device__ __forceinline__ u32 wave_scan_max(u32 x) {
  x = max(x, dpp<kRowShr + 1>(x));
  x = max(x, dpp<kRowShr + 2>(x));
  x = max(x, dpp<kRowShr + 4>(x));
  x = max(x, dpp<kRowShr + 8>(x));
  x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, kRowBcast15, 0xA, 0xF, false));
  x = max(x, (u32)__builtin_amdgcn_update_dpp(0, (int)x, kRowBcast31, 0xC, 0xF, false));
  return x;
}

__device__ __forceinline__ u32 lanes_below(u64 mask) {
  return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

// ------------------------------------------------------------------ diagnostic stamps
// TPZ_ABL_STAMPS (a timing-only diagnostic build, never shipped): per-wave cycle sums per phase,
// read with s_memtime (cdna_hip_programming.md §7 "In-kernel stamps"), stored once per wave in
// a buffer of their own (g_stamps). Phases: 0 wait for the prefetched block + stage it into
// LDS, 1 issue the next block's loads, 2 header + parse, 3 copy, 4 CRC, 5 status write + loop.
#ifdef TPZ_ABL_STAMPS
constexpr int kStampWaves = 256 * kWavesPerWG;
__device__ u64 g_stamps[2 * kStampWaves * 8];   // wave kernel, then the big kernel
struct Stamps {
  u64 t[7] = {0, 0, 0, 0, 0, 0, 0};
  u64 last = 0;
  u64 rare = 0;      // copy windows rewritten by copy_window (the fused copy's rare path)
};
__device__ __forceinline__ u64 stamp_now() {
  u64 t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define TPZ_STAMP(S, k)               \
  do {                                \
    const u64 now_ = stamp_now();     \
    (S).t[k] += now_ - (S).last;      \
    (S).last = now_;                  \
  } while (0)
#else
struct Stamps {};
#define TPZ_STAMP(S, k) \
  do {                  \
  } while (0)
#endif

// ------------------------------------------------------------------ per-block decode
struct Out {
  uint8_t* data;
  u32* ends;
  u32* count;
  uint8_t* status;
  u32* crc;
  u32* defer_list;
  u32* defer_count;
  u32* spill_list;
  u32* spill_count;
  u32* bw_list;        // long blocks with n < 64: decode_bigwave_kernel (tpz_bigwave.hip)
  u32* bw_count;
  const u64* efirst;   // exact ends layout (tpz_columns.d_entry_first), or null: slotted
  // flat layout (tpz_decode_blocks_flat), or null: slotted. Block b's keys go to
  // keys[kfirst[b] ..], its values to vals[vfirst[b] ..] (tpz_flat_layout's prefixes).
  uint8_t* keys;
  uint8_t* vals;
  const u64* kfirst;
  const u64* vfirst;
};

// The worklist pointers (rare paths) are read from a copy of the Out struct in LDS (wave path):
// kept as kernel arguments, the compiler hoists them out of the block loop into SGPRs that stay
// live across it, and the loop is at its SGPR limit (spilled SGPRs go to VGPR lanes, and the
// VGPRs are at their limit too). LDS loads are not hoisted past the loop's LDS stores.
// Lane 0 appends block b to a worklist (the big path's or the spill path's).
// (the lists are global memory: a pointer read from the LDS copy is generic, and flat atomics
// and stores would count in lgkmcnt too)
typedef __attribute__((address_space(1))) u32 gu32;
__device__ __forceinline__ void defer_to(u32* list, u32* count, u32 b) {
  gu32* l = (gu32*)list;
  gu32* c = (gu32*)count;
  if (lane_id() == 0) l[__hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = b;
}

// The lanes in `take` append their block bb to a worklist with one atomic per wave (a
// single-address atomic per block serialises at the memory side: 0.75 ms per 65,536 long
// blocks, profiles/r2/kernel_stats_64k.csv).
__device__ __forceinline__ void defer_lanes(u32* list, u32* count, bool take, u32 bb) {
  const u64 m = __ballot(take);
  if (!m) return;
  u32 base = 0;
  gu32* l = (gu32*)list;
  gu32* c = (gu32*)count;
  if (lane_id() == (u32)__builtin_ctzll(m))
    base = __hip_atomic_fetch_add(c, (u32)__builtin_popcountll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = __builtin_amdgcn_readlane(base, __builtin_ctzll(m));
  if (take) l[base + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u))] = bb;
}

// Lane 0 stores block b's status, count and crc. Every lane issues the three buffer stores
// (the others at an offset past the descriptor, which the hardware drops) instead of a
// lane-0 branch: no exec-skip branch and its scalar bookkeeping per block, and the block's
// entry-ends stores are written the same way. Measured 2.05 -> 1.96 ms per 2^20 4k blocks
// (profiles/r1/ablations_vmpad.jsonl, variant vm0 = this build).
constexpr u32 kOob = 0x7FFFFFF8u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t whole_rsrc(void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(p, (short)0, (int)0x7FFFFFF0, 0x00020000);
}
__device__ __forceinline__ void put_meta(const Out& o, u32 b, u32 st, u32 n, u32 crc) {
  const bool l0 = lane_id() == 0;
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)st, whole_rsrc(o.status), l0 ? b : kOob, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(n, whole_rsrc(o.count), l0 ? 4 * b : kOob, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(crc, whole_rsrc(o.crc), l0 ? 4 * b : kOob, 0, 0);
}
// Padding stores: K out-of-range stores (dropped by the descriptor's range check: no traffic)
// issued straight after the wave loop's prefetch loads. The loop waits for those loads at its
// top, one block later; vmcnt counts loads and stores in issue order, and the compiler waits
// vmcnt(N) with N = the fewest operations any path issues after the load. Without padding some
// path (a long block, a rejected one) issues none, the wait is vmcnt(0), and it also waits for
// the acknowledgement of the block's own copy stores, issued moments before. With K stores on
// every path it is vmcnt(K): the block's last K stores stay in flight into the next block.
// (Round 4 measured such a build 0.5-1.5 % slower, profiles/r4/vmpad/; it still waited vmcnt(0)
// in the parse and at the loop's latch, so the relaxed wait bought nothing. DESIGN 4g.)
// (The hot path stores 8 times per block: the ends, 3 x meta, 4 windows. 4 measured 1.733 /
// 1.735 ms per 2^20 4k blocks, 8 1.735 / 1.741, 0 1.743 / 1.742, the parent 1.762 / 1.759:
// profiles/prefetch/ab_4k_pads_*.jsonl.)
constexpr int kVmPad = 4;
template <int K>
__device__ __forceinline__ void vm_pad(__amdgpu_buffer_rsrc_t rs) {
  // (distinct, non-adjacent offsets: equal ones are merged into one store, adjacent ones into a
  // wider one)
#pragma unroll
  for (int k = 0; k < K; k++) __builtin_amdgcn_raw_buffer_store_b32(0u, rs, kOob - 64u * k, 0, 0);
}

// Bytes [lo, hi) of the 4-byte word d (lo, hi in 0..16, relative to the chunk start).
__device__ __forceinline__ u32 byte_mask(int lo, int hi, int d) {
  const int a = max(lo - 4 * d, 0), b = min(hi - 4 * d, 4);
  if (a >= b) return 0u;
  const u32 top = b >= 4 ? ~0u : ((1u << (8 * b)) - 1u);
  return top & (~0u << (8 * a));
}

// acc = bytes [0, m) of a, bytes [m, 16) of w (m in 0..16).
__device__ __forceinline__ uint4 merge_at(uint4 a, uint4 w, int m) {
  const u64 mlo = m >= 8 ? 0ull : (~0ull << (8 * m));          // bytes taken from w, low half
  const u64 mhi = m <= 8 ? ~0ull : (m >= 16 ? 0ull : (~0ull << (8 * (m - 8))));
  const u64 alo = (u64)a.y << 32 | a.x, ahi = (u64)a.w << 32 | a.z;
  const u64 wlo = (u64)w.y << 32 | w.x, whi = (u64)w.w << 32 | w.z;
  const u64 lo = (alo & ~mlo) | (wlo & mlo), hi = (ahi & ~mhi) | (whi & mhi);
  return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

// Source of the copy: the staged LDS window.
struct Src16 {
  const uint8_t* win;
  __device__ __forceinline__ uint4 operator()(int x) const { return lds_window16(win, x); }
};

// ------------------------------------------------------------------ copy destinations
// Slotted layout: chunk c of the block's stream goes to slot + 16 c; chunks up to npad (the
// 128-byte line) are written, bytes past the stream (tot) zeroed.
struct SlotDst {
  static constexpr bool kFlat = false;
  uint8_t* p;
  u32 npad, tot;
  __device__ __forceinline__ void put(u32 c, uint4 acc, bool act) const {
    const u32 x0 = 16 * c;
    if (act && x0 + 16 > tot) acc = keep_head(acc, tot - x0);
    const uint4 v = make_uint4(act ? acc.x : 0u, act ? acc.y : 0u, act ? acc.z : 0u, act ? acc.w : 0u);
#ifdef TPZ_ABL_NOSTORE
    asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
#else
    if (c < npad) *reinterpret_cast<uint4*>(p + x0) = v;
#endif
  }
};

// Flat layout: the block's keys go to keys[kf ..] and its values to vals[vf ..], back to back
// with the neighbouring blocks'. The copy runs over a virtual stream whose chunks line up with
// the columns' 16-byte chunks: key byte x at 16-aligned position dk + x (dk = kf mod 16), value
// byte y at 16 kch + dv + y (kch = the key chunks, dv = vf mod 16). Whole chunks are stored
// with one 16-byte store; a column's first and last chunk hold the neighbours' bytes too and
// are stored byte by byte, one byte per lane (the neighbours' bytes belong to the waves that
// decode those blocks). The stores go through two descriptors that end at the
// block's last key / value chunk.
struct FlatOut {
  __amdgpu_buffer_rsrc_t rk, rv;   // from the 16-aligned key / value chunk base, 16 kch / 16 vch bytes
  u32 rgk, rgv;                    // the keys' / values' stream bytes [start, end): start | end << 16
                                   // (the values start at 16 kch + dv; wave-path blocks: < 2^16)
  __device__ __forceinline__ void put(u32 c, uint4 acc, bool skip) const {
    const int x0 = (int)(16 * c);
    const int kb = (int)((rgv & 0xFFFFu) & ~15u);            // 16 kch
    const bool isk = x0 < kb;
    const u32 rg = isk ? rgk : rgv;
    const int cs = (int)(rg & 0xFFFFu), ce = (int)(rg >> 16);
    // the column's bytes [lo, hi) of this chunk (hi <= lo: none)
    const int lo = max(cs, x0) - x0, hi = min(ce, x0 + 16) - x0;
    const bool act = !skip && hi > lo;
    const bool full = act && lo == 0 && hi == 16;
    const u32 off = (u32)(isk ? x0 : x0 - kb);
    const auto v4 = __builtin_bit_cast(__attribute__((ext_vector_type(4))) u32, acc);
    __builtin_amdgcn_raw_buffer_store_b128(v4, rk, (full && isk) ? off : kOob, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(v4, rv, (full && !isk) ? off : kOob, 0, 0);
    // A column's first and last chunk (at most four per block): the wave stores each one's bytes
    // [lo, hi) one byte per lane (lanes 0-15, one store instruction), the chunk broadcast from
    // its lane. (A per-lane cascade of naturally aligned pieces cost ~300 VALU per block.)
    u64 pm = __ballot(act && !full);
    while (pm) {
      const int L = __builtin_ctzll(pm);
      pm &= pm - 1;
      const u32 w0 = readlane(v4.x, L), w1 = readlane(v4.y, L), w2 = readlane(v4.z, L),
                w3 = readlane(v4.w, L);
      const u32 Lk = readlane(isk ? 1u : 0u, L);
      const u32 Lbase = readlane(off, L);
      const u32 Llo = readlane((u32)lo, L), Lhi = readlane((u32)hi, L);
      const u32 i = lane_id();
      const u32 w = i < 8 ? (i < 4 ? w0 : w1) : (i < 12 ? w2 : w3);
      const bool mine = i >= Llo && i < Lhi;
      __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w >> (8 * (i & 3u))), Lk ? rk : rv,
                                           mine ? Lbase + i : kOob, 0, 0);
    }
  }
};
// The flat destination of block b with K key and V value bytes (dk / dv: its column starts mod 16).
__device__ __forceinline__ FlatOut flat_out(const Out& o, u64 kf, u64 vf, u32 K, u32 V) {
  FlatOut D;
  const u32 dk = (u32)kf & 15u, dv = (u32)vf & 15u;
  const u32 kch = K ? (dk + K + 15) >> 4 : 0u;
  const u32 vch = V ? (dv + V + 15) >> 4 : 0u;
  D.rk = __builtin_amdgcn_make_buffer_rsrc(o.keys + (kf & ~15ull), (short)0, (int)(16 * kch), 0x00020000);
  D.rv = __builtin_amdgcn_make_buffer_rsrc(o.vals + (vf & ~15ull), (short)0, (int)(16 * vch), 0x00020000);
  const u32 vs = 16 * kch + dv;
  D.rgk = dk | (dk + K) << 16;
  D.rgv = vs | (vs + V) << 16;
  return D;
}
// Where the virtual stream's values start: the key chunks, then dv (flat); value_start(K)
// (slotted).
template <bool FLAT>
__device__ __forceinline__ u32 stream_vstart(u32 K, u32 dk, u32 dv) {
  return FLAT ? (K ? (dk + K + 15) & ~15u : 0u) + dv : (K + 15) & ~15u;
}
// The flat destination's put as a copy_window destination (every active chunk stored).
struct FlatDst {
  static constexpr bool kFlat = true;
  const FlatOut* d;
  __device__ __forceinline__ void put(u32 c, uint4 acc, bool act) const { d->put(c, acc, !act); }
};

// Output-driven copy of a block's stream (tot bytes: the keys, a gap to the next 16-byte
// boundary, the values): the wave takes 64 output chunks of 16 B per window (lane l: chunk
// c = 64 w + l), so every store is a coalesced 1 KiB.
//   1. chunk -> segment: the parse scattered (1 + table index) of every segment into the chunk
//      map at t = ceil(end / 16), the first chunk starting at or after the segment's end, so a
//      wave prefix max of map[c] (carried across windows) is the number of segments that end at
//      or before the chunk start = the segment j holding its first byte. (Two segments ending in
//      one chunk race for one map slot; a lane that got the smaller index walks forward.)
//   2. segments j and j + 1 from the entry table.
//   3. the chunk's bytes from LDS at x0 + delta_j; a chunk crossing segment j's end takes segment
//      j+1's bytes after it (exec-masked second read + 64-bit mask select); chunks spanning 3+
//      segments (entries shorter than 16 B) take a loop. The key/value gap is such a crossing:
//      its bytes are unspecified.
//   4. store; pad chunks up to the 128-byte line are zeroed.
// One window of the copy (chunks 64 w .. 64 w + 63); returns the carry for the next window.
template <class Col, class MapT, class S, class D>
__device__ __forceinline__ u32 copy_window(const S& src, const Col& col, const MapT* map, u32 nk,
                                           u32 tot, const D& dst, u32 map_len, u32 w, u32 carry) {
  const u32 nch = (tot + 15) >> 4;
  const u32 lane = lane_id();
  const u32 last = nk ? nk - 1 : 0u;
  const u32 c = 64 * w + lane;
  const u32 x0 = 16 * c;
  const bool act = c < nch;
  // 1. chunk -> entry: prefix max of the map, carried across the column's windows
  u32 j = map[min(c, map_len - 1)];
  j = max(wave_scan_max(act ? j : 0u), carry);
  const u32 carry_out = readlane(j, 63);
  // 2. entries j and j + 1 (one ds_read2_b32)
  u32 e0, e1;
  int d0, d1;
  col.get2(min(j, last), e0, d0, e1, d1);
  // 3. the chunk's bytes; a chunk crossing entry j's end also reads entry j+1's bytes
  //    (exec-masked). Reads are issued before the rare-case checks so they overlap.
  uint4 acc = src(act ? (int)x0 + d0 : 0);
  bool cross = act && j + 1 < nk && e0 < x0 + 16;
  uint4 nx = make_uint4(0, 0, 0, 0);
  if (cross) nx = src((int)x0 + d1);
  if (__ballot(act && e0 <= x0)) {
    // a lost map race (two entries ended in one chunk): walk forward to the holding entry
    // (flat: bounded by the last segment, which a trailing chunk of the virtual stream may lie
    // past; in the slotted stream the last segment holds the stream's end)
    while (act && e0 <= x0 && (!D::kFlat || j < last)) {
      j++;
      col.get2(min(j, last), e0, d0, e1, d1);
    }
    acc = src(act ? (int)x0 + d0 : 0);
    cross = act && j + 1 < nk && e0 < x0 + 16;
    if (cross) nx = src((int)x0 + d1);
  }
  if (cross) acc = merge_at(acc, nx, (int)(e0 - x0));
  // chunks spanning three or more entries (entries shorter than 16 B)
  if (__ballot(cross && e1 < x0 + 16 && j + 2 < nk)) {
    u32 k = j + 1, end = e1;
    while (cross && end < x0 + 16 && k + 1 < nk) {
      const int lo = (int)(end - x0);
      k++;
      int delta;
      col.get(k, end, delta);
      const int hi = min((int)(end - x0), 16);
      const uint4 v = src((int)x0 + delta);
      acc.x = (acc.x & ~byte_mask(lo, hi, 0)) | (v.x & byte_mask(lo, hi, 0));
      acc.y = (acc.y & ~byte_mask(lo, hi, 1)) | (v.y & byte_mask(lo, hi, 1));
      acc.z = (acc.z & ~byte_mask(lo, hi, 2)) | (v.z & byte_mask(lo, hi, 2));
      acc.w = (acc.w & ~byte_mask(lo, hi, 3)) | (v.w & byte_mask(lo, hi, 3));
    }
  }
  // 4. store (slotted: bytes past the stream and pad chunks up to the 128-byte line are zeroed)
  dst.put(c, acc, act);
  return carry_out;
}

template <class Col, class MapT, class S, class D>
__device__ __forceinline__ void copy_stream(const S& src, const Col& col, const MapT* map, u32 nk,
                                            u32 tot, const D& dst, u32 map_len) {
  const u32 lane = lane_id();
  const u32 nch = (tot + 15) >> 4;
  const u32 npad = (nch + 7) & ~7u;                   // whole 128-byte lines
  const u32 nw = (npad + 63) >> 6;
#ifdef TPZ_ABL_MEMONLY
  for (u32 c = lane; c < npad; c += 64) dst.put(c, make_uint4(c, 0, 0, 0), c < nch);
  return;
#endif
  u32 carry = 0;
  for (u32 w = 0; w < nw; w++) carry = copy_window(src, col, map, nk, tot, dst, map_len, w, carry);
}

// The wave path defers a block's CRC combine and status write into the next block's decode
// (PendingCrc): the combine's six dependent LDS round trips then overlap the next block's header
// and parse round trips instead of ending the block's dependent chain.
struct PendingCrc {
  u32 live;            // (uniform) a block's combine is pending
  u32 b, st, cnt, stored, k;
  u32 lc;              // per lane: the raw CRC of the lane's 80-byte run
  u32 early;           // (uniform) run it behind the next block's header reads (the block took
                       // the short-segment copy, whose windows leave the combine no room)
};

// (Every decode_block exit that does not hand the pending combine to copy_crc_piped runs it.)
__device__ __forceinline__ void finish_pending(const u32* tab, const Out& o, PendingCrc& pd) {
  if (!pd.live) return;
  const u32 R = crc_combine(tab, pd.lc);
  const u32 crc = (R == crc_shift_small(tab, ~pd.stored, pd.k)) ? pd.stored
                                                                   : ~crc_unshift_small(tab, R, pd.k);
  const bool ok = crc == pd.stored;                                            // checksum.rs:17
  put_meta(o, pd.b, ok ? pd.st : TPZ_BLOCK_CHECKSUM_MISMATCH, ok ? pd.cnt : 0u, crc);
  pd.live = 0;
}

struct FinishAtExit {
  const u32* tab;
  const Out& o;
  PendingCrc& pd;
  bool on;
  __device__ __forceinline__ ~FinishAtExit() {
    if (on) finish_pending(tab, o, pd);
  }
};

// The previous block's CRC combine (PendingCrc, crc_combine's six tree levels) split into steps
// that the copy + CRC of the next block interleaves with its own: level J's lookups are issued
// in one step and used (XOR, DPP hand-down) in the next, so its six dependent LDS round trips
// overlap the copy's and the CRC's.
template <int J>
__device__ __forceinline__ bool comb_lane(u32 lane) {
  return J == 0 ? (lane & 1u) == 1u : J == 1 ? (lane & 3u) == 2u : J == 2 ? (lane & 7u) == 4u
       : J == 3 ? (lane & 15u) == 8u : J == 4 ? (lane & 31u) == 16u : (lane & 47u) == 32u;
}
struct CombLv {
  u32 r0, r1, r2, r3;
};
template <int J>
__device__ __forceinline__ CombLv comb_issue(const u32* tab, u32 A) {
  // (lanes outside level J's set never read c: no zero fill, which cost four moves per level)
  CombLv c;
  if (comb_lane<J>(lane_id())) {        // exec-masked: fewer lanes touch LDS at each level
    constexpr int b0 = 16 + 4 * J;
    c.r0 = tlook(tab, b0, A & 0xFF);
    c.r1 = tlook(tab, b0 + 1, (A >> 8) & 0xFF);
    c.r2 = tlook(tab, b0 + 2, (A >> 16) & 0xFF);
    c.r3 = tlook(tab, b0 + 3, A >> 24);
  }
  return c;
}
template <int J>
__device__ __forceinline__ u32 comb_use(u32 A, const CombLv& c) {
  if (comb_lane<J>(lane_id())) A = xor3(c.r0, c.r1, c.r2) ^ c.r3;
  if (J < 4) A ^= dpp<kRowShl + (1 << (J < 4 ? J : 0))>(A);
  return A;
}

// The previous block's status, count and CRC from its combined value (finish_pending's tail).
__device__ __forceinline__ void comb_finish(const u32* tab, const Out& o, PendingCrc& pd, u32 cA,
                                            u32 want) {
  if (!pd.live) return;
  const u32 R = readlane(cA, 0) ^ readlane(cA, 16) ^ readlane(cA, 32) ^ readlane(cA, 48);
  const u32 crc = R == want ? pd.stored : ~crc_unshift_small(tab, R, pd.k);
  const bool ok = crc == pd.stored;                                            // checksum.rs:17
  put_meta(o, pd.b, ok ? pd.st : TPZ_BLOCK_CHECKSUM_MISMATCH, ok ? pd.cnt : 0u, crc);
  pd.live = 0;
}

// ------------------------------------------------------------------ fused copy + CRC (wave path)
// A wave-path block has at most 5 copy windows (stream <= len + 2 <= 4338 B) and its CRC at most
// five 80-byte slice-by-16 steps per lane (P + k <= 4351 B). The copy's LDS round trips (map ->
// scan -> entry table -> source) and the CRC's lookups are independent chains: here step t of
// both runs in one straight-line block, so each hides the other's LDS latency. The copy takes only
// its common path (one entry per chunk, or a crossing into the next entry): branch-free reads (an
// idle lane reads the zeroed guard), the stores through a descriptor that ends at the slot's last
// line (no exec masking). A window where any lane needs the rare path (a lost map race, a chunk
// spanning 3+ entries) is recorded and rewritten afterwards by copy_window.
struct CrcLane {
  int seg;      // the lane's run [seg, seg + 80) relative to the payload start (end-aligned)
  bool act;     // the run overlaps the payload
  u32 c;        // the run's raw CRC so far
};

__device__ __forceinline__ void crc_step(const u32* tab, const uint8_t* win, int pb, CrcLane& L,
                                         int t) {
  typedef u32 u32x4 __attribute__((ext_vector_type(4)));
  // (lanes whose run lies before the payload read the zeroed guard: switching them off instead,
  // an exec-masked branch, measured 4 % slower, profiles/r4/cskip/)
  const int a = L.act ? pb + L.seg + 16 * t : -kGuard;  // 16-byte aligned either way
  const u32x4 w = *reinterpret_cast<const u32x4*>(win + a);
  L.c = slice16(tab, w.x ^ L.c, w.y, w.z, w.w);
}
__device__ __forceinline__ u32 crc_lane_value(const u32* tab, const CrcLane& L) { return L.c; }

struct FastWin {
  u32 nk, tot, nch, npad, last;
  __amdgpu_buffer_rsrc_t out;  // the slot, npad * 16 bytes
};

// The common path of copy_window, branch-free; returns the carry, sets bit w of `rare` when any
// lane of the window needs copy_window's rare path.
template <bool FLAT, class S>
__device__ __forceinline__ u32 copy_fast(const S& src, const ColSmall& col, const uint16_t* map,
                                         const FastWin& F, const FlatOut& D, u32 w, u32 carry,
                                         u32& rare) {
  const u32 lane = lane_id();
  const u32 c = 64 * w + lane;
  const u32 x0 = 16 * c;
  const bool act = c < F.nch;
  u32 j = map[min(c, (u32)kWaveMapLen - 1)];
  j = max(wave_scan_max(act ? j : 0u), carry);
  const u32 carry_out = readlane(j, 63);
  u32 e0, e1;
  int d0, d1;
  col.get2(min(j, F.last), e0, d0, e1, d1);
  const bool cross = act && j + 1 < F.nk && e0 < x0 + 16;
  uint4 acc = src(act ? (int)x0 + d0 : -kGuard);
  const uint4 nx = src(cross ? (int)x0 + d1 : -kGuard);
  // a window where a lane needs copy_window's rare path is left to it whole (no store here, so
  // the two never write the same bytes)
  const bool rw = __ballot(act && (e0 <= x0 || (cross && e1 < x0 + 16 && j + 2 < F.nk))) != 0;
  if (rw) rare |= 1u << w;
  if (cross) acc = merge_at(acc, nx, (int)(e0 - x0));
  if (FLAT) {
    D.put(c, acc, rw);
  } else {
    // an idle lane read the zeroed guard: its pad chunk stores zeros without a select
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) u32, acc),
                                           F.out, rw ? kOob : x0, 0, 0);
  }
  return carry_out;
}

// copy_fast for blocks with segments shorter than 16 bytes (the Zipf keys): a chunk may hold
// three segments, and two segments ending in one chunk may have lost the map race (the map
// then names the earlier one). Entries j .. j+3 come from two ds_read2_b32; the chunk starts in
// j or j + 1 and takes up to three segments' bytes. Anything longer (segments under 8 bytes)
// is left to copy_window.
template <bool FLAT, class S>
__device__ __forceinline__ u32 copy_fast3(const S& src, const ColSmall& col, const uint16_t* map,
                                          const FastWin& F, const FlatOut& D, u32 w, u32 carry,
                                          u32& rare) {
  const u32 lane = lane_id();
  const u32 c = 64 * w + lane;
  const u32 x0 = 16 * c;
  const bool act = c < F.nch;
  u32 j = map[min(c, (u32)kWaveMapLen - 1)];
  j = max(wave_scan_max(act ? j : 0u), carry);
  const u32 carry_out = readlane(j, 63);
  u32 e0, e1, e2, e3;
  int d0, d1, d2, d3;
  col.get2(min(j, F.last), e0, d0, e1, d1);
  col.get2(min(j + 2, F.last), e2, d2, e3, d3);
  if (act && e0 <= x0) {            // a lost map race: the next entry holds the chunk start
    j++;
    e0 = e1, d0 = d1, e1 = e2, d1 = d2, e2 = e3, d2 = d3;
  }
  const bool b1 = act && j + 1 < F.nk && e0 < x0 + 16;
  const bool b2 = b1 && j + 2 < F.nk && e1 < x0 + 16;
  uint4 acc = src(act ? (int)x0 + d0 : -kGuard);
  const uint4 n1 = src(b1 ? (int)x0 + d1 : -kGuard);
  const uint4 n2 = src(b2 ? (int)x0 + d2 : -kGuard);
  const bool rw = __ballot(act && (e0 <= x0 || (b2 && e2 < x0 + 16 && j + 3 < F.nk))) != 0;
  if (rw) rare |= 1u << w;
  if (b1) acc = merge_at(acc, n1, (int)(e0 - x0));
  if (b2) acc = merge_at(acc, n2, (int)(e1 - x0));
  if (FLAT)
    D.put(c, acc, rw);
  else
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) u32, acc),
                                           F.out, rw ? kOob : x0, 0, 0);
  return carry_out;
}

// Copy of a wave-path block's stream fused with its CRC: returns R0(payload' || 0^k) as
// wave_crc does (the caller prepared the window the same way). SHORT (segments under 16 bytes:
// copy_fast3) is a template argument so that each instantiation is one straight-line region:
// a per-window branch between the two copies kept the scheduler from interleaving the copy
// windows with the CRC steps (3 % slower on the 4k config, profiles/r3/bisect_4k.jsonl).
// The stream's last chunk carries no bytes of other blocks or of earlier ones: every byte a
// chunk reads past its last segment lies in the block or in the 16 zeroed bytes after the payload.
template <bool SHORT, bool FLAT, class S>
__device__ __forceinline__ u32 copy_crc_fused(const u32* tab, const S& src, const ColSmall& col,
                                              const uint16_t* map, u32 nk, u32 tot, uint8_t* dst,
                                              const FlatOut& D, const uint8_t* win, int pb, u32 Pa,
                                              u32 kshift, Stamps& St, u32 w3, const Out& o,
                                              PendingCrc& pd) {
  // SHORT: windows t < w3 can hold chunks that span three segments (copy_fast3); the others
  // take copy_fast (a chunk it cannot do sends its window to copy_window, so either is exact)
  const u32 lane = lane_id();
  FastWin F;
  F.nk = nk;
  F.tot = tot;
  F.nch = (tot + 15) >> 4;
  F.npad = FLAT ? F.nch : (F.nch + 7) & ~7u;   // flat: no line padding (the neighbours' bytes)
  F.last = nk ? nk - 1 : 0u;
  F.out = __builtin_amdgcn_make_buffer_rsrc(dst, (short)0, FLAT ? 0 : (int)(F.npad * 16), 0x00020000);
  const u32 nw = (F.npad + 63) >> 6;
  CrcLane L;
  L.seg = (int)Pa - kCrcLaneBytes * (int)(lane + 1);
  L.act = L.seg + kCrcLaneBytes > 0;
  L.c = 0;
  u32 carry = 0, rare = 0, cw[5];
  // the previous block's combine (if still pending), two tree levels per window (comb_issue)
  const bool pl = pd.live != 0;
  u32 cA = pd.lc, want = 0;
  CombLv cl{0u, 0u, 0u, 0u};
  if (pl) {
    cl = comb_issue<0>(tab, cA);
    want = crc_shift_small(tab, ~pd.stored, pd.k);
  }
#pragma unroll
  for (int t = 0; t < 4; t++) {
    cw[t] = carry;
    crc_step(tab, win, pb, L, t);
    carry = (SHORT && (u32)t < w3) ? copy_fast3<FLAT>(src, col, map, F, D, (u32)t, carry, rare)
                                   : copy_fast<FLAT>(src, col, map, F, D, (u32)t, carry, rare);
    if (pl) {
      if (t == 0) { cA = comb_use<0>(cA, cl); cl = comb_issue<1>(tab, cA); }
      if (t == 1) { cA = comb_use<1>(cA, cl); cl = comb_issue<2>(tab, cA); }
      if (t == 2) { cA = comb_use<2>(cA, cl); cl = comb_issue<3>(tab, cA); }
      if (t == 3) { cA = comb_use<3>(cA, cl); cl = comb_issue<4>(tab, cA); }
    }
  }
  cw[4] = carry;
  crc_step(tab, win, pb, L, 4);
  if (pl) {
    cA = comb_use<4>(cA, cl);
    cl = comb_issue<5>(tab, cA);
  }
  if (nw > 4)
    carry = (SHORT && 4u < w3) ? copy_fast3<FLAT>(src, col, map, F, D, 4u, carry, rare)
                               : copy_fast<FLAT>(src, col, map, F, D, 4u, carry, rare);
  if (pl) comb_finish(tab, o, pd, comb_use<5>(cA, cl), want);
  TPZ_STAMP(St, 4);
#ifdef TPZ_ABL_STAMPS
  St.rare += __builtin_popcount(rare);
#endif
  if (rare) {
    for (u32 w = 0; w < nw; w++)
      if (rare & (1u << w)) {
        if (FLAT)
          copy_window(src, col, map, nk, F.tot, FlatDst{&D}, (u32)kWaveMapLen, w, cw[w]);
        else
          copy_window(src, col, map, nk, F.tot, SlotDst{dst, F.npad, F.tot}, (u32)kWaveMapLen, w, cw[w]);
      }
  }
  return crc_lane_value(tab, L);   // the lane's raw run CRC: crc_combine gives R0 of the range
}

// ------------------------------------------------------------------ pipelined copy + CRC
// LDS reads return in issue order and `s_waitcnt lgkmcnt(N)` waits for all but the N youngest,
// so waiting for one read also waits for every read issued before it. copy_crc_fused interleaves
// the copy's and the CRC's chains instruction by instruction, and the compiler's order made
// almost every wait a full drain (lgkmcnt(0)): each window's map read waited for the CRC lookups
// issued just before it, its gathers for both, and so on — about five LDS round trips per window
// in series. Here the two chains are staged so that each wait targets reads issued one stage
// earlier, with the other chain's reads behind them still in flight:
//   A  map reads of windows 0-3, CRC data of step 0
//   B  the four windows' prefix max (their DPP chains interleave), carries, entry reads
//   C  lookups of step 0, data of step 1
//   D  gathers of window 0
//   then per t: CRC step t+1 (xor of step t's lookups, lookups of step t+1, data of step t+2),
//               window t stored and window t+1's gathers issued
// __builtin_amdgcn_sched_barrier(0) between stages keeps the compiler from re-merging them; the
// waitcnt pass then counts the waits (lgkmcnt(N), N > 0). Blocks whose stream needs a fifth window
// (more than 4096 B of keys and values) copy it afterwards with copy_fast.
typedef u32 u32x2v __attribute__((ext_vector_type(2)));
typedef u32 u32x4v __attribute__((ext_vector_type(4)));
// the five 4-byte-aligned LDS words holding bytes [x, x + 16): two ds_read2_b32 and a ds_read_b32
// (issued, not waited for); no dword select afterwards (three 8-byte-aligned ds_read_b64 need a
// five-way dword select: 2.0 % slower, profiles/r6/ng/)
struct Gath {
  u32 d0, d1, d2, d3, d4;
};
__device__ __forceinline__ Gath gath_issue(const uint8_t* base, int x) {
  const u32* p = reinterpret_cast<const u32*>(base + (x & ~3));
  Gath g;
  g.d0 = p[0];
  g.d1 = p[1];
  g.d2 = p[2];
  g.d3 = p[3];
  g.d4 = p[4];
  return g;
}
__device__ __forceinline__ uint4 gath_finish(Gath g, int x) {
  asm volatile("" : "+v"(g.d0), "+v"(g.d1), "+v"(g.d2), "+v"(g.d3), "+v"(g.d4));
  const u32 s = (u32)x & 3u;
  return make_uint4(__builtin_amdgcn_alignbyte(g.d1, g.d0, s), __builtin_amdgcn_alignbyte(g.d2, g.d1, s),
                    __builtin_amdgcn_alignbyte(g.d3, g.d2, s), __builtin_amdgcn_alignbyte(g.d4, g.d3, s));
}
// the 16 lookups of a slice-by-16 step over (w0 ^ c, w1, w2, w3), issued
struct Look16 {
  u32 r[16];
};
__device__ __forceinline__ Look16 look_issue(const u32* tab, u32x4v w, u32 c) {
  Look16 L;
  const u32 w0 = w.x ^ c;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    L.r[i] = tlook(tab, 15 - i, (w0 >> (8 * i)) & 0xFF);
    L.r[4 + i] = tlook(tab, 11 - i, (w.y >> (8 * i)) & 0xFF);
    L.r[8 + i] = tlook(tab, 7 - i, (w.z >> (8 * i)) & 0xFF);
    L.r[12 + i] = tlook(tab, 3 - i, (w.w >> (8 * i)) & 0xFF);
  }
  return L;
}
__device__ __forceinline__ u32 look_xor(const Look16& L) {
  u32 c = xor3(L.r[0], L.r[1], L.r[2]);
  c = xor3(c, L.r[3], L.r[4]);
  c = xor3(c, L.r[5], L.r[6]);
  c = xor3(c, L.r[7], L.r[8]);
  c = xor3(c, L.r[9], L.r[10]);
  c = xor3(c, L.r[11], L.r[12]);
  c = xor3(c, L.r[13], L.r[14]);
  return c ^ L.r[15];
}
#define TPZ_SB() __builtin_amdgcn_sched_barrier(0)

// One copy window of copy_crc_piped, stage by stage.
struct PWin {
  u32 m, j;          // map slot, then the chunk's first segment
  u32 e0, e1;
  int d0, d1;
  bool act, cross;
  Gath ga, gn;
  u32 a[4], g[8];    // the dword index (copy_crc_piped<.., DW>): four LDS addresses, their reads
};
// Windows w < K3 of copy_crc_piped<K3>: the key windows of a block with keys under 16 bytes (Zipf
// keys), copy_fast3's chunk rule: entries j .. j + 3, a lost map race taken back, up to three
// segments per chunk; a chunk beyond that sends the window to copy_window afterwards.
struct PWin3 {
  u32 e2, e3;
  int d2, d3;
  bool b2;
  Gath g2;
};

// A regular block (decode_block): n entries at db + i S, S = 4 + KL + VL, every key KL and every
// value VL bytes, both >= 16. Its stream is n keys back to back, then from vs = value_start(n KL)
// n values back to back, so the entry that holds an output chunk and where its bytes lie follow
// from the chunk index: no entry table, no chunk map.
struct RegGeom {
  u32 n, KL, VL, db;
};
// Division of y < 4352 by a wave-uniform d in 16..4336 as (y * m) >> 26. It is exact for every m
// with 0 <= m d - 2^26 < 2^26 / 4352 = 15420, which holds for floor(2^26 / d) + 1 .. + 3 (3 d <=
// 13008). v_rcp_f32 is good to 1 ulp, so the truncated 2^26 * rcp(d) <= 2^22 lies within 1 of
// floor(2^26 / d), and adding 2 lands in that range (tests/test_regular_index.py walks every
// divisor and dividend). y and m are below 2^24: the product is two 24-bit multiplies.
constexpr u32 kRegShift = 26;
__device__ __forceinline__ u32 reg_recip(u32 d) {
  float f = (float)d;
  asm volatile("" : "+v"(f));   // (the reciprocal stays where it is asked for: not hoisted above
                                // the index cache's key compare, onto the path of a hit)
  u32 m = (u32)(__builtin_amdgcn_rcpf(f) * (float)(1u << kRegShift)) + 2u;
  asm volatile("" : "+v"(m));   // (finished here, not behind the readfirstlane)
  return uni(m);
}
// (the masks tell the compiler that the factors fit 24 bits: full-rate v_mul_u32_u24 /
// v_mul_hi_u32_u24 instead of the quarter-rate 32-bit multiplies)
__device__ __forceinline__ u32 mul24(u32 a, u32 b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
__device__ __forceinline__ u32 reg_div(u32 y, u32 m) {
  const u64 p = (u64)(y & 0x1FFFu) * (u64)(m & 0x7FFFFFu);
  return __builtin_amdgcn_alignbit((u32)(p >> 32), (u32)p, kRegShift) & 0x3FFu;
}

// Chunk c of a regular block at x0 = 16 c lies in key j = x0 / KL (x0 < n KL: the values start on
// a chunk boundary, so no chunk holds both) or in value j = (x0 - vs) / VL. With L that entry's
// length, base the region's start in the stream (0 or vs) and r = x0 - base - j L the chunk's
// first byte within the entry, the source is db + j S + 2 (+ 2 + KL) + r, so d0 = source - x0 =
// C + j T with T = S - L and C uniform; the entry ends at e0 = base + (j + 1) L, and the next
// one's bytes lie T further on (d1 = d0 + T). A chunk crosses at most one boundary (L >= 16).
// The last key's chunk crosses into the key/value gap (unspecified bytes): it takes what the
// general path reads there, the bytes before value 0 (gap: where those lie from the chunk's
// own source). The last value has no successor (e0 out of reach).
struct RegForm {
  u32 n, KL, VL, kc, vs, S, mk, mv;
  int gap;
  __device__ __forceinline__ RegForm(u32 n_, u32 KL_, u32 VL_) : n(n_), KL(KL_), VL(VL_) {
    kc = n * KL, vs = (kc + 15) & ~15u, S = 4 + KL + VL;
    mk = reg_recip(KL), mv = reg_recip(VL);
    gap = (int)(2 + KL) - (int)vs - (int)((n - 1) * (4 + VL));
  }
  // (db: the entries region in the window; 0 gives the offsets the index cache holds)
  __device__ __forceinline__ void entry(u32 x0, u32 db, bool isk, u32& e0, int& d0, int& d1) const {
    const u32 L = isk ? KL : VL, base = isk ? 0u : vs, T = S - L;
    const u32 j = reg_div(x0 - base, isk ? mk : mv);
    const bool last = j + 1 == n;
    e0 = (!isk && last) ? 0xFFFFu : base + mul24(j + 1, L);     // (j < 2^10, L and T < 2^13)
    d0 = (int)((isk ? db + 2 : db + 4 + KL - vs) + mul24(j, T));
    d1 = d0 + ((isk && last) ? gap : (int)T);
  }
  __device__ __forceinline__ void index(u32 w, u32 lane, u32 db, u32& e0, int& d0, int& d1) const {
    const u32 x0 = 16 * (64 * w + lane);
    // (a window wholly in the keys or wholly in the values: scalar selects)
    if (1024 * (w + 1) <= kc) entry(x0, db, true, e0, d0, d1);
    else if (1024 * w >= vs) entry(x0, db, false, e0, d0, d1);
    else entry(x0, db, x0 < kc, e0, d0, d1);
  }
};
// The index cache: what the gathers and the merge of chunk c take, relative to db,
// in one word: bits 0-12 the chunk's source x0 + d0 - db, bits 13-25 its successor's x0 + d1 - db
// + kRegBias (a crossing chunk's only, else 0), bits 26-30 m = e0 - x0, the bytes before the
// boundary (1..15), or 16: no crossing; bit 31: no chunk c (it reads the guard). The block is at
// most 4336 bytes and every source lies in it (tests/test_regular_cache_pack.py walks the shapes).
constexpr u32 kRegBias = 16, kRegNoChunk = 0x80000000u | (16u << 26);
__device__ __forceinline__ u32 reg_pack(const RegForm& R, u32 w, u32 lane, u32 nch) {
  const u32 c = 64 * w + lane, x0 = 16 * c;
  u32 e0;
  int d0, d1;
  R.entry(x0, 0u, x0 < R.kc, e0, d0, d1);     // (once per geometry: per-lane selects will do)
  const bool cross = e0 < x0 + 16;
  const u32 word = ((x0 + (u32)d0) & 0x1FFFu) |
                   (cross ? (((x0 + (u32)d1 + kRegBias) & 0x1FFFu) << 13) | ((e0 - x0) << 26) : 16u << 26);
  return c < nch ? word : kRegNoChunk;
}
// The dword index: what the cache holds instead when KL and VL are multiples of 4 (reg_eligible).
// Then every entry boundary of the stream falls on a dword of its chunk (m is 4, 8, 12 or 16), so
// output dword k of chunk c is four whole bytes of one source, the chunk's own (4 k < m) or its
// successor's: at f_k = (4 k < m ? A : B) + 4 k from db, A, B, m the fields of reg_pack's word.
// Two words per lane and window, lo = f_0 | f_1 << 16, hi = f_2 | f_3 << 16 (each f_k < 2^13; the
// sources' byte phases may differ: a key lies at 2 mod 4 from db, a value and the gap's bytes at
// 0); no chunk c: both 0, and lo != 0 otherwise (f_0 = A >= 2). 32 bytes per lane: the whole entry
// table (tests/test_regular_dword_index.py walks the shapes).
__device__ __forceinline__ bool reg_eligible(u32 KL, u32 VL) { return ((KL | VL) & 3u) == 0; }
__device__ __forceinline__ void reg_dwords(u32 word, u32& lo, u32& hi) {
  const u32 A = word & 0x1FFFu, B = ((word >> 13) & 0x1FFFu) - kRegBias, m = (word >> 26) & 31u;
  u32 f[4];
#pragma unroll
  for (u32 k = 0; k < 4; k++) f[k] = (4 * k < m ? A : B) + 4 * k;
  const bool none = (int)word < 0;
  lo = none ? 0u : f[0] | f[1] << 16;
  hi = none ? 0u : f[2] | f[3] << 16;
}
// The geometry whose index the wave's cache holds, in one word (one register across the block
// loop: with two the loop's SGPR spills went from 33 to 347). A regular block has n (6 + KL + VL) <=
// 4329, so n >= 2 leaves KL, VL < 4096: n << 24 | VL << 12 | KL with n <= 113; n = 1 sets bit 31
// and takes 13 bits for each. kRegNone: no index (a wave's first block, and after a parse that
// wrote the entry table).
constexpr u32 kRegNone = 0u;
__device__ __forceinline__ u32 reg_key(u32 n, u32 KL, u32 VL) {
  return n == 1 ? 0x80000000u | VL << 13 | KL : n << 24 | VL << 12 | KL;
}
// (the key and the index words exist in the slotted wave kernel only: the other instances of
// decode_block and of the block loop compile to what they were)
template <bool ON>
struct RegKeyVar {
  u32 key = kRegNone;
  __device__ __forceinline__ u32* ptr() { return &key; }
};
template <>
struct RegKeyVar<false> {
  __device__ __forceinline__ u32* ptr() { return nullptr; }
};
template <bool ON>
struct RegWords {
  u32x4v v;
};
template <>
struct RegWords<false> {};

// REG: the block is regular (G) and the windows' sources, successors and crossings come from the
// packed index rix (reg_pack: the wave's cache or built for this block) instead of the map, the
// prefix max and the entry table (col, map, nk are not read).
// DW: key and value lengths are multiples of 4, and rix and the table's second KiB hold the dword
// index (reg_dwords): an output dword is four whole bytes of one source, one ds_read2_b32 and one
// v_alignbyte; no second gather, no merge. (The fifth window keeps the closed form and merge_at.)
template <bool FLAT, u32 K3, bool REG = false, bool DW = false>
__device__ __forceinline__ u32 copy_crc_piped(const u32* tab, const ColSmall& col,
                                              const uint16_t* map, u32 nk, u32 tot, uint8_t* dst,
                                              const FlatOut& D, const uint8_t* win, int pb, u32 Pa,
                                              const Out& o, PendingCrc& pd, u32 k3n = K3,
                                              const RegGeom G = RegGeom{0u, 0u, 0u, 0u},
                                              const u32x4v rix = u32x4v{0u, 0u, 0u, 0u}) {
  static_assert(!REG || (K3 == 0 && !FLAT), "the regular copy: slotted, no short keys");
  static_assert(!DW || REG, "the dword index: regular blocks only");
  // (k3n <= K3, uniform: the windows that hold short keys; the others take the plain rule)
  const u32 lane = lane_id();
  FastWin F;
  F.nk = nk;
  F.tot = tot;
  F.nch = (tot + 15) >> 4;
  F.npad = FLAT ? F.nch : (F.nch + 7) & ~7u;
  F.last = nk ? nk - 1 : 0u;
  F.out = __builtin_amdgcn_make_buffer_rsrc(dst, (short)0, FLAT ? 0 : (int)(F.npad * 16), 0x00020000);
  const u32 nw = (F.npad + 63) >> 6;
  const int seg = (int)Pa - kCrcLaneBytes * (int)(lane + 1);
  const bool cact = seg + kCrcLaneBytes > 0;
  // lanes before the payload read the guard at -kGuard + 16 t (within its 96 zero bytes), so
  // every step's address is one base plus the instruction's offset
  const int cbase = cact ? pb + seg : -kGuard;
  auto dread = [&](int t) -> u32x4v {   // CRC data of step t (lanes before the payload: the guard)
    return *reinterpret_cast<const u32x4v*>(win + cbase + 16 * t);
  };
  PWin W[4];
  PWin3 W3;
  // REG: a window's PWin holds d0, d1 = the LDS offsets its two gathers read (the guard where
  // there is no chunk or no crossing) and e0 = m, the bytes before the boundary. One add per
  // address: db changes with every block and is not in the index.
  auto reg_unpack = [&](PWin& P, u32 word) {
    P.e0 = (word >> 26) & 31u;
    P.d0 = (int)word < 0 ? -kGuard : (int)(G.db + (word & 0x1FFFu));
    P.d1 = P.e0 < 16 ? (int)(G.db - kRegBias + ((word >> 13) & 0x1FFFu)) : -kGuard;
    // (unpacked here, in stage B, not sunk between a window's store and the next one's gathers)
    asm volatile("" : "+v"(P.e0), "+v"(P.d0), "+v"(P.d1));
  };
  // DW: a window's PWin holds a[k], the LDS address of the four source bytes of output dword k
  // (the guard where there is no chunk: an index of zeros). One add per address, the window's
  // address and db in its uniform term. Window w is unpacked one stage before its reads are
  // issued (w0 in B, w1 in E, w2 in G, w3 in I) and pinned there: four addresses per window live
  // at a time, not sixteen.
  const u32 wlds = (u32)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)win;
  auto dw_unpack = [&](PWin& P, u32 lo, u32 hi) {
    const u32 base = lo ? wlds + G.db : wlds - (u32)kGuard;
    P.a[0] = base + (lo & 0xFFFFu);
    P.a[1] = base + (lo >> 16);
    P.a[2] = base + (hi & 0xFFFFu);
    P.a[3] = base + (hi >> 16);
    asm volatile("" : "+v"(P.a[0]), "+v"(P.a[1]), "+v"(P.a[2]), "+v"(P.a[3]));
  };
  // A: map reads, CRC data of step 0
  if constexpr (!REG) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const u32 c = 64 * w + lane;
      W[w].act = c < F.nch;
      W[w].m = map[min(c, (u32)kWaveMapLen - 1)];
    }
  }
  u32x4v dA = dread(0);
  // the pending combine: level 0, and shift_k(~stored), the value R is compared with
  u32 cA = pd.lc;
  CombLv cl = comb_issue<0>(tab, cA);
  const u32 want = crc_shift_small(tab, ~pd.stored, pd.k);
  TPZ_SB();
  // B: prefix max per window (independent DPP chains), carries, entries j and j + 1
  //    (REG: the packed index, unpacked)
  u32 cw[5];
  cw[0] = 0;
  if constexpr (DW) {
    dw_unpack(W[0], rix.x, rix.y);
  } else if (REG) {
    reg_unpack(W[0], rix.x);
    reg_unpack(W[1], rix.y);
    reg_unpack(W[2], rix.z);
    reg_unpack(W[3], rix.w);
  } else {
#pragma unroll
    for (int w = 0; w < 4; w++) W[w].j = wave_scan_max(W[w].act ? W[w].m : 0u);
#pragma unroll
    for (int w = 0; w < 4; w++) {
      W[w].j = max(W[w].j, cw[w]);
      cw[w + 1] = readlane(W[w].j, 63);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) col.get2(min(W[w].j, F.last), W[w].e0, W[w].d0, W[w].e1, W[w].d1);
  }
  if (K3) col.get2(min(W[0].j + 2, F.last), W3.e2, W3.d2, W3.e3, W3.d3);
  cA = comb_use<0>(cA, cl);
  cl = comb_issue<1>(tab, cA);
  TPZ_SB();
  // C: lookups of step 0, data of step 1
  Look16 LK = look_issue(tab, dA, 0u);
  u32x4v dB = dread(1);
  cA = comb_use<1>(cA, cl);
  cl = comb_issue<2>(tab, cA);
  TPZ_SB();
  u32 rare = 0;
  auto gissue = [&](PWin& P, u32 w) {
    if constexpr (DW) {
      if (w < 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const __attribute__((address_space(3))) u32* q =
              (const __attribute__((address_space(3))) u32*)(uintptr_t)(P.a[k] & ~3u);
          P.g[2 * k] = q[0];
          P.g[2 * k + 1] = q[1];
        }
        return;
      }
    }
    if constexpr (REG) {
      P.ga = gath_issue(win, P.d0);
      P.gn = gath_issue(win, P.d1);
      return;
    }
    const u32 x0 = 16 * (64 * w + lane);
    if (w < K3 && w < k3n) {
      // (window 0's entries j + 2, j + 3 were read with its others; a later window's are read
      // here, into the same registers: window 0 has been stored by then)
      if (w > 0) col.get2(min(P.j + 2, F.last), W3.e2, W3.d2, W3.e3, W3.d3);
      if (P.act && P.e0 <= x0) {      // a lost map race: the next entry holds the chunk start
        P.j++;
        P.e0 = P.e1, P.d0 = P.d1, P.e1 = W3.e2, P.d1 = W3.d2, W3.e2 = W3.e3, W3.d2 = W3.d3;
      }
      P.cross = P.act && P.j + 1 < F.nk && P.e0 < x0 + 16;
      W3.b2 = P.cross && P.j + 2 < F.nk && P.e1 < x0 + 16;
      if (__ballot(P.act && (P.e0 <= x0 || (W3.b2 && W3.e2 < x0 + 16 && P.j + 3 < F.nk))) != 0)
        rare |= 1u << w;
      W3.g2 = gath_issue(win, W3.b2 ? (int)x0 + W3.d2 : -kGuard);
    } else {
      P.cross = P.act && P.j + 1 < F.nk && P.e0 < x0 + 16;
    }
    P.ga = gath_issue(win, P.act ? (int)x0 + P.d0 : -kGuard);
    P.gn = gath_issue(win, P.cross ? (int)x0 + P.d1 : -kGuard);
  };
  auto finish = [&](PWin& P, u32 w) {
    const u32 c = 64 * w + lane;
    const u32 x0 = 16 * c;
    if constexpr (DW) {
      if (w < 4) {
        u32x4v acc;
        asm volatile("" : "+v"(P.g[0]), "+v"(P.g[1]), "+v"(P.g[2]), "+v"(P.g[3]), "+v"(P.g[4]),
                     "+v"(P.g[5]), "+v"(P.g[6]), "+v"(P.g[7]));
        // (v_alignbyte_b32 shifts by its third operand's low two bits: the address itself will do)
        acc.x = __builtin_amdgcn_alignbyte(P.g[1], P.g[0], P.a[0]);
        acc.y = __builtin_amdgcn_alignbyte(P.g[3], P.g[2], P.a[1]);
        acc.z = __builtin_amdgcn_alignbyte(P.g[5], P.g[4], P.a[2]);
        acc.w = __builtin_amdgcn_alignbyte(P.g[7], P.g[6], P.a[3]);
        __builtin_amdgcn_raw_buffer_store_b128(acc, F.out, x0, 0, 0);
        return;
      }
    }
    if constexpr (REG) {
      uint4 acc = gath_finish(P.ga, P.d0);
      const uint4 nx = gath_finish(P.gn, P.d1);
      if (P.e0 < 16) acc = merge_at(acc, nx, (int)P.e0);   // (no mask held across the stages)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, acc), F.out, x0, 0, 0);
      return;
    }
    // (no rare path outside a K3 window 0: the other windows hold values of 16 bytes or more,
    // so no two segments end in one chunk and no chunk meets three segments)
    const bool rw = w < K3 && w < k3n && (rare & (1u << w));
    uint4 acc = gath_finish(P.ga, P.act ? (int)x0 + P.d0 : -kGuard);
    const uint4 nx = gath_finish(P.gn, P.cross ? (int)x0 + P.d1 : -kGuard);
    if (P.cross) acc = merge_at(acc, nx, (int)(P.e0 - x0));
    if (w < K3 && w < k3n) {
      const uint4 n2 = gath_finish(W3.g2, W3.b2 ? (int)x0 + W3.d2 : -kGuard);
      if (W3.b2) acc = merge_at(acc, n2, (int)(P.e1 - x0));
    }
    if (FLAT)
      D.put(c, acc, rw);
    else
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, acc), F.out, rw ? kOob : x0, 0, 0);
  };
  // D: gathers of window 0
  gissue(W[0], 0);
  cA = comb_use<2>(cA, cl);
  cl = comb_issue<3>(tab, cA);
  TPZ_SB();
  u32 crc = 0;
  // E: CRC step 1 ; F: window 0 out, window 1 gathers
  crc = look_xor(LK);
  LK = look_issue(tab, dB, crc);
  dA = dread(2);
  u32x4v rix2;     // DW: the index words of windows 2 and 3, read here, used in G and I
  if constexpr (DW) {
    dw_unpack(W[1], rix.z, rix.w);
    rix2 = *reinterpret_cast<const u32x4v*>(reinterpret_cast<const uint8_t*>(col.t) + 1024 + 16 * lane);
  }
  cA = comb_use<3>(cA, cl);
  cl = comb_issue<4>(tab, cA);
  TPZ_SB();
  finish(W[0], 0);
  gissue(W[1], 1);
  cA = comb_use<4>(cA, cl);
  cl = comb_issue<5>(tab, cA);
  TPZ_SB();
  // G: CRC step 2 ; H: window 1 out, window 2 gathers
  crc = look_xor(LK);
  LK = look_issue(tab, dA, crc);
  dB = dread(3);
  if constexpr (DW) dw_unpack(W[2], rix2.x, rix2.y);
  cA = comb_use<5>(cA, cl);
  comb_finish(tab, o, pd, cA, want);
  TPZ_SB();
  finish(W[1], 1);
  gissue(W[2], 2);
  TPZ_SB();
  // I: CRC step 3 ; J: window 2 out, window 3 gathers
  crc = look_xor(LK);
  LK = look_issue(tab, dB, crc);
  dA = dread(4);
  if constexpr (DW) dw_unpack(W[3], rix2.z, rix2.w);
  TPZ_SB();
  finish(W[2], 2);
  gissue(W[3], 3);
  TPZ_SB();
  // K: CRC step 4 ; L: window 3 out
  crc = look_xor(LK);
  LK = look_issue(tab, dA, crc);
  TPZ_SB();
  finish(W[3], 3);
  TPZ_SB();
  crc = look_xor(LK);
  if (nw > 4) {
    if (REG) {              // the fifth window by the closed form (rare: not in the index)
      const RegForm R(G.n, G.KL, G.VL);
      const u32 x0 = 16 * (256 + lane);
      u32 e0;
      int d0, d1;
      R.index(4u, lane, G.db, e0, d0, d1);
      const bool act = 256 + lane < F.nch, cross = act && e0 < x0 + 16;
      W[0].e0 = cross ? e0 - x0 : 16u;
      W[0].d0 = act ? (int)x0 + d0 : -kGuard;
      W[0].d1 = cross ? (int)x0 + d1 : -kGuard;
      gissue(W[0], 4u);
      finish(W[0], 4u);
    } else {
      (void)copy_fast<FLAT>(Src16{win}, col, map, F, D, 4u, cw[4], rare);
    }
  }
  if (!REG && rare) {
    for (u32 w = 0; w < nw; w++)
      if (rare & (1u << w)) {
        if (FLAT)
          copy_window(Src16{win}, col, map, nk, F.tot, FlatDst{&D}, (u32)kWaveMapLen, w, cw[w]);
        else
          copy_window(Src16{win}, col, map, nk, F.tot, SlotDst{dst, F.npad, F.tot}, (u32)kWaveMapLen, w, cw[w]);
      }
  }
  return crc;
}


// The window made ready for the CRC of its P >= 4 payload bytes at a0 (after the parse: it
// changes payload bytes); returns k, the zero bytes from the payload end to the 16-byte boundary.
__device__ __forceinline__ u32 crc_prepare(uint8_t* win, u32 a0, u32 P) {
  const u32 lane = lane_id();
  const u32 k = ((a0 + P + 15) & ~15u) - (a0 + P);
  if (lane < 4) win[a0 + lane] ^= 0xFFu;
  // the k bytes to the 16-byte boundary for the CRC; 16 in all, so that the copy's last chunk,
  // which may read up to 15 bytes past the payload, reads zeros there (deterministic output)
  if (lane < 16) win[a0 + P + lane] = 0;
  __builtin_amdgcn_wave_barrier();
  return k;
}

// Decode the block whose bytes are at win[a0 .. a0+len) (LDS), block index b. `map` is the
// stream's chunk map (kMapLen slots, LDS), `col` its entry table.
template <class Col, class MapT, int kMapLen, bool BIG, bool FLAT = false>
__device__ __forceinline__ void decode_block(const u32* tab, uint8_t* win, const Col& col,
                                             MapT* map, u32 a0, u32 len, u32 b, u64 ext_b,
                                             const Out& o, u32 kshift, Stamps& S, PendingCrc& pd,
                                             u64 kf = 0, u64 vf = 0, u64 ef = 0,
                                             const Out* o_lds = nullptr, u32* rk = nullptr) {
  const u32 lane = lane_id();
  // the header reads are issued together (one LDS round trip); the checks keep the reference's
  // order
  const u32 tag = win[(int)(a0 + len) - 1];                                    // compress.rs:99
  const u32 stored = bswap32(lds_u32(win, len >= 5 ? a0 + len - 5 : a0));      // block.rs:51
  const u32 n = lds_be16(win, a0);                                             // block.rs:54
  // flat layout: kf / vf = the block's first key / value byte in the columns (tpz_flat_layout;
  // loaded by the caller with the block's prefetch)
  const u32 dk = (u32)kf & 15u, dv = (u32)vf & 15u;
  // The parse's first round reads (lane i: entry i's offset, then its key length) are issued
  // before the previous block's combine, so their two dependent LDS round trips overlap its six.
  // The offset is read with the header (speculatively: lanes past n discard it).
  u32 e_off = 0, e_kl = 0;
  bool e_ok = false;
  if (!BIG) {
    e_off = lds_be16(win, a0 + 2 + 2 * lane);
    const u32 Pn = len - 5, db0 = a0 + 2 + 2 * n;
    e_ok = len >= 7 && lane < n && Pn >= 2 + 2 * n && e_off + 2 <= Pn - 2 - 2 * n;
    e_kl = lds_be16(win, e_ok ? db0 + e_off : a0);
  }
  RegWords<!BIG && !FLAT> rix;   // the block's packed copy index (slotted wave path, regular)
  // The previous block's combine: after a short-segment block it runs here, behind this block's
  // header reads (whose round trips it overlaps); otherwise this block's copy runs it level by
  // level between its own steps (copy_crc_piped / copy_crc_fused), and every other exit of this
  // block runs it whole (FinishAtExit).
  if (pd.early) finish_pending(tab, o, pd);
  FinishAtExit fin{tab, o, pd, true};
  if (len == 0) { put_meta(o, b, TPZ_BLOCK_EMPTY, 0, 0); return; }           // compress.rs:96
  if (tag == 0 || tag > 3) { put_meta(o, b, TPZ_BLOCK_BAD_TAG, 0, 0); return; } // :44-53,102
  if (tag != 1) { put_meta(o, b, TPZ_BLOCK_UNSUPPORTED_CODEC, 0, 0); return; }
  if (len - 1 < 4) { put_meta(o, b, TPZ_BLOCK_MALFORMED, 0, 0); return; }     // block.rs:49
  const u32 P = len - 5;
  const int pb = (int)a0;
  // The parse and the copy run BEFORE the CRC (its result only selects the status): the copy's
  // HBM stores then drain while the CRC computes, instead of stalling the next block's
  // s_waitcnt on the prefetch loads (loads and stores share vmcnt on gfx950). A block whose CRC
  // turns out wrong reports CHECKSUM_MISMATCH with count 0; its slot holds unspecified bytes.
  u32 st = TPZ_BLOCK_OK, cnt = n;
  bool fuse = false;           // copy fused with the CRC (wave path)
  bool f_short = false;        // segments under 16 bytes (copy_fast3)
  u32 f_w3 = 0;                // the leading windows that can hold them
  u32 f_nk = 0, f_tot = 0;
  uint8_t* f_dst = nullptr;
  FlatOut fo;                  // flat: the block's destination in the key / value columns
  if (P < 2 || P < 2 + 2 * n) {                                                // block.rs:54-59
    st = TPZ_BLOCK_MALFORMED;
    cnt = 0;
  } else if (!BIG && n > kWaveMaxN) {
    // the LDS big path (slotted); the spill path writes the flat columns directly
    const Out& oc = o_lds ? *o_lds : o;
    if (FLAT) defer_to(oc.spill_list, oc.spill_count, b);
    else defer_to(oc.defer_list, oc.defer_count, b);
    return;
  } else {
    const u32 db = a0 + 2 + 2 * n;   // entries region (Block.data), LDS offset
    const u32 dl = P - 2 - 2 * n;
    // (flat: the exact ends, n pairs reserved for every block by tpz_flat_layout)
    const bool slots_fit = FLAT || 6u * n <= len;
    // (flat and exact ends: ef = efirst[b], a scalar load issued with the block's prefetch; no
    // memory access here, so nothing in the parse waits on vmcnt)
    // (uniform: readfirstlane'd, so that the store's descriptor is built in SGPRs; the compiler
    // could not tell and wrapped the store in a waterfall loop)
    uint2* ends_g = reinterpret_cast<uint2*>(o.ends) + uni64((FLAT || o.efirst) ? ef : entry_base(ext_b, b));
    // whole 128-byte lines of {kend, vend} in the slotted layout; exactly n in the exact one
    const u32 n_pad = o.efirst ? n : (n + 15) & ~15u;
    // Round 0's value lengths (slotted wave path), read before the map is cleared: the
    // regularity test needs them, and the general parse below takes them from here.
    u32 r_vl = 0;
    bool r_ok = false;
    if constexpr (!BIG && !FLAT) {
      r_ok = e_ok && e_off + 4 + e_kl <= dl;                                     // iterator.rs:77-81
      if (r_ok) { r_vl = lds_be16(win, db + e_off + 2 + e_kl); r_ok = e_off + 4 + e_kl + r_vl <= dl; }
      // A regular block: every entry KL key and VL value bytes (entry 0's), both >= 16, at
      // offset i es, es = 4 + KL + VL, and the reference's bounds checks pass. Then the ends, the
      // totals and the copy's chunk -> entry rule are closed forms of (n, KL, VL): no map clear,
      // no scans, no entry table, no map (copy_crc_piped<.., REG>). Anything else (a length that
      // differs or is under 16, a hole, permuted or repeated offsets, a bad entry) takes the
      // general parse below; slack after the last entry is allowed.
      const u32 KL = readlane(e_kl, 0), VL = readlane(r_vl, 0), es = 4 + KL + VL;
      bool reg = n != 0 && KL >= 16 && VL >= 16 && P >= 4 && slots_fit &&
                 !__ballot(lane < n && !(r_ok && e_off == mul24(lane, es) && e_kl == KL && r_vl == VL));
      for (u32 g0 = 64; reg && g0 < n; g0 += 64) {
        const u32 i = g0 + lane;
        bool same = true;
        if (i < n) {
          const u32 off = lds_be16(win, a0 + 2 + 2 * i);
          same = off == mul24(i, es) && off + 4 + KL + VL <= dl;
          if (same) same = lds_be16(win, db + off) == KL && lds_be16(win, db + off + 2 + KL) == VL;
        }
        reg = !__ballot(!same);
      }
      const u32 kc = n * KL, vc = n * VL, vs = stream_vstart<false>(kc, 0u, 0u);
      if (reg && vs + vc <= len + 2u) {
        for (u32 g0 = 0; g0 < n; g0 += 64) {
          const u32 i = g0 + lane;
          __builtin_amdgcn_raw_buffer_store_b64(
              __builtin_bit_cast(__attribute__((ext_vector_type(2))) u32,
                                 i < n ? make_uint2(mul24(i + 1, KL), mul24(i + 1, VL)) : make_uint2(0, 0)),
              whole_rsrc(ends_g), i < n_pad ? 8 * i : kOob, 0, 0);
        }
        TPZ_STAMP(S, 2);
        TPZ_STAMP(S, 3);
        // The copy index depends on (n, KL, VL) alone (db is added where it is used): a block
        // with the geometry of the wave's last regular block takes the wave's cached words. Any
        // other builds the index by the closed form, caches it and goes on from its own words.
        // (The cached words, lane l's four windows at the head of the entry table, are read here,
        // whatever they hold, and used only on a hit: the read's round trip overlaps the ends
        // store and crc_prepare. Read with the header, before the test, the 4k copy ran 0.1-0.4 %
        // faster and zipf batches, which never use it, 0.1-0.5 % slower: profiles/regcache/.)
        // A geometry whose lengths are multiples of 4 keeps the dword index instead (reg_dwords):
        // windows 0 and 1 in the first KiB of the table, 2 and 3 in the second, 16 bytes per lane
        // each. Which one the words are follows from the key's geometry (uniform: no new state).
        const u32 key = reg_key(n, KL, VL);
        const bool dw = kRegDwordFits && reg_eligible(KL, VL);
        rix.v = *reinterpret_cast<const u32x4v*>(reinterpret_cast<const uint8_t*>(col.t) + 16 * lane);
        if (*rk != key) {
          const RegForm R(n, KL, VL);
          const u32 nch = (vs + vc + 15) >> 4;
          // (a loop, not unrolled, and read back: a miss is rare and its code stays small)
#pragma nounroll
          for (u32 w = 0; w < 4; w++) {
            const u32 word = reg_pack(R, w, lane, nch);
            if (dw) {
              u32 lo, hi;
              reg_dwords(word, lo, hi);
              col.t[256 * (w >> 1) + 4 * lane + 2 * (w & 1)] = lo;
              col.t[256 * (w >> 1) + 4 * lane + 2 * (w & 1) + 1] = hi;
            } else {
              col.t[4 * lane + w] = word;
            }
          }
          rix.v = *reinterpret_cast<const u32x4v*>(reinterpret_cast<const uint8_t*>(col.t) + 16 * lane);
          *rk = key;
        }
        __builtin_amdgcn_wave_barrier();
        const u32 k = crc_prepare(win, a0, P);
        fin.on = false;     // the previous block's combine runs in the copy, before pd is reused
        const u32 lc = dw ? copy_crc_piped<false, 0u, true, true>(
            tab, *reinterpret_cast<const ColSmall*>(&col), reinterpret_cast<const uint16_t*>(map),
            2 * n, vs + vc, o.data + slot_base(ext_b, b), fo, win, pb, P + k, o, pd, 0u,
            RegGeom{n, KL, VL, db}, rix.v)
                          : copy_crc_piped<false, 0u, true>(
            tab, *reinterpret_cast<const ColSmall*>(&col), reinterpret_cast<const uint16_t*>(map),
            2 * n, vs + vc, o.data + slot_base(ext_b, b), fo, win, pb, P + k, o, pd, 0u,
            RegGeom{n, KL, VL, db}, rix.v);
        pd = PendingCrc{1u, b, st, cnt, stored, k, lc, 0u};   // combined during the next block
        return;
      }
      // the general parse writes the entry table over the cached index
      *rk = kRegNone;
    }
    {
      // clear the chunk map up to the largest chunk index a block that fits its slot can
      // produce (stream <= len + 2 bytes; the others go to the spill path)
      constexpr u32 per = 16 / sizeof(MapT);
      const u32 nz = min((u32)kMapLen, ((len >> 4) + 3 + per - 1) / per * per);
      for (u32 i = lane; i < nz / per; i += 64)
        reinterpret_cast<uint4*>(map)[i] = make_uint4(0, 0, 0, 0);
    }
    // The value segments follow the key segments in the table, and the values start at the
    // 16-byte boundary after the keys: both need the block's key totals before the first table
    // write. One parse round (n <= 64) has them after its scan; longer blocks count first.
    u32 ktot = 0, knz_all = 0;
    if (n > 64) {
      for (u32 g0 = 0; g0 < n; g0 += 64) {
        const u32 i = g0 + lane;
        u32 kl = 0;
        if (i < n) {
          const u32 off = lds_be16(win, a0 + 2 + 2 * i);
          if (off + 2 <= dl) {
            kl = lds_be16(win, db + off);
            if (off + 4 + kl > dl) kl = 0;
          }
        }
        knz_all += __builtin_popcountll(__ballot(kl != 0));
        ktot += readlane(wave_scan_incl(kl), 63);
      }
    }
    u32 kc = 0, vc = 0, knz = 0, vnz = 0;
    bool bad = false, short_k = false, short_v = false;
    for (u32 g0 = 0; g0 < n; g0 += 64) {
      const u32 i = g0 + lane;
      const bool act = i < n;
      u32 off = 0, kl = 0, vl = 0;
      bool ok = true;
      if (act) {
        if (!BIG && !FLAT && g0 == 0) { // (read for the regularity test above)
          off = e_off;
          kl = e_kl;
          vl = r_vl;
          ok = r_ok;
        } else {
          if (!BIG && g0 == 0) {        // (read before the combine: e_ok = act && off + 2 <= dl)
            off = e_off;
            ok = e_ok;
            if (ok) { kl = e_kl; ok = off + 4 + kl <= dl; }
          } else {
            off = lds_be16(win, a0 + 2 + 2 * i);                                  // iterator.rs:74
            ok = off + 2 <= dl;
            if (ok) { kl = lds_be16(win, db + off); ok = off + 4 + kl <= dl; }    // :77-81
          }
          if (ok) { vl = lds_be16(win, db + off + 2 + kl); ok = off + 4 + kl + vl <= dl; } // :81-82
        }
        if (!ok) kl = vl = 0;
      }
      bad |= __ballot(act && !ok) != 0;
      short_k |= __ballot(kl != 0 && kl < 16) != 0;
      short_v |= __ballot(vl != 0 && vl < 16) != 0;
      const u32 ki = wave_scan_incl(kl) + kc;
      const u32 vi = wave_scan_incl(vl) + vc;
      const u64 kmask = __ballot(kl != 0), vmask = __ballot(vl != 0);
      if (n <= 64) {
        ktot = readlane(ki, 63);
        knz_all = __builtin_popcountll(kmask);
      }
      const u32 vs = stream_vstart<FLAT>(ktot, dk, dv);  // value stream start (tpz_value_start)
      __builtin_amdgcn_raw_buffer_store_b64(
          __builtin_bit_cast(__attribute__((ext_vector_type(2))) u32,
                             act ? make_uint2(ki, vi) : make_uint2(0, 0)),
          whole_rsrc(ends_g), (slots_fit && i < n_pad) ? 8 * i : kOob, 0, 0);
      if (act && slots_fit) {
        // entry table + chunk map: the chunk t = ceil(end / 16) is the first one starting at or
        // after the segment's end (ends beyond the map only occur in blocks that spill)
        if (kl) {
          const u32 m = knz + lanes_below(kmask);
          const u32 ke = ki + dk;   // the key's end in the stream (flat: shifted by dk)
          col.put(m, ke, (int)(db + off + 2) - (int)(ke - kl));
          if (((ke + 15) >> 4) < (u32)kMapLen) map[(ke + 15) >> 4] = (MapT)(m + 1);
        }
        if (vl) {
          const u32 m = knz_all + vnz + lanes_below(vmask);
          const u32 ve = vs + vi;
          col.put(m, ve, (int)(db + off + 4 + kl) - (int)(ve - vl));
          if (((ve + 15) >> 4) < (u32)kMapLen) map[(ve + 15) >> 4] = (MapT)(m + 1);
        }
      }
      knz += __builtin_popcountll(kmask);
      vnz += __builtin_popcountll(vmask);
      kc = readlane(ki, 63);
      vc = readlane(vi, 63);
    }

    const u32 vs = stream_vstart<FLAT>(kc, dk, dv);
    TPZ_STAMP(S, 2);
    // the slot holds len + 129 bytes; the flat stream has at most len + 2 + 45 bytes for
    // entries that neither overlap nor repeat (the map's length)
    if (bad || !slots_fit || vs + vc > len + (FLAT ? 47u : 2u)) {
      // entries out of range (Ok(Block) with per-entry classes: TPZ_BLOCK_BAD_ENTRY), or
      // entries that overlap or repeat: the spill path decodes the block (CRC included)
      const Out& oc = o_lds ? *o_lds : o;
      defer_to(oc.spill_list, oc.spill_count, b);
      return;
    } else {
      if (BIG) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      }
      __builtin_amdgcn_wave_barrier();
      // The stream ends at its last byte: a chunk past it would hold no segment (and the map's
      // walk to its segment would not end). Slotted: value_start(K) + V. Flat: the values end at
      // 16 kch + dv + V; with no values the keys end at dk + K (no value chunk at all).
      const u32 tot = FLAT ? (vc ? vs + vc : (kc ? dk + kc : 0u)) : vs + vc;
#ifndef TPZ_ABL_NOCOPY
#if !defined(TPZ_ABL_NOCRC) && !defined(TPZ_ABL_MEMONLY)
#ifdef TPZ_ABL_UNFUSED
      if (false) {            // timing build: the copy, then the CRC (wave_crc), as the big path
#else
      if (!BIG && P >= 4) {   // the copy runs fused with the CRC below
#endif
        fuse = true;
        // short values: every window; short keys only: the windows of the key chunks (the
        // values start on a chunk of their own)
        f_w3 = short_v ? 5u : (short_k ? (((FLAT ? dk : 0u) + kc + 15) / 16 + 63) / 64 : 0u);
        f_short = f_w3 != 0;
        f_nk = knz + vnz;
        f_tot = tot;
        f_dst = FLAT ? nullptr : o.data + slot_base(ext_b, b);
        if (FLAT) fo = flat_out(o, kf, vf, kc, vc);
      } else
#endif
      if (FLAT) {
        fo = flat_out(o, kf, vf, kc, vc);
        copy_stream(Src16{win}, col, map, knz + vnz, tot, FlatDst{&fo}, (u32)kMapLen);
      } else {
        const u32 nch = (tot + 15) >> 4;
        copy_stream(Src16{win}, col, map, knz + vnz, tot,
                    SlotDst{o.data + slot_base(ext_b, b), (nch + 7) & ~7u, tot}, (u32)kMapLen);
      }
#endif
    }
    TPZ_STAMP(S, 3);
  }
  __builtin_amdgcn_wave_barrier();
  u32 crc;
  if (P >= 4) {
    // fold init 0xFFFFFFFF into the first four payload bytes; zero the k bytes from the payload
    // end to the next 16-byte boundary (stored CRC and tag are already in registers). Then
    // R = R0(payload' || 0^k) = shift_k(R0(payload')), which equals shift_k(~stored) iff the CRC
    // matches. (The window is not used after this, so nothing is restored.)
    const u32 k = crc_prepare(win, a0, P);
#if defined(TPZ_ABL_NOCRC) || defined(TPZ_ABL_MEMONLY)
    crc = stored;
#else
    u32 R;
    if (!BIG && fuse) {
      u32 lc;
      fin.on = false;      // the previous block's combine runs here, before pd is reused
      if (!f_short) {
        lc = copy_crc_piped<FLAT, 0u>(tab, *reinterpret_cast<const ColSmall*>(&col),
                                         reinterpret_cast<const uint16_t*>(map), f_nk, f_tot, f_dst,
                                         fo, win, pb, P + k, o, pd);
      } else if (f_w3 <= 2u) {
        // short keys within the first two copy windows, values of 16 bytes or more (the Zipf
        // shape)
        lc = copy_crc_piped<FLAT, 2u>(tab, *reinterpret_cast<const ColSmall*>(&col),
                                      reinterpret_cast<const uint16_t*>(map), f_nk, f_tot, f_dst,
                                      fo, win, pb, P + k, o, pd, FLAT ? 2u : f_w3);
        // (slotted zipf 1.8699 -> 1.8614 ms with the window count; the flat kernel ran 0.4 %
        // slower with it and keeps both windows: profiles/r6/decode_ab/k3n_*)
        f_short = false;   // (its combine ran interleaved: the next block need not run it early)
      } else
      {
        lc = f_short
          ? copy_crc_fused<true, FLAT>(tab, Src16{win}, *reinterpret_cast<const ColSmall*>(&col),
                                       reinterpret_cast<const uint16_t*>(map), f_nk, f_tot, f_dst,
                                       fo, win, pb, P + k, kshift, S, f_w3, o, pd)
          : copy_crc_fused<false, FLAT>(tab, Src16{win}, *reinterpret_cast<const ColSmall*>(&col),
                                        reinterpret_cast<const uint16_t*>(map), f_nk, f_tot, f_dst,
                                        fo, win, pb, P + k, kshift, S, 5u, o, pd);
      }
      pd = PendingCrc{1u, b, st, cnt, stored, k, lc, f_short ? 1u : 0u};   // combined during the next block
      return;
    } else {
        R = wave_crc(tab, win, pb, P + k);
    }
    if constexpr (BIG)
      crc = (R == crc_shift_small(tab, ~stored, k)) ? stored : ~crc_unshift_small(tab, R, k);
    else
      crc = (R == crc_shift_small(tab, ~stored, k)) ? stored : ~crc_unshift_small(tab, R, k);
#endif
  } else {
    u32 c = 0xFFFFFFFFu;
    for (u32 i = 0; i < P; i++) {
      c ^= win[a0 + i];
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    crc = ~c;
  }
  if (crc != stored) {                                                         // checksum.rs:17
    st = TPZ_BLOCK_CHECKSUM_MISMATCH;
    cnt = 0;
  }
  TPZ_STAMP(S, 6);
  put_meta(o, b, st, cnt, crc);
}

__device__ __forceinline__ void load_tables(u32* tab, const u32* gtab, int bytes = kTableBytes) {
  const uint4* s = reinterpret_cast<const uint4*>(gtab);
  uint4* d = reinterpret_cast<uint4*>(tab);
  for (int i = threadIdx.x; i < bytes / 16; i += blockDim.x) d[i] = s[i];
  __syncthreads();
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t window_rsrc(const uint8_t* src, u64 src_bytes,
                                                               u64 wstart) {
  u64 rem = src_bytes > wstart ? src_bytes - wstart : 0;
  if (rem > 0x7FFFFFF0ull) rem = 0x7FFFFFF0ull;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(src + wstart), (short)0, (int)rem, 0x00020000);
}

// A 16-byte piece that straddles the end of the source buffer comes back zeroed from the
// range-checked buffer load; refill its in-range bytes (only the batch's last blocks). Branch-free
// per lane: clamped byte loads and selects.
__device__ __forceinline__ void fix_tail(uint4& v, const uint8_t* src, u64 piece, u64 src_bytes) {
  const bool straddle = piece + 16 > src_bytes && piece < src_bytes;
  if (__ballot(straddle)) {
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
      const u64 a = piece + k;
      const u32 byte = src[a < src_bytes ? a : src_bytes - 1];
      w[k >> 2] |= (a < src_bytes ? byte : 0u) << (8 * (k & 3));
    }
    v.x = straddle ? w[0] : v.x;
    v.y = straddle ? w[1] : v.y;
    v.z = straddle ? w[2] : v.z;
    v.w = straddle ? w[3] : v.w;
  }
}

struct Params {
  u64* big_scratch;  // gridDim(big) x 2 x kBigMaxSlots u64
  u64* spill_used;   // the spill arena cursor, zeroed here for the spill kernel
  const uint8_t* src;
  const u64* ext;
  u64 src_bytes;
  u32 n_blocks;
  const u32* crc_tables;
  Out out;
  u32 xp[kBigSuper];  // big path: x^(8 * 5120 r) mod P, the shift of CRC super-round r
  u32 lane_shift[64]; // wave path: x^(8 * 80 l) mod P, lane l's CRC run to the range end
  u32 chunk_shift;    // wave path: blocks claimed at a time = 2^chunk_shift (<= the row)
  u32* row_ctr;       // wave path: the rows of 16 blocks claimed so far (tail + kTailRow)
  u32* err;           // sticky error word (tail + kTailError)
};


// A load through the constant address space: a scalar load for a uniform index (memory no
// kernel of the launch writes).
template <class T>
__device__ __forceinline__ T const_load(const T* base, u64 i) {
  return reinterpret_cast<const __attribute__((address_space(4))) T*>(reinterpret_cast<uintptr_t>(base))[i];
}

// ------------------------------------------------------------------ wave path kernel
#ifdef TPZ_ABL_ROWLATE
// Diagnostic build (tests/test_gpu_row_claims.py): near the end of the batch (the global row
// counter within two rows per workgroup of the last row) some claimers (the waves that take the
// first chunk of a slot) sleep ~100 us between taking it and reading claims_done (point 0: odd
// waves), others between that read and their claim from the row counter (point 1: waves 2 mod
// 4), while the rest of the workgroup goes on (a block per wave takes ~7 us): a later slot's
// claim reaches the counter first and takes an earlier row, and a claimer reads claims_done after
// later claimers have claimed rows and a row past the batch has been published: the orders a
// fast box produces only rarely.
__device__ __noinline__ void rowlate_delay(const Params& p, u32 wid, u32 point) {
  const u32 rows = (p.n_blocks + kRowBlocks - 1) / kRowBlocks;
  const u32 ctr = __hip_atomic_load(p.row_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool late = point == 0 ? (wid & 1u) != 0 : (wid & 3u) == 2;
  if (late && ctr + 2 * gridDim.x >= rows)
    for (int i = 0; i < 30; i++) __builtin_amdgcn_s_sleep(127);
}
#endif
#ifdef TPZ_ABL_ONCHIP
// diagnostic (timing only): every wave decodes blocks 0..4095 over and over, so loads and stores
// stay on chip (L2 / Infinity Cache) and the launch time is the kernel's compute time
constexpr u32 kOnchipMask = 4095;
#endif
// CS: log2 of the blocks a wave claims at a time (launch_decode's choice, a compile-time constant
// so that the claim's shifts and masks take no registers)
template <bool FLAT, u32 CS>
#if defined(TPZ_ABL_W20) && !defined(TPZ_ABL_NOCAP)
__global__ __launch_bounds__(kWGThreads) __attribute__((amdgpu_waves_per_eu(5, 5)))
#else
__global__ __launch_bounds__(kWGThreads, 4)
#endif
void decode_wave_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaveLds];
  u32* tab = reinterpret_cast<u32*>(lds);
  __shared__ u32 chunk_next;          // the workgroup's next unclaimed chunk
  __shared__ Out out_lds;             // the worklist pointers for the rare paths (see above)
  // The row (of 16 blocks) of row slot s of this workgroup: row_ent[s % kRowRing] = row | s << 32
  // once published (one 64-bit LDS access writes and reads both halves; see claim_chunk)
  __shared__ u64 row_ent[kRowRing];
  // claims_done: set once a row past the batch has been published (every later claim from the
  // counter would be past it too). exit_slot: no slot from it on holds a row (see claim_chunk).
  __shared__ u32 claims_done, exit_slot;
  if (threadIdx.x == 0) {                  // (before the claims below: the same wave)
    claims_done = 0;
    exit_slot = ~0u;
  }
  if (threadIdx.x < kRowAhead && CS < kRowShift) {   // slots 0 .. kRowAhead-1 (load_tables' barrier publishes)
    const u32 r0 = atomicAdd(p.row_ctr, 1u);
    row_ent[threadIdx.x] = (u64)r0 | (u64)threadIdx.x << 32;
    if ((u64)r0 * kRowBlocks >= p.n_blocks) {
      claims_done = 1;
      atomicMin(&exit_slot, kRowAhead);    // every claim after the barrier sees claims_done
    }
  } else if (threadIdx.x < kRowRing) {
    row_ent[threadIdx.x] = ~0ull;
  }
  if (threadIdx.x == 0) {             // (load_tables' barrier publishes both)
    chunk_next = 0;
    out_lds = p.out;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *p.spill_used = 0;   // the spill phase runs after
  load_tables(tab, p.crc_tables, kWaveTabBytes);

  const u32 wid = uni(threadIdx.x >> 6);
  const u32 lane = lane_id();
  const u32 kshift = p.lane_shift[lane];
  uint8_t* slot = lds + kWaveTabBytes + wid * kSlotBytes;
  uint8_t* win = slot + kGuard;
  uint8_t* etab = win + kWinBytes + 32;
  const ColSmall col{reinterpret_cast<u32*>(etab)};
  uint16_t* map = reinterpret_cast<uint16_t*>(etab + kWaveTabSlots * 4);

  if (lane < kGuard / 16) reinterpret_cast<uint4*>(slot)[lane] = make_uint4(0, 0, 0, 0);
  const u32 nw = gridDim.x * kWavesPerWG;
  Stamps S;
#ifdef TPZ_ABL_STAMPS
  S.last = stamp_now();
#endif

  // Rows of 16 consecutive blocks, claimed by the workgroups from one global counter, so that
  // every workgroup works near the others and the batch is read and written through a narrow
  // moving window (static rows, r * grid + blockIdx.x, let the workgroups drift apart and spread
  // the accesses in flight over the buffer: a persistent 4 KiB-chunk copy ran at 5.75 TB/s with
  // static rows and 6.24 TB/s with claimed rows, the one-shot copy's rate; tools/ubench_pipe.hip,
  // profiles/r5/). Within a workgroup the rows fill row slots 0, 1, 2, ...; a wave takes the
  // next chunk of kChunk consecutive blocks from an LDS counter when it finishes one: the waves
  // of a CU do not run at one speed (with a fixed block per wave, the first four waves of each
  // workgroup finished at 1.66 ms and the last four at 2.21 ms of a 2.26 ms launch,
  // a round-3 per-wave timing build), so a fixed split left the fast waves idle while the slow
  // ones finished.
  // Lane l of a chunk's extent group holds ext[] of the chunk's block l (loaded one chunk ahead,
  // so a block's extent is two readlanes instead of a memory round trip).
#ifdef TPZ_WAVE_CHUNK
  const u32 cshift = __builtin_ctz((u32)TPZ_WAVE_CHUNK);
#else
  const u32 cshift = CS;
#endif
  const u32 kChunk = 1u << cshift, rshift = kRowShift - cshift;   // chunks per row: 2^rshift
  // claim_chunk returns the chunk's first block (saturated at n_blocks: a chunk past the batch
  // is empty). The wave that takes the first chunk of row slot s claims the row of slot
  // s + kRowAhead from the global counter and publishes it at its next claim (the atomic's value
  // has arrived by then: the prefetch wait at the top of the loop covers it), long before any
  // wave reaches that slot (kRowAhead - 1 rows of claims later); a reader that gets there first
  // waits for it (bounded; a timeout sets the sticky error word, tpz_decode_check).
  u32 pend_slot = ~0u, pend_row = 0;   // (uniform / lane 0) a claimed row not yet published
  const u32 kq = 1u << rshift;           // chunks per row slot
  auto publish = [&]() {
    if (pend_slot != ~0u) {
      if (lane == 0) {

        if ((u64)pend_row * kRowBlocks >= p.n_blocks) {
          // claims_done first, then the chunk counter: a chunk q >= Q was taken after this read,
          // so its claimer reads claims_done = 1 and claims no row. Rows are claimed only for the
          // slots of chunks q < Q, the last being slot (Q - 1) / kq + kRowAhead.
          __hip_atomic_store(&claims_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const u32 Q = __hip_atomic_fetch_add(&chunk_next, 0u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
          atomicMin(&exit_slot, Q == 0 ? kRowAhead : (Q - 1) / kq + kRowAhead + 1);
        }
        __hip_atomic_store(&row_ent[pend_slot % kRowRing], (u64)pend_row | (u64)pend_slot << 32,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      pend_slot = ~0u;
    }
  };
  // (Batches of long blocks claim whole rows, kChunk = 16: there the wave path only routes
  // blocks, a window of claimed rows buys nothing, and a row per claim would be a global atomic
  // per 16 blocks waited for by the next 16 waves; their rows stay static, r * grid + blockIdx.x.)
  const bool dyn_rows = rshift != 0;
  // The rows of a workgroup's slots need not increase with the slots (two waves' claims can
  // reach the counter in either order, and a claimer can read claims_done late), so neither a
  // row past the batch nor a slot left without a row (kRowExit) ends a wave: both are passed
  // over. A wave ends at its first chunk in a slot >= exit_slot, which the publisher of a row past
  // the batch sets from the chunk counter (publish above): every slot with a row lies below it,
  // and every chunk below it has been taken, by the order of the chunk counter. So no claimed row
  // is left behind whatever the timing (tests/test_row_claims.py models the protocol; the
  // diagnostic build TPZ_ABL_ROWLATE delays claimers to force the orders; round 5 ended a wave
  // at the first kRowExit slot, which lost the rows of later slots claimed by an earlier read of
  // claims_done: 2 blocks of 20,000 once).
  // The chunk counter is read one claim ahead (a ticket): a claim takes the ticket its previous
  // claim fetched and fetches the next, so the atomic's round trip is off the claim's chain. A
  // wave's held ticket when it ends is past its last chunk, hence past exit_slot too.
  u32 q_tk = 0;
  if (lane == 0) q_tk = atomicAdd(&chunk_next, 1u);
  auto claim_chunk = [&]() -> u32 {
    for (;;) {
      publish();
      const u32 q_old = q_tk;
      if (lane == 0) q_tk = atomicAdd(&chunk_next, 1u);
      const u32 q = uni(q_old);
      if (!dyn_rows) {
        const u64 f = ((u64)q * gridDim.x + blockIdx.x) * kRowBlocks;
        return f < p.n_blocks ? (u32)f : p.n_blocks;
      }
      const u32 slot_q = q >> rshift;
      if (slot_q >= uni(__hip_atomic_load(&exit_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)))
        return p.n_blocks;
      if ((q & ((1u << rshift) - 1u)) == 0) {
#ifdef TPZ_ABL_ROWLATE
        rowlate_delay(p, wid, 0);
#endif
        if (!uni(__hip_atomic_load(&claims_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
          pend_slot = slot_q + kRowAhead;
#ifdef TPZ_ABL_ROWLATE
          rowlate_delay(p, wid, 1);
#endif
          if (lane == 0) pend_row = atomicAdd(p.row_ctr, 1u);
        } else if (lane == 0) {
          const u32 sx = slot_q + kRowAhead;
          __hip_atomic_store(&row_ent[sx % kRowRing], (u64)kRowExit | (u64)sx << 32, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      u32 row = 0;
      if (lane == 0) {
        u32 spins = 0;
        u64 ent;
        // (a slot's entry is overwritten kRowRing slots later; a reader that finds a later slot
        // there, or waits past the bound, reports it through the sticky error word: the launch
        // fails loudly at tpz_decode_check instead of passing blocks over)
        while ((u32)((ent = __hip_atomic_load(&row_ent[slot_q % kRowRing], __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP)) >> 32) != slot_q) {
          const u32 rs = (u32)(ent >> 32);
          if (rs != ~0u && (int)(rs - slot_q) > 0) {
            atomicOr(p.err, 4u);
            break;
          }
          __builtin_amdgcn_s_sleep(2);
          if (++spins == (1u << 22)) {
            atomicOr(p.err, 2u);
            break;
          }
        }
        row = (u32)(ent >> 32) != slot_q ? kRowExit : (u32)ent;
      }
      row = uni(row);
      if (row != kRowExit) {
        const u64 f = (u64)row * kRowBlocks + ((q & ((1u << rshift) - 1u)) << cshift);
        if (f < p.n_blocks) return (u32)f;
      }
      // (a row past the batch, or a chunk past the last row's blocks: the next chunk)
    }
  };
  auto chunk_first = [](u32 f) -> u32 { return f; };
  // Lane l <= kChunk holds ext[first + l]: block j of the chunk spans lanes j and j + 1 (one
  // u64 per lane per chunk in flight; two extents per lane cost the loop VGPRs it spilled)
  u64 gs_cur, gs_nxt;
  auto load_group = [&](u32 q, u64& gs) {
    // lanes past the chunk or the batch re-read an extent (unconditional: the loads write their
    // destination registers directly, nothing waits for them until the chunk is used)
#ifdef TPZ_ABL_ONCHIP
    // timing build: the same 4096 blocks over and over (L2/MALL-resident; chunks tile 4096)
    u32 bb = (chunk_first(q) & kOnchipMask) + (lane <= kChunk ? lane : 0u);
#else
    u32 bb = chunk_first(q) + (lane <= kChunk ? lane : 0u);
#endif
    bb = bb < p.n_blocks ? bb : p.n_blocks;
    gs = p.ext[bb];
  };
  auto lane64 = [](u64 x, u32 l) { return ((u64)readlane((u32)(x >> 32), l) << 32) | readlane((u32)x, l); };
  // Blocks that do not fit a wave slot are sent to their worklist when their chunk becomes
  // current: fewer than 64 entries -> the one-wave-per-block kernel, past the big path's window
  // -> the spill path, else the LDS big path. The decode loop then skips them.
  auto triage_group = [&](u32 q, u64 gs) {
    // lane l's block ends where lane l + 1's starts: a DPP row shift (no LDS), lane 15 from 16
    // (a chunk is at most a row of 16 blocks)
    // (no bound_ctrl: a lane whose source is outside its row keeps `old`, here lane 16's value,
    // in one instruction. A select between a DPP and a readlane became a branch, and DPP reads
    // of lanes the branch had switched off returned 0.)
    const u32 glo = (u32)__builtin_amdgcn_update_dpp((int)readlane((u32)gs, 16), (int)(u32)gs,
                                                     kRowShl + 1, 0xF, 0xF, false);
    const u32 ghi = (u32)__builtin_amdgcn_update_dpp((int)readlane((u32)(gs >> 32), 16),
                                                     (int)(u32)(gs >> 32), kRowShl + 1, 0xF, 0xF, false);
    const u64 ge = ((u64)ghi << 32) | glo;
    const u32 cf = chunk_first(q), bb = cf + lane;     // (lane < n_blocks - cf: no wrap)
    const bool lng = lane < kChunk && lane < p.n_blocks - cf && ge - gs > kWaveMaxLen;
    if (!__ballot(lng)) return;
    const Out& oc = out_lds;
    u32 nent = 0xFFFFu;
    if (lng) nent = ((u32)p.src[gs] << 8) | p.src[gs + 1];
    const bool to_bw = lng && nent < 64 && oc.bw_list && ge - gs <= TPZ_BIGWAVE_BLOCK_BYTES;
    // (flat: every long block to the spill path, which writes the columns directly)
    const bool to_spill = lng && !to_bw && (FLAT || ge - gs > kBigMaxLen);
    if (oc.bw_list) defer_lanes(oc.bw_list, oc.bw_count, to_bw, (u32)bb);
    defer_lanes(oc.spill_list, oc.spill_count, to_spill, (u32)bb);
    defer_lanes(oc.defer_list, oc.defer_count, lng && !to_bw && !to_spill, (u32)bb);
  };
  u32 q_cur = claim_chunk(), q_nxt = claim_chunk();
  load_group(q_cur, gs_cur);
  load_group(q_nxt, gs_nxt);
  triage_group(q_cur, gs_cur);
  u32 j = 0;                              // the block's position in its chunk
  u32 b = chunk_first(q_cur);

  // prefetch state for block b
  uint4 v[kWinRounds];
  u64 s_cur = 0, e_cur = 0;
  u64 kf_cur = 0, vf_cur = 0, ef_cur = 0;   // the block's column starts (flat) and ends start (flat
                                             // and exact ends), loaded one block ahead
  auto issue = [&](u32 bb, u32 jj, u64& s, u64& e) {
    // (The flat kernel keeps its two early returns, here and below: its loop is as it was.
    // Without them its <true, 0> instance spills 223 SGPRs and takes scratch, and with the
    // second alone it measured 0.5-1 % slower, profiles/prefetch/ab_flat4k_*.)
    if (FLAT && bb >= p.n_blocks) return;
    if (bb < p.n_blocks) {   // (past the batch the loop ends: the stale values are never used)
      if (FLAT) {   // (scalar loads: uniform, and no VGPRs held across the block)
        kf_cur = const_load(p.out.kfirst, bb);
        vf_cur = const_load(p.out.vfirst, bb);
        ef_cur = const_load(p.out.efirst, bb);
      } else if (p.out.efirst) {
        // exact ends: the block's first pair, a scalar load as well. (A vector load in the parse
        // made the compiler wait vmcnt(0) there on every block, in the slotted layout too: both
        // arms of the select wrote one register pair. That drained this prefetch and the
        // previous block's stores: one exposed HBM round trip per block.)
        ef_cur = const_load(p.out.efirst, bb);
      }
    }
    s = lane64(gs_cur, jj);
    e = lane64(gs_cur, jj + 1);
    // a block past the batch or too long for the wave path (decoded elsewhere): the same five
    // loads through an empty descriptor, which fetch nothing. Every path then issues the same
    // vector-memory operations and the loads' registers are written on every path (an early
    // return made the compiler copy them at the merge, behind a wait for the loads).
    const bool take = bb < p.n_blocks && e - s <= kWaveMaxLen;
    if (FLAT && !take) return;
    const u64 ws = s & ~15ull;
    const u32 nbytes = (u32)(e - ws);
    const u32 rounds = (nbytes + 1023) >> 10;
    // the descriptor ends at the block's last 16-byte piece: lanes past it fetch nothing (the
    // next block's bytes are loaded once, by the wave that decodes it)
    const u64 e16 = (e + 15) & ~(u64)15;
    const u64 lim = !take ? 0 : p.src_bytes < e16 ? p.src_bytes : e16;
    __amdgpu_buffer_rsrc_t rs = window_rsrc(p.src, lim, take ? ws : 0);
    // all five loads unconditionally: the descriptor drops the pieces past the block (no
    // traffic), and the loads issue back to back with no branch between them (measured 2.3 %
    // faster than loading only the block's rounds, profiles/r2/ablations.jsonl)
#pragma unroll
    for (int r = 0; r < kWinRounds; r++)
      v[r] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (u32)(r * 1024 + lane * 16), 0, 0));
    // (through the window's descriptor, which is in SGPRs already; it spans lim - ws <=
    // kWaveMaxLen + 30 bytes, or none: every padding offset is far outside it)
    static_assert(kWaveMaxLen + 64 < kOob - 64u * kVmPad, "padding stores stay out of range");
    vm_pad<FLAT ? 0 : kVmPad>(rs);
    if (take && e + 16 > p.src_bytes) {
#pragma unroll
      for (int r = 0; r < kWinRounds; r++)
        if ((u32)r < rounds) fix_tail(v[r], p.src, ws + r * 1024 + lane * 16, p.src_bytes);
    }
  };
  PendingCrc pd{0u, 0u, 0u, 0u, 0u, 0u, 0u};
  RegKeyVar<!FLAT> rk;                  // (uniform) the geometry of the wave's cached copy index
#ifndef TPZ_ABL_NOPF
  issue(b, 0, s_cur, e_cur);
#endif

  while (b < p.n_blocks) {
#ifdef TPZ_ABL_NOPF
    // timing build: no prefetch (the block's loads issued and waited for at its staging; frees
    // the 20 VGPRs the prefetch holds across a block)
    issue(b, j, s_cur, e_cur);
#endif
    const u64 s = s_cur, e = e_cur;
    const u64 kf = kf_cur, vf = vf_cur, ef = ef_cur;
    const u32 len64 = (e - s) > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)(e - s);
    const bool fits = (e - s) <= kWaveMaxLen;
    if (fits) {
      // every round: the loads past the block's last piece returned zeros (the descriptor), and
      // the window holds all of rounds 0-3 and the first 256 bytes of round 4 (no per-round
      // conditions: 0.x % per block)
#pragma unroll
      for (int r = 0; r < kWinRounds - 1; r++) *reinterpret_cast<uint4*>(win + r * 1024 + lane * 16) = v[r];
      static_assert(kWinBytes == 4 * 1024 + 256, "round 4 fills lanes 0-15");
      if (lane < 16) *reinterpret_cast<uint4*>(win + 4 * 1024 + lane * 16) = v[4];
      // the bytes of the first piece before the block (the previous block's tail) read as zero
      // for the CRC (one byte store per lane, in LDS order after the piece)
      if (lane < (u32)(s & 15u)) win[lane] = 0;
    }
    TPZ_STAMP(S, 0);
    const u32 bcur = b;
    if (++j == kChunk) {              // next chunk (its extent loads completed long ago)
      j = 0;
      q_cur = q_nxt;
      gs_cur = gs_nxt;
      q_nxt = claim_chunk();
      load_group(q_nxt, gs_nxt);
      triage_group(q_cur, gs_cur);
    }
    b = chunk_first(q_cur) + j;
    b = b < p.n_blocks ? b : p.n_blocks;
#ifndef TPZ_ABL_NOPF
    issue(b, j, s_cur, e_cur);       // next block's loads fly while this one decodes
#endif
    __builtin_amdgcn_wave_barrier();
    TPZ_STAMP(S, 1);
    if (fits) {
#ifdef TPZ_ABL_ONCHIP
      const u32 bdec = bcur & kOnchipMask;
#else
      const u32 bdec = bcur;
#endif
      decode_block<ColSmall, uint16_t, kWaveMapLen, false, FLAT>(tab, win, col, map, (u32)(s & 15u),
                                                           len64, bdec, s, p.out, kshift, S, pd, kf, vf,
                                                           ef, &out_lds, rk.ptr());
    }                                // (long blocks went to their worklist in triage_group)
    __builtin_amdgcn_wave_barrier();
    TPZ_STAMP(S, 5);
  }
  publish();                         // (a wave waiting for this slot's row reads past the end)
  finish_pending(tab, p.out, pd);    // the wave's last block
#ifdef TPZ_ABL_STAMPS
  const u32 gw = blockIdx.x * kWavesPerWG + wid;
  if (lane == 0 && gw < (u32)kStampWaves)
    for (int k = 0; k < 7; k++) g_stamps[gw * 8 + k] = S.t[k];
  if (lane == 0 && gw < (u32)kStampWaves) g_stamps[gw * 8 + 7] = S.rare;
#endif
}

// ------------------------------------------------------------------ big path kernel
// Blocks the wave path defers (len > 4336 B or n > 255 entries) are decoded by one 16-wave
// workgroup each (one workgroup per CU: the 92 KiB window). The phases run wave-parallel with
// workgroup barriers between them:
//   stage   every thread loads 16-B pieces of the block into the window (<= 6 per thread);
//   parse   pass 1: each wave sums its 64-entry groups (key/value bytes, non-empty counts, bad)
//           into LDS; pass 2: each wave re-parses its groups with the exclusive prefix of those
//           sums, writes the entry ends, the entry table and the chunk map (as decode_block);
//   copy    the maximum of the chunk map per 64-chunk window, then each wave copies its windows
//           with the carry = the maximum over the windows before it (copy_window);
//   CRC     wave w folds the 5120-B super-rounds r = w (mod 16) as wave_crc does and shifts each
//           by its distance to the block end (gf_mul with x^(8*5120 r)); the 16 wave values
//           XOR into R0 of the payload.
// Group sums in LDS: key bytes and value bytes as full u32 (entries may overlap or repeat, so a
// group's sums are bounded by 64 x 65535, not by the block length; a block's by 47096 x 65535 <
// 2^32), and cnt = non-empty keys [0,7) | non-empty values [7,14) | malformed [14].
__device__ __forceinline__ u32 wave_sum(u32 x) { return readlane(wave_scan_incl(x), 63); }
__device__ __forceinline__ u32 wave_max(u32 x) { return readlane(wave_scan_max(x), 63); }

struct GroupSums {
  u32* kb;
  u32* vb;
  uint16_t* cnt;
};

struct BigSums {
  u32 kb = 0, vb = 0, kn = 0, vn = 0;
  bool bad = false;
  // add the sums of groups [lo, hi) (wave-uniform)
  __device__ __forceinline__ void add(const GroupSums& gs, u32 lo, u32 hi) {
    const u32 lane = lane_id();
    for (u32 u0 = lo; u0 < hi; u0 += 64) {
      const u32 u = u0 + lane;
      const bool in = u < hi;
      kb += wave_sum(in ? gs.kb[u] : 0u);
      vb += wave_sum(in ? gs.vb[u] : 0u);
      const u32 g = in ? (u32)gs.cnt[u] : 0u;
      const u32 c = wave_sum((g & 0x7Fu) | (((g >> 7) & 0x7Fu) << 16));
      kn += c & 0xFFFFu;
      vn += c >> 16;
      bad |= __ballot((g >> 14) & 1u) != 0;
    }
  }
};

// Entry i's key and value lengths (iterator.rs:74-82); 0/0 and ok = false when malformed.
__device__ __forceinline__ void parse_entry(const uint8_t* win, u32 a0, u32 db, u32 dl, u32 i,
                                            u32& off, u32& kl, u32& vl, bool& ok) {
  off = lds_be16(win, a0 + 2 + 2 * i);
  ok = off + 2 <= dl;
  kl = vl = 0;
  if (ok) { kl = lds_be16(win, db + off); ok = off + 4 + kl <= dl; }
  if (ok) { vl = lds_be16(win, db + off + 2 + kl); ok = off + 4 + kl + vl <= dl; }
  if (!ok) kl = vl = 0;
}

// CRC super-round r of a big block's payload (wave_crc's lane runs), with decode_block's
// preparation applied in registers instead of in the window (init folded into payload bytes
// [0, 4), bytes [P, P + k) up to the 16-byte boundary zeroed), so the CRC can run while other
// waves parse and copy from the same window. Returns Z_{5120 r}(R0 of the round) (uniform).
__device__ __forceinline__ u32 big_crc_round(const Params& p, const u32* tab, const uint8_t* win,
                                             u32 a0, u32 P, u32 Pa, u32 r) {
  typedef u32 u32x4 __attribute__((ext_vector_type(4)));
  const u32 lane = lane_id();
  const int seg = (int)Pa - 5120 * (int)r - kCrcLaneBytes * (int)(lane + 1);
  u32 c = 0;
  if (seg + kCrcLaneBytes > 0) {
#pragma unroll
    for (int q = 0; q < kCrcLaneBytes / 16; q++) {
      const int base = seg + 16 * q;  // payload-relative offset of the 16 bytes
      u32x4 w = *reinterpret_cast<const u32x4*>(win + (int)a0 + base);
      if (base < 4 || base + 16 > (int)P) {   // the first or the last chunk of the payload
        const int zl = (int)P - base, zh = (int)Pa - base;
        w.x = (w.x ^ byte_mask(-base, 4 - base, 0)) & ~byte_mask(zl, zh, 0);
        w.y = (w.y ^ byte_mask(-base, 4 - base, 1)) & ~byte_mask(zl, zh, 1);
        w.z = (w.z ^ byte_mask(-base, 4 - base, 2)) & ~byte_mask(zl, zh, 2);
        w.w = (w.w ^ byte_mask(-base, 4 - base, 3)) & ~byte_mask(zl, zh, 3);
      }
      c = slice16(tab, w.x ^ c, w.y, w.z, w.w);
    }
  }
  return gf_mul(p.xp[r], crc_combine(tab, c));
}

// One big block after the header checks (all threads of the workgroup; n, stored read from the
// window). Phase 1: the waves that own 64-entry groups parse in two passes (group sums, then
// the ends and tables; with one group the same wave reads its own sums back, so no barrier sits
// between the passes) while the other waves fold the CRC super-rounds
// (round r on wave 15 - r mod 16); phase 2: the copy's window maxima; phase 3: the copy; then
// the wave CRCs are combined and the status stored.
template <class Col, bool kGlobalCol>
__device__ __forceinline__ void big_block(const Params& p, const u32* tab, uint8_t* win,
                                          const Col& col, uint16_t* map, const GroupSums& gsum, u32* wmax,
                                          u32* xs, u32 a0, u32 len, u32 n, u32 stored, u32 b,
                                          u64 ext_b, Stamps& S) {
  const u32 wid = uni(threadIdx.x >> 6), lane = lane_id();
  const Out& o = p.out;
  const u32 P = len - 5;
  const u32 k = ((a0 + P + 15) & ~15u) - (a0 + P);
  const u32 Pa = P + k;
#if defined(TPZ_ABL_NOCRC) || defined(TPZ_ABL_MEMONLY)
  const bool crc_wave = false;
#else
  const bool crc_wave = P >= 4;
#endif
  const u32 Sr = crc_wave ? (Pa + 5119) / 5120 : 0u;
  u32 A = 0;
  for (u32 r = kBigWaves - 1 - wid; r < Sr; r += kBigWaves) A ^= big_crc_round(p, tab, win, a0, P, Pa, r);
  if (lane == 0) xs[wid] = A;
  TPZ_STAMP(S, 4);

  u32 st = TPZ_BLOCK_OK, bcnt = n;
  u32 nk = 0, tot = 0;
  bool copy = false, spill = false;
  if (P < 2 || P < 2 + 2 * n) {                                                // block.rs:54-59
    st = TPZ_BLOCK_MALFORMED;
    bcnt = 0;
    __syncthreads();
  } else {
    const u32 db = a0 + 2 + 2 * n, dl = P - 2 - 2 * n;
    const bool slots_fit = 6u * n <= len;
    // (exact ends: a scalar load, as in the wave path; no vmcnt wait on the slotted arm)
    uint2* ends_g = reinterpret_cast<uint2*>(o.ends) +
                    uni64(o.efirst ? const_load(o.efirst, b) : entry_base(ext_b, b));
    const u32 n_pad = o.efirst ? n : (n + 15) & ~15u;
    const u32 G = (n + 63) >> 6;
    // pass 1: group sums (read back by the same wave when there is one group)
    for (u32 g = wid; g < G; g += kBigWaves) {
      const u32 i = 64 * g + lane;
      u32 off = 0, kl = 0, vl = 0;
      bool ok = true;
      if (i < n) parse_entry(win, a0, db, dl, i, off, kl, vl, ok);
      const u32 kb = wave_sum(kl), vb = wave_sum(vl);
      const u32 kn = __builtin_popcountll(__ballot(kl != 0)), vn = __builtin_popcountll(__ballot(vl != 0));
      const bool bad = __ballot(!ok) != 0;
      if (lane == 0) {
        gsum.kb[g] = kb;
        gsum.vb[g] = vb;
        gsum.cnt[g] = (uint16_t)(kn | (vn << 7) | ((u32)bad << 14));
      }
    }
    if (G > 1) __syncthreads();
    // pass 2: entry ends, entry table, chunk map
    if (wid < G) {
      BigSums T;
      T.add(gsum, 0, G);
      const u32 vs = (T.kb + 15) & ~15u;  // value stream start (tpz_value_start)
      BigSums C;
      u32 done = 0;
      for (u32 g = wid; g < G; g += kBigWaves) {
        C.add(gsum, done, g);
        done = g;
        const u32 i = 64 * g + lane;
        const bool act = i < n;
        u32 off = 0, kl = 0, vl = 0;
        bool ok = true;
        if (act) parse_entry(win, a0, db, dl, i, off, kl, vl, ok);
        const u32 ki = wave_scan_incl(kl) + C.kb;
        const u32 vi = wave_scan_incl(vl) + C.vb;
        const u64 kmask = __ballot(kl != 0), vmask = __ballot(vl != 0);
        __builtin_amdgcn_raw_buffer_store_b64(
            __builtin_bit_cast(__attribute__((ext_vector_type(2))) u32,
                               act ? make_uint2(ki, vi) : make_uint2(0, 0)),
            whole_rsrc(ends_g), (slots_fit && i < n_pad) ? 8 * i : kOob, 0, 0);
        if (act && slots_fit) {
          if (kl) {
            const u32 m = C.kn + lanes_below(kmask);
            col.put(m, ki, (int)(db + off + 2) - (int)(ki - kl));
            if (((ki + 15) >> 4) < (u32)kBigMapLen) map[(ki + 15) >> 4] = (uint16_t)(m + 1);
          }
          if (vl) {
            const u32 m = T.kn + C.vn + lanes_below(vmask);
            const u32 ve = vs + vi;
            col.put(m, ve, (int)(db + off + 4 + kl) - (int)(ve - vl));
            if (((ve + 15) >> 4) < (u32)kBigMapLen) map[(ve + 15) >> 4] = (uint16_t)(m + 1);
          }
        }
      }
      if (kGlobalCol) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      }
    }
    __syncthreads();
    BigSums T;
    T.add(gsum, 0, G);
    const u32 vs = (T.kb + 15) & ~15u;
    if (T.bad || !slots_fit || (u64)vs + T.vb > (u64)len + 2) {  // the slot holds len + 129 B
      spill = true;   // entries out of range, or overlapping / repeated: the spill path
    } else {
      copy = true;
      nk = T.kn + T.vn;
      tot = vs + T.vb;
    }
  }
  TPZ_STAMP(S, 1);
#ifdef TPZ_ABL_NOCOPY
  copy = false;
#endif
  if (copy) {
    const u32 nch = (tot + 15) >> 4;
    const u32 npad = (nch + 7) & ~7u;
    const u32 nw = (npad + 63) >> 6;
    for (u32 v = wid; v < nw; v += kBigWaves) {
      const u32 c = 64 * v + lane;
      const u32 m = wave_max(c < nch ? (u32)map[min(c, (u32)kBigMapLen - 1)] : 0u);
      if (lane == 0) wmax[v] = m;
    }
    __syncthreads();
    TPZ_STAMP(S, 2);
    uint8_t* dst = o.data + slot_base(ext_b, b);
    for (u32 j = wid; j < nw; j += kBigWaves) {
      u32 m = lane < j ? wmax[lane] : 0u;
      if (lane + 64 < j) m = max(m, wmax[lane + 64]);
      copy_window(Src16{win}, col, map, nk, tot, SlotDst{dst, npad, tot}, (u32)kBigMapLen, j, wave_max(m));
    }
    TPZ_STAMP(S, 3);
  }
  if (wid == 0 && spill) {
    defer_to(o.spill_list, o.spill_count, b);
  } else if (wid == 0) {
    u32 crc;
    if (crc_wave) {
      u32 R = 0;
#pragma unroll
      for (int w = 0; w < kBigWaves; w++) R ^= xs[w];
      crc = (R == crc_shift_small(tab, ~stored, k)) ? stored : ~crc_unshift_small(tab, R, k);
    } else {
      u32 c = 0xFFFFFFFFu;
      for (u32 i = 0; i < P; i++) {
        c ^= win[a0 + i];
        for (int q = 0; q < 8; q++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
      }
      crc = ~c;
    }
#if defined(TPZ_ABL_NOCRC) || defined(TPZ_ABL_MEMONLY)
    crc = stored;
#endif
    if (crc != stored) {                                                       // checksum.rs:17
      st = TPZ_BLOCK_CHECKSUM_MISMATCH;
      bcnt = 0;
    }
    put_meta(o, b, st, bcnt, crc);
  }
}

// Phase B of decode_tail_kernel: the cnt blocks of the big list, one per workgroup, claimed
// from the ticket counter (a workgroup only ever waits on blocks that running workgroups hold);
// *done counts the finished ones. Every thread of the workgroup calls it.
__device__ __forceinline__ void big_phase(const Params& p, uint8_t* lds, u32 cnt, u32* ticket,
                                          u32* done, u32* bcast) {
  u32* tab = reinterpret_cast<u32*>(lds);
  load_tables(tab, p.crc_tables);
  const u32 tid = threadIdx.x, wid = uni(tid >> 6), lane = lane_id();
  uint8_t* win = lds + kTableBytes + kGuard;
  uint16_t* map = reinterpret_cast<uint16_t*>(win + kBigWinBytes + 32);
  u32* wmax = reinterpret_cast<u32*>(map + kBigMapLen);
  u32* xs = wmax + kBigMaxWin;
  u64* ltab = reinterpret_cast<u64*>(xs + kBigWaves);        // 8-aligned: see static_assert
  GroupSums gsum;
  gsum.kb = reinterpret_cast<u32*>(ltab + kBigLdsSlots);
  gsum.vb = gsum.kb + kBigMaxGroups;
  gsum.cnt = reinterpret_cast<uint16_t*>(gsum.vb + kBigMaxGroups);
  if (tid < kGuard / 16) reinterpret_cast<uint4*>(win - kGuard)[tid] = make_uint4(0, 0, 0, 0);
  auto claim = [&]() -> u32 {
    __syncthreads();
    if (tid == 0) *bcast = atomicAdd(ticket, 1u);
    __syncthreads();
    return uni(*bcast);
  };
  // The next block's bytes are loaded into registers while this one decodes (16 B x <= 6 per
  // thread); workgroup barriers only wait for LDS, so the loads stay in flight across them.
  uint4 t[kBigStage];
  u32 b_nx = 0;
  u64 s_nx = 0, e_nx = 0;
  auto issue = [&](u32 it) {
    b_nx = uni(p.out.defer_list[it]);
    s_nx = p.ext[b_nx];
    e_nx = p.ext[b_nx + 1];
    const u64 ws = s_nx & ~15ull;
    const u32 nbytes = (u32)(e_nx - ws);
    const u64 e16 = (e_nx + 15) & ~(u64)15;
    __amdgpu_buffer_rsrc_t rs = window_rsrc(p.src, p.src_bytes < e16 ? p.src_bytes : e16, ws);
#pragma unroll
    for (int r = 0; r < kBigStage; r++) {
      const u32 off = (u32)r * 16 * kBigThreads + 16 * tid;
      t[r] = off < nbytes ? __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0))
                          : make_uint4(0, 0, 0, 0);
    }
  };
  const u32 it0 = claim();
  if (it0 >= cnt) return;
  issue(it0);
  u32 nxt = claim();                       // the block after the one in flight
  Stamps S;
#ifdef TPZ_ABL_STAMPS
  S.last = stamp_now();
#endif
  for (;;) {
    const u32 b = b_nx;
    const u64 s = s_nx, e = e_nx;
    const u32 len = (u32)(e - s);
    const u64 ws = s & ~15ull;
    const u32 nbytes = (u32)(e - ws);
    __syncthreads();  // the previous block is done with the window
    {
      // clear the chunk map up to the largest chunk index a slot-fitting block can produce
      const u32 nz = min((u32)kBigMapLen, ((len >> 4) + 3 + 7) / 8 * 8);
      for (u32 i = tid; i < nz / 8; i += kBigThreads) reinterpret_cast<uint4*>(map)[i] = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < kBigStage; r++) {
      const u32 off = (u32)r * 16 * kBigThreads + 16 * tid;
      if (off < nbytes) {
        fix_tail(t[r], p.src, ws + off, p.src_bytes);
        if (off == 0) t[r] = zero_head(t[r], (u32)(s & 15u));
        *reinterpret_cast<uint4*>(win + off) = t[r];
      }
    }
    __syncthreads();
    TPZ_STAMP(S, 0);
    const bool more = nxt < cnt;
    if (more) issue(nxt);
    [&]() {
      const u32 a0 = (u32)(s & 15u);
      const u32 tag = win[(int)(a0 + len) - 1];                                  // compress.rs:99
      const u32 stored = bswap32(lds_u32(win, len >= 5 ? a0 + len - 5 : a0));    // block.rs:51
      const u32 n = lds_be16(win, a0);                                           // block.rs:54
      u32 st0 = 0;
      if (len == 0) st0 = TPZ_BLOCK_EMPTY;                                       // compress.rs:96
      else if (tag == 0 || tag > 3) st0 = TPZ_BLOCK_BAD_TAG;                      // :44-53,102
      else if (tag != 1) st0 = TPZ_BLOCK_UNSUPPORTED_CODEC;
      else if (len - 1 < 4) st0 = TPZ_BLOCK_MALFORMED;                            // block.rs:49
      if (st0) {
        if (wid == 0) put_meta(p.out, b, st0, 0, 0);
        return;
      }
      if (2 * n + 1 <= (u32)kBigLdsSlots)
        big_block<ColLds, false>(p, tab, win, ColLds{ltab}, map, gsum, wmax, xs, a0, len, n, stored, b, s, S);
      else
        big_block<ColBig, true>(p, tab, win, ColBig{p.big_scratch + (u64)blockIdx.x * 2 * kBigMaxSlots},
                                map, gsum, wmax, xs, a0, len, n, stored, b, s, S);
    }();
    TPZ_STAMP(S, 5);
    __threadfence();                       // the block's outputs and spill-list entry, then its count
    __syncthreads();
    if (tid == 0) atomicAdd(done, 1u);
    if (!more) break;
    nxt = claim();
  }
#ifdef TPZ_ABL_STAMPS
  const u32 gw = blockIdx.x * kBigWaves + wid;
  if (lane == 0 && gw < (u32)kStampWaves)
    for (int q = 0; q < 6; q++) g_stamps[(kStampWaves + gw) * 8 + q] = S.t[q];
#endif
  (void)lane;
}

// Everything after the wave path, in one launch (an empty worklist costs a counter load, not a
// launch): A, the bigwave list (it may hand blocks with 64+ entries to the big list and blocks
// with bad entries to the spill list); B, the big list (it may hand blocks to the spill list);
// C, the spill list. A phase starts once every block of the one before is done; blocks are
// claimed from ticket counters, so a workgroup only waits on blocks running workgroups hold.
constexpr int kTailLds = (int)sizeof(sp::SpillLds) > kBigLds ? (int)sizeof(sp::SpillLds) : kBigLds;
static_assert(kTailLds + 16 <= 163840, "tail LDS");
static_assert(sp::kThreads == kBigThreads, "tail workgroup shape");

__global__ __launch_bounds__(kBigThreads, 1) void decode_tail_kernel(Params p, sp::SpillParams spp,
                                                                    u32* ctr) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kTailLds];
  __shared__ u32 bcast;
  // whether blocks of a phase are left to claim (a workgroup that finds none skips the phase's
  // table upload)
  auto open = [&](const u32* ticket, u32 n) -> bool {
    __syncthreads();
    if (threadIdx.x == 0) bcast = tail_load(ticket) < n ? 1u : 0u;
    __syncthreads();
    return uni(bcast) != 0;
  };
  // both list lengths in one round trip (the bigwave kernel before this one has appended to them);
  // the spill list is read again only after the big phase, which can append to it
  const u32 nb = uni(tail_load(ctr + kTailBig)), nc0 = uni(tail_load(ctr + kTailSpill));
  bool big_done = true;
  if (nb) {
    if (open(ctr + kTailBigTicket, nb)) big_phase(p, lds, nb, ctr + kTailBigTicket, ctr + kTailBigDone, &bcast);
    big_done = tail_wait(ctr + kTailBigDone, nb, ctr + kTailError, &bcast);
  }
  // (a timed-out wait leaves the spill list to the workgroups whose wait ended, and the error
  // word set: the spill count read here would not be final)
  const u32 nc = !big_done ? 0u : nb ? uni(tail_load(ctr + kTailSpill)) : nc0;
  if (nc && open(ctr + kTailSpillTicket, nc)) sp::spill_phase(spp, lds, nc, ctr + kTailSpillTicket);
  // the last workgroup out zeroes the counters for the next decode on the stream: no memset
  // launch, and a captured graph replays correctly
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(ctr + kTailExit, 1u) == gridDim.x - 1)
    for (int i = 0; i < kTailCounters; i++) __hip_atomic_store(ctr + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x^(8 * 5120 r) mod P (reflected), r < kBigSuper: bit by bit from x^0 (0x80000000).
static const u32* big_super_shifts() {
  static const struct Xp {
    u32 v[kBigSuper];
    Xp() {
      u32 x = 0x80000000u;
      for (int r = 0; r < kBigSuper; r++) {
        v[r] = x;
        for (int i = 0; i < 8 * 5120; i++) x = (x >> 1) ^ ((x & 1u) ? 0xEDB88320u : 0u);
      }
    }
  } xp;
  return xp.v;
}

// x^(8 * 80 l) mod P (reflected), l < 64: lane l's CRC run ends 80 l bytes before the range end.
static const u32* lane_run_shifts() {
  static const struct Ls {
    u32 v[64];
    Ls() {
      u32 x = 0x80000000u;
      for (int l = 0; l < 64; l++) {
        v[l] = x;
        for (int i = 0; i < 8 * kCrcLaneBytes; i++) x = (x >> 1) ^ ((x & 1u) ? 0xEDB88320u : 0u);
      }
    }
  } ls;
  return ls.v;
}

void launch_decode(const LaunchArgs& a, hipStream_t stream) {
  Params p;
  p.src = a.src;
  p.ext = a.ext;
  p.src_bytes = a.src_bytes;
  p.n_blocks = a.n_blocks;
  p.crc_tables = a.crc_tables;
  p.big_scratch = a.big_scratch;
  p.spill_used = a.spill_used;
  p.out = Out{a.data, a.ends, a.count, a.status, a.crc, a.defer_list, a.defer_count,
              a.spill_list, a.spill_count, a.bw_list, a.bw_count, a.efirst,
              a.keys, a.vals, a.kfirst, a.vfirst};
  const u32* xp = big_super_shifts();
  for (int r = 0; r < kBigSuper; r++) p.xp[r] = xp[r];
  const u32* ls = lane_run_shifts();
  for (int l = 0; l < 64; l++) p.lane_shift[l] = ls[l];
  // Blocks claimed at a time by a wave of the wave path. Claims of single blocks balanced the
  // waves of a CU best with static rows (the first waves issue first; same box, 4k: 1.875 ms with
  // 1, 1.89 with 2 or 4, 1.95 with 16, 2.10 with a fixed split; zipf 2.04 against 2.28;
  // profiles/r3/wave_chunks.jsonl); with rows claimed from the global counter 4 slots ahead and
  // the chunk shift a runtime value, pairs were better (4k 1.872-1.877 against 1.881-1.890 ms,
  // zipf 1.986 against 2.010; 4 blocks 1.920 / 2.045: profiles/r5/chunk_ab.jsonl); see below for
  // the shipped choice. A batch of long blocks (the 64k config,
  // where the wave path only routes blocks to the bigwave kernel) takes whole rows: its
  // per-chunk extent and header round trips are not hidden by any decode (64k: 2.07 ms with 16,
  // 2.20 with 4, 2.78 with 1).
  const u64 avg = a.n_blocks ? a.src_bytes / a.n_blocks : 0;
  // Rows claimed 3 slots ahead and the chunk shift a compile-time constant: single blocks per
  // claim beat pairs in the slotted decode (4k 1.821 vs 1.827 ms and 1.824 vs 1.856 on two boxes,
  // zipf equal: profiles/r5/chunk_cs/). The flat decode kept pairs (zipf 2.483 vs 2.506) until its
  // partial-chunk stores got cheaper; since then single blocks are 0.7 % faster there too (4k and
  // zipf, two boxes: profiles/r6/flat_put/ab_cs0_*).
  p.chunk_shift = avg > kWaveMaxLen ? kRowShift : 0u;
  // (the kernel takes it as a template argument, CS)
  p.row_ctr = a.tail + kTailRow;
  p.err = a.tail + kTailError;
  u32 wgs_needed = (a.n_blocks + kRowBlocks - 1) / kRowBlocks;
#if defined(TPZ_ABL_W20) && !defined(TPZ_ABL_GRID1)
  u32 grid = 2 * a.num_cus;
#else
  u32 grid = a.num_cus;
#endif
  if (wgs_needed < grid) grid = wgs_needed ? wgs_needed : 1;
  if (a.keys) {
    if (p.chunk_shift == 0u)
      hipLaunchKernelGGL((decode_wave_kernel<true, 0u>), dim3(grid), dim3(kWGThreads), 0, stream, p);
    else
      hipLaunchKernelGGL((decode_wave_kernel<true, kRowShift>), dim3(grid), dim3(kWGThreads), 0, stream, p);
  } else {
    if (p.chunk_shift == 0u)
      hipLaunchKernelGGL((decode_wave_kernel<false, 0u>), dim3(grid), dim3(kWGThreads), 0, stream, p);
    else
      hipLaunchKernelGGL((decode_wave_kernel<false, kRowShift>), dim3(grid), dim3(kWGThreads), 0, stream, p);
  }
  if (a.bw_list)
    launch_bigwave(BigWaveLaunch{a.src, a.ext, a.src_bytes, a.rep, a.crc_tables, a.bw_list, a.data, a.ends,
                                 a.count, a.status, a.crc, a.spill_list, a.spill_count, a.defer_list,
                                 a.defer_count, a.efirst},
                   a.tail, a.big_grid, stream);
  const sp::SpillParams spp = sp::spill_params(SpillLaunch{a.src, a.ext, a.src_bytes, a.crc_tables,
                                                           a.spill_list, a.spill, a.spill_cap,
                                                           a.spill_off, a.spill_used, a.count,
                                                           a.status, a.crc, a.ends, a.efirst,
                                                           a.keys, a.vals, a.kfirst, a.vfirst});
  hipLaunchKernelGGL(decode_tail_kernel, dim3(a.big_grid), dim3(kBigThreads), 0, stream, p, spp, a.tail);
}

}  // namespace tpz

#ifdef TPZ_ABL_STAMPS
// Diagnostic build only: copies the per-wave phase sums (8 u64 per wave, 6 used) to the host.
extern "C" int tpz_debug_stamps(unsigned long long* host, int n_waves) {
  if (n_waves > 2 * tpz::kStampWaves) n_waves = 2 * tpz::kStampWaves;  // wave, then big kernel
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(tpz::g_stamps), (size_t)n_waves * 8 * 8);
}
#endif

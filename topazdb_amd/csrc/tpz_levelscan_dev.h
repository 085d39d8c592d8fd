// tpz_levelscan_dev.h — the device code of the level scan (tpz_level_scan_ranges; tpz_levelscan.hip)
// beside tpz_scan_dev.h's: the per-call index of the tables (what a scan would otherwise read from
// every table: can it be opened, its biggest key, its head record), the per-level links over it,
// and the seek of one cursor per run, per L0 table and per non-empty level below L0. The merge is
// tpz_scan_dev.h's merge_body with kLvl.
//
// A level below L0 is sorted by smallest key and disjoint (tpz_get_keys' precondition), so the
// reference's per-table cursors over it (level_tables_sorted, src/level.rs:538-579; lsm_storage.rs:
// 350-365), merged, yield the concatenation of the surviving tables T[a..z]. Every T[j], j > a, is
// sought with a key below all of its keys: the outcome (its head) does not depend on the scan.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_internal.h"
#include "tpz_scan_dev.h"
#include "tpz_seek_dev.h"

namespace tpz {
namespace lvldev {

using scandev::Cur;
using scandev::kFail;
using scandev::kInvalid;
using scandev::kNone;
using scandev::kUnopened;
using scandev::kValid;
using scandev::Levels;
using scandev::TabIndex;
using seekdev::u32;
using seekdev::u64;

// The per-call passes' view of the set: L0 = tables [0, l0); non-empty level k below L0 = tables
// [cf[k], cf[k + 1]) (cf[0] = l0: empty levels hold no table, so the non-empty ones are adjacent).
struct Shape {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 l0;
  u32 n_lv;
  u32 cf[TPZ_GET_MAX_LEVELS + 1];
};

// One thread per table: the open check and the biggest key (SsTable::open, table.rs:143-151) and,
// for a table that has a predecessor in its level, the two heads: create_and_seek_to_key with a
// key below every key of the table (the predecessor's biggest key is one) and
// create_and_seek_to_first (an Unbounded lower bound; table/iterator.rs:39-42 stays in block 0).
__device__ __forceinline__ void index_body(const Shape& s, TabIndex* idx) {
  const u32 t = blockIdx.x * 256 + threadIdx.x;
  if (t >= s.n_tables) return;
  const tpz_table& tab = s.tabs[t].table;
  TabIndex x;
  x.big = nullptr;
  u64 bigl = 0;
  u32 fst, fb;
  const bool open = scandev::biggest_key(tab, x.big, bigl, fst, fb);
  x.bigl = (u32)bigl;
  x.os = open ? 0u : (fst | kUnopened);
  x.ob = fb;
  for (u32 k = 0; k < 2; k++) {
    x.hb[k] = x.he[k] = kNone;
    x.hk[k] = kInvalid;
    x.hs[k] = TPZ_BLOCK_OK;
  }
  bool follows = false;                           // a table of its level stands before it
  for (u32 k = 0; k < s.n_lv; k++) follows |= t > s.cf[k] && t < s.cf[k + 1];
  if (open && follows) {
    const uint8_t* pk = nullptr;
    u64 pkl = 0;
    u32 pst, pb;
    if (scandev::biggest_key(s.tabs[t - 1].table, pk, pkl, pst, pb)) {
      const seekdev::SeekPos p = seekdev::seek_table(tab, pk, pkl);
      x.hb[0] = p.block;
      x.he[0] = p.entry;
      x.hs[0] = (uint8_t)p.status;
      x.hk[0] = p.status != TPZ_BLOCK_OK ? kFail : p.valid ? kValid : kInvalid;
    }
    Cur c;
    u32 st = TPZ_BLOCK_OK;
    const u32 r = scandev::first_of_block(tab, c, 0, st);
    x.hb[1] = c.b;
    x.he[1] = c.e;
    x.hs[1] = (uint8_t)st;
    x.hk[1] = (uint8_t)r;
  }
  idx[t] = x;
}

// One wave per non-empty level below L0: for every table of the level and both head kinds, the
// next table at or after it whose head fails (nf) and whose head is valid (nv), kNone past the
// last: chunks of 64 tables from the level's end, a ballot each. The wave after the last level's
// finds the first table that cannot be opened in priority order.
__device__ __forceinline__ void links_body(const Shape& s, const TabIndex* idx, u32* nf, u32* nv,
                                           u32* first_unopened) {
  const u32 lane = copydev::lane_id();
  const u32 k = blockIdx.x;
  if (k >= s.n_lv) {
    u32 found = kNone;
    for (u32 p0 = 0; p0 < s.n_tables && found == kNone; p0 += 64) {
      const u32 p = p0 + lane;
      const u32 t = p < s.n_tables ? scandev::table_of(p, s.l0) : 0u;
      const u64 bad = __ballot(p < s.n_tables && idx[t].os != 0);
      if (bad) found = __shfl(t, __builtin_ctzll(bad), 64);
    }
    if (lane == 0) *first_unopened = found;
    return;
  }
  const u32 lo = s.cf[k], hi = s.cf[k + 1];
  u32 cf0 = kNone, cf1 = kNone, cv0 = kNone, cv1 = kNone;   // the links carried from the chunk above
  for (u32 end = hi; end > lo;) {
    const u32 base = end - lo > 64 ? end - 64 : lo;
    const u32 j = base + lane;
    const bool in = j < end;
    const u32 k0 = in ? idx[j].hk[0] : (u32)kInvalid, k1 = in ? idx[j].hk[1] : (u32)kInvalid;
    const u64 f0 = __ballot(k0 == kFail), f1 = __ballot(k1 == kFail);
    const u64 v0 = __ballot(k0 == kValid), v1 = __ballot(k1 == kValid);
    if (in) {
      const u64 a0 = f0 >> lane, a1 = f1 >> lane, b0 = v0 >> lane, b1 = v1 >> lane;
      nf[j] = a0 ? j + __builtin_ctzll(a0) : cf0;
      nf[s.n_tables + j] = a1 ? j + __builtin_ctzll(a1) : cf1;
      nv[j] = b0 ? j + __builtin_ctzll(b0) : cv0;
      nv[s.n_tables + j] = b1 ? j + __builtin_ctzll(b1) : cv1;
    }
    if (f0) cf0 = base + __builtin_ctzll(f0);
    if (f1) cf1 = base + __builtin_ctzll(f1);
    if (v0) cv0 = base + __builtin_ctzll(v0);
    if (v1) cv1 = base + __builtin_ctzll(v1);
    end = base;
  }
}

// partition_point(smallest_key <= key) over tables [lo, hi), as getdev::level_table bisects it.
__device__ __forceinline__ u32 smallest_pp(const tpz_get_table* tabs, u32 lo, u32 hi,
                                           const uint8_t* qk, u64 ql) {
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const tpz_table& t = tabs[mid].table;
    u64 a = 0, len = 0;
    if (t.n_blocks) {           // (a table without blocks cannot be opened: its key reads empty)
      a = t.d_first_pos[0];
      len = t.d_first_pos[1] - a;
    }
    if (seekdev::key_cmp(t.d_first_keys + a, len, qk, ql) <= 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One cursor of one scan: thread g of n_scans x n_cur, a scan's cursors adjacent in priority
// order: the runs (kMem), the L0 tables newest first, the non-empty levels. It stores (table,
// block, entry, z) and a status; z = the last table the cursor may enter.
template <bool kMem>
__device__ __forceinline__ void seek_body(const scandev::SeekParams& p, const scandev::Runs& m,
                                          const Shape& s, const Levels& L) {
  const u32 n_runs = kMem ? m.n_runs : 0u;
  const u32 n_cur = L.n_cur;
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= (u64)p.n_scans * n_cur) return;
  const u32 i = (u32)(g / n_cur);
  const u32 pc = (u32)(g % n_cur);
  const u32 lk = p.lo_kind[i], hk = p.hi_kind[i];
  u32 t = kNone, b = kNone, e = kNone, z = kNone, cs = TPZ_BLOCK_OK;
  // (a kind out of range, or a table that cannot be opened: the merge reports it)
  if (lk <= TPZ_BOUND_AFTER && hk <= TPZ_BOUND_EXCLUDED && *L.first_unopened == kNone) {
    const u64 la = p.lo_pos[i], ha = p.hi_pos[i];
    const uint8_t* lo = p.lo + la;
    const uint8_t* hi = p.hi + ha;
    const u64 lol = p.lo_pos[i + 1] - la, hil = p.hi_pos[i + 1] - ha;
    const bool lo_ub = lk == TPZ_BOUND_UNBOUNDED, hi_ub = hk == TPZ_BOUND_UNBOUNDED;
    if (kMem && pc < n_runs) {
      scandev::run_range(m.runs[n_runs - 1 - pc], lk, hk, lo, lol, hi, hil, b, e);
    } else if (pc - n_runs < s.l0) {
      t = z = s.l0 - 1 - (pc - n_runs);
      const tpz_table& tab = s.tabs[t].table;
      const TabIndex& x = L.idx[t];
      // level_tables_sorted's filter (level.rs:554-568)
      bool keep = lo_ub || seekdev::key_cmp(x.big, x.bigl, lo, lol) >= 0;
      if (keep && !hi_ub) {
        const u64 sa = tab.d_first_pos[0];
        keep = seekdev::key_cmp(tab.d_first_keys + sa, tab.d_first_pos[1] - sa, hi, hil) <= 0;
      }
      if (keep) {
        Cur c;
        u32 fst;
        const u32 r = scandev::seek_lower(tab, lk, lo, lol, c, fst);
        if (r != kInvalid) {
          b = c.b;
          e = c.e;
        }
        if (r == kFail) cs = fst;
      }
    } else {
      const u32 k = pc - n_runs - s.l0;
      const u32 first = s.cf[k], end = s.cf[k + 1];       // first < end <= n_tables
      // T[a..zz] survive the filter: a = the first table whose biggest key >= lower, zz = the
      // last whose smallest key <= upper
      u32 a = first, zz = end - 1;
      bool any = true;
      if (!lo_ub) {
        const u32 pp = smallest_pp(s.tabs, first, end, lo, lol);
        a = pp > first ? pp - 1 : first;
        if (seekdev::key_cmp(L.idx[a].big, L.idx[a].bigl, lo, lol) < 0) a++;
      }
      if (!hi_ub) {
        const u32 pp = smallest_pp(s.tabs, first, end, hi, hil);
        any = pp > first;
        zz = any ? pp - 1 : first;
      }
      if (any && a <= zz && a < end) {
        const u32 kd = lo_ub ? 1u : 0u;                   // which head the later tables take
        const u32* nf = L.nf + (u64)kd * s.n_tables;
        const u32* nv = L.nv + (u64)kd * s.n_tables;
        t = a;
        z = zz;
        Cur c;
        u32 fst;
        const u32 r = scandev::seek_lower(s.tabs[a].table, lk, lo, lol, c, fst);
        const u32 f = a < zz ? nf[a + 1] : kNone;         // the first failing head of (a, zz]
        if (r == kFail) {
          b = c.b;
          e = c.e;
          cs = fst;
        } else if (f <= zz) {                             // (kNone > zz)
          const TabIndex& x = L.idx[f];
          t = f;
          b = x.hb[kd];
          e = x.he[kd];
          cs = x.hs[kd];
        } else if (r == kValid) {
          b = c.b;
          e = c.e;
        } else {                                          // Excluded at T[a]'s biggest key
          const u32 v = a < zz ? nv[a + 1] : kNone;
          if (v <= zz) {
            t = v;
            b = L.idx[v].hb[kd];
            e = L.idx[v].he[kd];
          }
        }
      }
    }
  }
  uint4 out;
  out.x = t;
  out.y = b;
  out.z = e;
  out.w = z;
  reinterpret_cast<uint4*>(p.cur)[g] = out;
  p.cst[g] = (uint8_t)cs;
}

}  // namespace lvldev
}  // namespace tpz

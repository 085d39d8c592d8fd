// tpz_scan_dev.h — the bodies of the scan's kernels, shared by tpz_scan.hip's two sets of them
// (tpz_scan_ranges, tpz_scan_entries: the SST half of LsmStorage::scan; tpz_lsm_scan_ranges,
// tpz_lsm_scan_entries: the whole scan, memtable runs merged in). kMem = false is the SST half as
// it always was; kMem = true puts one cursor per run in front of the tables' (a wave's lanes
// 0 .. n_runs - 1, the newest run first) and adds TwoMergeIterator's eager step to the merge.
// kLvl (tpz_levelscan.hip: tpz_level_scan_ranges) gives a lane to every non-empty level below L0
// instead of to every table of it: a level lane's cursor walks the level's surviving tables.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpz_copy.h"
#include "tpz_internal.h"
#include "tpz_mem_dev.h"
#include "tpz_seek_dev.h"

namespace tpz {
namespace scandev {

using memdev::cmp_tied;
using memdev::key_prefix;
using seekdev::u32;
using seekdev::u64;

constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u64 kLaneCopyMax = 256;   // the get gather's threshold (tpz_get_dev.h)
constexpr u32 kUnopened = 0x80u;    // cursor status flag: the table could not have been opened
constexpr u32 kWaves = 4;           // scans per workgroup of the wave-per-scan kernels

// The memtable side of a launch (kMem): the runs, in MemTables::view() order.
struct Runs {
  const tpz_mem_run* runs;
  u32 n_runs;
};

// Cursor `p` of a scan in priority order -> index into d_tables (level.rs:570-577: L0 reversed,
// then every level as stored). l0 = the number of L0 tables.
__device__ __forceinline__ u32 table_of(u32 p, u32 l0) { return p < l0 ? l0 - 1 - p : p; }

// An SsTableIterator's position and what the merge reads there. A run's cursor (kMem) uses e (the
// entry's index in the run) and n (the end of map.range((lower, upper)), exclusive).
struct Cur {
  u32 b, e, n;             // block, entry, the block's entry count
  seekdev::BlockView v;    // block b
  const uint8_t* key;
  u64 klen, vlen;
};
enum : u32 { kValid = 0, kInvalid = 1, kFail = 2 };   // kFail: (c.b, c.e) and `fst` say where / what

// BlockIterator::seek_to(c.e) in the open block (block/iterator.rs:74-82) and is_valid().
__device__ __forceinline__ u32 land(Cur& c, u32& fst) {
  if (c.e >= c.n) return kInvalid;
  if (c.v.seek_panics(c.e)) {
    fst = TPZ_BLOCK_MALFORMED;
    return kFail;
  }
  c.key = seekdev::entry_key(c.v, c.e, c.klen);
  if (c.klen == 0) return kInvalid;
  seekdev::entry_value(c.v, c.n, c.e, c.vlen);
  return kValid;
}
__device__ __forceinline__ void open_block(const tpz_table& t, Cur& c, u32 b, u32 st) {
  c.b = b;
  c.n = t.d_count[b];
  c.v = seekdev::block_view(t, b, st);
}
// SsTableIterator::seek_to_first_inner(table, b) (table/iterator.rs:39-42).
__device__ __forceinline__ u32 first_of_block(const tpz_table& t, Cur& c, u32 b, u32& fst) {
  c.b = b;
  c.e = 0;
  const u32 st = t.d_status[b];
  if (!block_decoded(st)) {
    fst = st;
    return kFail;
  }
  open_block(t, c, b, st);
  return land(c, fst);
}
// SsTableIterator::next (table/iterator.rs:88-95) of a valid cursor.
__device__ __forceinline__ u32 advance(const tpz_table& t, Cur& c, u32& fst) {
  c.e++;
  u32 r = land(c, fst);
  if (r == kInvalid && c.b + 1 < t.n_blocks) r = first_of_block(t, c, c.b + 1, fst);
  return r;
}

// MemTableIterator at entry c.e of the run's range [.., c.n) (src/mem_table.rs:248-270): the item
// past the range's end is the empty pair, and is_valid() is "the key is non-empty".
__device__ __forceinline__ u32 run_land(const tpz_entries& e, Cur& c) {
  if (c.e >= c.n) return kInvalid;
  c.key = memdev::run_key(e, c.e, c.klen);
  if (c.klen == 0) return kInvalid;
  memdev::run_value(e, c.e, c.vlen);
  return kValid;
}
// The level scan's per-call index of a table (tpz_levelscan_dev.h index_body): whether the
// reference could have opened it (os: 0, or the status | kUnopened; ob: the block), its biggest
// key, and its head: where a cursor created below all of its keys stands ([0]: by
// create_and_seek_to_key, [1]: by create_and_seek_to_first), or how creating it fails.
struct TabIndex {
  const uint8_t* big;
  u32 bigl;
  u32 ob;
  u32 hb[2], he[2];      // block and entry
  uint8_t hk[2];         // kValid / kInvalid / kFail
  uint8_t hs[2];         // the status of a failing head
  uint8_t os;
};
// What the level scan's seek and merge read beside the tables (kLvl).
struct Levels {
  const tpz_get_table* tabs;
  u32 n_tables;
  const TabIndex* idx;
  const u32* nf;             // 2 x n_tables: the next table at or after t whose head fails
  const u32* nv;             // 2 x n_tables: ... whose head is valid (kNone: none in the level)
  const u32* first_unopened; // one u32: the first table that cannot be opened, in priority order
  u32 n_cur;                 // cursors per scan: runs + L0 tables + non-empty levels below L0
};

// A table cursor's next. kLvl: a level's cursor at the end of table t enters the next table of
// (t, z] whose head is valid, at that head (the reference created that table's cursor there when
// the scan began; the tables between have invalid heads, and MergeIterator::create dropped them).
// Only the end of a table pays for it: the step within a table is advance alone.
template <bool kLvl>
__device__ __forceinline__ u32 table_step(const tpz_table*& tab, u32& t, u32 z, u32 kd, Cur& c,
                                          u32& fst, const Levels& L) {
  u32 r = advance(*tab, c, fst);
  if (kLvl && r == kInvalid && t < z) {
    const u32 v = L.nv[(u64)kd * L.n_tables + t + 1];
    if (v <= z && v < L.n_tables) {
      const TabIndex& x = L.idx[v];
      t = v;
      tab = &L.tabs[v].table;
      c.b = x.hb[kd];
      c.e = x.he[kd];
      if (c.b < tab->n_blocks) {
        const u32 bst = tab->d_status[c.b];
        if (block_decoded(bst)) {
          open_block(*tab, c, c.b, bst);
          r = land(c, fst);
        }
      }
    }
  }
  return r;
}
// A cursor's next: the table's, or the run's (which cannot fail).
template <bool kMem, bool kLvl>
__device__ __forceinline__ u32 step(const tpz_table*& tab, const tpz_mem_run* run, u32& t, u32 z,
                                    u32 kd, Cur& c, u32& fst, const Levels& L) {
  if (kMem && run) {
    c.e++;
    return run_land(run->entries, c);
  }
  return table_step<kLvl>(tab, t, z, kd, c, fst, L);
}

// SsTable::open's init_samllest_biggest_key (table.rs:143-151): the last entry's key of the last
// block. False where the reference fails there: `fst` and `fb` (the block, or kNone) say how.
__device__ __forceinline__ bool biggest_key(const tpz_table& t, const uint8_t*& k, u64& kl,
                                            u32& fst, u32& fb) {
  fst = TPZ_BLOCK_MALFORMED;
  fb = kNone;
  if (t.n_blocks == 0) return false;             // block_metas[0]
  const u32 b = t.n_blocks - 1;
  fb = b;
  const u32 st = t.d_status[b];
  if (!block_decoded(st)) {                      // read_block(..)?
    fst = st;
    return false;
  }
  const u32 n = t.d_count[b];
  if (n == 0) return false;                      // seek_to_last: offsets.len() - 1
  const seekdev::BlockView v = seekdev::block_view(t, b, st);
  if (v.seek_panics(0) || v.seek_panics(n - 1)) return false;   // seek_to_first, seek_to_last
  k = seekdev::entry_key(v, n - 1, kl);
  return kl > 0;                                 // assert!(iter.is_valid())
}

// map.range((lower, upper)) (src/mem_table.rs:199-219) as entries [lb, ub): the cursor is
// (lb, ub), or (kNone, kNone) where it starts invalid (an empty range, or the empty key first:
// MergeIterator::create drops it).
__device__ __forceinline__ void run_range(const tpz_mem_run& run, u32 lk, u32 hk, const uint8_t* lo,
                                          u64 lol, const uint8_t* hi, u64 hil, u32& b, u32& e) {
  const u32 n = run.entries.n_entries;
  const u32 lb = lk == TPZ_BOUND_UNBOUNDED
                     ? 0u : memdev::run_bound(run, lo, lol, key_prefix(lo, lol),
                                              lk != TPZ_BOUND_INCLUDED);
  const u32 ub = hk == TPZ_BOUND_UNBOUNDED
                     ? n : memdev::run_bound(run, hi, hil, key_prefix(hi, hil),
                                             hk == TPZ_BOUND_INCLUDED);
  if (lb < ub && lb < n) {
    u64 kl;
    memdev::run_key(run.entries, lb, kl);
    if (kl) {
      b = lb;
      e = ub < n ? ub : n;
    }
  }
}

// The cursor of a surviving table (lsm_storage.rs:350-365): create_and_seek_to_first for an
// Unbounded lower bound, else create_and_seek_to_key and the Excluded / After step. (c.b, c.e) is
// where it stands, or with kFail where the reference fails and `fst` how.
__device__ __forceinline__ u32 seek_lower(const tpz_table& tab, u32 lk, const uint8_t* lo, u64 lol,
                                          Cur& c, u32& fst) {
  if (lk == TPZ_BOUND_UNBOUNDED) return first_of_block(tab, c, 0, fst);   // create_and_seek_to_first
  const seekdev::SeekPos s = seekdev::seek_table(tab, lo, lol);           // create_and_seek_to_key
  c.b = s.block;
  c.e = s.entry;
  fst = s.status;
  u32 r = s.status != TPZ_BLOCK_OK ? kFail : s.valid ? kValid : kInvalid;
  if (r == kValid && lk != TPZ_BOUND_INCLUDED) {   // lsm_storage.rs:356-362
    open_block(tab, c, c.b, tab.d_status[c.b]);
    c.key = seekdev::entry_key(c.v, c.e, c.klen);
    if (c.klen == lol && seekdev::key_cmp(c.key, c.klen, lo, lol) == 0) r = advance(tab, c, fst);
  }
  return r;
}

struct SeekParams {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 l0;
  const uint8_t* lo;
  const u64* lo_pos;
  const uint8_t* lo_kind;
  const uint8_t* hi;
  const u64* hi_pos;
  const uint8_t* hi_kind;
  u32 n_scans;
  u32* cur;          // 2 x n_scans x cursors (kMem: the runs' cursors, then the tables')
  uint8_t* cst;      // n_scans x cursors
};

// One cursor of one scan: thread g of n_scans x (n_runs + n_tables), a scan's cursors adjacent in
// priority order.
template <bool kMem>
__device__ __forceinline__ void seek_body(const SeekParams& p, const Runs& m) {
  const u32 n_cur = p.n_tables + (kMem ? m.n_runs : 0u);
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= (u64)p.n_scans * n_cur) return;
  const u32 i = (u32)(g / n_cur);
  const u32 pc = (u32)(g % n_cur);
  const u32 lk = p.lo_kind[i], hk = p.hi_kind[i];
  u32 b = kNone, e = kNone, cs = TPZ_BLOCK_OK;
  if (lk <= TPZ_BOUND_AFTER && hk <= TPZ_BOUND_EXCLUDED) {   // (else the merge reports the kind)
    const u64 la = p.lo_pos[i], ha = p.hi_pos[i];
    const uint8_t* lo = p.lo + la;
    const uint8_t* hi = p.hi + ha;
    const u64 lol = p.lo_pos[i + 1] - la, hil = p.hi_pos[i + 1] - ha;
    if (kMem && pc < m.n_runs) {
      run_range(m.runs[m.n_runs - 1 - pc], lk, hk, lo, lol, hi, hil, b, e);   // view().rev()
    } else {
      const u32 t = table_of(kMem ? pc - m.n_runs : pc, p.l0);
      const tpz_table& tab = p.tabs[t].table;
      const uint8_t* big = nullptr;
      u64 bigl = 0;
      u32 fst, fb;
      if (!biggest_key(tab, big, bigl, fst, fb)) {
        cs = fst | kUnopened;
        b = fb;
      } else {
        // level_tables_sorted's filter (level.rs:554-568)
        bool keep = lk == TPZ_BOUND_UNBOUNDED || seekdev::key_cmp(big, bigl, lo, lol) >= 0;
        if (keep && hk != TPZ_BOUND_UNBOUNDED) {
          const u64 sa = tab.d_first_pos[0];
          keep = seekdev::key_cmp(tab.d_first_keys + sa, tab.d_first_pos[1] - sa, hi, hil) <= 0;
        }
        if (keep) {
          Cur c;
          const u32 r = seek_lower(tab, lk, lo, lol, c, fst);
          if (r != kInvalid) {
            b = c.b;
            e = c.e;
          }
          if (r == kFail) cs = fst;
        }
      }
    }
  }
  p.cur[2 * g] = b;
  p.cur[2 * g + 1] = e;
  p.cst[g] = (uint8_t)cs;
}

__device__ __forceinline__ const uint8_t* shfl_ptr(const uint8_t* p, int l) {
  return reinterpret_cast<const uint8_t*>((uintptr_t)__shfl((u64)(uintptr_t)p, l, 64));
}

struct MergeParams {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 l0;
  const uint8_t* hi;
  const u64* hi_pos;
  const uint8_t* lo_kind;
  const uint8_t* hi_kind;
  u32 n_scans;
  u32 limit;
  const u32* cur;
  const uint8_t* cst;
  uint8_t* result;
  uint8_t* status;
  u32* where;
  u32* hit_table;
  u32* hit_block;
  u32* hit_entry;
  u64* first;
  u64* key_first;
  u64* val_first;
};

// One wave per scan, one cursor per lane in priority order. kLvl: the seek stored (table, block,
// entry, z) per cursor, and a lane's table changes as a level's cursor walks on.
template <bool kMem, bool kLvl = false>
__device__ __forceinline__ void merge_body(const MergeParams& p, const Runs& m,
                                           const Levels& L = Levels{}) {
  const u32 lane = copydev::lane_id();
  const u32 i = blockIdx.x * kWaves + threadIdx.x / 64;
  if (i >= p.n_scans) return;                    // (the whole wave)
  const u32 n_runs = kMem ? m.n_runs : 0u;
  const u32 n_cur = kLvl ? L.n_cur : p.n_tables + n_runs;
  const u32 lk = p.lo_kind[i], hk = p.hi_kind[i];
  const u32 fu = kLvl ? *L.first_unopened : kNone;
  u32 res = TPZ_SCAN_DONE, st = TPZ_BLOCK_OK, w0 = kNone, w1 = kNone, w2 = kNone, count = 0;
  u64 kb = 0, vb = 0;
  if (lk > TPZ_BOUND_AFTER || hk > TPZ_BOUND_EXCLUDED) {
    res = TPZ_SCAN_ERROR;
    st = TPZ_BLOCK_MALFORMED;
  } else if (kLvl && fu != kNone) {              // found before any seek (tpz_levelscan_dev.h)
    res = TPZ_SCAN_ERROR;
    st = L.idx[fu].os & ~kUnopened;
    w0 = fu;
    w1 = L.idx[fu].ob;
  } else {
    Cur c;
    c.b = c.e = kNone;
    c.n = 0;
    c.key = nullptr;
    c.klen = c.vlen = 0;
    u32 cs = TPZ_BLOCK_OK, t = 0, z = 0;
    const u32 kd = lk == TPZ_BOUND_UNBOUNDED ? 1u : 0u;   // (kLvl: the head a level's tables take)
    const tpz_table* tab = nullptr;
    const tpz_mem_run* run = nullptr;
    if (lane < n_cur) {
      const u64 g = (u64)i * n_cur + lane;
      if (kLvl) {
        const uint4 q = reinterpret_cast<const uint4*>(p.cur)[g];
        t = q.x;
        c.b = q.y;
        c.e = q.z;
        z = q.w;
      } else {
        c.b = p.cur[2 * g];
        c.e = p.cur[2 * g + 1];
      }
      cs = p.cst[g];
      if (kMem && lane < n_runs) {
        t = TPZ_HIT_MEM | (n_runs - 1 - lane);
        run = &m.runs[n_runs - 1 - lane];
      } else if (kLvl) {
        if (t < p.n_tables) tab = &p.tabs[t].table;         // (kNone: the cursor has no table)
      } else {
        t = table_of(lane - n_runs, p.l0);
        tab = &p.tabs[t].table;
      }
    }
    // Failures while the cursors are created: a table that could not have been opened is found
    // by the filter, before any seek; either way the first one in priority order is reported.
    const u64 unopened = __ballot((cs & kUnopened) != 0), failed = __ballot(cs != TPZ_BLOCK_OK);
    if (failed) {
      const int f = __builtin_ctzll(unopened ? unopened : failed);
      res = TPZ_SCAN_ERROR;
      st = __shfl(cs & ~kUnopened, f, 64);
      w0 = __shfl(t, f, 64);
      w1 = __shfl(c.b, f, 64);
      w2 = __shfl(c.e, f, 64);
    } else {
      // MergeIterator::create keeps the valid cursors (merge_iterator.rs:47-57)
      bool live = false;
      if (kMem && run) {                           // the seek stored (lb, ub)
        const u32 lb = c.b, ub = c.e, n = run->entries.n_entries;
        c.b = 0;
        c.e = lb;
        c.n = ub < n ? ub : n;
        live = lb != kNone && run_land(run->entries, c) == kValid;
      } else if (tab && c.b < tab->n_blocks) {
        const u32 bst = tab->d_status[c.b];
        if (block_decoded(bst)) {
          open_block(*tab, c, c.b, bst);
          u32 fst;
          live = land(c, fst) == kValid;
        }
      }
      u64 pfx = live ? key_prefix(c.key, c.klen) : 0;
      const u64 ha = p.hi_pos[i];
      const uint8_t* hi = p.hi + ha;
      const u64 hil = p.hi_pos[i + 1] - ha;
      const u64 sst_lanes = kMem ? ~0ull << n_runs : ~0ull;   // (n_runs <= 16)
      bool e0 = lk != TPZ_BOUND_AFTER;           // element 0 is not end-checked
      while (__ballot(live)) {
        // the minimum (key, lane)
        u64 mn = live ? pfx : ~0ull;
        for (int o = 32; o; o >>= 1) {
          const u64 x = __shfl_xor(mn, o, 64);
          mn = x < mn ? x : mn;
        }
        u64 tied = __ballot(live && pfx == mn);
        u64 eq = tied;
        int ld = __builtin_ctzll(tied);
        const uint8_t* lkey = shfl_ptr(c.key, ld);
        u64 lklen = __shfl(c.klen, ld, 64);
        if (tied & (tied - 1)) {
          for (;;) {       // the candidate is the first lane of `tied`; lanes below it lost
            int cmp = 1;
            if ((tied >> lane) & 1) cmp = cmp_tied(c.key, c.klen, lkey, lklen);
            const u64 less = __ballot(cmp < 0);
            if (!less) {
              eq = __ballot(cmp == 0);
              break;
            }
            tied = less;
            ld = __builtin_ctzll(tied);
            lkey = shfl_ptr(c.key, ld);
            lklen = __shfl(c.klen, ld, 64);
          }
        }
        u32 r = kValid, fst = TPZ_BLOCK_OK;
        if (kMem && (u32)ld < n_runs && (eq & sst_lanes)) {
          // TwoMergeIterator (two_merge_iterator.rs:20-24, :64-68): the memtable side stands at
          // this key, so the SST side moves past it before the key is looked at: its
          // MergeIterator::next, the other cursors at the key first, its current one (the first
          // SST lane at the key) last. A failure there ends the scan before the key is yielded.
          const u64 skip = eq & sst_lanes;
          if ((skip >> lane) & 1) {
            do {
              r = table_step<kLvl>(tab, t, z, kd, c, fst, L);
            } while (r == kValid && c.klen == lklen &&
                     seekdev::key_cmp(c.key, c.klen, lkey, lklen) == 0);
            live = r == kValid;
            if (live) pfx = key_prefix(c.key, c.klen);
          }
          const u64 fails = __ballot(r == kFail);
          if (fails) {
            const u64 others = fails & ~(1ull << __builtin_ctzll(skip));
            const int f = __builtin_ctzll(others ? others : fails);
            res = TPZ_SCAN_ERROR;
            st = __shfl(fst, f, 64);
            w0 = __shfl(t, f, 64);
            w1 = __shfl(c.b, f, 64);
            w2 = __shfl(c.e, f, 64);
            break;
          }
          eq &= ~sst_lanes;
        }
        const u64 lvlen = __shfl(c.vlen, ld, 64);
        // LsmIterator::next_inner's end check (lsm_iterator.rs:46-50), tombstones included
        if (!e0 && hk != TPZ_BOUND_UNBOUNDED) {
          const int cc = seekdev::key_cmp(lkey, lklen, hi, hil);
          if (hk == TPZ_BOUND_INCLUDED ? cc > 0 : cc >= 0) break;
        }
        e0 = false;
        if (lvlen) {                              // (an empty value is skipped)
          if (count == p.limit) {
            res = TPZ_SCAN_MORE;
            break;
          }
          if (lane == (u32)ld) {
            const u64 h = (u64)i * p.limit + count;
            p.hit_table[h] = t;
            p.hit_block[h] = c.b;
            p.hit_entry[h] = c.e;
          }
          count++;
          kb += lklen;
          vb += lvlen;
        }
        // MergeIterator::next: the other cursors at this key first, the current one last
        r = kValid;
        if ((eq >> lane) & 1) {
          if (lane == (u32)ld) {
            r = step<kMem, kLvl>(tab, run, t, z, kd, c, fst, L);
          } else {
            do {
              r = step<kMem, kLvl>(tab, run, t, z, kd, c, fst, L);
            } while (r == kValid && c.klen == lklen &&
                     seekdev::key_cmp(c.key, c.klen, lkey, lklen) == 0);
          }
          live = r == kValid;
          if (live) pfx = key_prefix(c.key, c.klen);
        }
        const u64 fails = __ballot(r == kFail);
        if (fails) {
          const u64 others = fails & ~(1ull << ld);
          const int f = __builtin_ctzll(others ? others : fails);
          res = TPZ_SCAN_ERROR;
          st = __shfl(fst, f, 64);
          w0 = __shfl(t, f, 64);
          w1 = __shfl(c.b, f, 64);
          w2 = __shfl(c.e, f, 64);
          break;
        }
      }
    }
  }
  if (lane == 0) {
    p.result[i] = (uint8_t)res;
    p.status[i] = (uint8_t)st;
    p.where[3 * (u64)i] = w0;
    p.where[3 * (u64)i + 1] = w1;
    p.where[3 * (u64)i + 2] = w2;
    p.first[i] = count;
    p.key_first[i] = kb;
    p.val_first[i] = vb;
  }
}

struct EntriesParams {
  const tpz_get_table* tabs;
  u32 n_tables;
  u32 n_scans;
  u32 limit;
  const u32* hit_table;
  const u32* hit_block;
  const u32* hit_entry;
  const u64* first;
  u64* kbase;        // n_scans + 1: the scans' key bytes, scanned in place between the passes
  u64* vbase;
  uint8_t* keys;
  u64 key_cap;
  u64* kpos;
  uint8_t* vals;
  u64 val_cap;
  u64* vpos;
};

__device__ __forceinline__ void wave_copies(uint8_t* dst, u64 cap, u64 d, const uint8_t* src,
                                            u64 len, u32 lane) {
  if (len && len <= kLaneCopyMax) copydev::lane_copy(dst, cap, d, src, len);
  u64 mask = __ballot(len > kLaneCopyMax);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    copydev::wave_copy(dst, cap, __shfl(d, l, 64), shfl_ptr(src, l), __shfl(len, l, 64), lane);
  }
}

template <bool kCopy, bool kMem>
__device__ __forceinline__ void entries_body(const EntriesParams& p, const Runs& m) {
  const u32 lane = copydev::lane_id();
  const u32 i = blockIdx.x * kWaves + threadIdx.x / 64;
  if (i >= p.n_scans) return;
  const u64 f0 = p.first[i], f1 = p.first[i + 1], total = p.first[p.n_scans];
  u64 cnt = f1 > f0 ? f1 - f0 : 0;
  if (cnt > p.limit) cnt = p.limit;
  if (f0 >= total) cnt = 0;
  else if (cnt > total - f0) cnt = total - f0;
  u64 kb = kCopy ? p.kbase[i] : 0, vb = kCopy ? p.vbase[i] : 0;
  for (u64 c0 = 0; c0 < cnt; c0 += 64) {
    const u64 j = c0 + lane;
    const uint8_t* ksrc = nullptr;
    const uint8_t* vsrc = nullptr;
    u64 kl = 0, vl = 0;
    if (j < cnt) {
      const u64 h = (u64)i * p.limit + j;
      const u32 t = p.hit_table[h], b = p.hit_block[h], e = p.hit_entry[h];
      if (kMem && t != kNone && (t & TPZ_HIT_MEM)) {
        const u32 r = t & ~TPZ_HIT_MEM;
        if (r < m.n_runs && e < m.runs[r].entries.n_entries) {
          ksrc = memdev::run_key(m.runs[r].entries, e, kl);
          vsrc = memdev::run_value(m.runs[r].entries, e, vl);
        }
      } else if (t < p.n_tables) {
        const tpz_table& tab = p.tabs[t].table;
        if (b < tab.n_blocks) {
          const u32 st = tab.d_status[b];
          const u32 n = tab.d_count[b];
          if (block_decoded(st) && e < n) {
            const seekdev::BlockView v = seekdev::block_view(tab, b, st);
            ksrc = seekdev::entry_key(v, e, kl);
            vsrc = seekdev::entry_value(v, n, e, vl);
          }
        }
      }
    }
    u64 ks = kl, vs = vl;                          // inclusive sums over the wave
    for (u32 o = 1; o < 64; o <<= 1) {
      const u64 a = __shfl_up(ks, o, 64), c = __shfl_up(vs, o, 64);
      if (lane >= o) {
        ks += a;
        vs += c;
      }
    }
    if (kCopy) {
      const u64 kd = kb + ks - kl, vd = vb + vs - vl;
      if (j < cnt) {
        p.kpos[f0 + j] = kd;
        p.vpos[f0 + j] = vd;
      }
      wave_copies(p.keys, p.key_cap, kd, ksrc, kl, lane);
      wave_copies(p.vals, p.val_cap, vd, vsrc, vl, lane);
    }
    kb += __shfl(ks, 63, 64);
    vb += __shfl(vs, 63, 64);
  }
  if (lane == 0) {
    if (!kCopy) {
      p.kbase[i] = kb;
      p.vbase[i] = vb;
    } else if (i == p.n_scans - 1) {
      p.kpos[total] = kb;
      p.vpos[total] = vb;
    }
  }
}

// Host side, for the launchers of tpz_scan.hip and tpz_levelscan.hip: the cursors' part of a
// ranges call's workspace (`words` u32 per scan and cursor: 2, or kLvl's 4; then a status byte
// each, padded to 8; then the scans' partial sums) and the kernels' parameters from a ScanLaunch.
struct CursorWork {
  u32* cur;
  uint8_t* cst;
  u64* part;
};
inline uint64_t cursor_work_bytes(uint32_t n_scans, uint64_t cells, u32 words) {
  return 4 * words * cells + ((cells + 7) & ~7ull) + 8 * (flat_scan_parts_words(n_scans) / 3);
}
inline CursorWork carve_cursors(void* work, uint64_t cells, u32 words) {
  u32* cur = static_cast<u32*>(work);
  uint8_t* cst = reinterpret_cast<uint8_t*>(cur + words * cells);
  return {cur, cst, reinterpret_cast<u64*>(cst + ((cells + 7) & ~7ull))};
}
inline SeekParams seek_params(const ScanLaunch& a, const CursorWork& w) {
  return {a.tabs, a.n_tables, a.l0(), a.lo, a.lo_pos, a.lo_kind, a.hi, a.hi_pos, a.hi_kind,
          a.n_scans, w.cur, w.cst};
}
inline MergeParams merge_params(const ScanLaunch& a, const CursorWork& w) {
  return {a.tabs, a.n_tables, a.l0(), a.hi, a.hi_pos, a.lo_kind, a.hi_kind, a.n_scans, a.limit,
          w.cur, w.cst, a.result, a.status, a.where, a.hit_table, a.hit_block, a.hit_entry,
          a.first, a.key_first, a.val_first};
}

}  // namespace scandev
}  // namespace tpz

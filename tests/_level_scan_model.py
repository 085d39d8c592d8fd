"""The level scan (tpz_level_scan_ranges; include/tpz_gpu.h) restated over the facade's host tables
(test infrastructure, CPU only): one cursor per run, per L0 table and per non-empty level below L0.

`Index` is what the device computes once per call: per table whether the reference could have
opened it, and its two head records (where create_and_seek_to_key with a key below all of its keys
and create_and_seek_to_first leave a cursor, or how they fail); per level the links (the next
failing and the next valid head at or after each table); the first unopenable table in priority
order. `level_scan` builds the cursors from it (a level's: the survivors T[a..z] by bisection on the
smallest keys plus one look at a biggest key, T[a]'s real seek, the creation-error order, the start
at the next valid head) and merges them with tests/_scan_model.py's MergeIterator, LsmIterator and
FusedIterator under tests/_lsm_model.py's TwoMergeIterator. tests/test_level_scan_model.py compares
it with `lsm_scan` / `lsm_scan_mem` (one cursor per table, the reference line by line) over honest
sets whose lower levels are sorted and disjoint: that comparison is the equivalence claim.
"""
from __future__ import annotations

from collections import namedtuple

import _get_model as G
import _lsm_model as M
import _scan_model as S
from _scan_model import DONE, ERROR, MORE, Scan, ScanFailure
from topazdb_amd import _lib
from topazdb_amd.table import BlockError, BlockIterator, ReferencePanic, SsTableIterator

VALID, INVALID, FAIL = range(3)
NONE = G.NONE
KEYED, FIRST = 0, 1          # which head: a keyed lower bound, an Unbounded one

# kind VALID: the cursor stands at (block, entry); FAIL: creating it fails there with `status`
Head = namedtuple("Head", "kind block entry status")
NO_HEAD = Head(INVALID, NONE, NONE, _lib.BLOCK_OK)


def head_first(table) -> Head:
    """create_and_seek_to_first (table/iterator.rs:39-42): block 0, entry 0, no bisection."""
    try:
        it = SsTableIterator.create_and_seek_to_first(table)
    except (BlockError, ReferencePanic) as e:
        return Head(FAIL, 0, 0, G._err_status(e))
    return Head(VALID if it.is_valid() else INVALID, it.idx, it.block_iter.idx, _lib.BLOCK_OK)


def head_keyed(table, below: bytes) -> Head:
    """create_and_seek_to_key with a key below every key of the table (table/iterator.rs:44-72)."""
    try:
        it = SsTableIterator.create_and_seek_to_key(table, below)
    except (BlockError, ReferencePanic):
        b, e, st = G.seek_failure(table, below)
        return Head(FAIL, b, e, st)
    return Head(VALID if it.is_valid() else INVALID, it.idx, it.block_iter.idx, _lib.BLOCK_OK)


class Index:
    """The per-call index and links over `levels` (host tables; levels[0] is L0 in push order)."""

    def __init__(self, levels):
        self.levels = levels
        self.tables = [t for lv in levels for t in lv]
        n = len(self.tables)
        self.first = [0]
        for lv in levels:
            self.first.append(self.first[-1] + len(lv))
        self.open_failure = [S.open_failure(t) for t in self.tables]   # (sets the two keys)
        self.head = [[NO_HEAD, NO_HEAD] for _ in range(n)]
        self.nf = [[NONE] * n, [NONE] * n]
        self.nv = [[NONE] * n, [NONE] * n]
        for lv in range(1, len(levels)):
            lo, hi = self.first[lv], self.first[lv + 1]
            for t in range(lo + 1, hi):              # a table with a predecessor in its level
                if self.open_failure[t] is None:
                    if self.open_failure[t - 1] is None:
                        self.head[t][KEYED] = head_keyed(self.tables[t], self.tables[t - 1].biggest_key)
                    self.head[t][FIRST] = head_first(self.tables[t])
            for kd in (KEYED, FIRST):                # the links: one pass from the level's end
                f = v = NONE
                for t in reversed(range(lo, hi)):
                    f = t if self.head[t][kd].kind == FAIL else f
                    v = t if self.head[t][kd].kind == VALID else v
                    self.nf[kd][t], self.nv[kd][t] = f, v
        l0 = self.first[1] if levels else 0
        order = list(reversed(range(l0))) + list(range(l0, n))
        self.first_unopened = next((t for t in order if self.open_failure[t] is not None), NONE)


def _partition_point(tables, key: bytes) -> int:
    """partition_point(smallest_key <= key) (level.rs:449-451), by bisection."""
    lo, hi = 0, len(tables)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if tables[mid].smallest_key <= key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def survivors(tables, lower, upper):
    """(a, z) of a sorted, disjoint level: level_tables_sorted's filter keeps T[a..z]; None when
    it keeps nothing."""
    a, z = 0, len(tables) - 1
    if lower is not None:
        a = max(_partition_point(tables, lower[1]) - 1, 0)
        if tables[a].biggest_key < lower[1]:
            a += 1
    if upper is not None:
        z = _partition_point(tables, upper[1]) - 1
    return (a, z) if 0 <= a <= z < len(tables) else None


def _seek(t: int, table, lower, stats) -> S.Cursor:
    """The reference's cursor of a surviving table (lsm_storage.rs:350-365)."""
    try:
        if lower is None:
            it = SsTableIterator.create_and_seek_to_first(table)
        else:
            it = SsTableIterator.create_and_seek_to_key(table, lower[1])
    except (BlockError, ReferencePanic) as e:
        if lower is None:
            raise ScanFailure(G._err_status(e), t, 0, 0)
        b, en, st = G.seek_failure(table, lower[1])
        raise ScanFailure(st, t, b, en)
    cur = S.Cursor(t, it, stats)
    if lower is not None and lower[0] == "ex" and cur.is_valid() and cur.key() == lower[1]:
        crossings = stats["crossings"]
        cur.next()
        stats["crossings"] = crossings
    return cur


class LevelCursor:
    """One cursor over the surviving tables [a, z] of a level (table indices into the
    concatenation of the levels)."""

    def __init__(self, ix: Index, a: int, z: int, lower, stats):
        self.ix, self.z, self.stats = ix, z, stats
        self.kd = FIRST if lower is None else KEYED
        self.cur = _seek(a, ix.tables[a], lower, stats)          # T[a]'s own seek comes first
        f = ix.nf[self.kd][a + 1] if a < z else NONE
        if f <= z:                                               # a failing head in (a, z]
            h = ix.head[f][self.kd]
            raise ScanFailure(h.status, f, h.block, h.entry)
        if not self.cur.is_valid():
            self._enter_next()

    def _enter_next(self):
        t = self.cur.t
        v = self.ix.nv[self.kd][t + 1] if t < self.z else NONE
        if v > self.z:
            return
        h = self.ix.head[v][self.kd]
        table = self.ix.tables[v]
        bi = BlockIterator(table.read_block_cached(h.block))
        bi._seek_to(h.entry)
        self.cur = S.Cursor(v, SsTableIterator(table, h.block, bi), self.stats)
        self.stats["tables_entered"] += 1

    def key(self):
        return self.cur.key()

    def value(self):
        return self.cur.value()

    def is_valid(self):
        return self.cur.is_valid()

    def where(self):
        return self.cur.where()

    def next(self):
        self.cur.next()
        if not self.cur.is_valid():
            self._enter_next()


def level_scan(runs, levels, lower, upper, limit: int, ix: Index | None = None) -> Scan:
    """What tpz_level_scan_ranges + tpz_level_scan_entries report for the scan. stats adds
    tables_entered (level cursors moving into a next table) and level_cursors."""
    ix = ix or Index(levels)
    stats = dict(tombstones=0, ties=0, crossings=0, dropped_lo=0, dropped_hi=0, quirk=0, cursors=0,
                 skips=0, mem=dict(ties=0), mem_cursors=0, tables_entered=0, level_cursors=0)
    after = False
    if lower is not None and lower[0] == "after":
        lower, after = ("ex", lower[1]), True
    hits, entries = [], []

    def failed(status, where):
        return Scan(ERROR, status, tuple(where), hits, entries, stats)

    for b in (lower, upper):
        if b is not None and b[0] not in ("in", "ex"):
            return failed(_lib.BLOCK_MALFORMED, (NONE, NONE, NONE))
    if ix.first_unopened != NONE:                                # found before any seek
        status, block = ix.open_failure[ix.first_unopened]
        return failed(status, (ix.first_unopened, block, NONE))
    mem_iters = [M.MemCursor(r, runs[r], lower, upper) for r in reversed(range(len(runs)))]
    stats["mem_cursors"] = sum(1 for c in mem_iters if c.is_valid())
    try:
        iters = []
        l0 = levels[0] if levels else []
        for j in reversed(range(len(l0))):                       # L0, newest first
            table = l0[j]
            if lower is not None and table.biggest_key < lower[1]:
                continue
            if upper is not None and table.smallest_key > upper[1]:
                continue
            iters.append(_seek(j, table, lower, stats))
        for lv in range(1, len(levels)):                         # one cursor per non-empty level
            if not levels[lv]:
                continue
            az = survivors(levels[lv], lower, upper)
            if az is None:
                continue
            base = ix.first[lv]
            iters.append(LevelCursor(ix, base + az[0], base + az[1], lower, stats))
            stats["level_cursors"] += 1
        stats["cursors"] = sum(1 for c in iters if c.is_valid())
        mem_iter = S.MergeIterator(mem_iters, stats["mem"])
        sst_iter = S.MergeIterator(iters, stats)
        two = M.TwoMergeIterator(mem_iter, sst_iter, stats)
        it = S.FusedIterator(S.LsmIterator(two, upper, stats, after))
        while it.is_valid():
            if len(hits) == limit:
                return Scan(MORE, _lib.BLOCK_OK, (NONE, NONE, NONE), hits, entries, stats)
            hits.append(it.where())
            entries.append((it.key(), it.value()))
            it.next()
    except ScanFailure as f:
        return failed(f.status, f.where)
    return Scan(DONE, _lib.BLOCK_OK, (NONE, NONE, NONE), hits, entries, stats)


def same(a: Scan, b: Scan) -> bool:
    """Everything the device reports (stats are the models' own)."""
    return (a.result, a.status, a.where, a.hits, a.entries) == \
        (b.result, b.status, b.where, b.hits, b.entries)

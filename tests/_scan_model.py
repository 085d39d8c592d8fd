"""What LsmStorage::scan answers over SSTs alone, restated twice (test infrastructure, CPU only).

`lsm_scan` follows the reference line by line over the facade's host objects (SsTable.smallest_key
and biggest_key, SsTableIterator): LevelController::level_tables_sorted (src/level.rs:538-579),
the cursor creation of LsmStorage::scan (src/lsm_storage.rs:335-374), MergeIterator
(src/iterators/merge_iterator.rs:41-106), TwoMergeIterator with an invalid memtable side,
LsmIterator and FusedIterator (src/lsm_iterator.rs). It returns what tpz_scan_ranges and
tpz_scan_entries report for the scan (include/tpz_gpu.h). `closed_scan` is the closed form for
honest table sets. tests/test_scan_model.py checks that the two agree and that the reference's own
scan tests come out; the GPU tests compare the device against `lsm_scan`.

Bounds are None (Unbounded), ("in", key), ("ex", key) and, as a lower bound, ("after", key):
Excluded with the first merged element end-checked (the continuation of a scan that reported
MORE).
"""
from __future__ import annotations

import re
from collections import namedtuple

from _get_model import NONE, _err_status, seek_failure
from topazdb_amd import _lib
from topazdb_amd.table import BlockError, ReferencePanic, SsTableIterator

DONE, MORE, ERROR = _lib.SCAN_DONE, _lib.SCAN_MORE, _lib.SCAN_ERROR

# tpz_scan_ranges' outputs for one scan: `where` = (table, block, entry) of a failure, `hits` =
# the yielded entries' (table, block, entry), `entries` = their (key, value); `stats` counts what
# the scan met on its way (what the tests' coverage assertions read).
Scan = namedtuple("Scan", "result status where hits entries stats")


class ScanFailure(Exception):
    """The reference's Err / panic inside a scan, as tpz_scan_ranges reports it."""

    def __init__(self, status: int, table: int, block: int, entry: int):
        super().__init__(status, table, block, entry)
        self.status, self.where = status, (table, block, entry)


def open_failure(table):
    """SsTable::open's init_samllest_biggest_key (table.rs:143-151) over the host table: None, or
    (status, block) where the reference fails (the table could not have been opened). Sets
    smallest_key and biggest_key."""
    if not table.block_metas:                                    # block_metas[0]
        return _lib.BLOCK_MALFORMED, NONE
    try:
        table.init_samllest_biggest_key()
    except BlockError as e:
        return _err_status(e), table.num_of_blocks() - 1
    except ReferencePanic:
        return _lib.BLOCK_MALFORMED, table.num_of_blocks() - 1
    return None


class Cursor:
    """An SsTableIterator of table `t` (its index in the concatenation of the levels) whose
    failures carry the block and entry tpz_seek_keys' convention names: the block whose read is
    an Err (entry 0), or the entry whose read panics."""

    def __init__(self, t: int, it: SsTableIterator, stats: dict):
        self.t, self.it, self.stats = t, it, stats

    def key(self):
        return self.it.key()

    def value(self):
        return self.it.value()

    def is_valid(self):
        return self.it.is_valid()

    def where(self):
        return self.t, self.it.idx, self.it.block_iter.idx

    def next(self):
        before = self.it.idx
        try:
            self.it.next()                                       # table/iterator.rs:88-95
        except BlockError as e:                                  # (idx already names the block)
            raise ScanFailure(_err_status(e), self.t, self.it.idx, 0)
        except ReferencePanic as e:
            entry = int(re.match(r"entry (\d+) of", str(e)).group(1))
            raise ScanFailure(_lib.BLOCK_MALFORMED, self.t, self.it.idx, entry)
        if self.it.idx != before:
            self.stats["crossings"] += 1


class MergeIterator:
    """merge_iterator.rs:41-106. The heap orders by (key, id), smallest first (HeapWrapper's
    reversed comparison); PeekMut is the heap's top edited in place."""

    def __init__(self, iters: list, stats: dict):
        self.stats = stats
        self.iters = [[i, it] for i, it in enumerate(x for x in iters if x.is_valid())]   # :48-53
        self.current = self._pop()                                                         # :55

    def _top(self):
        return min(self.iters, key=lambda w: (w[1].key(), w[0])) if self.iters else None

    def _pop(self):
        w = self._top()
        if w is not None:
            self.iters.remove(w)
        return w

    def key(self):
        return self.current[1].key()

    def value(self):
        return self.current[1].value()

    def where(self):
        return self.current[1].where()

    def is_valid(self):
        return self.current is not None

    def next(self):
        key = self.key()                                         # :74
        while True:                                              # :76
            inner = self._top()
            if inner is None or key != inner[1].key():           # :77-79
                break
            self.stats["ties"] += 1
            try:
                inner[1].next()                                  # :80
            except ScanFailure:
                self.iters.remove(inner)                         # :81-82
                raise
            if not inner[1].is_valid():                          # :85-87
                self.iters.remove(inner)
        current = self.current
        current[1].next()                                        # :91
        if not current[1].is_valid():                            # :93-96
            self.current = self._pop()
            return
        top = self._top()                                        # :98-102
        if top is not None and (top[1].key(), top[0]) < (current[1].key(), current[0]):
            self.iters.remove(top)
            self.iters.append(current)
            self.current = top


class InvalidIterator:
    """MergeIterator::create over no memtables."""

    def is_valid(self):
        return False


class TwoMergeIterator:
    """two_merge_iterator.rs with an always-invalid A: B passes through."""

    def __init__(self, a, b):
        assert not a.is_valid()
        self.b = b

    def key(self):
        return self.b.key()

    def value(self):
        return self.b.value()

    def where(self):
        return self.b.where()

    def is_valid(self):
        return self.b.is_valid()

    def next(self):
        self.b.next()


def _past_end(end, key: bytes) -> bool:
    """lsm_iterator.rs:46-50."""
    if end is None:
        return False
    kind, k = end
    return key > k if kind == "in" else key >= k


class LsmIterator:
    """lsm_iterator.rs:15-75. `after`: the first element is end-checked too (the device's
    TPZ_BOUND_AFTER; the reference has no such mode)."""

    def __init__(self, inner, end, stats: dict, after: bool = False):
        self.inner, self.end, self.stats = inner, end, stats
        self.valid = inner.is_valid()                            # :24
        if self.valid and _past_end(end, inner.key()):
            if after:
                self.valid = False
            elif len(inner.value()):
                stats["quirk"] = 1                               # e0 is past the end and is yielded
        while self.valid and len(self.value()) == 0:             # :29-31
            self.stats["tombstones"] += 1
            self.next_inner()

    def next_inner(self):
        if not self.valid:                                       # :36-38
            return
        self.inner.next()                                        # :40
        if not self.inner.is_valid():                            # :41-44
            self.valid = False
            return
        if _past_end(self.end, self.inner.key()):                # :46-50
            self.valid = False

    def is_valid(self):
        return self.valid

    def key(self):
        return self.inner.key()

    def value(self):
        return self.inner.value()

    def where(self):
        return self.inner.where()

    def next(self):
        self.next_inner()                                        # :69
        while self.valid and len(self.value()) == 0:             # :70-72
            self.stats["tombstones"] += 1
            self.next_inner()


class FusedIterator:
    """lsm_iterator.rs:79-108."""

    def __init__(self, it):
        self.it = it

    def is_valid(self):
        return self.it.is_valid()

    def key(self):
        return self.it.key()

    def value(self):
        return self.it.value()

    def where(self):
        return self.it.where()

    def next(self):
        if not self.is_valid():
            return
        self.it.next()


def level_tables_sorted(levels, lower, upper, stats: dict):
    """level.rs:538-579 as (table index, table) in priority order."""
    first = [0]
    for lv in levels:
        first.append(first[-1] + len(lv))
    order = []
    if levels:
        order += [(first[0] + j, levels[0][j]) for j in reversed(range(len(levels[0])))]   # :570-572
    for i in range(1, len(levels)):                                                       # :574-577
        order += [(first[i] + j, t) for j, t in enumerate(levels[i])]
    res = []
    for t, table in order:                                       # filter_push, :554-568
        if lower is not None and table.biggest_key < lower[1]:
            stats["dropped_lo"] += 1
            continue
        if upper is not None and table.smallest_key > upper[1]:
            stats["dropped_hi"] += 1
            continue
        res.append((t, table))
    return order, res


def lsm_scan(levels, lower, upper, limit: int, after: bool = False) -> Scan:
    """LsmStorage::scan(lower, upper) over the SSTs of `levels` (`levels[0]` is L0 in push
    order), at most `limit` entries, as tpz_scan_ranges + tpz_scan_entries report it."""
    stats = dict(tombstones=0, ties=0, crossings=0, dropped_lo=0, dropped_hi=0, quirk=0, cursors=0)
    if lower is not None and lower[0] == "after":
        lower, after = ("ex", lower[1]), True
    if after:
        assert lower is not None and lower[0] == "ex"
    hits, entries = [], []

    def failed(status, where):
        return Scan(ERROR, status, tuple(where), hits, entries, stats)

    for b, kinds in ((lower, ("in", "ex")), (upper, ("in", "ex"))):
        if b is not None and b[0] not in kinds:                  # a kind the device cannot read
            return failed(_lib.BLOCK_MALFORMED, (NONE, NONE, NONE))
    order_all = [t for lv in levels for t in lv]
    for table in order_all:
        table._open_failure = open_failure(table)
    order, ssts = level_tables_sorted(levels, lower, upper, stats)
    for t, table in order:                                       # SsTable::open would have failed
        if table._open_failure is not None:
            status, block = table._open_failure
            return failed(status, (t, block, NONE))
    try:
        iters = []
        for t, table in ssts:                                    # lsm_storage.rs:350-365
            try:
                if lower is None:
                    it = SsTableIterator.create_and_seek_to_first(table)
                else:
                    it = SsTableIterator.create_and_seek_to_key(table, lower[1])
            except (BlockError, ReferencePanic) as e:
                if lower is None:                                # block 0's read, or its entry 0
                    raise ScanFailure(_err_status(e), t, 0, 0)
                b, en, st = seek_failure(table, lower[1])
                raise ScanFailure(st, t, b, en)
            cur = Cursor(t, it, stats)
            if lower is not None and lower[0] == "ex" and cur.is_valid() and cur.key() == lower[1]:
                crossings = stats["crossings"]
                cur.next()
                stats["crossings"] = crossings                   # (counted for the merge only)
            iters.append(cur)
        stats["cursors"] = sum(1 for c in iters if c.is_valid())
        sst_iter = MergeIterator(iters, stats)                   # :366
        two = TwoMergeIterator(InvalidIterator(), sst_iter)      # :367
        it = FusedIterator(LsmIterator(two, upper, stats, after))   # :373
        while it.is_valid():
            if len(hits) == limit:
                return Scan(MORE, _lib.BLOCK_OK, (NONE, NONE, NONE), hits, entries, stats)
            hits.append(it.where())
            entries.append((it.key(), it.value()))
            it.next()
    except ScanFailure as f:
        return failed(f.status, f.where)
    return Scan(DONE, _lib.BLOCK_OK, (NONE, NONE, NONE), hits, entries, stats)


def closed_scan(entry_lists, lower, upper):
    """Honest table sets as entry lists (every table sorted by key without repeats): the tables
    passing the filter, newest wins per key, the keys satisfying the lower bound in order, the
    first of them exempt from the end test, which ends the scan at its first failure, tombstones
    dropped. Returns the yielded (key, value) list."""
    order = list(reversed(entry_lists[0])) if entry_lists else []
    for lv in entry_lists[1:]:
        order += lv
    merged = {}
    for ents in order:
        if not ents:
            continue
        if lower is not None and ents[-1][0] < lower[1]:
            continue
        if upper is not None and ents[0][0] > upper[1]:
            continue
        for k, v in ents:
            merged.setdefault(k, v)
    out = []
    n = 0
    for k in sorted(merged):
        if lower is not None and (k < lower[1] or (lower[0] == "ex" and k == lower[1])):
            continue
        if n > 0 and _past_end(upper, k):
            break
        n += 1
        if merged[k]:
            out.append((k, merged[k]))
    return out


def paged_scan(levels, lower, upper, limit: int):
    """The pages a consumer pulls: each MORE page continued with ("after", its last key).
    Returns (entries, last page's Scan)."""
    entries = []
    s = lsm_scan(levels, lower, upper, limit)
    while True:
        entries += s.entries
        if s.result != MORE:
            return entries, s
        s = lsm_scan(levels, ("after", s.entries[-1][0]), upper, limit)


def reference_cases() -> dict:
    """The four SST-visible scan tests of src/tests/storage.rs:110-246 as (L0 tables in push
    order, [(lower, upper, expected entries)]); every memtable is the L0 table sync() makes of
    it, a delete its empty value."""
    def scans(full, in12, ex13):
        return [(None, None, full), (("in", b"1"), ("in", b"2"), in12),
                (("ex", b"1"), ("ex", b"3"), ex13)]
    e1, e2, e3 = (b"1", b"233"), (b"2", b"2333"), (b"3", b"23333")
    return {
        "scan_memtable_1": ([[e1, (b"2", b""), e3]], scans([e1, e3], [e1], [])),
        "scan_memtable_2": ([[(b"1", b""), e2, e3]], scans([e2, e3], [e2], [e2])),
        "scan_memtable_1_after_sync": ([[e1, e2], [(b"2", b""), e3]], scans([e1, e3], [e1], [])),
        "scan_memtable_2_after_sync": ([[e1, e2], [e3], [(b"1", b"")]],
                                       scans([e2, e3], [e2], [e2])),
    }

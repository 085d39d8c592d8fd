"""Inputs of the level scan's tests (test infrastructure, CPU only): table sets whose levels below
L0 hold more tables than a merge wave has lanes, honest by construction (sorted and disjoint, which
`assert_honest` checks from the entries), their corrupted variants, and the per-table models'
answers (tests/_scan_model.py lsm_scan, tests/_lsm_model.py lsm_scan_mem), computed once per
process and shared by tests/test_level_scan_model.py and tests/test_gpu_level_scan.py.

Shapes are tiny: tables of 2-8 keys of five bytes, block size 64, so a table has 2-4 blocks."""
from __future__ import annotations

import copy
import functools
import random

import numpy as np

import _get_model as G
import _lsm_cases as C
import _lsm_model as M
import _scan_cases as K
import _scan_model as S
import badentry_util as B

BLOCK = 64
LIMITS = K.LIMITS + (1 << 12,)          # (1, 3, 64) and one above every scan's length
BIG = LIMITS[-1]
ERROR_LIMITS = (1, BIG)                 # the damaged variants'


def key(i: int) -> bytes:
    return b"k%04d" % i


def table_of(rng, lv: int, t: int, ids) -> list:
    """Entries of 15 value bytes (or a tombstone): three or four to a 64-byte block."""
    return [(key(i), b"" if rng.random() < 0.2 else b"L%d.%03d=%s...." % (lv, t, key(i)))
            for i in ids]


def wide_levels(rng, n_ids: int, l0: int, lower: list[int]) -> list:
    """Entry lists: `l0` overlapping L0 tables and one level of `n` disjoint tables of 2-8 keys in
    key order per entry of `lower` (0: an empty level), over the keys key(0 .. n_ids - 1)."""
    ents = [[table_of(rng, 0, t, sorted(rng.sample(range(n_ids), rng.randint(2, 8))))
             for t in range(l0)]]
    for lv, n in enumerate(lower, 1):
        sizes = [rng.randint(2, 8) for _ in range(n)]
        ids = sorted(rng.sample(range(n_ids), sum(sizes)))
        tabs, at = [], 0
        for t, m in enumerate(sizes):
            tabs.append(table_of(rng, lv, t, ids[at:at + m]))
            at += m
        ents.append(tabs)
    return ents


def assert_honest(ents) -> None:
    """From the entries alone: keys increase inside every table, and the tables of a level below
    L0 are in key order and disjoint."""
    for lv, tabs in enumerate(ents):
        for e in tabs:
            ks = [k for k, _ in e]
            assert ks == sorted(set(ks)) and all(ks), lv
        if lv:
            assert all(a[-1][0] < b[0][0] for a, b in zip(tabs, tabs[1:]) if a and b), lv


class LevelCase(C.LsmCase):
    """Runs (maybe none), a table set and ranges; `model` is the per-table model's answer."""

    def model(self, r: int, limit: int):
        if (r, limit) not in self._models:
            lo, hi = self.ranges[r]
            self._models[r, limit] = (M.lsm_scan_mem(self.runs, self.host, lo, hi, limit)
                                      if self.runs else S.lsm_scan(self.host, lo, hi, limit))
        return self._models[r, limit]


def gap_pairs(ents) -> list:
    """Bounds placed by hand at the levels' seams: in the gap between two tables, at a table's
    biggest and smallest key, below and above a whole level."""
    out = []
    for tabs in ents[1:]:
        if len(tabs) < 4:
            continue
        j = len(tabs) // 2
        big, small = tabs[j][-1][0], tabs[j + 1][0][0]
        gap = big + b"\0"                                       # between T[j] and T[j + 1]
        assert big < gap < small
        out += [(gap, tabs[j + 2][-1][0]), (tabs[j - 1][0][0], gap), (big, small), (big, big),
                (small, big), (b"a", b"j"), (b"l", b"z"), (tabs[j][0][0], tabs[j + 3][0][0])]
    return out


@functools.lru_cache(maxsize=None)
def wide_case() -> LevelCase:
    """3 L0 tables, 70 tables in L1 and 100 in L2: 173 tables, 5 cursors."""
    rng = random.Random(2024)
    ents = wide_levels(rng, 1500, 3, [70, 100])
    assert_honest(ents)
    pairs = K.bound_pairs(rng, ents, 8) + gap_pairs(ents)
    ranges = K.ranges_of(pairs)
    return LevelCase([], ents, K.pieces_of(ents, BLOCK), ranges)


def quirk_case() -> LevelCase:
    """L1 = {a, d}, {f, g}: scan(In(b), In(c)) yields d; scan(Ex(d), In(e)) yields nothing."""
    ents = [[], [[(b"a", b"1"), (b"d", b"4")], [(b"f", b"6"), (b"g", b"7")]]]
    ranges = [(("in", b"b"), ("in", b"c")), (("ex", b"d"), ("in", b"e")), (("ex", b"d"), None),
              (("in", b"e"), ("in", b"e")), (None, ("in", b"e")), (("after", b"d"), ("in", b"e"))]
    return LevelCase([], ents, K.pieces_of(ents, BLOCK), ranges)


# ------------------------------------------------------------------------------- corrupted variants
def corrupt(p: G.Pieces, block: int) -> None:
    region = bytearray(p.region)
    region[int(p.ext[block]) + 7] ^= 0x80                      # the block's CRC no longer matches
    p.region = bytes(region)


def bad_probe(p: G.Pieces) -> int:
    """Block 0 rebuilt with the entry its bisection probes first (n // 2) made unreadable
    (badentry_util "key_off": BAD_KEY). Returns that entry's index."""
    ents0 = [e for e in p.ents if len(p.first_keys) < 2 or e[0] < p.first_keys[1]]
    bad = len(ents0) // 2
    assert bad > 0                                              # entry 0 stays readable
    blk = B.bad_block(ents0, bad, "key_off")
    old = int(p.ext[1])
    p.region = blk + p.region[old:]
    ext = p.ext.astype(np.int64) + (len(blk) - old)
    ext[0] = 0
    p.ext = ext.astype(np.uint64)
    return bad


def empty_block0(p: G.Pieces) -> None:
    """Block 0 replaced by a block without entries (a valid CRC)."""
    blk = B.raw_block([], b"")
    old = int(p.ext[1])
    p.region = blk + p.region[old:]
    ext = p.ext.astype(np.int64) + (len(blk) - old)
    ext[0] = 0
    p.ext = ext.astype(np.uint64)


def variant(base: LevelCase, edits, ranges=None, runs=None) -> LevelCase:
    """`base` with edits [(level, table, function of its Pieces)] applied to copies."""
    pieces = [list(lv) for lv in base.pieces]
    for lv, t, fn in edits:
        pieces[lv][t] = copy.deepcopy(pieces[lv][t])
        fn(pieces[lv][t])
    return LevelCase(base.runs if runs is None else runs, base.ents, pieces,
                     base.ranges if ranges is None else ranges)


def n_blocks(p: G.Pieces) -> int:
    return len(p.first_keys)


def pick(base: LevelCase, lv: int, lo: int, hi: int, blocks: int) -> int:
    """A table of level lv in [lo, hi) with at least `blocks` blocks."""
    return next(t for t in range(lo, hi) if n_blocks(base.pieces[lv][t]) >= blocks)


@functools.lru_cache(maxsize=None)
def error_cases() -> dict:
    """name -> (case, level, table): the wide set with one table of a level below L0 damaged,
    under every second range (all nine kind pairs still)."""
    base = wide_case()
    base = LevelCase([], base.ents, base.pieces, base.ranges[::2])
    out = {}
    t = pick(base, 2, 55, 100, 2)
    out["block0"] = (variant(base, [(2, t, lambda p: corrupt(p, 0))]), 2, t)
    t = pick(base, 1, 30, 70, 3)
    out["middle"] = (variant(base, [(1, t, lambda p: corrupt(p, 1))]), 1, t)
    t = pick(base, 2, 45, 100, 2)
    out["last"] = (variant(base, [(2, t, lambda p: corrupt(p, n_blocks(p) - 1))]), 2, t)
    t = next(t for t in range(35, 70) if n_blocks(base.pieces[1][t]) >= 2 and
             sum(1 for e in base.ents[1][t] if e[0] < base.pieces[1][t].first_keys[1]) >= 2)
    out["probe"] = (variant(base, [(1, t, bad_probe)]), 1, t)
    t = pick(base, 1, 20, 70, 2)
    out["empty0"] = (variant(base, [(1, t, empty_block0)]), 1, t)
    return out


def table_index(case: LevelCase, lv: int, t: int) -> int:
    return sum(len(x) for x in case.pieces[:lv]) + t


# ------------------------------------------------------------------------------- runs on top
@functools.lru_cache(maxsize=None)
def runs_case() -> LevelCase:
    """16 runs, 4 L0 tables and three levels of 30 tables. Run 15 holds the last key of a level
    table (TwoMergeIterator's eager skip then carries the level cursor across the boundary) and
    run 14 a tombstone for a key only L3 holds with a value."""
    rng = random.Random(77)
    ents = wide_levels(rng, 900, 4, [30, 30, 30])
    assert_honest(ents)
    others = {k for lv in ents[:3] for e in lv for k, _ in e}
    last = next(e[-1][0] for e in ents[1][5:25])                # the last key of an L1 table
    hidden = next(k for e in ents[3] for k, v in e if v and k not in others)
    runs = []
    for r in range(16):
        ids = sorted(rng.sample(range(900), rng.randint(1, 6)))
        runs.append({key(i): (b"" if rng.random() < 0.2 else b"run%d" % r) for i in ids})
    for run in runs:
        run.pop(hidden, None)
        run.pop(last, None)
    runs[15][last] = b"newest"
    runs[14][hidden] = b""
    runs = [sorted(r.items()) for r in runs]
    pairs = K.bound_pairs(rng, ents + [runs], 6) + gap_pairs(ents)[:6]
    ranges = [(None, None), (("in", last), None), (("in", hidden), ("in", hidden))] + K.ranges_of(pairs)
    case = LevelCase(runs, ents, K.pieces_of(ents, BLOCK), ranges)
    case.last, case.hidden = last, hidden
    return case


@functools.lru_cache(maxsize=None)
def max_case() -> LevelCase:
    """16 runs, 42 L0 tables and 6 non-empty levels of 12 tables: 64 cursors, 114 tables; every
    cursor is live at the start of the unbounded scan."""
    rng = random.Random(5)
    ents = wide_levels(rng, 600, 42, [12] * 6)
    assert_honest(ents)
    runs = [sorted({key(i): b"run%d" % r for i in rng.sample(range(600), 1 + r % 4)}.items())
            for r in range(16)]
    ranges = [(None, None), (("in", key(100)), ("ex", key(400)))]
    return LevelCase(runs, ents, K.pieces_of(ents, BLOCK), ranges)

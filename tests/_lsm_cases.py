"""Inputs of the LsmStorage::scan tests over memtable runs plus tables and the model's answers for
them (test infrastructure, CPU only): tests/_scan_cases.py's table sets with runs over the same
alphabet, the ranges, and `lsm_scan_mem` over each, computed once per process and shared by
tests/test_lsm_model.py and tests/test_gpu_lsm_scan.py."""
from __future__ import annotations

import functools
import random

import _get_model as G
import _lsm_model as M
import _scan_cases as K

#          table set (K.RANDOM's index, or the long keys), runs
RANDOM = [(0, 3), (1, 1), (2, 5), (3, 0), (len(K.RANDOM), 2)]
RANDOM_IDS = [f"{K.RANDOM_IDS[t]}_runs{r}" for t, r in RANDOM]


class LsmCase:
    """Runs, a table set, ranges over them, and the model's answer per (range, limit), computed
    on first use and then kept."""

    def __init__(self, runs, ents, pieces, ranges):
        self.runs, self.ents, self.pieces, self.ranges = runs, ents, pieces, ranges
        self.host = K.host_levels(pieces)
        self._models = {}

    def model(self, r: int, limit: int):
        if (r, limit) not in self._models:
            lo, hi = self.ranges[r]
            self._models[r, limit] = M.lsm_scan_mem(self.runs, self.host, lo, hi, limit)
        return self._models[r, limit]

    def models(self, limit: int, idx=None) -> list:
        return [self.model(r, limit) for r in (range(len(self.ranges)) if idx is None else idx)]


def small_case(runs, level_ents, ranges, block_size=64) -> LsmCase:
    return LsmCase(runs, level_ents, K.pieces_of(level_ents, block_size), ranges)


@functools.lru_cache(maxsize=None)
def random_case(i: int) -> LsmCase:
    """Case i of RANDOM_IDS: a table set of tests/_scan_cases.py (the same entries) under runs of
    at most 60 keys drawn like the tables' keys, 25 % tombstones; bounds from the keys held by
    tables and runs, their neighbours and absent keys, crossed with every kind pair."""
    t, n_runs = RANDOM[i]
    base = K.random_case(t)
    rng = random.Random(100 + i)
    if t == len(K.RANDOM):                       # the long keys: runs from the tables' own keys
        universe = sorted({k for lv in base.ents for e in lv for k, _ in e})
        runs = [[(k, b"" if rng.random() < 0.25 else b"m%d=" % r + k[-8:])
                 for k in sorted(rng.sample(universe, 40))] for r in range(n_runs)]
        n_pairs = 24
    else:
        runs = [M.random_run(rng, r) for r in range(n_runs)]
        n_pairs = 40
    pairs = K.bound_pairs(rng, base.ents + [runs], n_pairs)
    return LsmCase(runs, base.ents, base.pieces, K.ranges_of(pairs))


def hidden_keys(case: LsmCase) -> set:
    """Keys whose newest run copy is a tombstone while some table holds a value for them."""
    newest = {}
    for run in reversed(case.runs):
        for k, v in run:
            newest.setdefault(k, v)
    in_tables = {k for lv in case.ents for e in lv for k, v in e if v}
    return {k for k, v in newest.items() if not v and k in in_tables}


def in_run(t: int) -> bool:
    return t != G.NONE and bool(t & M.HIT_MEM)

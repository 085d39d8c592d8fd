"""Inputs of the scan tests and the model's answers for them (test infrastructure, CPU only):
table sets as entry lists, their host tables (tests/_get_model.py's builders), the ranges, and
`lsm_scan` over each, computed once per process and shared by tests/test_scan_model.py and
tests/test_gpu_scan.py."""
from __future__ import annotations

import functools
import random

import numpy as np

import _get_model as G
import _scan_model as S

ALPHABET = b"ab\x00\xff"
LOWER_KINDS = (None, "in", "ex")
UPPER_KINDS = (None, "in", "ex")
KIND_PAIRS = [(lk, hk) for lk in LOWER_KINDS for hk in UPPER_KINDS]
LIMITS = (1, 3, 64)

#          seed, L0, lower levels, block size   (the shapes of tests/test_gpu_get.py's RANDOM)
RANDOM = [(11, 5, [4, 0, 1], 64),
          (12, 3, [1, 2, 0], 256),
          (13, 0, [0, 1, 4], 64),
          (14, 1, [2, 1, 0], 256)]
RANDOM_IDS = [f"l0_{c[1]}_b{c[3]}" for c in RANDOM] + ["long_keys"]


def bound(kind, key):
    return None if kind is None else (kind, key)


def neighbours(k: bytes) -> list[bytes]:
    return [k[:-1] + bytes([(k[-1] + 1) & 0xFF]), k[:-1] + bytes([(k[-1] - 1) & 0xFF]),
            k + b"\0", k[:-1]]


def pieces_of(ents, block_size):
    """Tables without filters (a scan reads none)."""
    return [[G.build_pieces(e, block_size, None) for e in tabs] for tabs in ents]


def host_levels(pieces):
    out, tid = [], 0
    for lv in pieces:
        out.append([p.host_table(tid + j) for j, p in enumerate(lv)])
        tid += len(lv)
    return out


def flat(levels):
    return [t for lv in levels for t in lv]


class Case:
    """A table set, ranges over it, and the model's answer per (range, limit), computed on
    first use and then kept."""

    def __init__(self, ents, pieces, ranges):
        self.ents, self.pieces, self.ranges = ents, pieces, ranges
        self.host = host_levels(pieces)
        self._models = {}

    def model(self, r: int, limit: int) -> S.Scan:
        if (r, limit) not in self._models:
            lo, hi = self.ranges[r]
            self._models[r, limit] = S.lsm_scan(self.host, lo, hi, limit)
        return self._models[r, limit]

    def models(self, limit: int, idx=None) -> list:
        return [self.model(r, limit) for r in (range(len(self.ranges)) if idx is None else idx)]


def bound_pairs(rng, ents, n_pairs):
    """(lower key, upper key) pairs drawn from the keys held, their neighbours and absent keys:
    ordered, equal and inverted ones."""
    held = sorted({k for lv in ents for tab in lv for k, _ in tab})
    pool = list(held)
    for k in held:
        pool += neighbours(k)
    pool += [k + b"\0\0\0" for k in held[::3]]                  # absent: just after a key
    pool += [b"", b"\x00", b"\xff" * 50]                        # below all, above all
    pairs = []
    for j in range(n_pairs):
        a, b = rng.choice(pool), rng.choice(pool)
        if j % 4 == 0:
            b = a                                               # an empty or one-key range
        elif j % 4 != 3 and a > b:
            a, b = b, a                                         # (j % 4 == 3: as drawn)
        pairs.append((a, b))
    return pairs


def ranges_of(pairs):
    return [(bound(lk, a), bound(hk, b)) for a, b in pairs for lk, hk in KIND_PAIRS]


@functools.lru_cache(maxsize=None)
def random_case(i: int) -> Case:
    """Case i of RANDOM_IDS: tables of up to 60 keys of at most 3 bytes over a 4-letter alphabet
    (so the tables overlap heavily), or the long-key set."""
    if i == len(RANDOM):
        return long_key_case()
    seed, l0, lower, block_size = RANDOM[i]
    rng = random.Random(seed)
    ents = G.random_set(rng, l0, lower, 60, ALPHABET, 3, 0.25, min_keys=1)
    return Case(ents, pieces_of(ents, block_size), ranges_of(bound_pairs(rng, ents, 40)))


def long_key_case() -> Case:
    """40-byte keys sharing 32-byte prefixes: the merge's 8-byte prefixes tie within a group and
    across groups, so the full comparison decides."""
    rng = random.Random(15)
    groups = [b"tenant-00/collection-%02d/object::" % g for g in range(3)]
    assert all(len(g) == 32 for g in groups)
    universe = sorted({g + bytes(rng.choice(b"xyz\x00") for _ in range(8)) for g in groups
                       for _ in range(60)})
    assert all(len(k) == 40 for k in universe)

    def table(lv, t, keys):
        return [(k, b"" if rng.random() < 0.25 else b"%d.%d=" % (lv, t) + k[-8:]) for k in keys]

    l0 = [table(0, t, sorted(rng.sample(universe, rng.randint(20, 60)))) for t in range(3)]
    ks = sorted(rng.sample(universe, 90))
    l1 = [table(1, t, ks[30 * t:30 * t + 30]) for t in range(3)]
    ents = [l0, l1]
    return Case(ents, pieces_of(ents, 256), ranges_of(bound_pairs(rng, ents, 24)))


def expected(models: list, limit: int) -> dict:
    """The arrays tpz_scan_ranges and tpz_scan_entries report for the scans `models`."""
    n = len(models)
    first = np.zeros(n + 1, np.uint64)
    kfirst = np.zeros(n + 1, np.uint64)
    vfirst = np.zeros(n + 1, np.uint64)
    np.cumsum([len(m.hits) for m in models], out=first[1:])
    np.cumsum([sum(len(k) for k, _ in m.entries) for m in models], out=kfirst[1:])
    np.cumsum([sum(len(v) for _, v in m.entries) for m in models], out=vfirst[1:])
    ents = [e for m in models for e in m.entries]
    kpos = np.zeros(len(ents) + 1, np.uint64)
    vpos = np.zeros(len(ents) + 1, np.uint64)
    np.cumsum([len(k) for k, _ in ents], out=kpos[1:])
    np.cumsum([len(v) for _, v in ents], out=vpos[1:])
    return {"result": np.array([m.result for m in models], np.uint8),
            "status": np.array([m.status for m in models], np.uint8),
            "where": np.array([m.where for m in models], np.uint32).reshape(n, 3),
            "hits": [np.array(m.hits, np.uint32).reshape(len(m.hits), 3) for m in models],
            "first": first, "key_first": kfirst, "val_first": vfirst, "kpos": kpos, "vpos": vpos,
            "keys": b"".join(k for k, _ in ents), "values": b"".join(v for _, v in ents)}

"""Inputs of the key-length tests of the device xxh3_64 (test infrastructure, CPU only): one
random key per length over every branch of tpz_xxh3.h's hash64, single-bit mutants of each key,
their hashes from the xxhash package, a packer that puts key starts on every alignment, and
Bloom::may_contain a probe round at a time. tests/test_xxh3_cases.py pins what these inputs reach;
tests/test_gpu_xxh3_lengths.py runs the device over them.
"""
from __future__ import annotations

import functools

import numpy as np
import xxhash

from _bloom_model import from_hashes
from topazdb_amd import _lib
from topazdb_amd.table import Bloom

# every length to 2200 (all of the short paths, the 129-240 path at every round count, the long
# path with 0, 1 and 2 whole blocks and every stripe count after each), then block counts 2, 3, 4,
# 7, 8 and 63 (the longest key the reference's u16 key length allows)
LENGTHS = list(range(2201)) + [3000, 4095, 4096, 4097, 8191, 8192, 8193, 65535]
FLIP = 0x10
LEADS = range(16)
PROBE_FPP = 1e-30        # the probe test's filter: k = 15
TINY = 1e-300            # about 1,438 bits a key: several slices with 2,209 keys
# lengths of the single-key filters (one side of every branch of hash64)
SINGLE = [0, 3, 8, 16, 17, 128, 129, 240, 241, 1024, 1025, 65535]
# key lengths of the get and SST tests
TABLE_LENGTHS = [1, 16, 17, 64, 65, 96, 97, 128, 129, 160, 240, 241, 256, 1024, 1025, 1089, 2048,
                 2049, 3000, 4000]
TABLE_FPP = 0.01
SST_ENTRIES = 60
# (keys, fpp) of every filter the GPU tests build or compare (the get test's tables hold 40, 60
# and 40 keys)
GEOMETRIES = [(len(LENGTHS), PROBE_FPP), (len(LENGTHS), TINY), (len(LENGTHS), 0.1), (1, TINY),
              (SST_ENTRIES, TABLE_FPP), (40, TABLE_FPP), (60, TABLE_FPP)]


def branch(n: int):
    """The path hash64 takes for a key of n bytes, restated from the XXH3 specification: the
    path's name and what varies inside it (the 129-240 path's round count; the long path's whole
    1 KiB blocks and the 64-byte stripes after them)."""
    if n == 0:
        return "0", None
    if n <= 3:
        return "1-3", None
    if n <= 8:
        return "4-8", None
    if n <= 16:
        return "9-16", None
    if n <= 128:
        return ("17-32", "33-64", "65-96", "97-128")[(n - 1) // 32], None
    if n <= 240:
        return "129-240", n // 16
    nb = (n - 1) // 1024
    return "long", (nb, (n - 1 - 1024 * nb) // 64)


@functools.lru_cache(maxsize=None)
def keys() -> tuple:
    """One key per entry of LENGTHS, drawn in that order from one generator."""
    rng = np.random.default_rng(7)
    return tuple(rng.bytes(n) for n in LENGTHS)


def flip_positions(n: int) -> list[int]:
    """Where a key of n > 0 bytes is mutated: its ends and middle, the start of the last 64 bytes
    (the long path reads them a second time), the end of the first stripe, and both sides of the
    first 1 KiB block's end."""
    return sorted({0, n // 2, n - 1, max(0, n - 64), min(n - 1, 63), min(n - 1, 1023),
                   min(n - 1, 1024)})


def mutants_of(key: bytes) -> list[bytes]:
    out = []
    for p in flip_positions(len(key)) if key else []:
        m = bytearray(key)
        m[p] ^= FLIP
        out.append(bytes(m))
    return out


@functools.lru_cache(maxsize=None)
def mutants() -> tuple:
    """(index into LENGTHS, flipped position, mutant) for every non-empty key and position."""
    return tuple((i, p, m) for i, k in enumerate(keys())
                 for p, m in zip(flip_positions(len(k)), mutants_of(k)))


def hashes(items) -> np.ndarray:
    """xxh3_64 (seed 0) of every item, from the xxhash package."""
    return np.fromiter((xxhash.xxh3_64_intdigest(b) for b in items), np.uint64, len(items))


@functools.lru_cache(maxsize=None)
def key_hashes() -> np.ndarray:
    return hashes(keys())


@functools.lru_cache(maxsize=None)
def mutant_hashes() -> np.ndarray:
    return hashes([m for _, _, m in mutants()])


@functools.lru_cache(maxsize=None)
def model_filter(fpp: float) -> bytes:
    """Bloom::from_keys over the keys' hashes (tests/_bloom_model.py)."""
    return from_hashes(key_hashes(), fpp)


def may_contain(filt: bytes, hs: np.ndarray) -> np.ndarray:
    """Bloom::may_contain (src/bloom.rs:72-84) of `filt` for every hash, as booleans."""
    f = np.frombuffer(filt, np.uint8)
    k, limit = int(f[-1]), np.uint64((len(f) - 1) * 8)
    h = np.ascontiguousarray(hs, np.uint64).copy()
    delta = (h >> np.uint64(34)) | (h << np.uint64(30))
    ok = np.ones(len(h), bool)
    for _ in range(k):
        pos = h % limit
        ok &= (f[(pos >> np.uint64(3)).astype(np.int64)] >> (pos & np.uint64(7)).astype(np.uint8)) & 1 == 1
        h += delta                                             # wraps mod 2^64
    return ok


def pack(items, lead: int = 0):
    """The items back to back after `lead` filler bytes: (byte column, len(items) + 1 uint64
    positions, the first one `lead`)."""
    pos = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(b) for b in items], out=pos[1:])
    col = np.frombuffer(b"\xa5" * lead + b"".join(items), np.uint8)
    return col, pos + np.uint64(lead)


def reach(n: int, fpp: float):
    """(slices, workgroups, keys a workgroup, k) of tpz_bloom_build's partitioned route for n keys
    at fpp, from tpz_bloom_geometry and the kernel constants mirrored in topazdb_amd._lib."""
    geo = _lib.bloom_geometry(n, fpp)
    assert geo == Bloom.geometry(n, fpp)
    limit = (geo[0] - 1) * 8
    per_wg = _lib.BLOOM_WG_PROBES // geo[1]
    S = (limit + _lib.BLOOM_SLICE_BITS - 1) // _lib.BLOOM_SLICE_BITS
    return S, max(1, (n + per_wg - 1) // per_wg), per_wg, geo[1]


def table_sets():
    """The get test's entries: ([L0 older, L0 newer], [L1]) as sorted (key, value) lists, and the
    held keys. Five keys per length of TABLE_LENGTHS share their first len - 1 bytes; by last byte:
    0x10 the older L0 table alone, 0x30 the newer alone, 0x50 level 1 alone, 0x70 both L0 tables,
    0x90 the newer L0 table and level 1. A value names its table; for every second length the newer
    table's copy of the keys it shares is a tombstone, for every third level 1's own key is."""
    def val(t, key):
        return b"t%d:%d:" % (t, len(key)) + key[-4:]

    rng = np.random.default_rng(11)
    t0, t1, t2 = [], [], []
    for i, n in enumerate(TABLE_LENGTHS):
        stem = rng.bytes(n - 1)
        k = [stem + bytes([c]) for c in (0x10, 0x30, 0x50, 0x70, 0x90)]
        t0 += [(k[0], val(0, k[0])), (k[3], val(0, k[3]))]
        t1 += [(k[1], val(1, k[1])), (k[3], b"" if i % 2 == 0 else val(1, k[3])),
               (k[4], b"" if i % 2 == 1 else val(1, k[4]))]
        t2 += [(k[2], b"" if i % 3 == 0 else val(2, k[2])), (k[4], val(2, k[4]))]
    held = sorted({k for t in (t0, t1, t2) for k, _ in t})
    return [[sorted(t0), sorted(t1)], [sorted(t2)]], held


def sst_entries():
    """SST_ENTRIES sorted entries whose key lengths cycle through TABLE_LENGTHS (the first byte
    counts up, the rest is random)."""
    rng = np.random.default_rng(13)
    out = []
    for i in range(SST_ENTRIES):
        n = TABLE_LENGTHS[i % len(TABLE_LENGTHS)]
        out.append((bytes([i + 1]) + rng.bytes(n - 1), b"v%02d" % i if i % 7 else b""))
    return out

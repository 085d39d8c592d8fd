"""tpz_mem_prefix, tpz_lsm_get_keys / tpz_lsm_get_values and tpz_lsm_scan_ranges /
tpz_lsm_scan_entries refuse bad arguments before any device work (no GPU needed): too many runs,
more than 64 cursors, a level table that breaks its rules, a zero or overflowing limit, null and
misaligned pointers. The constants are the header's and the ABI version is unchanged."""
import ctypes as C
import re

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first

KEYS = dict(runs=0x800, tabs=0x1000, keys=0x2000, kpos=0x3000, res=0x4000, st=0x5000, tab=0x6000,
            blk=0x7000, ent=0x8000, vpos=0x9000)


def get_keys(lf, n_levels, n_runs=2, n_tables=4, n=5, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(KEYS, **over).items()}
    lf = None if lf is None else np.ascontiguousarray(lf, np.uint32)
    return _lib.lib().tpz_lsm_get_keys(
        ctx, p["runs"], n_runs, p["tabs"], n_tables,
        None if lf is None else C.c_void_p(lf.ctypes.data), n_levels, p["keys"], p["kpos"], n,
        p["res"], p["st"], p["tab"], p["blk"], p["ent"], p["vpos"], None)


VALUES = dict(runs=0x800, tabs=0x1000, res=0x4000, tab=0x6000, blk=0x7000, ent=0x8000, vpos=0x9000,
              vals=0xA000)


def get_values(n_runs=2, n_tables=4, n=5, val_cap=64, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(VALUES, **over).items()}
    return _lib.lib().tpz_lsm_get_values(ctx, p["runs"], n_runs, p["tabs"], n_tables, n, p["res"],
                                         p["tab"], p["blk"], p["ent"], p["vpos"], p["vals"],
                                         val_cap, None)


def test_lsm_get_keys_argument_checks():
    ok = [0, 2, 4]
    assert _lib.MEM_MAX_RUNS == 16
    assert get_keys(ok, 2, n_runs=17) == _lib.ERR_INVALID_ARG
    assert get_keys(ok, 2, runs=0) == _lib.ERR_INVALID_ARG              # runs, but no descriptors
    assert get_keys(ok, 2, runs=KEYS["runs"] + 4) == _lib.ERR_INVALID_ARG
    levels = _lib.GET_MAX_LEVELS + 1
    assert get_keys([0] + [4] * levels, levels) == _lib.ERR_INVALID_ARG
    for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
        assert get_keys(lf, len(lf) - 1) == _lib.ERR_INVALID_ARG, lf
    assert get_keys([0], 0) == _lib.ERR_INVALID_ARG           # tables, but no level holds them
    assert get_keys(None, 2) == _lib.ERR_INVALID_ARG
    assert get_keys(ok, 2, n=0xFFFFFFFF) == _lib.ERR_INVALID_ARG
    assert get_keys(ok, 2, tabs=0) == _lib.ERR_INVALID_ARG
    for name in ("tabs", "kpos", "vpos"):                                 # u64 / pointers
        assert get_keys(ok, 2, **{name: KEYS[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("tab", "blk", "ent"):                                    # u32 columns
        assert get_keys(ok, 2, **{name: KEYS[name] + 2}) == _lib.ERR_INVALID_ARG, name
    for name in ("kpos", "res", "st", "tab", "blk", "ent", "vpos"):
        assert get_keys(ok, 2, **{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert get_keys(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG


def test_lsm_get_values_argument_checks():
    assert get_values(n_runs=17) == _lib.ERR_INVALID_ARG
    assert get_values(runs=0) == _lib.ERR_INVALID_ARG
    assert get_values(runs=VALUES["runs"] + 4) == _lib.ERR_INVALID_ARG
    assert get_values(vals=VALUES["vals"] + 8) == _lib.ERR_INVALID_ARG   # 16-byte aligned
    assert get_values(vals=0) == _lib.ERR_INVALID_ARG
    for name in ("tabs", "vpos"):
        assert get_values(**{name: VALUES[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("tab", "blk", "ent"):
        assert get_values(**{name: VALUES[name] + 2}) == _lib.ERR_INVALID_ARG, name
    for name in ("tabs", "res", "tab", "blk", "ent", "vpos"):
        assert get_values(**{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert get_values(ctx=None) == _lib.ERR_INVALID_ARG


RANGES = dict(runs=0x800, tabs=0x1000, lok=0x2000, lop=0x3000, lokind=0x3100, hik=0x2800,
              hip=0x3800, hikind=0x3900, res=0x4000, st=0x5000, where=0x5800, htab=0x6000,
              hblk=0x7000, hent=0x8000, first=0x9000, kfirst=0x9800, vfirst=0xA000, info=0xA800)


def ranges(lf, n_levels, n_runs=2, n_tables=4, n=5, limit=3, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(RANGES, **over).items()}
    lf = None if lf is None else np.ascontiguousarray(lf, np.uint32)
    return _lib.lib().tpz_lsm_scan_ranges(
        ctx, p["runs"], n_runs, p["tabs"], n_tables,
        None if lf is None else C.c_void_p(lf.ctypes.data), n_levels, p["lok"], p["lop"],
        p["lokind"], p["hik"], p["hip"], p["hikind"], n, limit, p["res"], p["st"], p["where"],
        p["htab"], p["hblk"], p["hent"], p["first"], p["kfirst"], p["vfirst"], p["info"], None)


ENTRIES = dict(runs=0x800, tabs=0x1000, htab=0x6000, hblk=0x7000, hent=0x8000, first=0x9000,
               keys=0xB000, kpos=0xC000, vals=0xD000, vpos=0xE000)


def entries(n_runs=2, n_tables=4, n=5, limit=3, key_cap=64, val_cap=64, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(ENTRIES, **over).items()}
    return _lib.lib().tpz_lsm_scan_entries(ctx, p["runs"], n_runs, p["tabs"], n_tables, n, limit,
                                           p["htab"], p["hblk"], p["hent"], p["first"], p["keys"],
                                           key_cap, p["kpos"], p["vals"], val_cap, p["vpos"], None)


def test_lsm_scan_ranges_argument_checks():
    ok = [0, 2, 4]
    assert ranges(ok, 2, n_runs=17) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, runs=0) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, runs=RANGES["runs"] + 4) == _lib.ERR_INVALID_ARG
    assert ranges([0, 40, 49], 2, n_runs=16, n_tables=49) == _lib.ERR_INVALID_ARG   # 65 cursors
    assert ranges([0, 60, 65], 2, n_runs=0, n_tables=65) == _lib.ERR_INVALID_ARG
    levels = _lib.GET_MAX_LEVELS + 1
    assert ranges([0] + [4] * levels, levels) == _lib.ERR_INVALID_ARG
    for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
        assert ranges(lf, len(lf) - 1) == _lib.ERR_INVALID_ARG, lf
    assert ranges([0], 0) == _lib.ERR_INVALID_ARG
    assert ranges(None, 2) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, limit=0) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, n=1 << 16, limit=1 << 16) == _lib.ERR_INVALID_ARG    # n * limit = 2^32
    assert ranges(ok, 2, tabs=0) == _lib.ERR_INVALID_ARG
    for name in ("tabs", "lop", "hip", "first", "kfirst", "vfirst", "info"):  # u64 / pointers
        assert ranges(ok, 2, **{name: RANGES[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("where", "htab", "hblk", "hent"):                            # u32 columns
        assert ranges(ok, 2, **{name: RANGES[name] + 2}) == _lib.ERR_INVALID_ARG, name
    for name in ("lop", "lokind", "hip", "hikind", "res", "st", "where", "htab", "hblk", "hent",
                 "first", "kfirst", "vfirst", "info"):
        assert ranges(ok, 2, **{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert ranges(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG


def test_lsm_scan_entries_argument_checks():
    assert entries(n_runs=17) == _lib.ERR_INVALID_ARG
    assert entries(runs=0) == _lib.ERR_INVALID_ARG
    assert entries(runs=ENTRIES["runs"] + 4) == _lib.ERR_INVALID_ARG
    assert entries(n_runs=16, n_tables=49) == _lib.ERR_INVALID_ARG
    assert entries(limit=0) == _lib.ERR_INVALID_ARG
    assert entries(n=1 << 16, limit=1 << 16) == _lib.ERR_INVALID_ARG
    for name in ("keys", "vals"):                                             # 16-byte aligned
        assert entries(**{name: ENTRIES[name] + 8}) == _lib.ERR_INVALID_ARG, name
        assert entries(**{name: 0}) == _lib.ERR_INVALID_ARG, name
    for name in ("tabs", "first", "kpos", "vpos"):
        assert entries(**{name: ENTRIES[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("htab", "hblk", "hent"):
        assert entries(**{name: ENTRIES[name] + 2}) == _lib.ERR_INVALID_ARG, name
    for name in ("tabs", "htab", "hblk", "hent", "first", "kpos", "vpos"):
        assert entries(**{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert entries(ctx=None) == _lib.ERR_INVALID_ARG


def test_mem_prefix_argument_checks():
    L = _lib.lib()
    ent = _lib.Entries(0x1000, 0x2000, 0x3000, 0x4000, 5, 40, 40)
    assert L.tpz_mem_prefix(None, C.byref(ent), C.c_void_p(0x5000), None) == _lib.ERR_INVALID_ARG
    assert L.tpz_mem_prefix(CTX, None, C.c_void_p(0x5000), None) == _lib.ERR_INVALID_ARG
    assert L.tpz_mem_prefix(CTX, C.byref(ent), None, None) == _lib.ERR_INVALID_ARG
    assert L.tpz_mem_prefix(CTX, C.byref(ent), C.c_void_p(0x5004), None) == _lib.ERR_INVALID_ARG
    for bad in (_lib.Entries(0x1000, 0x2004, 0x3000, 0x4000, 5, 40, 40),
                _lib.Entries(0x1000, None, 0x3000, 0x4000, 5, 40, 40),
                _lib.Entries(None, 0x2000, 0x3000, 0x4000, 5, 40, 40)):
        assert L.tpz_mem_prefix(CTX, C.byref(bad), C.c_void_p(0x5000), None) == _lib.ERR_INVALID_ARG
    empty = _lib.Entries(None, None, None, None, 0, 0, 0)       # nothing to do: no device work
    assert L.tpz_mem_prefix(CTX, C.byref(empty), None, None) == _lib.SUCCESS


def test_constants_match_the_header_and_the_abi_stays():
    hdr = open(_lib.HEADER).read()
    for name, val in (("TPZ_HAS_MEM", 1), ("TPZ_MEM_MAX_RUNS", _lib.MEM_MAX_RUNS),
                      ("TPZ_HIT_MEM", _lib.HIT_MEM), ("TPZ_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, hdr).group(1), 0) == val
    assert _lib.lib().tpz_abi_version() == 8
    for f in ("tpz_mem_prefix", "tpz_lsm_get_keys", "tpz_lsm_get_values", "tpz_lsm_scan_ranges",
              "tpz_lsm_scan_entries"):
        assert f in _lib.header_functions() and hasattr(_lib.lib(), f)
    assert C.sizeof(_lib.MemRun) == C.sizeof(_lib.Entries) + 8

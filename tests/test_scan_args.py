"""tpz_scan_ranges / tpz_scan_entries refuse bad arguments before any device work (no GPU
needed): too many tables, a level table that breaks its rules, a zero or overflowing limit, null
and misaligned pointers. The constants are the header's and the ABI version is unchanged."""
import ctypes as C
import re

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first

RANGES = dict(tabs=0x1000, lok=0x2000, lop=0x3000, lokind=0x3100, hik=0x2800, hip=0x3800,
              hikind=0x3900, res=0x4000, st=0x5000, where=0x5800, htab=0x6000, hblk=0x7000,
              hent=0x8000, first=0x9000, kfirst=0x9800, vfirst=0xA000, info=0xA800)


def ranges(lf, n_levels, n_tables=4, n=5, limit=3, ctx=CTX, **over):
    a = dict(RANGES, **over)
    lf = None if lf is None else np.ascontiguousarray(lf, np.uint32)
    p = {k: C.c_void_p(v) for k, v in a.items()}
    return _lib.lib().tpz_scan_ranges(
        ctx, p["tabs"], n_tables, None if lf is None else C.c_void_p(lf.ctypes.data), n_levels,
        p["lok"], p["lop"], p["lokind"], p["hik"], p["hip"], p["hikind"], n, limit, p["res"],
        p["st"], p["where"], p["htab"], p["hblk"], p["hent"], p["first"], p["kfirst"],
        p["vfirst"], p["info"], None)


ENTRIES = dict(tabs=0x1000, htab=0x6000, hblk=0x7000, hent=0x8000, first=0x9000, keys=0xB000,
               kpos=0xC000, vals=0xD000, vpos=0xE000)


def entries(n_tables=4, n=5, limit=3, key_cap=64, val_cap=64, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(ENTRIES, **over).items()}
    return _lib.lib().tpz_scan_entries(ctx, p["tabs"], n_tables, n, limit, p["htab"], p["hblk"],
                                       p["hent"], p["first"], p["keys"], key_cap, p["kpos"],
                                       p["vals"], val_cap, p["vpos"], None)


def test_scan_ranges_argument_checks():
    ok = [0, 2, 4]
    big = _lib.SCAN_MAX_TABLES + 1
    assert big == 65
    assert ranges([0, 60, big], 2, n_tables=big) == _lib.ERR_INVALID_ARG      # 65 tables
    levels = _lib.GET_MAX_LEVELS + 1
    assert ranges([0] + [4] * levels, levels) == _lib.ERR_INVALID_ARG
    for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
        assert ranges(lf, len(lf) - 1) == _lib.ERR_INVALID_ARG, lf
    assert ranges([0], 0) == _lib.ERR_INVALID_ARG             # tables, but no level holds them
    assert ranges(None, 2) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, limit=0) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, n=1 << 16, limit=1 << 16) == _lib.ERR_INVALID_ARG    # n * limit = 2^32
    assert ranges(ok, 2, n=0xFFFFFFFF, limit=2) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, tabs=0) == _lib.ERR_INVALID_ARG
    for name in ("tabs", "lop", "hip", "first", "kfirst", "vfirst", "info"):  # u64 / pointers
        assert ranges(ok, 2, **{name: RANGES[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("where", "htab", "hblk", "hent"):                            # u32 columns
        assert ranges(ok, 2, **{name: RANGES[name] + 2}) == _lib.ERR_INVALID_ARG, name
    for name in ("lop", "lokind", "hip", "hikind", "res", "st", "where", "htab", "hblk", "hent",
                 "first", "kfirst", "vfirst", "info"):
        assert ranges(ok, 2, **{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert ranges(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG


def test_scan_entries_argument_checks():
    assert entries(n_tables=65) == _lib.ERR_INVALID_ARG
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


def test_constants_match_the_header_and_the_abi_stays():
    hdr = open(_lib.HEADER).read()
    for name, val in (("TPZ_HAS_SCAN", 1), ("TPZ_SCAN_MAX_TABLES", _lib.SCAN_MAX_TABLES),
                      ("TPZ_BOUND_UNBOUNDED", _lib.BOUND_UNBOUNDED),
                      ("TPZ_BOUND_INCLUDED", _lib.BOUND_INCLUDED),
                      ("TPZ_BOUND_EXCLUDED", _lib.BOUND_EXCLUDED),
                      ("TPZ_BOUND_AFTER", _lib.BOUND_AFTER), ("TPZ_SCAN_DONE", _lib.SCAN_DONE),
                      ("TPZ_SCAN_MORE", _lib.SCAN_MORE), ("TPZ_SCAN_ERROR", _lib.SCAN_ERROR),
                      ("TPZ_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val, name
    assert _lib.lib().tpz_abi_version() == 8
    for f in ("tpz_scan_ranges", "tpz_scan_entries"):
        assert f in _lib.header_functions() and hasattr(_lib.lib(), f)

"""tpz_level_scan_ranges / tpz_level_scan_entries refuse bad arguments before any device work (no
GPU needed): more than 64 cursors (runs + L0 tables + non-empty levels below L0) however they
come about, too many levels, a level table that breaks its rules, a zero or overflowing limit, null
and misaligned pointers. The constants are the header's, the ABI version is unchanged and the Rust
declarations name the new symbols."""
import ctypes as C
import os
import re

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first

RANGES = dict(runs=0x800, tabs=0x1000, lok=0x2000, lop=0x3000, lokind=0x3100, hik=0x2800,
              hip=0x3800, hikind=0x3900, res=0x4000, st=0x5000, where=0x5800, htab=0x6000,
              hblk=0x7000, hent=0x8000, first=0x9000, kfirst=0x9800, vfirst=0xA000, info=0xA800)


def ranges(lf, n_levels, n_runs=2, n_tables=4, n=5, limit=3, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(RANGES, **over).items()}
    lf = None if lf is None else np.ascontiguousarray(lf, np.uint32)
    return _lib.lib().tpz_level_scan_ranges(
        ctx, p["runs"], n_runs, p["tabs"], n_tables,
        None if lf is None else C.c_void_p(lf.ctypes.data), n_levels, p["lok"], p["lop"],
        p["lokind"], p["hik"], p["hip"], p["hikind"], n, limit, p["res"], p["st"], p["where"],
        p["htab"], p["hblk"], p["hent"], p["first"], p["kfirst"], p["vfirst"], p["info"], None)


ENTRIES = dict(runs=0x800, tabs=0x1000, htab=0x6000, hblk=0x7000, hent=0x8000, first=0x9000,
               keys=0xB000, kpos=0xC000, vals=0xD000, vpos=0xE000)


def entries(n_runs=2, n_tables=4, n=5, limit=3, key_cap=64, val_cap=64, ctx=CTX, **over):
    p = {k: C.c_void_p(v) for k, v in dict(ENTRIES, **over).items()}
    return _lib.lib().tpz_level_scan_entries(ctx, p["runs"], n_runs, p["tabs"], n_tables, n, limit,
                                             p["htab"], p["hblk"], p["hent"], p["first"],
                                             p["keys"], key_cap, p["kpos"], p["vals"], val_cap,
                                             p["vpos"], None)


def test_sixty_five_cursors_three_ways():
    assert _lib.LEVEL_SCAN_MAX_CURSORS == 64
    # 65 L0 tables
    assert ranges([0, 65], 1, n_runs=0, n_tables=65) == _lib.ERR_INVALID_ARG
    # 16 runs + 49 L0 tables
    assert ranges([0, 49], 1, n_runs=16, n_tables=49) == _lib.ERR_INVALID_ARG
    # 16 runs + 43 L0 tables + 6 non-empty levels (of 100 tables each, one empty level between)
    lf = [0, 43, 143, 243, 243, 343, 443, 543, 643]
    assert len(lf) - 1 == 8 and sum(b > a for a, b in zip(lf[1:], lf[2:])) == 6
    assert ranges(lf, 8, n_runs=16, n_tables=643) == _lib.ERR_INVALID_ARG
    # a huge L0 does not wrap the count
    assert ranges([0, 0xFFFFFFF0], 1, n_runs=16, n_tables=0xFFFFFFF0) == _lib.ERR_INVALID_ARG


def test_level_scan_ranges_argument_checks():
    ok = [0, 2, 4]
    assert ranges(ok, 2, n_runs=17) == _lib.ERR_INVALID_ARG
    assert ranges(ok, 2, runs=0) == _lib.ERR_INVALID_ARG                 # runs, but no descriptors
    assert ranges(ok, 2, runs=RANGES["runs"] + 4) == _lib.ERR_INVALID_ARG
    levels = _lib.GET_MAX_LEVELS + 1
    assert ranges([0] + [4] * levels, levels) == _lib.ERR_INVALID_ARG
    for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):                # a broken h_level_first
        assert ranges(lf, len(lf) - 1) == _lib.ERR_INVALID_ARG, lf
    assert ranges([0], 0) == _lib.ERR_INVALID_ARG             # tables, but no level holds them
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
    # 1,000 tables in a level are no reason to refuse: these fail for their pointers alone
    assert ranges([0, 4, 1004], 2, n_tables=1004, info=0) == _lib.ERR_INVALID_ARG


def test_level_scan_entries_argument_checks():
    assert entries(n_runs=17) == _lib.ERR_INVALID_ARG
    assert entries(runs=0) == _lib.ERR_INVALID_ARG
    assert entries(runs=ENTRIES["runs"] + 4) == _lib.ERR_INVALID_ARG
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
    for name, val in (("TPZ_HAS_LEVEL_SCAN", 1),
                      ("TPZ_LEVEL_SCAN_MAX_CURSORS", _lib.LEVEL_SCAN_MAX_CURSORS),
                      ("TPZ_SCAN_MAX_TABLES", _lib.SCAN_MAX_TABLES),
                      ("TPZ_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, hdr).group(1), 0) == val
    assert _lib.lib().tpz_abi_version() == 8
    for f in ("tpz_level_scan_ranges", "tpz_level_scan_entries"):
        assert f in _lib.header_functions() and hasattr(_lib.lib(), f)


def test_the_rust_declarations_name_the_new_symbols():
    rs = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "rust", "tpz-gpu-sys", "src",
                           "lib.rs")).read()
    for f in ("tpz_level_scan_ranges", "tpz_level_scan_entries"):
        assert re.search(r"pub fn %s\(" % f, rs), f
    assert re.search(r"pub const TPZ_HAS_LEVEL_SCAN: u32 = 1;", rs)
    assert re.search(r"pub const TPZ_LEVEL_SCAN_MAX_CURSORS: u32 = 64;", rs)

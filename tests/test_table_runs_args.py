"""tpz_table_runs_layout / tpz_table_runs_entries refuse bad arguments before any device work (no
GPU needed): too many runs, a block table that breaks its rules, misaligned or null columns, a
null context."""
import ctypes as C

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first


def layout(bf, n_runs, ctx=CTX, tabs=0x1000, first=0x2000, run_first=0x3000, info=0x4000):
    bf = np.ascontiguousarray(bf, np.uint32)
    return _lib.lib().tpz_table_runs_layout(ctx, C.c_void_p(tabs), n_runs,
                                            C.c_void_p(bf.ctypes.data if len(bf) else 0),
                                            C.c_void_p(first), C.c_void_p(run_first),
                                            C.c_void_p(info), None)


def entries(bf, n_runs, ctx=CTX, tabs=0x1000, first=0x2000, keys=0x5000, key_cap=64, kpos=0x6000,
            vals=0x7000, val_cap=64, vpos=0x8000, entry_cap=10):
    bf = np.ascontiguousarray(bf, np.uint32)
    return _lib.lib().tpz_table_runs_entries(ctx, C.c_void_p(tabs), n_runs,
                                             C.c_void_p(bf.ctypes.data if len(bf) else 0),
                                             C.c_void_p(first), C.c_void_p(keys), key_cap,
                                             C.c_void_p(kpos), C.c_void_p(vals), val_cap,
                                             C.c_void_p(vpos), entry_cap, None)


BAD_TABLES = ([1, 10], [0, 7, 5, 10], [0, 4, 3])


def test_table_runs_layout_argument_checks():
    big = _lib.MERGE_MAX_RUNS + 1
    assert layout([0] * big + [10], big) == _lib.ERR_INVALID_ARG
    for bf in BAD_TABLES:
        assert layout(bf, len(bf) - 1) == _lib.ERR_INVALID_ARG, bf
    ok = [0, 4, 10]
    assert layout([], 2) == _lib.ERR_INVALID_ARG                       # h_block_first is NULL
    assert layout(ok, 2, tabs=0x1004) == _lib.ERR_INVALID_ARG           # descriptors: 8-byte
    assert layout(ok, 2, first=0x2004) == _lib.ERR_INVALID_ARG          # u64 prefixes
    assert layout(ok, 2, info=0x4004) == _lib.ERR_INVALID_ARG
    assert layout(ok, 2, run_first=0x3002) == _lib.ERR_INVALID_ARG      # u32 run table
    for null in ("tabs", "first", "run_first", "info"):
        assert layout(ok, 2, **{null: 0}) == _lib.ERR_INVALID_ARG, null
    assert layout(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG
    assert layout([0], 0, ctx=None, tabs=0) == _lib.ERR_INVALID_ARG


def test_table_runs_entries_argument_checks():
    big = _lib.MERGE_MAX_RUNS + 1
    assert entries([0] * big + [10], big) == _lib.ERR_INVALID_ARG
    for bf in BAD_TABLES:
        assert entries(bf, len(bf) - 1) == _lib.ERR_INVALID_ARG, bf
    ok = [0, 4, 10]
    assert entries([], 2) == _lib.ERR_INVALID_ARG
    assert entries(ok, 2, keys=0x5001) == _lib.ERR_INVALID_ARG          # 16-byte columns
    assert entries(ok, 2, keys=0x5008) == _lib.ERR_INVALID_ARG
    assert entries(ok, 2, vals=0x7008) == _lib.ERR_INVALID_ARG
    assert entries(ok, 2, kpos=0x6004) == _lib.ERR_INVALID_ARG          # u64 positions
    assert entries(ok, 2, vpos=0x8004) == _lib.ERR_INVALID_ARG
    assert entries(ok, 2, first=0x2004) == _lib.ERR_INVALID_ARG
    assert entries(ok, 2, tabs=0x1004) == _lib.ERR_INVALID_ARG
    for null in ("tabs", "first", "keys", "kpos", "vals", "vpos"):
        assert entries(ok, 2, **{null: 0}) == _lib.ERR_INVALID_ARG, null
    assert entries(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG
    assert entries([0], 0, ctx=None, tabs=0) == _lib.ERR_INVALID_ARG

"""The in-place table calls (tpz_raw_verify, tpz_raw_seek_keys, tpz_raw_get_keys / _values,
tpz_raw_lsm_get_keys / _values) exist, are announced by TPZ_HAS_RAW_TABLES, and refuse bad
arguments before any device work (no GPU needed), with the rules of their decoded counterparts
(tests/test_get_args.py, tests/test_lsm_args.py)."""
import ctypes as C
import re

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case ends in its argument checks
BAD = _lib.ERR_INVALID_ARG
RAW = ["tpz_raw_verify", "tpz_raw_seek_keys", "tpz_raw_get_keys", "tpz_raw_get_values",
       "tpz_raw_lsm_get_keys", "tpz_raw_lsm_get_values"]


def p(x):
    return C.c_void_p(x)


def keys(lf, n_levels, n_tables=4, tabs=0x1000, q=0x2000, qpos=0x3000, n=5, res=0x4000, st=0x5000,
         tab=0x6000, blk=0x7000, ent=0x8000, vpos=0x9000, ctx=CTX, runs=None):
    lf = np.ascontiguousarray(lf, np.uint32)
    args = [p(tabs), n_tables, p(lf.ctypes.data), n_levels, p(q), p(qpos), n, p(res), p(st),
            p(tab), p(blk), p(ent), p(vpos), None]
    if runs is None:
        return _lib.lib().tpz_raw_get_keys(ctx, *args)
    return _lib.lib().tpz_raw_lsm_get_keys(ctx, p(runs[0]), runs[1], *args)


def values(n_tables=4, tabs=0x1000, n=5, res=0x4000, tab=0x6000, blk=0x7000, ent=0x8000,
           vpos=0x9000, vals=0xA000, cap=64, ctx=CTX, runs=None):
    args = [p(tabs), n_tables, n, p(res), p(tab), p(blk), p(ent), p(vpos), p(vals), cap, None]
    if runs is None:
        return _lib.lib().tpz_raw_get_values(ctx, *args)
    return _lib.lib().tpz_raw_lsm_get_values(ctx, p(runs[0]), runs[1], *args)


def test_symbols_and_header():
    hdr = open(_lib.HEADER).read()
    assert re.search(r"#define\s+TPZ_HAS_RAW_TABLES\s+1\b", hdr) and _lib.HAS_RAW_TABLES == 1
    fns = _lib.header_functions()
    L = _lib.lib()
    for f in RAW:
        assert f in fns and hasattr(L, f), f
    assert L.tpz_abi_version() == 8
    # tpz_raw_table: five pointers and n_blocks, then the filter and its length
    assert C.sizeof(_lib.RawTable) == 64
    assert [f[0] for f in _lib.RawTable._fields_] == [
        "d_first_keys", "d_first_pos", "d_src", "d_ext", "n_blocks", "d_status", "d_filter",
        "filter_len"]
    m = re.search(r"struct tpz_raw_table \{(.*?)\};", hdr, re.S)
    assert re.findall(r"(\w+);", m.group(1)) == [f[0] for f in _lib.RawTable._fields_]


def test_get_keys_argument_checks():
    for runs in (None, (0xB000, 2)):
        big = _lib.GET_MAX_LEVELS + 1
        assert keys([0] + [4] * big, big, runs=runs) == BAD
        for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
            assert keys(lf, len(lf) - 1, runs=runs) == BAD, lf
        assert keys([0], 0, runs=runs) == BAD                 # tables, but no level holds them
        ok = [0, 2, 4]
        assert keys(ok, 2, tabs=0, runs=runs) == BAD
        assert keys(ok, 2, tabs=0x1004, runs=runs) == BAD     # descriptors hold pointers
        assert keys(ok, 2, qpos=0x3004, runs=runs) == BAD     # u64 positions
        assert keys(ok, 2, vpos=0x9004, runs=runs) == BAD
        for name in ("tab", "blk", "ent"):                    # u32 columns
            assert keys(ok, 2, runs=runs, **{name: 0x6002}) == BAD, name
        for name in ("qpos", "res", "st", "tab", "blk", "ent", "vpos"):
            assert keys(ok, 2, runs=runs, **{name: 0}) == BAD, name
        assert keys(ok, 2, ctx=None, runs=runs) == BAD
        assert keys(ok, 2, n=0xFFFFFFFF, runs=runs) == BAD
    # a null level table with levels
    assert _lib.lib().tpz_raw_get_keys(CTX, p(0x1000), 4, None, 2, *[p(0x2000)] * 2, 5,
                                       *[p(0x4000)] * 6, None) == BAD
    ok = [0, 2, 4]
    assert keys(ok, 2, runs=(0, 2)) == BAD                    # runs counted but absent
    assert keys(ok, 2, runs=(0xB004, 2)) == BAD
    assert keys(ok, 2, runs=(0xB000, _lib.MEM_MAX_RUNS + 1)) == BAD


def test_get_values_argument_checks():
    for runs in (None, (0xB000, 2)):
        assert values(vals=0xA008, runs=runs) == BAD          # 16-byte aligned values
        assert values(vals=0, runs=runs) == BAD
        assert values(tabs=0, runs=runs) == BAD
        assert values(vpos=0x9004, runs=runs) == BAD
        assert values(tab=0x6002, runs=runs) == BAD
        for name in ("res", "tab", "blk", "ent", "vpos"):
            assert values(runs=runs, **{name: 0}) == BAD, name
        assert values(ctx=None, runs=runs) == BAD
        # nothing to do: no keys (also with no tables), or no room
        assert values(n=0, runs=runs) == _lib.SUCCESS
        assert values(n=0, n_tables=0, tabs=0, runs=runs) == _lib.SUCCESS
        assert values(cap=0, vals=0, runs=runs) == _lib.SUCCESS
    assert values(runs=(0xB000, _lib.MEM_MAX_RUNS + 1)) == BAD


def test_seek_and_verify_argument_checks():
    L = _lib.lib()
    t = _lib.RawTable(0x1000, 0x2000, 0x3000, 0x4000, 3, 0x5000, None, 0)
    out = [p(0x6000), p(0x7000), p(0x8000), p(0x9000)]

    def seek(table=t, q=0xA000, qpos=0xB000, n=4, outs=out, ctx=CTX):
        return L.tpz_raw_seek_keys(ctx, C.byref(table) if table is not None else None, p(q),
                                   p(qpos), n, *outs, None)

    assert seek(ctx=None) == BAD and seek(table=None) == BAD and seek(qpos=0) == BAD
    for i in range(4):
        assert seek(outs=out[:i] + [None] + out[i + 1:]) == BAD, i
    for field in ("d_first_keys", "d_first_pos", "d_src", "d_ext", "d_status"):
        bad = _lib.RawTable(0x1000, 0x2000, 0x3000, 0x4000, 3, 0x5000, None, 0)
        setattr(bad, field, None)
        assert seek(table=bad) == BAD, field
    assert seek(n=0) == _lib.SUCCESS                          # no keys: nothing to do

    b = _lib.Batch(0x1000, 0x2000, 3, 100)
    assert L.tpz_raw_verify(CTX, C.byref(b), None, p(0x4000), None) == BAD
    assert L.tpz_raw_verify(CTX, C.byref(b), p(0x3000), None, None) == BAD
    assert L.tpz_raw_verify(CTX, C.byref(b), p(0x3000), p(0x4002), None) == BAD   # u32 CRCs
    assert L.tpz_raw_verify(None, C.byref(b), p(0x3000), p(0x4000), None) == BAD
    assert L.tpz_raw_verify(CTX, None, p(0x3000), p(0x4000), None) == BAD
    for field in ("d_src", "d_ext"):
        bb = _lib.Batch(0x1000, 0x2000, 3, 100)
        setattr(bb, field, None)
        assert L.tpz_raw_verify(CTX, C.byref(bb), p(0x3000), p(0x4000), None) == BAD, field
    empty = _lib.Batch(None, None, 0, 0)
    assert L.tpz_raw_verify(CTX, C.byref(empty), p(0x3000), p(0x4000), None) == _lib.SUCCESS

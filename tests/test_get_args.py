"""tpz_get_keys / tpz_get_values refuse bad arguments before any device work (no GPU needed):
too many levels, a level table that breaks its rules, null and misaligned pointers."""
import ctypes as C

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first


def keys(lf, n_levels, n_tables=4, tabs=0x1000, q=0x2000, qpos=0x3000, n=5, res=0x4000, st=0x5000,
         tab=0x6000, blk=0x7000, ent=0x8000, vpos=0x9000, ctx=CTX):
    lf = np.ascontiguousarray(lf, np.uint32)
    return _lib.lib().tpz_get_keys(ctx, C.c_void_p(tabs), n_tables, C.c_void_p(lf.ctypes.data),
                                   n_levels, C.c_void_p(q), C.c_void_p(qpos), n, C.c_void_p(res),
                                   C.c_void_p(st), C.c_void_p(tab), C.c_void_p(blk),
                                   C.c_void_p(ent), C.c_void_p(vpos), None)


def values(n_tables=4, tabs=0x1000, n=5, res=0x4000, tab=0x6000, blk=0x7000, ent=0x8000,
           vpos=0x9000, vals=0xA000, cap=64, ctx=CTX):
    return _lib.lib().tpz_get_values(ctx, C.c_void_p(tabs), n_tables, n, C.c_void_p(res),
                                     C.c_void_p(tab), C.c_void_p(blk), C.c_void_p(ent),
                                     C.c_void_p(vpos), C.c_void_p(vals), cap, None)


def test_get_keys_argument_checks():
    big = _lib.GET_MAX_LEVELS + 1
    assert keys([0] + [4] * big, big) == _lib.ERR_INVALID_ARG
    for lf in ([1, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
        assert keys(lf, len(lf) - 1) == _lib.ERR_INVALID_ARG, lf
    assert keys([0], 0) == _lib.ERR_INVALID_ARG             # tables, but no level holds them
    ok = [0, 2, 4]
    assert _lib.lib().tpz_get_keys(CTX, C.c_void_p(0x1000), 4, None, 2, *[C.c_void_p(0x2000)] * 2,
                                   5, *[C.c_void_p(0x4000)] * 6, None) == _lib.ERR_INVALID_ARG
    assert keys(ok, 2, tabs=0) == _lib.ERR_INVALID_ARG
    assert keys(ok, 2, tabs=0x1004) == _lib.ERR_INVALID_ARG    # descriptors hold pointers
    assert keys(ok, 2, qpos=0x3004) == _lib.ERR_INVALID_ARG    # u64 positions
    assert keys(ok, 2, vpos=0x9004) == _lib.ERR_INVALID_ARG
    for name in ("tab", "blk", "ent"):                         # u32 columns
        assert keys(ok, 2, **{name: 0x6002}) == _lib.ERR_INVALID_ARG, name
    for name in ("qpos", "res", "st", "tab", "blk", "ent", "vpos"):
        assert keys(ok, 2, **{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert keys(ok, 2, ctx=None) == _lib.ERR_INVALID_ARG


def test_get_values_argument_checks():
    assert values(vals=0xA008) == _lib.ERR_INVALID_ARG         # 16-byte aligned values
    assert values(vals=0) == _lib.ERR_INVALID_ARG
    assert values(tabs=0) == _lib.ERR_INVALID_ARG
    assert values(vpos=0x9004) == _lib.ERR_INVALID_ARG
    assert values(tab=0x6002) == _lib.ERR_INVALID_ARG
    for name in ("res", "tab", "blk", "ent", "vpos"):
        assert values(**{name: 0}) == _lib.ERR_INVALID_ARG, name
    assert values(ctx=None) == _lib.ERR_INVALID_ARG


def test_constants_and_descriptor_layout():
    """The binding's constants are the header's, and GetTable is tpz_get_table: a tpz_table, the
    filter pointer and its length."""
    import re
    hdr = open(_lib.HEADER).read()
    for name, val in (("TPZ_GET_MAX_LEVELS", _lib.GET_MAX_LEVELS), ("TPZ_GET_ABSENT", _lib.GET_ABSENT),
                      ("TPZ_GET_FOUND", _lib.GET_FOUND), ("TPZ_GET_DELETED", _lib.GET_DELETED),
                      ("TPZ_GET_ERROR", _lib.GET_ERROR), ("TPZ_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == val, name
    assert _lib.lib().tpz_abi_version() == 8
    assert C.sizeof(_lib.GetTable) == C.sizeof(_lib.Table) + 16
    assert _lib.GetTable.d_filter.offset == C.sizeof(_lib.Table)

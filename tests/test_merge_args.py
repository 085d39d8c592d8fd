"""tpz_merge_runs / tpz_flat_entry_pos refuse bad arguments before any device work (no GPU
needed): too many runs, a run table that breaks its rules, misaligned outputs, null pointers."""
import ctypes as C

import numpy as np

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first


def call(ent, rf, n_runs, keys=0x1000, kpos=0x2000, vals=0x3000, vpos=0x4000, src=0x5000,
         info=0x6000):
    rf = np.ascontiguousarray(rf, np.uint32)
    return _lib.lib().tpz_merge_runs(CTX, C.byref(ent), C.c_void_p(rf.ctypes.data), n_runs,
                                     C.c_void_p(keys), C.c_void_p(kpos), C.c_void_p(vals),
                                     C.c_void_p(vpos), C.c_void_p(src), C.c_void_p(info), None)


def test_merge_runs_argument_checks():
    ent = _lib.Entries(0x100, 0x200, 0x300, 0x400, 10, 64, 64)
    big = _lib.MERGE_MAX_RUNS + 1
    assert call(ent, [0] * big + [10], big) == _lib.ERR_INVALID_ARG
    for rf in ([1, 10], [0, 7, 5, 10], [0, 4, 9], [0, 4, 11]):
        assert call(ent, rf, len(rf) - 1) == _lib.ERR_INVALID_ARG, rf
    ok = [0, 4, 10]
    assert call(ent, ok, 2, keys=0x1001) == _lib.ERR_INVALID_ARG        # 16-byte columns
    assert call(ent, ok, 2, vals=0x3008) == _lib.ERR_INVALID_ARG
    assert call(ent, ok, 2, kpos=0x2004) == _lib.ERR_INVALID_ARG        # u64 positions
    assert call(ent, ok, 2, info=0x6004) == _lib.ERR_INVALID_ARG
    assert call(ent, ok, 2, src=0x5002) == _lib.ERR_INVALID_ARG         # u32 source column
    assert call(ent, ok, 2, info=0) == _lib.ERR_INVALID_ARG
    assert call(ent, ok, 2, kpos=0) == _lib.ERR_INVALID_ARG
    assert _lib.lib().tpz_merge_runs(None, C.byref(ent), None, 0, None, None, None, None, None,
                                     None, None) == _lib.ERR_INVALID_ARG


def test_flat_entry_pos_argument_checks():
    cols = _lib.FlatColumns(0x100, 0x200, 0, 0x400, 0x500, 0x600, 0x700, None, 0, 0x900, 0xA00)
    f = _lib.lib().tpz_flat_entry_pos
    assert f(CTX, C.byref(cols), 3, C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000),
             None) == _lib.ERR_INVALID_ARG                               # d_ends is NULL
    assert f(CTX, C.byref(cols), 0, None, C.c_void_p(0x2000), C.c_void_p(0x3000),
             None) == _lib.ERR_INVALID_ARG

"""tpz_entries_bound / tpz_table_cut / tpz_sst_finish refuse bad arguments before any device work
(no GPU needed), tpz_sst_image_bytes is the layout's arithmetic, and compact_task refuses the
bounds the reference panics on before it touches the device."""
import ctypes as C

import pytest

from topazdb_amd import _lib
from topazdb_amd.compact import compact_task
from topazdb_amd.table import ReferencePanic

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first
BAD = _lib.ERR_INVALID_ARG


def ent(n=10, kpos=0x200, vpos=0x400, keys=0x100):
    return _lib.Entries(keys, kpos, 0x300, vpos, n, 64, 64)


def bound(e=None, keys=0x1000, pos=0x2000, incl=0x3000, n=2, out=0x4000, ctx=CTX):
    return _lib.lib().tpz_entries_bound(ctx, C.byref(e or ent()), C.c_void_p(keys), C.c_void_p(pos),
                                        C.c_void_p(incl), n, C.c_void_p(out), None)


def test_entries_bound_argument_checks():
    assert bound(ctx=None) == BAD
    assert bound(pos=0) == BAD and bound(incl=0) == BAD and bound(out=0) == BAD
    assert bound(pos=0x2004) == BAD                                     # u64 positions
    assert bound(out=0x4002) == BAD                                     # u32 counts
    assert bound(ent(kpos=0)) == BAD and bound(ent(vpos=0)) == BAD
    assert bound(ent(kpos=0x204)) == BAD
    assert bound(ent(keys=0)) == BAD                                    # key bytes without a column
    assert bound(ent(n=0xFFFFFFFF)) == BAD
    assert _lib.lib().tpz_entries_bound(CTX, None, None, None, None, 0, None, None) == BAD
    assert bound(n=0) == _lib.SUCCESS                                   # no probes: nothing to do


def cut(e=None, start=2, win=4, seg_end=8, first=0x1000, ext=0x2000, cext=0x3000, info=0x4000,
        block_size=4096, capacity=1 << 26, out=0x5000, ctx=CTX):
    return _lib.lib().tpz_table_cut(ctx, C.byref(e or ent()), start, win, seg_end,
                                    C.c_void_p(first), C.c_void_p(ext), C.c_void_p(cext),
                                    C.c_void_p(info), block_size, capacity, C.c_void_p(out), None)


def test_table_cut_argument_checks():
    assert cut(ctx=None) == BAD and cut(out=0) == BAD and cut(out=0x5004) == BAD
    assert cut(capacity=0) == BAD                   # the reference builds an empty table and panics
    for bs in (0, 2, 65537, 1 << 20):               # tpz_plan_blocks' range is (2, 65536]
        assert cut(block_size=bs) == BAD, bs
    assert cut(seg_end=11) == BAD                                       # past the entries
    assert cut(start=9, win=0) == BAD                                   # starts past the range
    assert cut(start=2, win=7) == BAD                                   # window past the range
    for name in ("first", "ext", "cext", "info"):
        assert cut(**{name: 0}) == BAD, name
    assert cut(first=0x1002) == BAD and cut(info=0x4002) == BAD         # u32 columns
    assert cut(ext=0x2004) == BAD and cut(cext=0x3004) == BAD           # u64 columns
    assert cut(ent(vpos=0x404)) == BAD


def finish(e=None, images=0x1000, n=2, max_blocks=8, base=0x10000, span=1 << 20, info=0x2000,
           ctx=CTX):
    return _lib.lib().tpz_sst_finish(ctx, C.byref(e or ent()), C.c_void_p(images), n, max_blocks,
                                     C.c_void_p(base), span, C.c_void_p(info), None)


def test_sst_finish_argument_checks():
    assert finish(ctx=None) == BAD
    assert finish(images=0) == BAD and finish(base=0) == BAD and finish(info=0) == BAD
    assert finish(images=0x1004) == BAD and finish(info=0x2004) == BAD  # 8-byte descriptors, info
    assert finish(n=65536) == BAD                                       # a grid dimension
    assert finish(span=(1 << 35) + 1) == BAD                            # the range CRC's limit
    assert finish(ent(kpos=0)) == BAD
    assert finish(n=0) == _lib.SUCCESS                                  # no images: nothing to do


def test_sst_image_bytes():
    """data | metas (6 per block + the first keys) | meta offset | [filter | bloom offset] | CRC."""
    f = _lib.sst_image_bytes
    assert f(0, 0, 0, 0) == 8
    assert f(1000, 3, 30, 0) == 1000 + 18 + 30 + 4 + 4
    assert f(1000, 3, 30, 17) == 1000 + 18 + 30 + 4 + 17 + 4 + 4
    assert f(1 << 33, 1 << 20, 1 << 24, 1) == (1 << 33) + 6 * (1 << 20) + (1 << 24) + 4 + 5 + 4


def test_sst_image_struct_matches_the_header():
    """tpz_sst_image: 4 pointers, 2 u64 and 2 u32, no padding beyond natural alignment."""
    assert C.sizeof(_lib.SstImage) == 56
    assert _lib.SstImage.entry_base.offset == 36 and _lib.SstImage.d_filter.offset == 40


@pytest.mark.parametrize("bounds,what", [
    ([(None, (b"z", True))], "invalid lower"),              # Unbounded lower
    ([((b"a", False), (b"z", True))], "invalid lower"),     # Excluded lower
    ([(b"a", None)], "invalid upper"),                      # Unbounded upper
    ([(b"a", (b"m", False)), (b"m", None)], "invalid upper")])
def test_compact_task_refuses_the_bounds_the_reference_panics_on(bounds, what):
    """src/level.rs:190-193 and :199-205, checked before any device work (ctx is never used)."""
    with pytest.raises(ReferencePanic, match=what):
        compact_task(None, [], bounds)
    with pytest.raises(ValueError):
        compact_task(None, [], [(b"a", (b"z", True))], table_capacity=0)
    with pytest.raises(ValueError):
        compact_task(None, [], [(b"a", (b"z", True))], codec=4)

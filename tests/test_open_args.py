"""tpz_open_index / tpz_open_metas refuse bad arguments before any device work (no GPU needed),
n_files == 0 is valid, and tpz_open_scratch_bytes is the layout's arithmetic."""
import ctypes as C
import os
import re

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first
BAD = _lib.ERR_INVALID_ARG
SPAN = 1 << 20


def index(src=0x1000, span_bytes=SPAN, span=0x2000, n=3, info=0x3000, fb=0x4000, fk=0x5000,
          scratch=0x6000, scratch_bytes=None, ctx=CTX):
    sb = _lib.open_scratch_bytes(span_bytes, n) if scratch_bytes is None else scratch_bytes
    return _lib.lib().tpz_open_index(ctx, C.c_void_p(src), span_bytes, C.c_void_p(span), n,
                                     C.c_void_p(info), C.c_void_p(fb), C.c_void_p(fk),
                                     C.c_void_p(scratch), sb, None)


def metas(src=0x1000, span_bytes=SPAN, span=0x2000, n=3, info=0x3000, fb=0x4000, fk=0x5000,
          scratch=0x6000, scratch_bytes=None, ext=0x7000, pos=0x8000, keys=0x9001, block_cap=10,
          key_cap=100, ctx=CTX):
    sb = _lib.open_scratch_bytes(span_bytes, n) if scratch_bytes is None else scratch_bytes
    return _lib.lib().tpz_open_metas(ctx, C.c_void_p(src), span_bytes, C.c_void_p(span), n,
                                     C.c_void_p(info), C.c_void_p(fb), C.c_void_p(fk),
                                     C.c_void_p(scratch), sb, C.c_void_p(ext), C.c_void_p(pos),
                                     C.c_void_p(keys), block_cap, key_cap, None)


def test_open_index_argument_checks():
    assert index(ctx=None) == BAD
    for name in ("src", "span", "info", "fb", "fk", "scratch"):
        assert index(**{name: 0}) == BAD, name
    for name, p in (("span", 0x2004), ("info", 0x3004), ("fb", 0x4002), ("fk", 0x5001),
                    ("scratch", 0x6004)):
        assert index(**{name: p}) == BAD, name                           # u64 arrays: 8-byte
    assert index(src=0x1003, n=0) == _lib.SUCCESS                        # images: any address
    full = _lib.open_scratch_bytes(SPAN, 3)
    assert index(scratch_bytes=full - 1) == BAD and index(scratch_bytes=0) == BAD
    assert index(n=0x80000000) == BAD                                    # a grid dimension
    assert index(n=0) == _lib.SUCCESS                                    # no files: nothing to do
    assert index(n=0, scratch_bytes=_lib.open_scratch_bytes(SPAN, 0)) == _lib.SUCCESS


def test_open_metas_argument_checks():
    assert metas(ctx=None) == BAD
    for name in ("src", "span", "info", "fb", "fk", "scratch", "ext", "pos", "keys"):
        assert metas(**{name: 0}) == BAD, name
    for name, p in (("span", 0x2004), ("info", 0x3004), ("fb", 0x4002), ("fk", 0x5001),
                    ("scratch", 0x6004), ("ext", 0x7004), ("pos", 0x8002)):
        assert metas(**{name: p}) == BAD, name
    assert metas(scratch_bytes=_lib.open_scratch_bytes(SPAN, 3) - 16) == BAD
    assert metas(block_cap=2**64 - 2) == BAD                             # block_cap + n_files wraps
    assert metas(n=0) == _lib.SUCCESS


def test_open_scratch_bytes():
    """16 B per TPZ_OPEN_TILE of the span plus two tiles per file; the header's inline, the
    binding's copy and the exported constant agree."""
    f = _lib.open_scratch_bytes
    assert _lib.OPEN_TILE == 4096
    assert f(0, 0) == 0 and f(4095, 0) == 0 and f(4096, 0) == 16
    assert f(0, 1) == 32 and f(8191, 3) == (1 + 6) * 16
    assert f(518 << 20, 8) == ((518 << 20) // 4096 + 16) * 16
    hdr = open(_lib.HEADER).read()
    assert re.search(r"#define TPZ_OPEN_TILE 4096u", hdr)
    assert "(span_bytes / TPZ_OPEN_TILE + 2 * n_files) * 16" in hdr
    assert [_lib.OPEN_OK, _lib.OPEN_SHORT, _lib.OPEN_BLOOM_RANGE, _lib.OPEN_META_RANGE,
            _lib.OPEN_META_TRUNCATED, _lib.OPEN_BAD_EXTENTS, _lib.OPEN_NO_BLOCKS,
            _lib.OPEN_UNSUPPORTED] == [int(re.search(r"#define TPZ_OPEN_%s (\d+)" % n, hdr).group(1))
                                       for n in ("OK", "SHORT", "BLOOM_RANGE", "META_RANGE",
                                                 "META_TRUNCATED", "BAD_EXTENTS", "NO_BLOCKS",
                                                 "UNSUPPORTED")]
    assert os.path.exists(_lib.LIB_PATH)

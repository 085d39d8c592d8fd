"""tpz_mem_build and tpz_wal_entries refuse bad arguments before any device work (no GPU needed):
null and misaligned pointers, an unknown mode, PUT without versions. The constants are the header's
and the ABI version is unchanged."""
import ctypes as C
import re

from topazdb_amd import _lib

CTX = C.c_void_p(0x10)    # never dereferenced: every case fails its argument checks first

BUILD = dict(ver=0x900, okeys=0x5000, okpos=0x6000, ovals=0x7000, ovpos=0x8000, opre=0xA000,
             src=0xB000, over=0xC000, info=0xD000)
ENT = dict(keys=0x1000, kpos=0x2000, vals=0x3000, vpos=0x4000)


def build(mode=_lib.MEM_PUT, ctx=CTX, n=5, ent=None, no_entries=False, **over):
    e = dict(ENT, **(ent or {}))
    s = _lib.Entries(e["keys"], e["kpos"], e["vals"], e["vpos"], n, 40, 40)
    p = {k: (C.c_void_p(v) if v else None) for k, v in dict(BUILD, **over).items()}
    return _lib.lib().tpz_mem_build(ctx, None if no_entries else C.byref(s), mode, p["ver"],
                                    p["okeys"], p["okpos"], p["ovals"], p["ovpos"], p["opre"],
                                    p["src"], p["over"], p["info"], None)


def test_mem_build_argument_checks():
    assert build(ctx=None) == _lib.ERR_INVALID_ARG
    assert build(no_entries=True) == _lib.ERR_INVALID_ARG
    assert build(mode=2) == _lib.ERR_INVALID_ARG
    assert build(mode=0xFFFFFFFF) == _lib.ERR_INVALID_ARG
    assert build(ver=0) == _lib.ERR_INVALID_ARG                       # PUT without versions
    assert build(n=0xFFFFFFFF) == _lib.ERR_INVALID_ARG
    for name in ("okpos", "ovpos", "info", "okeys", "ovals"):
        assert build(**{name: 0}) == _lib.ERR_INVALID_ARG, name
        assert build(mode=_lib.MEM_REPLAY, **{name: 0}) == _lib.ERR_INVALID_ARG, name
    for name in ("okeys", "ovals"):                                   # 16-byte aligned
        assert build(**{name: BUILD[name] + 8}) == _lib.ERR_INVALID_ARG, name
    for name in ("ver", "okpos", "ovpos", "opre", "over", "info"):    # u64 columns
        assert build(**{name: BUILD[name] + 4}) == _lib.ERR_INVALID_ARG, name
    assert build(src=BUILD["src"] + 2) == _lib.ERR_INVALID_ARG        # u32 column
    for name in ("kpos", "vpos"):
        assert build(ent={name: ENT[name] + 4}) == _lib.ERR_INVALID_ARG, name
    for name in ("keys", "kpos", "vals", "vpos"):
        assert build(ent={name: 0}) == _lib.ERR_INVALID_ARG, name
        assert build(mode=_lib.MEM_REPLAY, ent={name: 0}) == _lib.ERR_INVALID_ARG, name


WAL = dict(img=0x1000, rec=0x2000, keys=0x3000, kpos=0x4000, vals=0x5000, vpos=0x6000, info=0x7000)


def wal(ctx=CTX, n=5, image_bytes=100, **over):
    p = {k: (C.c_void_p(v) if v else None) for k, v in dict(WAL, **over).items()}
    return _lib.lib().tpz_wal_entries(ctx, p["img"], image_bytes, p["rec"], n, p["keys"], p["kpos"],
                                      p["vals"], p["vpos"], p["info"], None)


def test_wal_entries_argument_checks():
    assert wal(ctx=None) == _lib.ERR_INVALID_ARG
    assert wal(n=0xFFFFFFFF) == _lib.ERR_INVALID_ARG
    for name in ("img", "rec", "keys", "kpos", "vals", "vpos", "info"):
        assert wal(**{name: 0}) == _lib.ERR_INVALID_ARG, name
    for name in ("keys", "vals"):
        assert wal(**{name: WAL[name] + 8}) == _lib.ERR_INVALID_ARG, name
    for name in ("rec", "kpos", "vpos", "info"):
        assert wal(**{name: WAL[name] + 4}) == _lib.ERR_INVALID_ARG, name


def test_constants_match_the_header_and_the_abi_stays():
    hdr = open(_lib.HEADER).read()
    for name, val in (("TPZ_HAS_MEM_BUILD", 1), ("TPZ_MEM_REPLAY", _lib.MEM_REPLAY),
                      ("TPZ_MEM_PUT", _lib.MEM_PUT), ("TPZ_WAL_END_IMAGE", _lib.WAL_END_IMAGE),
                      ("TPZ_WAL_END_EMPTY_KEY", _lib.WAL_END_EMPTY_KEY),
                      ("TPZ_WAL_TRUNCATED", _lib.WAL_TRUNCATED),
                      ("TPZ_ABI_VERSION", _lib.ABI_VERSION)):
        assert int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, hdr).group(1), 0) == val
    assert _lib.lib().tpz_abi_version() == 8
    for f in ("tpz_mem_build", "tpz_wal_index", "tpz_wal_entries"):
        assert f in _lib.header_functions() and hasattr(_lib.lib(), f)

"""tpz_decode_blocks_host / tpz_verify_blocks_host refuse bad arguments, and answer an empty
batch, before any device work (no GPU needed): null pointers, a capacity without its buffer,
decreasing extents, a snappy / lz4 batch without the decoded-extents or decoded-bytes output."""
import ctypes as C

import numpy as np

from topazdb_amd import _lib

CTX = 0x10    # never dereferenced: every case returns before the pipeline touches the context

BLOCKS = [b"\x00\x01" + b"x" * 9 + b"\x01", b"", b"y" * 20 + b"\x01"]
SNAPPY = BLOCKS[:2] + [b"\x03abc\x02"]           # the tag byte alone makes the batch a codec one
LZ4 = [b"\x03\x00\x00\x00\x30abc\x03"] + BLOCKS[1:]


def region(blocks, lead=0):
    src = np.frombuffer(b"\xee" * lead + b"".join(blocks), np.uint8).copy()
    ext = (lead + np.concatenate([[0], np.cumsum([len(b) for b in blocks])])).astype(np.uint64)
    return src, ext


class Outputs:
    """Real, writable outputs for n blocks (an accepted call would fill them)."""

    def __init__(self, n):
        self.a = {"data": np.zeros(4096, np.uint8), "ends": np.zeros(64, np.uint32),
                  "first": np.full(n + 1, 77, np.uint64), "count": np.zeros(n + 1, np.uint32),
                  "status": np.zeros(n + 1, np.uint8), "crc": np.zeros(n + 1, np.uint32),
                  "spill": np.zeros(256, np.uint8), "spill_off": np.zeros(n + 1, np.uint64),
                  "spill_used": np.full(1, 77, np.uint64), "dext": np.full(n + 1, 77, np.uint64),
                  "plain": np.zeros(256, np.uint8)}

    def ptr(self, name, null=()):
        return None if name in null else self.a[name].ctypes.data

    def columns(self, null=(), ends_cap=64, spill_cap=256):
        p = lambda name: self.ptr(name, null)   # noqa: E731
        return _lib.HostColumns(p("data"), p("ends"), ends_cap, p("first"), p("count"),
                                p("status"), p("crc"), p("spill"), spill_cap, p("spill_off"),
                                p("spill_used"), p("dext"), 4096)


def decode(src, ext, out, null=(), ctx=CTX, **caps):
    n = len(ext) - 1
    cols = out.columns(null, **caps)
    return _lib.lib().tpz_decode_blocks_host(
        C.c_void_p(ctx), C.c_void_p(None if "src" in null else src.ctypes.data),
        C.c_void_p(None if "ext" in null else ext.ctypes.data), n,
        None if "out" in null else C.byref(cols), 4)


def verify(src, ext, out, null=(), ctx=CTX, plain_cap=256):
    n = len(ext) - 1
    p = lambda name: C.c_void_p(out.ptr(name, null))   # noqa: E731
    return _lib.lib().tpz_verify_blocks_host(
        C.c_void_p(ctx), C.c_void_p(None if "src" in null else src.ctypes.data),
        C.c_void_p(None if "ext" in null else ext.ctypes.data), n, p("status"), p("crc"),
        p("count"), p("plain"), plain_cap, p("dext"), 4)


def test_decode_host_null_pointers():
    src, ext = region(BLOCKS)
    out = Outputs(3)
    assert decode(src, ext, out, ctx=None) == _lib.ERR_INVALID_ARG
    for name in ("ext", "out", "first", "count", "status", "crc", "spill_off", "spill_used",
                 "src", "data"):
        assert decode(src, ext, out, null=(name,)) == _lib.ERR_INVALID_ARG, name


def test_decode_host_capacity_without_buffer():
    src, ext = region(BLOCKS)
    out = Outputs(3)
    assert decode(src, ext, out, null=("ends",), ends_cap=2) == _lib.ERR_INVALID_ARG
    assert decode(src, ext, out, null=("spill",), spill_cap=1) == _lib.ERR_INVALID_ARG


def test_verify_host_null_pointers():
    src, ext = region(BLOCKS)
    out = Outputs(3)
    assert verify(src, ext, out, ctx=None) == _lib.ERR_INVALID_ARG
    for name in ("ext", "status", "crc", "count", "src"):
        assert verify(src, ext, out, null=(name,)) == _lib.ERR_INVALID_ARG, name
    assert verify(src, ext, out, null=("plain",), plain_cap=1) == _lib.ERR_INVALID_ARG


def test_decreasing_extents():
    src, _ = region(BLOCKS)
    out = Outputs(3)
    for ext in ([0, 12, 11, 33], [5, 0, 12, 33], [0, 12, 33, 32]):
        e = np.array(ext, np.uint64)
        assert decode(src, e, out) == _lib.ERR_INVALID_ARG, ext
        assert verify(src, e, out) == _lib.ERR_INVALID_ARG, ext


def test_codec_batch_needs_its_outputs():
    for blocks in (SNAPPY, LZ4):
        src, ext = region(blocks)
        out = Outputs(3)
        assert decode(src, ext, out, null=("dext",)) == _lib.ERR_INVALID_ARG
        assert verify(src, ext, out, null=("dext",)) == _lib.ERR_INVALID_ARG
        assert verify(src, ext, out, null=("plain",), plain_cap=0) == _lib.ERR_INVALID_ARG


def test_empty_batch():
    """n == 0 is a success that needs no source and no data buffer: no pairs, no spill bytes,
    and the decoded extents start where the caller's do."""
    ext = np.array([1000], np.uint64)
    out = Outputs(0)
    assert decode(None, ext, out, null=("src", "data", "ends", "spill"), ends_cap=0,
                  spill_cap=0) == _lib.SUCCESS
    assert out.a["first"][0] == 0 and out.a["spill_used"][0] == 0 and out.a["dext"][0] == 1000
    out = Outputs(0)
    assert verify(None, ext, out, null=("src", "plain"), plain_cap=0) == _lib.SUCCESS
    assert out.a["dext"][0] == 1000
    assert verify(None, ext, out, null=("src", "plain", "dext"), plain_cap=0) == _lib.SUCCESS

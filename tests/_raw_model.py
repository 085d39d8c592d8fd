"""A Python restatement of the in-place block view (csrc/tpz_raw_dev.h RawView) and of
tpz_raw_verify's rule (test infrastructure, CPU only): what the device reads from the bytes of an
Uncompress block payload | crc u32 BE | tag, with the reference's reads
(src/block.rs:46-59, src/block/compress.rs:95-113, src/block/iterator.rs:63-109).
tests/test_raw_model.py pins it against the oracle."""
from __future__ import annotations

import struct
import zlib

from topazdb_amd import _lib

OK, BAD_VALUE, BAD_KEY = _lib.ENTRY_OK, _lib.ENTRY_BAD_VALUE, _lib.ENTRY_BAD_KEY


def be16(b: bytes, at: int) -> int:
    return struct.unpack_from(">H", b, at)[0]


def verify(blk: bytes) -> tuple[int, int]:
    """tpz_raw_verify for one block: (status, crc). The tag dispatch, the CRC over the payload,
    n and the n offsets readable; no entry is read."""
    n = len(blk)
    if n == 0:
        return _lib.BLOCK_EMPTY, 0                                   # compress.rs:96-98
    tag = blk[-1]
    if tag == 0 or tag > 3:
        return _lib.BLOCK_BAD_TAG, 0                                 # :44-53, :102
    if tag != 1:
        return _lib.BLOCK_UNSUPPORTED_CODEC, 0                       # the codec step comes first
    if n - 1 < 4:
        return _lib.BLOCK_MALFORMED, 0                               # block.rs:49
    p = n - 5
    crc = zlib.crc32(blk[:p])
    if crc != struct.unpack_from(">I", blk, p)[0]:
        return _lib.BLOCK_CHECKSUM_MISMATCH, crc                     # checksum.rs:17-21
    if p < 2 or p < 2 + 2 * be16(blk, 0):
        return _lib.BLOCK_MALFORMED, crc                             # block.rs:54-59
    return _lib.BLOCK_OK, crc


class RawView:
    """The view of a block tpz_raw_verify reports OK."""

    def __init__(self, blk: bytes):
        self.blk = blk
        self.n = be16(blk, 0)
        self.data = blk[2 + 2 * self.n:len(blk) - 5]
        self.dl = len(self.data)

    def off(self, j: int) -> int:
        return be16(self.blk, 2 + 2 * j)

    def _key_at(self, j: int):
        o = self.off(j)
        if o + 2 > self.dl:
            return None
        kl = be16(self.data, o)
        if o + 2 + kl > self.dl:
            return None
        return o, kl

    def key_panics(self, j: int) -> bool:
        return self._key_at(j) is None

    def seek_panics(self, j: int) -> bool:
        k = self._key_at(j)
        if k is None:
            return True
        v = k[0] + 2 + k[1]
        if v + 2 > self.dl:
            return True
        return v + 2 + be16(self.data, v) > self.dl

    def entry_class(self, j: int) -> int:
        return BAD_KEY if self.key_panics(j) else BAD_VALUE if self.seek_panics(j) else OK

    def entry_key(self, j: int) -> bytes:
        k = self._key_at(j)
        return b"" if k is None else self.data[k[0] + 2:k[0] + 2 + k[1]]

    def entry_value(self, j: int) -> bytes:
        if self.seek_panics(j):
            return b""
        o, kl = self._key_at(j)
        v = o + 2 + kl
        return self.data[v + 2:v + 2 + be16(self.data, v)]

"""What LevelController::get answers, restated twice, and host-side table builders for the get
tests (test infrastructure, CPU only).

`level_get` follows the reference's routine (src/level.rs:427-465) line by line over the facade's
host objects: SsTable.may_contain, SsTable.smallest_key and SsTableIterator.
create_and_seek_to_key, which tests/test_table_host.py pins to the oracle. It returns what
tpz_get_keys reports for the query (include/tpz_gpu.h), the value included. `closed_get` is the
closed form for honest table sets: the value in the first table that holds the key, in priority
order, a tombstone giving None. tests/test_get_model.py checks that the two agree; the GPU tests
compare the device against `level_get`.

Tables are built on the host: tpz_build_blocks for the data region, BlockMeta.encode_block_meta
and Bloom.from_keys over the library's xxh3_64 for the tail; the blocks of the host SsTable are
decoded by the oracle, as tests/test_table_host.py host_table() does.
"""
from __future__ import annotations

import bisect
import re
import struct
import zlib
from collections import namedtuple

import numpy as np

import _oracle as O
from topazdb_amd import _lib, synth
from topazdb_amd.table import (Block, BlockError, BlockIterator, BlockMeta, Bloom, FileObject,
                               ReferencePanic, SsTable, SsTableIterator, _status_error)

ABSENT, FOUND, DELETED, ERROR = _lib.GET_ABSENT, _lib.GET_FOUND, _lib.GET_DELETED, _lib.GET_ERROR
NONE = _lib.GET_NONE

# tpz_get_keys' outputs for one query, plus the value (b"" unless FOUND)
Get = namedtuple("Get", "result status table block entry value")


def _err_status(e: Exception) -> int:
    """The tpz_block_status behind an exception of the facade (table.py _status_error)."""
    if isinstance(e, ReferencePanic):
        return _lib.BLOCK_MALFORMED
    msg = str(e)
    if msg.startswith("checksum: expected"):
        return _lib.BLOCK_CHECKSUM_MISMATCH
    for st in (_lib.BLOCK_EMPTY, _lib.BLOCK_BAD_TAG, _lib.BLOCK_UNSUPPORTED_CODEC,
               _lib.BLOCK_SPILL_FULL, _lib.BLOCK_CODEC_ERROR):
        if msg == _lib.format_block_error(st):
            return st
    raise AssertionError(msg)


def seek_failure(table: SsTable, key: bytes) -> tuple[int, int, int]:
    """(block, entry, status) where SsTableIterator::create_and_seek_to_key(table, key) fails, as
    tpz_seek_keys reports it: the block whose read is an Err or a panic (entry 0), or the entry
    whose read panics (iterator.rs:74-82, :95-98)."""
    if not table.block_metas:                                # block_metas[0]
        return 0, 0, _lib.BLOCK_MALFORMED
    idx = table.find_block_idx(key)
    for step in (0, 1):
        blk = table._blocks[idx]
        if isinstance(blk, Exception):
            return idx, 0, _err_status(blk)
        it = BlockIterator(blk)
        try:
            if step == 0:
                it.seek_to_key(key)
            else:
                it.seek_to_first()
        except ReferencePanic as e:
            return idx, int(re.match(r"entry (\d+) of", str(e)).group(1)), _lib.BLOCK_MALFORMED
        idx += 1
    raise AssertionError("the seek did not fail")


def level_get(levels: list[list[SsTable]], key: bytes) -> Get:
    """LevelController::get (src/level.rs:427-465). `levels[0]` is L0 in push order; the table
    index reported is the table's position in the concatenation of the levels."""
    first = [0]
    for lv in levels:
        first.append(first[-1] + len(lv))

    def try_table(t: int, table: SsTable):
        try:
            if not table.may_contain(key):                                   # :431 / :453
                return None
        except (IndexError, ZeroDivisionError):                              # bloom.rs:72-84 panics
            return Get(ERROR, _lib.BLOCK_MALFORMED, t, NONE, NONE, b"")
        try:
            it = SsTableIterator.create_and_seek_to_key(table, key)          # :434 / :456 (`?`)
        except (BlockError, ReferencePanic):
            b, e, st = seek_failure(table, key)
            return Get(ERROR, st, t, b, e, b"")
        if it.is_valid() and it.key() == key:                                # :435 / :457
            if len(it.value()) == 0:                                         # :436-438
                return Get(DELETED, _lib.BLOCK_OK, t, it.idx, it.block_iter.idx, b"")
            return Get(FOUND, _lib.BLOCK_OK, t, it.idx, it.block_iter.idx, it.value())  # :439
        return None

    tables = levels[0] if levels else []                                     # :428
    if tables:                                                               # :429
        for j in reversed(range(len(tables))):                               # :430 iter().rev()
            r = try_table(first[0] + j, tables[j])
            if r is not None:
                return r
    for i in range(1, len(levels)):                                          # :444
        tables = levels[i]                                                   # :445
        if not tables:                                                       # :446-448
            continue
        # :449-451 partition_point(|table| table.smallest_key <= key).saturating_sub(1)
        lo, hi = 0, len(tables)
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if tables[mid].smallest_key <= key:
                lo = mid + 1
            else:
                hi = mid
        idx = max(lo - 1, 0)
        r = try_table(first[i] + idx, tables[idx])                           # :452-462
        if r is not None:
            return r
    return Get(ABSENT, _lib.BLOCK_OK, NONE, NONE, NONE, b"")                 # :464


def closed_get(levels: list[list[list[tuple[bytes, bytes]]]], key: bytes):
    """Honest table sets (every table sorted by key without repeats, its filter built from its
    keys, the tables of a level below L0 disjoint and in key order): the value of `key` in the
    first table that holds it, L0's tables newest first and then the levels in order; an empty
    value there, or no table, gives None."""
    order = list(reversed(levels[0])) if levels else []
    for lv in levels[1:]:
        order += lv
    for ents in order:
        ks = [k for k, _ in ents]
        j = bisect.bisect_left(ks, key)
        if j < len(ks) and ks[j] == key:
            return ents[j][1] or None
    return None


# ------------------------------------------------------------------------------- builders
def data_region(ents: list[tuple[bytes, bytes]], block_size: int):
    """tpz_build_blocks over the entries: (region uint8 array, ext)."""
    ks, vs = [k for k, _ in ents], [v for _, v in ents]
    kpos = np.zeros(len(ents) + 1, np.uint64)
    vpos = np.zeros(len(ents) + 1, np.uint64)
    np.cumsum([len(k) for k in ks], out=kpos[1:])
    np.cumsum([len(v) for v in vs], out=vpos[1:])
    keys = np.frombuffer(b"".join(ks) or b"\0", np.uint8)
    vals = np.frombuffer(b"".join(vs) or b"\0", np.uint8)
    return synth.build_blocks(keys, kpos, vals, vpos, block_size)


def bloom_of(keys: list[bytes], fpp: float) -> bytes:
    """SsTableBuilder::build_bloom (builder.rs:132-141): Bloom::from_keys over xxh3_64."""
    return Bloom.from_keys([_lib.xxh3_64(k) for k in keys], fpp).encode()


class Pieces:
    """A table as the parts SsTable::open reads: the data region, its block extents, the block
    metas' first keys and the filter (None: the file has none)."""

    def __init__(self, region, ext, first_keys, bloom, ents=None):
        self.region = bytes(region)
        self.ext = np.asarray(ext, np.uint64)
        self.first_keys = list(first_keys)
        self.bloom = bloom
        self.ents = ents

    def image(self) -> bytes:
        """The SST file (builder.rs:97-141, file_object.rs:33-48)."""
        metas = [BlockMeta(int(self.ext[b]), fk) for b, fk in enumerate(self.first_keys)]
        data = self.region + BlockMeta.encode_block_meta(metas) + struct.pack(">I", len(self.region))
        # the bloom section and its offset; an empty section reads as no filter (table.rs:75-87)
        data += (self.bloom or b"") + struct.pack(">I", len(data))
        return data + struct.pack(">I", zlib.crc32(data))

    @staticmethod
    def from_image(f: bytes) -> "Pieces":
        """The parts of an SST file, read as SsTable::open reads them (table.rs:75-112)."""
        fo = FileObject("image", f)
        offset, bloom = SsTable._read_bloom(fo)
        meta_off = int.from_bytes(fo.read(offset - 4, 4), "big")
        metas = BlockMeta.decode_block_meta(fo.read(meta_off, offset - 4 - meta_off))
        return Pieces(f[:meta_off], [m.offset for m in metas] + [meta_off],
                      [m.first_key for m in metas], None if bloom is None else bloom.filter)

    def host_table(self, id: int = 0) -> SsTable:
        """SsTable::open's host side with the blocks decoded by the oracle: a Block, or the
        exception the reference's read_block raises for the block's status."""
        src = np.frombuffer(self.region, np.uint8)
        d = O.decode_batch(src, self.ext)
        blocks = []
        for b in range(len(self.ext) - 1):
            st = int(d.status[b])
            if st in (O.OK, O.BAD_ENTRY):
                blocks.append(Block.from_dense(d, b, int(self.ext[b + 1] - self.ext[b]) - 5))
            else:
                blocks.append(_status_error(st, int(d.crc_expected[b]), int(d.crc_actual[b])))
        metas = [BlockMeta(int(self.ext[b]), fk) for b, fk in enumerate(self.first_keys)]
        fo = FileObject("t%d" % id, self.region + b"\0\0\0\0")
        t = SsTable(id, fo, metas, len(self.region), None if self.bloom is None else Bloom(self.bloom),
                    blocks)
        if metas:
            t.smallest_key = metas[0].first_key              # table.rs:143-151 (the half get uses)
        return t


def build_pieces(ents: list[tuple[bytes, bytes]], block_size: int, fpp: float | None = 0.1,
                 codec: str | None = None) -> Pieces:
    """A table of the sorted entries `ents` (fpp None: no filter; codec "snappy" / "lz4": the
    blocks re-encoded with compress::encode)."""
    src, ext = data_region(ents, block_size)
    d = O.decode_batch(src, ext)
    assert (d.status == O.OK).all()
    first_keys = [d.entries(b)[0][0] for b in range(len(ext) - 1)]
    if codec == "snappy":
        src, ext = synth.snappy_blocks(src, ext)
    elif codec == "lz4":
        src, ext = synth.lz4_blocks(src, ext)
    bloom = None if fpp is None else bloom_of([k for k, _ in ents], fpp)
    return Pieces(src.tobytes(), ext, first_keys, bloom, ents)


# ------------------------------------------------------------------------------- inputs
def key_of(i: int) -> bytes:
    return b"key_%04d" % i                       # src/level/test.rs:17-19


def value_of(i: int, info: str) -> bytes:
    return b"value_%04d_%s" % (i, info.encode())  # :21-23


def reference_cases() -> dict:
    """The four get tests of src/level/test.rs:117-183 as (L0 tables in push order, [(key,
    expected Option)]): ten keys, block size 64."""
    def tab(info):
        return [(key_of(i), b"" if info is None else value_of(i, info)) for i in range(10)]
    keys = [key_of(i) for i in range(10)]
    return {
        "get_simple_key": ([tab("")], [(k, value_of(i, "")) for i, k in enumerate(keys)]),
        "get_simple_not_exist_empty": ([], [(b"aaaaa", None)]),
        "get_simple_not_exist": ([tab("")], [(b"aaaaa", None)]),
        "get_key_new_old": ([tab("old"), tab("new")],
                            [(k, value_of(i, "new")) for i, k in enumerate(keys)]),
        "get_key_delete": ([tab("old"), tab(None)], [(k, None) for k in keys]),
    }


def random_key(rng, alphabet: bytes, max_len: int) -> bytes:
    return bytes(rng.choice(alphabet) for _ in range(rng.randint(1, max_len)))


def random_set(rng, l0: int, lower: list[int], per_table: int, alphabet: bytes = b"ab\x00\xff",
               max_len: int = 3, tomb: float = 0.2, pool: int | None = None, min_keys: int = 1):
    """An honest table set as entry lists: `l0` overlapping L0 tables, then one level of disjoint
    tables in key order per entry of `lower` (its table count; 0: an empty level). Every table
    holds min_keys to per_table sorted distinct keys, drawn from a pool of `pool` random keys when one
    is asked for (long keys then still repeat across tables); a value names its level and table,
    or is empty (a tombstone) with probability `tomb`. `rng` is a random.Random."""
    source = None if pool is None else sorted({random_key(rng, alphabet, max_len)
                                               for _ in range(pool)})

    def table(lv, t, keys):
        return [(k, b"" if rng.random() < tomb else b"%d.%d=" % (lv, t) + k) for k in keys]

    def keys(n, half=False):
        if source is not None:     # (a level takes at most half the pool: the next one is reached)
            return sorted(rng.sample(source, min(n, len(source) // 2 if half else len(source))))
        return sorted({random_key(rng, alphabet, max_len) for _ in range(n)})

    levels = [[table(0, t, ks) for t in range(l0) for ks in [keys(rng.randint(min_keys, per_table))]]]
    for lv, nt in enumerate(lower, 1):
        ks = keys(per_table * max(nt, 1), half=True)
        nt = min(nt, len(ks))                     # every table holds a key
        cuts = [len(ks) * t // nt for t in range(nt + 1)] if nt else []
        levels.append([table(lv, t, ks[cuts[t]:cuts[t + 1]]) for t in range(nt)])
    return levels

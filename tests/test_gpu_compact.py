"""The device compaction path: tpz_flat_entry_pos (flat columns -> tpz_entries) against the flat
decode's own dense view, and compact() (decode -> merge -> plan -> encode -> compress, entries
staying in HBM) against the host builder over the merge model's entries."""
import random

import numpy as np
import pytest
import torch

import _oracle as O
import badentry_util as BU
from _merge_model import merge_rule, merged_entries
from test_encode_host import pack
from topazdb_amd import _lib, synth
from topazdb_amd.batch import DeviceBatch, decode_flat, decompress_batch
from topazdb_amd.compact import compact, entries_from_flat
from topazdb_amd.table import BlockError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def ents(lo: int, n: int):
    return [(BU.key(i), BU.val(i)) for i in range(lo, lo + n)]


def mixed_batch(order):
    """Blocks by kind: "ok" (BlockBuilder's layout), "crc" (one payload byte flipped: checksum
    mismatch, decodes nothing, keeps its reservation) and "bad" (entry 1's value unreadable under
    a valid CRC: TPZ_BLOCK_BAD_ENTRY)."""
    blocks, i = [], 0
    for kind in order:
        e = ents(i, 5 + len(blocks))
        i += len(e)
        if kind == "bad":
            blocks.append(BU.bad_block(e, 1, "value"))
        else:
            b = bytearray(BU.raw_block(*BU.entries_block(e)))
            if kind == "crc":
                b[len(b) // 2] ^= 0x20
            blocks.append(bytes(b))
    ext = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
    return np.frombuffer(b"".join(blocks), np.uint8), ext


@pytest.mark.parametrize("order,first_bad", [
    (["ok", "ok", "bad", "ok", "crc", "ok"], 2), (["ok", "crc", "crc", "bad"], 1),
    (["crc"], 0), (["ok", "ok", "ok"], -1), ([], -1)])
def test_entries_from_flat(ctx, order, first_bad):
    src, ext = mixed_batch(order)
    cols = decode_flat(ctx, DeviceBatch(src, ext)).complete()
    d = cols.dense()
    ent = entries_from_flat(ctx, cols, check=False)
    assert ent.bad_block == first_bad
    nb = len(order)
    first = cols.first.cpu().numpy()
    kpos, vpos = ent.kpos.cpu().numpy(), ent.vpos.cpu().numpy()
    keys, vals = cols.keys.cpu().numpy(), cols.values.cpu().numpy()
    assert ent.n == int(first[0][nb]) == len(kpos) - 1
    assert kpos[-1] == first[1][nb] and vpos[-1] == first[2][nb]      # the column totals
    assert (np.diff(kpos) >= 0).all() and (np.diff(vpos) >= 0).all()
    for b, kind in enumerate(order):
        e0, n = int(first[0][b]), int(first[0][b + 1] - first[0][b])
        assert n == 5 + b                                               # the header's n slots
        if kind == "crc":
            # decoded nothing: the first slot owns the block's reserved bytes, the others are empty
            assert d.count[b] == 0
            assert kpos[e0] == first[1][b] and (kpos[e0 + 1:e0 + n + 1] == first[1][b + 1]).all()
            assert vpos[e0] == first[2][b] and (vpos[e0 + 1:e0 + n + 1] == first[2][b + 1]).all()
            continue
        got = [(keys[kpos[e]:kpos[e + 1]].tobytes(), vals[vpos[e]:vpos[e + 1]].tobytes())
               for e in range(e0, e0 + n)]
        assert got == d.entries(b)
        if kind == "bad":
            assert got[1][0] == BU.key(e0 + 1) and got[1][1] == b""      # unreadable value: empty
    if first_bad >= 0:
        with pytest.raises(BlockError) as e:
            entries_from_flat(ctx, cols)
        assert e.value.block == first_bad
    else:
        assert entries_from_flat(ctx, cols).n == ent.n


def overlapping_tables(seed: int, n: int = 1500, tables: int = 3):
    """Sorted tables (three unless told otherwise) over one key space: about half of each table's
    keys are in another table too; some values are tombstones."""
    rng = random.Random(seed)
    space = [b"user%07d" % i + bytes([0x80 + i % 100]) * (i % 9) for i in range(3 * n)]
    runs = []
    for t in range(tables):
        keys = sorted(rng.sample(space, n))
        runs.append([(k, b"" if rng.random() < 0.1 else (b"t%d-" % t + k) * rng.randint(1, 5))
                     for k in keys])
    return runs


def table_region(run, block_size: int, codec: int = 1):
    """A table's data region from the host builder, its blocks under `codec` (1 plain, 2 snappy,
    3 lz4). A table of no entries has no blocks."""
    if not run:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    src, ext = synth.build_blocks(*pack(run), block_size)
    if codec == 2:
        src, ext = synth.snappy_blocks(src, ext)
    elif codec == 3:
        src, ext = synth.lz4_blocks(src, ext)
    return src, ext


def assert_compacted(ctx, out, runs, block_size: int, codec: int):
    """compact()'s output over the tables `runs` is the host builder's over the merge model's
    entries: first entries, extents and region bytes (through the device codec for tags 2, 3)."""
    want = merged_entries(runs)
    assert out.entries.n == len(want) < sum(len(r) for r in runs)
    w_region, w_ext = synth.build_blocks(*pack(want), block_size)
    o_region, o_ext, w_first = O.build_blocks(*pack(want), block_size)
    assert o_ext.tolist() == w_ext.tolist() and o_region.tobytes() == w_region.tobytes()
    assert out.n_blocks == len(w_ext) - 1
    assert out.first.cpu().numpy().tolist() == w_first.astype(np.int64).tolist()
    region, ext = out.region, out.ext
    if codec != 1:
        tags = region[(ext[1:] - 1)].cpu().numpy()
        assert (tags == codec).all()
        plain, st = decompress_batch(ctx, DeviceBatch(region, ext))
        torch.cuda.synchronize()
        assert (st[:out.n_blocks].cpu().numpy() == _lib.BLOCK_OK).all()
        region, ext = plain.src[:plain.src_bytes], plain.ext
    assert ext.cpu().numpy().view(np.uint64).tolist() == w_ext.tolist()
    assert region.cpu().numpy().tobytes() == w_region.tobytes()
    return want


@pytest.mark.parametrize("codec", [1, 2, 3])
@pytest.mark.parametrize("snappy_inputs", [False, True, "mixed"])
@pytest.mark.parametrize("block_size", [256, 4096])
def test_compact_three_tables(ctx, block_size, snappy_inputs, codec):
    """Inputs all plain, tables 0 and 2 as snappy, or mixed (table 0 lz4, table 1 plain, table 2
    snappy); outputs plain, snappy and lz4."""
    runs = overlapping_tables(block_size + codec)
    in_codecs = {False: (1, 1, 1), True: (2, 1, 2), "mixed": (3, 1, 2)}[snappy_inputs]
    regions = [table_region(run, block_size, c) for run, c in zip(runs, in_codecs)]
    for (src, ext), c in zip(regions, in_codecs):
        assert (src[ext[1:].astype(np.int64) - 1] == c).all()          # every block's tag
    out = compact(ctx, regions, block_size=block_size, codec=codec)
    assert_compacted(ctx, out, runs, block_size, codec)


@pytest.mark.parametrize("block_size", [256, 4096])
def test_compact_six_tables_one_empty_one_shadowed(ctx, block_size):
    """Six tables: table 2 has no blocks at all (an empty run in the middle), every key of
    table 3 is in table 0 or 1 (it contributes nothing), the others overlap."""
    five = overlapping_tables(block_size + 6, n=900, tables=5)
    rng = random.Random(block_size)
    earlier = sorted(set(k for run in five[:2] for k, _ in run))
    shadowed = [(k, b"shadowed-" + k) for k in sorted(rng.sample(earlier, 700))]
    runs = [five[0], five[1], [], shadowed, five[2], five[3]]
    assert len(runs) == 6 and not any(r == 3 for r, _ in merge_rule(runs))
    regions = [table_region(run, block_size) for run in runs]
    assert len(regions[2][1]) == 1 and all(len(ext) > 2 for i, (_, ext) in enumerate(regions) if i != 2)
    out = compact(ctx, regions, block_size=block_size, codec=1)
    want = assert_compacted(ctx, out, runs, block_size, 1)
    assert not any(v.startswith(b"shadowed-") for _, v in want)


def long_entry_tables(seed: int, n: int = 400):
    """Three sorted tables of n entries over 3n / 2 keys of 20..300 bytes; values of 0..3,000
    bytes, about one in ten a tombstone."""
    rng = random.Random(seed)
    space = [b"%07d/" % i + bytes((i * 31 + j) & 0xFF for j in range(12 + (i * 37) % 281))
             for i in range(3 * n // 2)]
    assert min(map(len, space)) == 20 and max(map(len, space)) == 300
    runs = []
    for t in range(3):
        keys = sorted(rng.sample(space, n))
        runs.append([(k, b"" if rng.random() < 0.1 else
                      ((b"t%d:" % t + k[:24]) * 130)[:rng.randint(0, 3000)]) for k in keys])
    return runs


@pytest.mark.parametrize("codec", [1, 2])
def test_compact_64k_blocks_long_entries(ctx, codec):
    """65,536-byte blocks of long entries: keys and values past the merge's lane-copy limit (the
    whole wave copies them) on their way through compact()."""
    runs = long_entry_tables(codec)
    want = merged_entries(runs)
    lane = _lib.MERGE_LANE_COPY_MAX
    assert sum(len(k) > lane for k, _ in want) > 20 and sum(len(v) > lane for _, v in want) > 200
    assert sum(len(k) <= lane for k, _ in want) > 200 and sum(v == b"" for _, v in want) > 20
    regions = [table_region(run, 65536) for run in runs]
    out = compact(ctx, regions, block_size=65536, codec=codec)
    assert_compacted(ctx, out, runs, 65536, codec)


def test_compact_no_inputs_and_a_failing_block(ctx):
    out = compact(ctx, [])
    assert out.n_blocks == 0 and out.region.numel() == 0 and out.entries.n == 0
    src, ext = synth.build_blocks(*pack(ents(0, 200)), 256)
    src = src.copy()
    src[int(ext[3]) + 9] ^= 1                                           # block 3 fails its CRC
    with pytest.raises(BlockError) as e:
        compact(ctx, [(src, ext)], block_size=256)
    assert e.value.block == 3

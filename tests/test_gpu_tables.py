"""compact_task on the device (tpz_entries_bound, tpz_table_cut, tpz_sst_finish): a task's input
tables in, the reference's list of SST file images out.

Codec 1 is checked byte for byte: the table cuts against tests/_tables_model.py, every image
against table.SsTableBuilder.build_image() over that table's entries (the path the golden SSTs pin)
plus the big-endian tpz_host_crc32. Codecs 2 and 3 write their own streams, so the cut rule is
checked on the stored sizes read from each image's metas, and the blocks after the device codec
step against the host builder. Inputs: overlapping_tables (3 x 1,500 entries) at block sizes 256
and 4096, long_entry_tables at 65536."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

import _oracle as O
import _tables_model as M
from test_gpu_compact import long_entry_tables, overlapping_tables, table_region
from topazdb_amd import _lib, synth
from topazdb_amd.batch import DeviceBatch, decompress_batch
from topazdb_amd.compact import TableDesc, compact_task, entries_bound, sub_ranges
from topazdb_amd.encode import DeviceEntries
from topazdb_amd.levels import DeviceLevels
from topazdb_amd.table import FileObject, SsTable, SsTableBuilder

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [256, 4096, 65536]


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(block_size: int):
    """(runs, regions, merged entries, the task's sub_ranges) for a block size, computed once.
    The task: table 0 is the L0 table, tables 1 and 2 are the next level's, each stored as three
    tables of 500 consecutive entries (RwsSlice cuts only at table boundaries: with three whole
    tables every cut point lies at an end of the key space). Seven input tables, in priority
    order; their merge is the merge of the three runs."""
    runs = long_entry_tables(7) if block_size == 65536 else overlapping_tables(block_size)
    tables = [runs[0]]
    for run in runs[1:]:
        n = len(run) // 3
        tables += [run[:n], run[n:2 * n], run[2 * n:]]
    regions = [table_region(t, block_size) for t in tables]
    descs = []
    for t, (_, ext) in zip(tables, regions):
        _, _, first = O.build_blocks(*M.pack(t), block_size)
        descs.append(TableDesc(t[0][0], t[-1][0], [t[int(f)][0] for f in first[:-1]],
                               ext[:-1], int(ext[-1])))
    bounds = sub_ranges(descs[:1], descs[1:], 0)
    assert 3 <= len(bounds) <= 4
    merged = M.merged_entries(runs)
    assert merged == M.merged_entries(tables)
    return tables, regions, merged, bounds


def host_crc32(b: bytes) -> int:
    f = _lib.lib().tpz_host_crc32
    f.argtypes, f.restype = [C.c_char_p, C.c_uint64], C.c_uint32
    return f(b, len(b))


@functools.lru_cache(maxsize=None)
def _want(block_size: int, fpp: float, t0: int, n: int, ctx) -> bytes:
    b = SsTableBuilder(ctx, block_size, fpp)
    for k, v in inputs(block_size)[2][t0:t0 + n]:
        b.add(k, v)
    img = b.build_image()
    return img + struct.pack(">I", host_crc32(img))


def images_of(out) -> list[bytes]:
    """Every image as host bytes, from one copy of the used part of the arena."""
    if not out:
        return []
    base = out.arena.data_ptr()
    offs = [t.image.data_ptr() - base for t in out]
    assert all(o % 256 == 0 for o in offs)                       # image starts: 256-byte aligned
    assert all(a + t.size <= b for a, b, t in zip(offs, offs[1:], out))   # disjoint, in key order
    host = out.arena[:offs[-1] + out[-1].size].cpu().numpy()
    return [host[o:o + t.size].tobytes() for o, t in zip(offs, out)]


def check_ranges(out, want_tables):
    assert [(t.first_entry, t.n_entries, t.n_blocks) for t in out] == \
        [(t0, n, len(firsts)) for t0, n, firsts in want_tables]


def check_images(ctx, out, block_size, fpp):
    imgs = images_of(out)
    for t, img in zip(out, imgs):
        want = _want(block_size, fpp, t.first_entry, t.n_entries, ctx)
        assert t.size == len(want) and img == want, (t.first_entry, t.n_entries)
        assert t.meta_off == struct.unpack(">I", img[t.bloom_off - 4 if t.bloom_off else -8:][:4])[0]
        assert (t.bloom_off is None) == (fpp < 0 or str(fpp) == "-0.0")
    return imgs


def check_opens(ctx, out, imgs, merged):
    """With a bloom section the files open: the whole-file CRC (one batch), SsTable.open (every
    table up to 64 of them, evenly spaced ones and the last beyond that: an open decodes the table),
    and the oracle's parse and iterator yield the table's entries."""
    files = FileObject.open_many([(f"t{i}", img) for i, img in enumerate(imgs)], ctx)
    step = max(1, len(out) // 64)
    for i, (t, img) in enumerate(zip(out, imgs)):
        ext, meta_off, bloom_off = O.sst_parse(img)
        assert (len(ext) - 1, meta_off, bloom_off) == (t.n_blocks, t.meta_off, t.bloom_off)
        it = O.SstIter(img)
        it.seek_to_first()
        got = []
        while it.is_valid():
            got.append((it.key(), it.value()))
            it.next()
        assert got == merged[t.first_entry:t.first_entry + t.n_entries]
        if i % step == 0 or i + 1 == len(out):
            s = SsTable.open(i, files[i], ctx)
            assert s.smallest_key == got[0][0] and s.biggest_key == got[-1][0]
            assert s.num_of_blocks() == t.n_blocks and s.may_contain(got[len(got) // 2][0])


EXACT_BLOCK = 1


def exact_capacity(block_size: int) -> int:
    """A capacity that equals estimated_size() right after a block is built: the size at block 1
    of the first range's first table (from the model)."""
    _, _, merged, bounds = inputs(block_size)
    lo, hi = M.in_bounds(merged, *bounds[0])
    sizes = M.cumulative_sizes(merged[lo:hi], block_size)
    assert len(sizes) >= EXACT_BLOCK + 3
    return sizes[EXACT_BLOCK]


CAPS = ["1", "exact", "exact+1", "4096", "2^26"]


def capacity_of(kind: str, block_size: int) -> int:
    return {"1": 1, "exact": exact_capacity(block_size), "exact+1": exact_capacity(block_size) + 1,
            "4096": 4096, "2^26": 1 << 26}[kind]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_codec1_tables_and_images(ctx, block_size, cap):
    """The task's sub_ranges (four at block size 256, three at the others) at five capacities:
    entry ranges and block counts are the model's, every image is the host-assembled file, and the files open."""
    runs, regions, merged, bounds = inputs(block_size)
    capacity = capacity_of(cap, block_size)
    _, want = M.task_tables(runs, bounds, block_size, capacity)
    out = compact_task(ctx, regions, bounds, block_size=block_size, table_capacity=capacity)
    check_ranges(out, want)
    assert out.entries.n == len(merged)
    if cap == "2^26":
        assert len(out) == len(bounds)                          # one table per range
    if cap.startswith("exact"):
        # `>=`: the first table ends a block earlier at the exact size than one past it
        assert out[0].n_blocks == EXACT_BLOCK + 2 + (cap == "exact+1")
    imgs = check_images(ctx, out, block_size, 0.1)
    check_opens(ctx, out, imgs, merged)


@pytest.mark.parametrize("fpp", [0.01, -1.0])
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_codec1_other_filter_rates(ctx, block_size, fpp):
    """fpp 0.01 (a longer filter, k = 7) and -1.0 (not sign-positive: no bloom section; such a
    file is what the reference writes but cannot open, so bytes only)."""
    runs, regions, merged, bounds = inputs(block_size)
    capacity = exact_capacity(block_size)
    _, want = M.task_tables(runs, bounds, block_size, capacity)
    out = compact_task(ctx, regions, bounds, block_size=block_size, table_capacity=capacity,
                       false_positive_rate=fpp)
    check_ranges(out, want)
    imgs = check_images(ctx, out, block_size, fpp)
    if fpp > 0:
        check_opens(ctx, out, imgs, merged)
    else:
        assert all(t.bloom_off is None for t in out)


def test_entries_bound_against_python(ctx):
    """tpz_entries_bound alone: existing keys, keys between, below and above every key, a proper
    prefix and an extension of a key, the empty key; < and <=."""
    merged = inputs(256)[2]
    keys = [k for k, _ in merged]
    probes = [keys[0], keys[-1], keys[700], keys[700][:-1], keys[700] + b"\x00", b"", b"\x00",
              b"\xff" * 20, b"user", keys[1234][:6], keys[2000] + b"\xff"]
    probes = [(p, inc) for p in probes for inc in (False, True)]
    ent = DeviceEntries(*M.pack(merged), ctx.device)
    got = entries_bound(ctx, ent, probes)
    want = [sum(1 for k in keys if (k <= p if inc else k < p)) for p, inc in probes]
    assert got.tolist() == want


def _handcrafted(merged):
    keys = [k for k, _ in merged]
    below, above = b"\x01", b"\xff\xff"
    assert below < keys[0] and above > keys[-1]
    between = keys[1000] + b"\x00"
    assert keys[1000] < between < keys[1001]
    return {
        "lower-below-every-key": [(below, (keys[10], True))],
        "upper-existing-included": [(keys[5], (keys[900], True))],
        "upper-existing-excluded": [(keys[5], (keys[900], False))],
        "bounds-between-keys": [(between, (keys[2000] + b"\x00", False))],
        "empty-range": [(between, (between, True)), (keys[7], (keys[7], False))],
        "upper-below-every-key": [(below, (below + b"\x01", True))],
        "last-upper-drops-the-tail": [(keys[0], (keys[1500], False)),
                                      (keys[1500], (keys[-40], True))],
        "tiling-with-a-shared-key": [(below, (keys[800], False)), (keys[800], (between, False)),
                                     (between, (above, True))],
    }


@pytest.mark.parametrize("case", ["lower-below-every-key", "upper-existing-included",
                                  "upper-existing-excluded", "bounds-between-keys", "empty-range",
                                  "upper-below-every-key", "last-upper-drops-the-tail",
                                  "tiling-with-a-shared-key"])
def test_handcrafted_bounds(ctx, case):
    runs, regions, merged, _ = inputs(256)
    bounds = _handcrafted(merged)[case]
    _, want = M.task_tables(runs, bounds, 256, 4096)
    out = compact_task(ctx, regions, bounds, block_size=256, table_capacity=4096)
    check_ranges(out, want)
    if case in ("empty-range", "upper-below-every-key"):
        assert len(out) == 0 and out.arena.numel() == 0
    if case == "upper-existing-included":
        assert out[-1].first_entry + out[-1].n_entries == 901
    if case == "upper-existing-excluded":
        assert out[-1].first_entry + out[-1].n_entries == 900
    if case == "last-upper-drops-the-tail":
        assert out[-1].first_entry + out[-1].n_entries == len(merged) - 39
    if case == "tiling-with-a-shared-key":
        assert sum(t.n_entries for t in out) == len(merged)
        assert 801 not in [t.first_entry for t in out] and 800 in [t.first_entry for t in out]
    check_images(ctx, out, 256, 0.1)


CODEC_CAPS = {256: 4096, 4096: 4096, 65536: 150000}


@pytest.mark.parametrize("codec", [2, 3])
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_codecs_2_3_cut_rule_and_blocks(ctx, block_size, codec):
    runs, regions, merged, bounds = inputs(block_size)
    capacity = CODEC_CAPS[block_size]
    out = compact_task(ctx, regions, bounds, block_size=block_size, codec=codec,
                       table_capacity=capacity)
    imgs = images_of(out)
    FileObject.open_many([(f"t{i}", img) for i, img in enumerate(imgs)], ctx)
    spans = [M.in_bounds(merged, lo, up) for lo, up in bounds]
    ends = {hi for _, hi in spans}
    stream, at = [], None
    assert len(out) > len(bounds)                               # the capacity does cut tables
    for t, img in zip(out, imgs):
        ext, meta_off, bloom_off = O.sst_parse(img)
        nb = len(ext) - 1
        assert (nb, meta_off, bloom_off) == (t.n_blocks, t.meta_off, t.bloom_off)
        assert all(img[int(e) - 1] == codec for e in ext[1:])   # every block carries the tag
        # the rule, on the device's own stored sizes
        cum = [int(ext[j + 1]) + 2 * (j + 1) for j in range(nb)]
        assert all(c < capacity for c in cum[:max(nb - 2, 0)])
        it = O.SstIter(img)
        it.seek_to_first()
        got, per_block = [], [0] * nb
        while it.is_valid():
            got.append((it.key(), it.value()))
            per_block[it.block_idx()] += 1
            it.next()
        assert got == merged[t.first_entry:t.first_entry + t.n_entries]
        reached = nb >= 2 and cum[nb - 2] >= capacity
        if reached:
            assert per_block[-1] == 1
        last_of_range = t.first_entry + t.n_entries in ends
        if not last_of_range:
            assert reached
        # each range restarts the chain; inside a range the tables follow each other
        if at is not None and at not in ends:
            assert t.first_entry == at
        at = t.first_entry + t.n_entries
        stream += got
        # after the device codec step the region is the host builder's over the table's entries
        w_region, w_ext = synth.build_blocks(*M.pack(got), block_size)
        plain, st = decompress_batch(ctx, DeviceBatch(np.frombuffer(img[:meta_off], np.uint8),
                                                      ext.astype(np.uint64)))
        torch.cuda.synchronize()
        assert (st[:nb].cpu().numpy() == _lib.BLOCK_OK).all()
        assert plain.ext.cpu().numpy().view(np.uint64).tolist() == w_ext.tolist()
        assert plain.src[:plain.src_bytes].cpu().numpy().tobytes() == w_region.tobytes()
    assert stream == [e for lo, hi in sorted(spans) for e in merged[lo:hi]]


@pytest.mark.parametrize("codec", [1, 2])
def test_two_runs_give_identical_images(ctx, codec):
    """Image for image (the arena's padding between images is not compared)."""
    _, regions, _, bounds = inputs(4096)
    a = compact_task(ctx, regions, bounds, codec=codec, table_capacity=20000)
    b = compact_task(ctx, regions, bounds, codec=codec, table_capacity=20000)
    assert len(a) == len(b) > 4
    assert images_of(a) == images_of(b)


def test_output_images_answer_gets_like_the_inputs(ctx):
    """End to end: the task's output, opened as level 1 of a DeviceLevels, answers get_batch over
    present, absent and tombstoned keys as the input tables do as level 0 (input table 0 is the
    newest: it wins a key, as it does in the merge)."""
    runs, regions, merged, _ = inputs(4096)
    keys = [k for k, _ in merged]
    bounds = [(b"", (keys[900], False)), (keys[900], (keys[2100] + b"\x00", False)),
              (keys[2100] + b"\x00", (b"\xff", True))]
    out = compact_task(ctx, regions, bounds, table_capacity=30000)
    assert len(out) > 6 and sum(t.n_entries for t in out) == len(merged)

    def opened(images):
        files = FileObject.open_many([(f"f{i}", img) for i, img in enumerate(images)], ctx)
        return [SsTable.open(i, f, ctx) for i, f in enumerate(files)]

    ins = []
    for run in runs[:1] + [runs[1] + runs[2] + runs[3], runs[4] + runs[5] + runs[6]]:
        b = SsTableBuilder(ctx, 4096, 0.1)
        for k, v in run:
            b.add(k, v)
        img = b.build_image()
        ins.append(img + struct.pack(">I", host_crc32(img)))
    in_tables, out_tables = opened(ins), opened(images_of(out))
    # the facade's overlap_size is the descriptor's, and sub_ranges takes opened tables as they are
    for t in in_tables + out_tables[:3]:
        d = TableDesc.of(t)
        for lo, hi in ((keys[3], keys[1700]), (keys[900], keys[901]), (b"", b"\xff"), (keys[-1], keys[0])):
            assert t.overlap_size(lo, hi) == d.overlap_size(lo, hi)
        assert t.overlap_size(t.smallest_key, t.biggest_key) == t.block_metas[-1].offset
    assert sub_ranges(in_tables[:1], out_tables, 0) == \
        sub_ranges([TableDesc.of(t) for t in in_tables[:1]], [TableDesc.of(t) for t in out_tables], 0)
    assert len(sub_ranges(in_tables[:1], out_tables, 0)) == 4
    before = DeviceLevels(ctx, [in_tables[::-1]])               # L0: oldest first
    after = DeviceLevels(ctx, [[], out_tables])
    absent = [k + b"?" for k in keys[::7]] + [b"", b"\x01", b"zzz"]
    tomb = [k for k, v in merged if v == b""]
    assert len(tomb) > 100
    q = keys + absent
    r0, r1 = before.get_batch(q), after.get_batch(q)
    assert (r0["result"] == r1["result"]).all() and (r0["status"] == r1["status"]).all()
    assert set(np.unique(r1["result"])) == {_lib.GET_ABSENT, _lib.GET_FOUND, _lib.GET_DELETED}
    assert (r1["result"][[keys.index(k) for k in tomb[:50]]] == _lib.GET_DELETED).all()
    assert (r0["val_pos"] == r1["val_pos"]).all()
    assert r0["values"] == r1["values"] == b"".join(v for _, v in merged)


@pytest.mark.parametrize("codec", [1, 2])
def test_an_entry_no_block_holds_fails_the_task(ctx, codec):
    """SsTableBuilder::add recurses without end on it (table/builder.rs:57-60): EntryError with
    the entry's index in the merged entries, as compact() reports it; here the first one inside
    the range (entries below the lower bound are never added)."""
    from topazdb_amd.encode import EntryError
    _, regions, merged, _ = inputs(256)
    lower = merged[40][0]
    want = next(i for i, (k, v) in enumerate(merged) if i >= 40 and 4 + len(k) + len(v) + 2 > 128)
    with pytest.raises(EntryError) as e:
        compact_task(ctx, regions, [(lower, (b"\xff", True))], block_size=128, codec=codec,
                     table_capacity=1000)
    assert e.value.index == want == 173          # (entry 31, below the lower bound, is too long too)
    with pytest.raises(ValueError) as m:
        M.sub_compact(merged[40:], 128, 1000)
    assert 40 + m.value.args[0] == want

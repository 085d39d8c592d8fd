"""compact() and compact_task() over resident DeviceTables (entries_from_tables: no host
concatenation, upload or second decode) against the same calls over the tables' host regions, the
task's sub_ranges from resident tables, and the whole cycle on the device: flush -> serve ->
compact -> open -> serve, with the same answers before and after the compaction."""
import random

import numpy as np
import pytest
import torch

import _oracle as O
import _tables_model as M
from test_gpu_tables import images_of, inputs
from topazdb_amd import _lib
from topazdb_amd.compact import (TableDesc, compact, compact_task, flush_runs, open_output,
                                 sub_ranges)
from topazdb_amd.levels import DeviceLevels, DeviceRun
from topazdb_amd.table import DeviceTable

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def resident(ctx, block_size: int):
    """inputs(block_size)'s seven tables as DeviceTables with their block first keys."""
    tables, regions, _, _ = inputs(block_size)
    out = []
    for t, (src, ext) in zip(tables, regions):
        _, _, first = O.build_blocks(*M.pack(t), block_size)
        out.append(DeviceTable(ctx, np.asarray(src, np.uint8).tobytes(), ext,
                               [t[int(f)][0] for f in first[:-1]]))
    return out


@pytest.mark.parametrize("block_size,codec", [(256, 1), (4096, 1), (65536, 1), (4096, 2)])
def test_task_over_resident_tables_equals_the_regions(ctx, block_size, codec):
    _, regions, merged, bounds = inputs(block_size)
    capacity = (256 << 10) if block_size == 65536 else (16 << 10)
    want = compact_task(ctx, regions, bounds, block_size=block_size, codec=codec,
                        table_capacity=capacity)
    got = compact_task(ctx, resident(ctx, block_size), bounds, block_size=block_size, codec=codec,
                       table_capacity=capacity)
    assert len(want) >= len(bounds) and got.entries.n == want.entries.n == len(merged)
    assert [(t.first_entry, t.n_entries, t.n_blocks) for t in got] == \
        [(t.first_entry, t.n_entries, t.n_blocks) for t in want]
    assert images_of(got) == images_of(want)


@pytest.mark.parametrize("block_size,codec", [(256, 1), (4096, 1), (65536, 1), (4096, 2)])
def test_compact_over_resident_tables_equals_the_regions(ctx, block_size, codec):
    _, regions, merged, _ = inputs(block_size)
    want = compact(ctx, regions, block_size=block_size, codec=codec)
    got = compact(ctx, resident(ctx, block_size), block_size=block_size, codec=codec)
    assert got.n_blocks == want.n_blocks > 0 and got.entries.n == len(merged)
    assert torch.equal(got.region, want.region)
    assert torch.equal(got.ext, want.ext) and torch.equal(got.first, want.first)


@pytest.mark.parametrize("block_size", [256, 4096])
def test_sub_ranges_over_resident_tables(ctx, block_size):
    tables, regions, _, bounds = inputs(block_size)
    dts = resident(ctx, block_size)
    for t, dt, (_, ext) in zip(tables, dts, regions):
        d = TableDesc.of(dt)
        assert (d.smallest_key, d.biggest_key) == (t[0][0], t[-1][0])
        assert d.offsets == [int(x) for x in ext[:-1]] and d.meta_off == int(ext[-1])
    assert sub_ranges(dts[:1], dts[1:], 0) == bounds
    assert sub_ranges(dts[:4], dts[4:], 1) == sub_ranges(
        [TableDesc.of(x) for x in dts[:4]], [TableDesc.of(x) for x in dts[4:]], 1)


def test_mixed_inputs_are_refused(ctx):
    _, regions, _, bounds = inputs(256)
    dts = resident(ctx, 256)
    with pytest.raises(TypeError):
        compact(ctx, [dts[0], regions[1]], block_size=256)
    with pytest.raises(TypeError):
        compact_task(ctx, [regions[0]] + dts[1:], bounds, block_size=256)


# ------------------------------------------------------------------------------- the cycle
def flushed(ctx, *memtables):
    """Memtable runs (newest first) -> one L0 image on the device, opened where it lies."""
    table, _ = flush_runs(ctx, [DeviceRun(ctx, m) for m in memtables], block_size=4096)
    return open_output(ctx, table)


def answers(levels: DeviceLevels, keys, ranges):
    g = levels.get_batch(keys)
    vp = g["val_pos"].astype(np.int64)
    gets = [(int(r), g["values"][vp[i]:vp[i + 1]]) for i, r in enumerate(g["result"])]
    s = levels.scan_batch(ranges, 60)
    scans = (s["result"].tolist(), s["first"].tolist(), s["kpos"].tolist(), s["vpos"].tolist(),
             s["keys"], s["values"])
    return gets, scans


def test_flush_serve_compact_serve(ctx):
    """flush_runs builds L0 images, open_output opens them; an L1 of three tables lies below. The
    levels answer gets and scans; compact_task over the resident L0 + L1 tables (bounds from
    sub_ranges over them) writes new images, TaskTables.open opens them as the new L1, and the same
    gets and scans give the same results and values: compaction keeps tombstones, so nothing may
    change. No table byte is copied to the host on the way."""
    rng = random.Random(5)
    space = [b"key%06d" % i for i in range(0, 6000, 2)]          # odd numbers are never written

    def pick(n):
        """n keys plus both ends of the key space: every L0 table and the L1 then span the same
        keys, so that no range of RwsSlice::create has size 0 (split drops such a range when it
        comes first, range.rs:22-24, a quirk sub_ranges keeps) and the bounds cover every key."""
        return sorted(set(rng.sample(space[1:-1], n)) | {space[0], space[-1]})

    old = pick(1800)
    l1 = [flushed(ctx, [(k, b"old-" + k * 3) for k in old[i:i + 601]]) for i in (0, 601, 1202)]
    l0 = []
    for t in range(3):                           # l0[-1] is the newest: get and scan read L0 reversed
        newer = [(k, b"" if rng.random() < 0.2 else b"l0-%d-" % t + k) for k in pick(500)]
        older = [(k, b"mem-%d-" % t + k * 2) for k in pick(300)]
        l0.append(flushed(ctx, newer, older))
    before = DeviceLevels(ctx, [l0, l1])
    keys = rng.sample(space, 400) + [b"key%06d" % i for i in range(1, 400, 2)] + [b"", b"zzz"]
    ranges = [(None, None), (("in", b"key001000"), ("ex", b"key001400")),
              (("ex", b"key004000"), None), (("in", b"key000999"), ("in", b"key001001")),
              (("in", b"nothing"), None)]
    want = answers(before, keys, ranges)
    results = [r for r, _ in want[0]]
    assert {_lib.GET_FOUND, _lib.GET_ABSENT, _lib.GET_DELETED} <= set(results)
    assert _lib.GET_ERROR not in results and 2 not in want[1][0]          # no SCAN_ERROR

    bounds = sub_ranges(l0, l1, 0)
    assert len(bounds) >= 2 and bounds[0][0] == space[0] and bounds[-1][1] == (space[-1], True)
    assert all(a[1][0] == b[0] for a, b in zip(bounds, bounds[1:]))     # no key between two ranges
    # the task's tables in the readers' priority order (level.rs:430, :538-579: the newest L0
    # table first), so that the merge keeps the entry a get returns
    out = compact_task(ctx, l0[::-1] + l1, bounds, block_size=4096, table_capacity=32 << 10)
    assert len(out) >= 3
    after = DeviceLevels(ctx, [[], out.open(ctx)])
    assert answers(after, keys, ranges) == want

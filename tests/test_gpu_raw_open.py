"""open_images(raw=True): compaction and flush outputs opened where their images lie as in-place
RawTables, against the default open (DeviceTables) of the same images: the table attributes, the
answers of get_batch, the exception a corrupted image raises, the refusal of scans, and the
accounting of resident_bytes."""
import random

import numpy as np
import pytest
import torch

import _lsm_model as L
from conftest import read_golden
from test_gpu_compact import merged_entries, table_region
from test_gpu_open import answers_equal, pack_arena, small_tables
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import compact
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import BlockError, DeviceTable, RawTable, open_images

pytestmark = pytest.mark.gpu

ATTRS = ("smallest_key", "biggest_key", "size", "block_meta_offset", "n_blocks", "bloom_len")


def same_attrs(raw, dec):
    assert isinstance(raw, RawTable) and isinstance(dec, DeviceTable)
    for a in ATTRS:
        assert getattr(raw, a) == getattr(dec, a), a
    assert not hasattr(raw, "cols")


def accounted(t: RawTable, image_bytes: int):
    """At most the image, 64 bytes per block and the first keys."""
    first_keys = int(t.first_keys.numel())
    assert t.resident_bytes <= image_bytes + 64 * t.n_blocks + first_keys
    assert t.resident_bytes >= image_bytes


@pytest.mark.parametrize("codec", [1, 2])
def test_compact_output_opened_in_place(ctx, codec):
    runs = small_tables(21 + codec)
    regions = [table_region(run, 128) for run in runs]
    merged = merged_entries(runs)
    bounds = [(merged[0][0], (merged[-1][0], True))]
    out = compact.compact_task(ctx, regions, bounds, block_size=128, codec=codec,
                               table_capacity=2 << 10)
    assert len(out) >= 3
    raw, dec = out.open(ctx, raw=True), out.open(ctx)
    for r, d, o in zip(raw, dec, out):
        same_attrs(r, d)
        assert (r.codec is not None) == (codec != 1)
        if codec == 1:
            assert r.batch.src.data_ptr() == o.image.data_ptr()          # served where it lies
            accounted(r, o.size)
    keys = [k for k, _ in merged]
    qs = keys[::3] + [k + b"\0" for k in keys[::7]] + [b"", b"zzzz", b"a"]
    a, b = DeviceLevels(ctx, [[], raw]), DeviceLevels(ctx, [[], dec])
    assert a.raw and not b.raw
    got = a.get_batch(qs)
    answers_equal(got, b.get_batch(qs))
    assert (got["result"] == 1).sum() >= 50
    with pytest.raises(ValueError, match="in-place tables answer gets; scans need DeviceTables"):
        a.scan_batch([(None, None)], 7)
    assert out.open(ctx, verify=True, raw=True)[0].smallest_key == dec[0].smallest_key


def test_flush_output_opened_in_place(ctx):
    rng = random.Random(47)
    view = [L.random_run(rng, r, 60) for r in range(3)]
    t, _ = compact.flush_like_sync(ctx, [DeviceRun(ctx, r) for r in view], 128, 1)
    raw, dec = compact.open_output(ctx, t, raw=True), compact.open_output(ctx, t)
    same_attrs(raw, dec)
    assert raw.n_blocks == t.n_blocks > 1
    accounted(raw, t.size)
    top = DeviceRun(ctx, L.random_run(rng, 9, 30))
    a, b = DeviceLsm(ctx, [top], [[raw]]), DeviceLsm(ctx, [top], [[dec]])
    qs = sorted({k for r in view for k, _ in r}) + [b"zz", b"\x01"]
    answers_equal(a.get_batch(qs), b.get_batch(qs))
    with pytest.raises(ValueError, match="in-place tables answer gets; scans need DeviceTables"):
        a.scan_batch([(None, None)], 7)


def test_corrupted_images_raise_the_same(ctx):
    good = read_golden("sst_100_b128.sst")
    dev = torch.device("cuda", ctx.device)
    # a flipped byte in the last block (init_samllest_biggest_key reads it), a file CRC left stale
    last = bytearray(good)
    meta_off = int.from_bytes(good[int.from_bytes(good[-8:-4], "big") - 4:][:4], "big")
    last[meta_off - 20] ^= 0x08
    # a flipped byte in the first block: the open succeeds, a get that reads the block fails
    mid = bytearray(good)
    mid[20] ^= 0x40
    arena_h, spans = pack_arena([good, bytes(last), bytes(mid)])
    arena = torch.from_numpy(arena_h).to(dev)
    errs = []
    for raw in (True, False):
        with pytest.raises(BlockError) as e:
            open_images(ctx, arena, spans, verify=False, raw=raw)
        errs.append(str(e.value))
        with pytest.raises(BlockError) as e:
            open_images(ctx, arena, spans, verify=True, raw=raw)
        errs.append(str(e.value))
    assert errs[0] == errs[2] and errs[1] == errs[3] and errs[0].startswith("checksum: expected ")
    r = open_images(ctx, arena, spans, verify=False, strict=False, raw=True)
    d = open_images(ctx, arena, spans, verify=False, strict=False)
    same_attrs(r[0], d[0])
    accounted(r[0], len(good))
    assert type(r[1]) is type(d[1]) and str(r[1]) == str(d[1])
    same_attrs(r[2], d[2])
    a, b = DeviceLevels(ctx, [[r[2]]]), DeviceLevels(ctx, [[d[2]]])
    qs = [d[2].smallest_key, d[2].biggest_key]
    answers_equal(a.get_batch(qs), b.get_batch(qs))
    with pytest.raises(BlockError) as ea:
        a.get(d[2].smallest_key)
    with pytest.raises(BlockError) as eb:
        b.get(d[2].smallest_key)
    assert str(ea.value) == str(eb.value) and str(ea.value).startswith("checksum: expected ")

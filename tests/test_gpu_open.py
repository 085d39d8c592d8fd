"""SsTable::open over file images resident in HBM (tpz_open_index, tpz_open_metas,
table.open_images, TaskTables.open, compact.open_output), checked against tests/_open_model.py and
against the host route (SsTable.open on the images' bytes)."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import _lsm_model as L
import _open_model as M
from conftest import GOLDEN, read_golden
from test_gpu_compact import merged_entries, table_region
from test_open_model import SSTS, facade_parse
from topazdb_amd import _lib, compact
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import BlockError, DeviceTable, FileObject, ReferencePanic, SsTable, open_images

pytestmark = pytest.mark.gpu

TILE = _lib.OPEN_TILE
CANARY = 0x5A


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def pack_arena(images, seed=1):
    """The images at 16-byte aligned starts with random filler before, between and after them."""
    rng = random.Random(seed)
    parts, spans, at = [], [], 0
    for img in images:
        gap = 16 * rng.randint(0, 3) + (-at) % 16
        parts.append(bytes(rng.getrandbits(8) for _ in range(gap)))
        at += gap
        spans.append((at, len(img)))
        parts.append(img)
        at += len(img)
    parts.append(bytes(rng.getrandbits(8) for _ in range(40)))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), spans


def device_open(ctx, images, seed=1):
    """Both calls over `images` in one batch, with canaries after the stated capacities; returns
    host copies of every output. Asserts d_src unchanged and the canaries intact."""
    arena_h, spans = pack_arena(images, seed)
    dev = torch.device("cuda", ctx.device)
    arena = torch.from_numpy(arena_h).to(dev)
    n = len(images)
    span = torch.from_numpy(np.asarray(spans, np.int64)).to(dev)
    sb = _lib.open_scratch_bytes(len(arena_h), n)
    info = torch.full((n, 8), -7, dtype=torch.int64, device=dev)
    fb = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    fk = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    scratch = torch.empty(sb + 64, dtype=torch.uint8, device=dev)
    scratch[sb:] = CANARY
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.open_index_ptrs(arena.data_ptr(), len(arena_h), span.data_ptr(), n, info.data_ptr(),
                        fb.data_ptr(), fk.data_ptr(), scratch.data_ptr(), sb, s)
    nb, kb = int(fb[n].cpu()), int(fk[n].cpu())
    ext = torch.full((nb + n + 8,), -3, dtype=torch.int64, device=dev)
    pos = torch.full((nb + n + 8,), -3, dtype=torch.int64, device=dev)
    keys = torch.full((kb + 64,), CANARY, dtype=torch.uint8, device=dev)
    ctx.open_metas_ptrs(arena.data_ptr(), len(arena_h), span.data_ptr(), n, info.data_ptr(),
                        fb.data_ptr(), fk.data_ptr(), scratch.data_ptr(), sb, ext.data_ptr(),
                        pos.data_ptr(), keys.data_ptr(), nb, kb, s)
    torch.cuda.synchronize(dev)
    r = {"info": info.cpu().numpy().view(np.uint64), "fb": fb.cpu().numpy(), "fk": fk.cpu().numpy(),
         "ext": ext.cpu().numpy(), "pos": pos.cpu().numpy(), "keys": keys.cpu().numpy(),
         "spans": spans}
    assert (arena.cpu().numpy() == arena_h).all()                     # d_src is never written
    assert (scratch[sb:].cpu().numpy() == CANARY).all()
    assert (r["ext"][nb + n:] == -3).all() and (r["pos"][nb + n:] == -3).all()
    assert (r["keys"][kb:] == CANARY).all()
    return r


def check_against_model(r, images):
    """Every d_info row, the prefix sums, and every extent, position and key byte."""
    nb = kb = 0
    for i, img in enumerate(images):
        m = M.parse(img)
        assert [int(x) for x in r["info"][i]] == m.info, (i, m.info)
        assert (int(r["fb"][i]), int(r["fk"][i])) == (nb, kb), i
        if m.status == M.OK:
            n, b0 = len(m.first_keys), nb + i
            assert r["ext"][b0:b0 + n + 1].tolist() == m.ext, i
            assert r["pos"][b0:b0 + n + 1].tolist() == m.first_pos, i
            want = b"".join(m.first_keys)
            assert r["keys"][kb:kb + len(want)].tobytes() == want, i
            nb, kb = nb + n, kb + len(want)
        else:
            # a failed file owns one untouched slot and no key bytes
            assert r["ext"][nb + i] == -3 and r["pos"][nb + i] == -3, i
    assert (int(r["fb"][-1]), int(r["fk"][-1])) == (nb, kb)


# ---------------------------------------------------------------------------- 1. golden files
def test_golden_ssts_in_one_batch(ctx):
    images = [read_golden(n + ".sst") for n in SSTS]
    r = device_open(ctx, images)
    check_against_model(r, images)
    flags = {n: int(r["info"][i][7]) for i, n in enumerate(SSTS)}
    assert all(v == int("snappy" in n or "lz4" in n) for n, v in flags.items()) and sum(flags.values()) == 4
    assert all(s % 16 == 0 for s, _ in r["spans"]) and any(
        b > a + n for (a, n), (b, _) in zip(r["spans"], r["spans"][1:]))


# ---------------------------------------------------------------------------- 2. status classes
def boundary_batch():
    """The boundary cases with good files interleaved (two golden files and the OK cases)."""
    cases = M.boundary_cases()
    good = [read_golden("sst_b16.sst"), read_golden("sst_snappy_4k.sst")]
    images = []
    for j, (_, img, _) in enumerate(cases):
        images.append(img)
        if j % 3 == 0:
            images.append(good[(j // 3) % 2])
    return images


def test_every_status_class_and_boundary(ctx):
    images = boundary_batch()
    statuses = {M.parse(img).status for img in images}
    assert statuses == {M.OK, M.SHORT, M.BLOOM_RANGE, M.META_RANGE, M.META_TRUNCATED,
                        M.BAD_EXTENTS, M.NO_BLOCKS}
    r = device_open(ctx, images, seed=2)
    check_against_model(r, images)


def test_unsupported_spans(ctx):
    """Not a reference outcome: a span past span_bytes, or one that starts before its
    predecessor ends, is TPZ_OPEN_UNSUPPORTED; its neighbours open."""
    good = read_golden("sst_b16.sst")
    arena_h, spans = pack_arena([good, good, good])
    dev = torch.device("cuda", ctx.device)
    arena = torch.from_numpy(arena_h).to(dev)
    bad = [spans[0], (spans[1][0], len(arena_h)), (spans[0][0] + 16, len(good))]
    from topazdb_amd.batch import open_index
    idx = open_index(ctx, arena, bad)
    info = idx.info.cpu().numpy()
    assert info[:, 0].tolist() == [M.OK, M.UNSUPPORTED, M.UNSUPPORTED]
    assert idx.file_block.cpu().numpy().tolist() == [0, 6, 6, 6]


# ---------------------------------------------------------------------------- 3. tile phases
def synthetic(n_blocks: int, lead: int, filt=b"\x09\x03", pad_region=0) -> bytes:
    """n_blocks metas whose key lengths cycle 0..40, a few of them several tiles long (tables of
    64 blocks and more), the first key `lead` bytes longer; block lengths cycle 5..20 with a
    snappy tag on one block of every 50."""
    keys = [bytes([97 + (i + j) % 26 for j in range(i % 41)]) for i in range(n_blocks)]
    if n_blocks >= 64:
        keys[7] = bytes(range(256)) * 36                     # 9,216 bytes: over two tiles
        keys[n_blocks - 3] = b"q" * 13000
    keys[0] = b"L" * lead + keys[0]
    lens = [5 + i % 16 for i in range(n_blocks)]
    lens[0] += pad_region
    tags = [2 if i % 50 == 49 else 1 for i in range(n_blocks)]
    return M.build_image(M.regular_metas(lens, keys), filt, lens, tags)


@functools.lru_cache(maxsize=None)
def tile_phase_images():
    images = [synthetic(n, lead) for n in (1, 2, 63, 64, 65, 3000) for lead in range(6 + 40 + 1)]
    # (the section starts 16-byte aligned in the images below: tile coordinates = section offsets)
    region = b"\x01" * 32
    # a 65,535-byte key that starts in the last 6 bytes of a tile: its header starts at 4,086
    metas = [(0, b"a" * (TILE - 10 - 6)), (8, b"\xEE" * 65535), (16, b"tail"), (24, b"")]
    images.append(M.assemble(region, M.encode_metas(metas), filt=b"\x01"))
    for phase in range(1, 6):      # and its header across the boundary at every phase
        metas[0] = (0, b"a" * (TILE - 6 - phase))
        images.append(M.assemble(region, M.encode_metas(metas)))
    # a section that ends exactly on a tile boundary (two tiles), and one record longer
    sec = M.encode_metas([(i // 8, b"k" * 26) for i in range(255)])
    sec += M.encode_metas([(31, b"z" * (2 * TILE - len(sec) - 6))])
    assert len(sec) == 2 * TILE
    images.append(M.assemble(region, sec))
    images.append(M.assemble(region, sec + M.encode_metas([(32, b"")])))
    return images


def test_tile_phases(ctx):
    images = tile_phase_images()
    assert max(len(M.parse(i).first_keys) for i in images[:6 * 47]) == 3000
    # a record header meets a tile boundary at each of its 6 phases somewhere in the batch
    phases = set()
    for img in images[5 * 47:6 * 47]:
        m = M.parse(img)
        a = m.info[2] % 16                      # image starts are 16-byte aligned
        p = a
        for k in m.first_keys:
            if p // TILE != (p + 5) // TILE:
                phases.add(TILE - p % TILE)
            p += 6 + len(k)
    assert phases >= {1, 2, 3, 4, 5}
    r = device_open(ctx, images, seed=3)
    check_against_model(r, images)
    assert int(r["fb"][-1]) == sum(M.parse(i).info[6] for i in images) > 47 * 3000
    assert all(int(row[7]) == (1 if int(row[6]) >= 50 else 0) for row in r["info"][:6 * 47])


# ---------------------------------------------------------------------------- 4. the loop
def answers_equal(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tolist() == b[k].tolist(), k
        else:
            assert a[k] == b[k], k


def image_bytes(t) -> bytes:
    return t.image.cpu().numpy().tobytes()


RANGES = [(None, None), (("in", b"user0000100"), ("ex", b"user0000400")),
          (("ex", b"user0000050"), None), (None, ("in", b"user0000300")),
          (("in", b"zzz"), None), (("after", b"user0000200"), ("in", b"user0000205"))]


def small_tables(seed: int, n: int = 300, tables: int = 3):
    """Sorted tables over one key space whose entries fit 128-byte blocks: about half of each
    table's keys are in another table too; about one value in ten is a tombstone."""
    rng = random.Random(seed)
    space = [b"user%07d" % i + bytes([0x80 + i % 100]) * (i % 5) for i in range(3 * n)]
    return [[(k, b"" if rng.random() < 0.1 else (b"t%d-" % t + k)[:rng.randint(1, 19)] * 2)
             for k in sorted(rng.sample(space, n))] for t in range(tables)]


@pytest.mark.parametrize("codec", [1, 2, 3])
def test_compact_then_serve_without_leaving_the_device(ctx, codec):
    runs = small_tables(11 + codec)
    regions = [table_region(run, 128) for run in runs]
    merged = merged_entries(runs)
    bounds = [(merged[0][0], (merged[-1][0], True))]
    out = compact.compact_task(ctx, regions, bounds, block_size=128, codec=codec,
                               table_capacity=2 << 10)
    assert len(out) >= 3
    opened = out.open(ctx)
    assert all(isinstance(t, DeviceTable) for t in opened)
    host = [SsTable.open(i, FileObject(f"t{i}", image_bytes(t)), ctx) for i, t in enumerate(out)]
    for t, h, o in zip(opened, host, out):
        assert (t.smallest_key, t.biggest_key) == (h.smallest_key, h.biggest_key)
        assert (t.n_blocks, t.block_meta_offset, t.size) == (o.n_blocks, o.meta_off, o.size - 4)
        assert (t.codec is not None) == (codec != 1)
        assert t.batch.src.data_ptr() == o.image.data_ptr() or codec != 1    # decoded in place
    keys = [k for k, _ in merged]
    qs = keys[::3] + [k + b"\0" for k in keys[::7]] + [b"", b"zzzz", b"a"]
    assert sum(v == b"" for k, v in merged if k in set(qs)) >= 5           # tombstones
    a, b = DeviceLevels(ctx, [[], opened]), DeviceLevels(ctx, [[], host])
    answers_equal(a.get_batch(qs), b.get_batch(qs))
    answers_equal(a.scan_batch(RANGES, 7), b.scan_batch(RANGES, 7))
    assert out.open(ctx, verify=True)[0].smallest_key == host[0].smallest_key


@pytest.mark.parametrize("codec", [1, 2, 3])
def test_flush_then_serve_without_leaving_the_device(ctx, codec):
    rng = random.Random(40 + codec)
    view = [L.random_run(rng, r, 60) for r in range(3)]
    t, _ = compact.flush_like_sync(ctx, [DeviceRun(ctx, r) for r in view], 128, codec)
    opened = compact.open_output(ctx, t)
    host = SsTable.open(0, FileObject("l0", image_bytes(t)), ctx)
    assert (opened.smallest_key, opened.biggest_key) == (host.smallest_key, host.biggest_key)
    assert opened.n_blocks == t.n_blocks > 1 and opened.bloom_len == len(host.bloom.filter)
    top = DeviceRun(ctx, L.random_run(rng, 9, 30))
    a, b = DeviceLsm(ctx, [top], [[opened]]), DeviceLsm(ctx, [top], [[host]])
    qs = sorted({k for r in view for k, _ in r}) + [b"zz", b"\x01"]
    answers_equal(a.get_batch(qs), b.get_batch(qs))
    ranges = [(None, None), (("in", b"a"), ("ex", b"b")), (("ex", b"a\x00"), None)]
    answers_equal(a.scan_batch(ranges, 7), b.scan_batch(ranges, 7))


# ---------------------------------------------------------------------------- 5. a flipped byte
def test_flipped_byte_in_a_block(ctx):
    good = read_golden("sst_100_b128.sst")
    m = M.parse(good)
    blk = 11
    img = bytearray(good)
    img[m.ext[blk] + 9] ^= 0x40
    dev = torch.device("cuda", ctx.device)
    arena_h, spans = pack_arena([good, bytes(img)])
    arena = torch.from_numpy(arena_h).to(dev)
    opened = open_images(ctx, arena, spans, verify=False)
    assert [t.n_blocks for t in opened] == [25, 25]
    host = SsTable.open(1, FileObject("flipped", bytes(img)), ctx)
    key = m.first_keys[blk]
    a, b = DeviceLevels(ctx, [[opened[1]]]), DeviceLevels(ctx, [[host]])
    with pytest.raises(BlockError) as ea:
        a.get(key)
    with pytest.raises(BlockError) as eb:
        b.get(key)
    assert str(ea.value) == str(eb.value) and str(ea.value).startswith("checksum: expected ")
    want = json.load(open(os.path.join(GOLDEN, "sst_100_b128.json")))["blocks"][blk]["entries"][0]
    assert bytes.fromhex(want[0]) == key
    assert DeviceLevels(ctx, [[opened[0]]]).get(key) == bytes.fromhex(want[1])   # the good image
    with pytest.raises(BlockError) as ef:                                   # FileObject::open
        FileObject.open_many([("flipped", bytes(img))], ctx)
    with pytest.raises(BlockError) as ev:
        open_images(ctx, arena, spans, verify=True)
    assert str(ev.value) == str(ef.value)
    got = open_images(ctx, arena, spans, verify=True, strict=False)
    assert isinstance(got[0], DeviceTable) and str(got[1]) == str(ef.value)
    with pytest.raises(ValueError):
        open_images(ctx, arena, [(spans[0][0] + 8, spans[0][1] - 8)])      # not 16-byte aligned


# ---------------------------------------------------------------------------- 6. strict=False
def test_strict_false_returns_the_facades_exceptions(ctx):
    images = boundary_batch()
    arena_h, spans = pack_arena(images, seed=6)
    arena = torch.from_numpy(arena_h).to(torch.device("cuda", ctx.device))
    got = open_images(ctx, arena, spans, verify=False, strict=False)
    first_bad = None
    for i, (img, g) in enumerate(zip(images, got)):
        stage, want = facade_parse(img)
        if stage is None:
            # the synthetic regions are filler: their last block does not decode, and the facade
            # raises read_block's error from init_samllest_biggest_key
            try:
                want = SsTable.open(i, FileObject(f"f{i}", img), ctx)
            except (ReferencePanic, BlockError) as e:
                want = e
        if isinstance(want, Exception):
            assert type(g) is type(want) and str(g) == str(want), i
            first_bad = i if first_bad is None else first_bad
        else:
            assert isinstance(g, DeviceTable), i
            assert (g.smallest_key, g.biggest_key) == (want.smallest_key, want.biggest_key)
    assert sum(isinstance(g, DeviceTable) for g in got) >= 9
    with pytest.raises(type(got[first_bad])) as e:
        open_images(ctx, arena, spans, verify=False, strict=True)
    assert str(e.value) == str(got[first_bad])
    assert open_images(ctx, arena, []) == []

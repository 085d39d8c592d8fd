"""tpz_raw_get_keys / tpz_raw_get_values / tpz_raw_seek_keys: point gets served from the encoded
blocks in place (RawTable), against the line-by-line model (tests/_get_model.py level_get) and
against the decoded route (DeviceLevels over DeviceTables of the same pieces). Every case compares
result, status, table, block, entry, val_pos and the value bytes, exactly."""
import functools
import os

import numpy as np
import pytest
import torch

import _get_model as M
import badentry_util as U
from test_bad_entry import TABLES
from test_gpu_get import (RANDOM, assert_equal, bad_entry_case, corrupt_case, device_levels,
                          expected_arrays, flat, model_of, neighbours, random_case)
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels
from topazdb_amd.table import BlockError, DeviceTable, RawTable, ReferencePanic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("result", "status", "table", "block", "entry", "val_pos")


def raw_table(ctx, p) -> RawTable:
    return RawTable(ctx, p.region, p.ext, p.first_keys, p.bloom)


def raw_levels(ctx, pieces) -> DeviceLevels:
    dl = DeviceLevels(ctx, [[raw_table(ctx, p) for p in lv] for lv in pieces])
    assert dl.raw or not dl.tables
    assert not any(hasattr(t, "cols") for t in dl.tables)        # no decoded columns anywhere
    return dl


def assert_same(got, want):
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert got["values"] == want["values"]


def odd_starts(pieces):
    """Every multi-block table has blocks that start at odd byte offsets."""
    for p in flat(pieces):
        if len(p.ext) > 3:
            assert any(int(e) % 2 for e in p.ext[1:-1]), p.ext[:8]


def check(ctx, pieces, queries, model=None) -> DeviceLevels:
    model = model if model is not None else model_of(pieces, queries)
    rl = raw_levels(ctx, pieces)
    got = rl.get_batch(queries)
    assert_equal(got, model, queries)
    assert_same(got, device_levels(ctx, pieces).get_batch(queries))
    return rl


def blocks_table(blocks, first_keys=None, bloom=None) -> M.Pieces:
    """A table of hand-made blocks: each a list of entries (BlockBuilder's layout, valid CRC) or
    ready bytes."""
    raw, fks = [], []
    for i, b in enumerate(blocks):
        if isinstance(b, bytes):
            raw.append(b)
            fks.append(first_keys[i])
        else:
            raw.append(U.raw_block(*U.entries_block(b)))
            fks.append(first_keys[i] if first_keys else b[0][0])
    ext = np.zeros(len(raw) + 1, np.uint64)
    np.cumsum([len(b) for b in raw], out=ext[1:])
    return M.Pieces(b"".join(raw), ext, fks, bloom)


# ------------------------------------------------------------------------------- reference, random
def test_reference_get_cases(ctx):
    for name, (l0, asks) in M.reference_cases().items():
        pieces = [[M.build_pieces(e, 64) for e in l0]]
        queries = [k for k, _ in asks]
        model = model_of(pieces, queries)
        assert [(g.value if g.result == M.FOUND else None) for g in model] == [w for _, w in asks]
        odd_starts(pieces)
        rl = check(ctx, pieces, queries, model)
        for k, want in asks[::7]:
            assert rl.get(k) == want, (name, k)


@functools.lru_cache(maxsize=None)
def random_set(i):
    return random_case(*RANDOM[i])


@pytest.mark.parametrize("i", range(len(RANDOM)), ids=[f"l0_{c[1]}_b{c[3]}" for c in RANDOM])
def test_random_sets(ctx, i):
    ents, pieces, qs, model = random_set(i)
    assert any(p.bloom is None for p in flat(pieces)) and any(p.bloom for p in flat(pieces))
    assert any(not lv for lv in pieces[1:])
    assert min(sum(1 for g in model if g.result == r) for r in (M.FOUND, M.DELETED, M.ABSENT)) >= 50
    odd_starts(pieces)
    check(ctx, pieces, qs, model)


def test_seek_keys_match_the_decoded_seek(ctx):
    """tpz_raw_seek_keys against DeviceTable.seek_keys on the same tables and queries."""
    ents, pieces, qs, _ = random_set(1)
    tables = [(p, qs[::3]) for p in flat(pieces)[:3]]
    for name, spec in TABLES:
        f, _ = U.table(spec)
        tables.append((M.Pieces.from_image(f), U.probe_keys(sum(m for m, *_ in spec))))
    panics = 0
    for p, q in tables:
        got = raw_table(ctx, p).seek_keys(q)
        want = DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom).seek_keys(q)
        for k in ("block", "entry", "status", "valid"):
            assert np.array_equal(got[k], want[k]), k
        panics += int((got["status"] == _lib.BLOCK_MALFORMED).sum())
    assert panics >= 3


# ------------------------------------------------------------------------------- bad entries
@pytest.mark.parametrize("name,spec", TABLES, ids=[t[0] for t in TABLES])
def test_bad_entry_tables(ctx, name, spec):
    """Gets that land on, bisect over and avoid the bad entries of the newest table: ERROR with
    MALFORMED at that block and entry exactly where the decoded route reports it."""
    pieces, qs, model = bad_entry_case(spec)
    errors = [g for g in model if g.result == M.ERROR]
    assert errors and all((g.status, g.table) == (_lib.BLOCK_MALFORMED, 1) for g in errors)
    assert any(g.result == M.FOUND and g.table == 1 for g in model)
    rl = check(ctx, pieces, qs, model)
    with pytest.raises(ReferencePanic, match="out of range"):
        rl.get(qs[model.index(errors[0])])


def test_bad_entry_seek_steps_into_the_next_block(ctx):
    """A key past the last key of a block: the block's iterator ends invalid and the seek reads
    the next block's first entry (SsTableIterator::seek_to_key, table/iterator.rs:62-68), also
    where that entry or the block before it holds bad entries."""
    stepped = 0
    for name, spec in TABLES:
        if len(spec) < 2:
            continue
        pieces, qs, model = bad_entry_case(spec)
        p = pieces[0][1]
        ask = []
        for fk in p.first_keys[1:]:
            below = [q for q in qs if q < fk]
            if below:
                ask += sorted(below)[-2:]              # the block's last key and the gap behind it
        want = DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom).seek_keys(ask)
        got = raw_table(ctx, p).seek_keys(ask)
        for k in ("block", "entry", "status", "valid"):
            assert np.array_equal(got[k], want[k]), (name, k)
        stepped += sum(1 for q, b, e in zip(ask, want["block"], want["entry"])
                       if e == 0 and b >= 1 and q < p.first_keys[int(b)])
        assert_equal(raw_levels(ctx, pieces).get_batch(ask), [model[qs.index(q)] for q in ask], ask)
    assert stepped >= 2


# ------------------------------------------------------------------------------- block errors
def broken_tables():
    keys = [b"bk%04d" % i for i in range(200)]
    ents = [(k, b"v:" + k) for k in keys]
    out = {}
    for kind in ("crc", "tag", "empty"):
        p = M.build_pieces(ents, 256, None)
        bad = 2
        e0, e1 = int(p.ext[bad]), int(p.ext[bad + 1])
        region = bytearray(p.region)
        if kind == "crc":
            region[e0 + 9] ^= 0x20
        elif kind == "tag":
            region[e1 - 1] = 9
        else:
            del region[e0:e1]
            p.ext = np.concatenate([p.ext[:bad + 1], p.ext[bad + 1:] - np.uint64(e1 - e0)])
        p.region = bytes(region)
        out[kind] = (p, bad)
    return keys, out


@pytest.mark.parametrize("kind,status", [("crc", _lib.BLOCK_CHECKSUM_MISMATCH),
                                         ("tag", _lib.BLOCK_BAD_TAG),
                                         ("empty", _lib.BLOCK_EMPTY)])
def test_block_errors(ctx, kind, status):
    keys, tabs = broken_tables()
    p, bad = tabs[kind]
    pieces = [[p]]
    qs = keys + [k + b"\0" for k in keys[::5]]
    model = model_of(pieces, qs)
    hit = [g for g in model if g.result == M.ERROR]
    assert hit and all((g.status, g.table, g.block) == (status, 0, bad) for g in hit)
    assert sum(1 for g in model if g.result == M.FOUND) >= 100          # bisections elsewhere
    rl = check(ctx, pieces, qs, model)
    q = qs[model.index(hit[0])]
    with pytest.raises(BlockError, match={"crc": r"checksum: expected \d+, actual \d+",
                                          "tag": "invaild data", "empty": "data is empty"}[kind]):
        rl.get(q)
    want = None
    try:
        device_levels(ctx, pieces).get(q)
    except BlockError as e:
        want = str(e)
    try:
        rl.get(q)
    except BlockError as e:
        assert str(e) == want


def test_corrupt_block_under_filters(ctx):
    keys, pieces, bad, lo, hi = corrupt_case()
    qs = keys + [k + b"\0" for k in keys]
    model = model_of(pieces, qs)
    assert sum(1 for g in model if g.result == M.ERROR) >= 10
    check(ctx, pieces, qs, model)


# ------------------------------------------------------------------------------- shape edges
LONG = bytes(range(256)) * 234 + b"tail" * 24          # 60,000 bytes


def edge_cases():
    assert len(LONG) == 60000
    out = {}
    a = [(b"a%03d" % i, b"x%d" % i) for i in range(5)]
    z = [(b"z%03d" % i, b"y%d" % i) for i in range(5)]
    # a block with n = 0 between two ordinary ones
    out["n0"] = (blocks_table([a, U.raw_block([], b""), z], [a[0][0], b"m", z[0][0]]),
                 [b"a002", b"a004\0", b"m", b"m5", b"yy", b"z000", b"z004", b"zz"])
    out["n1"] = (blocks_table([[(b"a", b"1")], [(b"c", b"22")], [(b"e", b"")]]),
                 [b"", b"a", b"b", b"c", b"d", b"e", b"f"])
    many = [(b"k%05d" % i, bytes([i % 251 + 1])) for i in range(300)]
    out["n300"] = (blocks_table([many, z]),
                   [k for k, _ in many] + [b"k00100\0", b"k", b"k99999", b"z001"])
    big = [(b"big%04d" % i, bytes([i + 1]) * 5000) for i in range(9)]
    out["offsets_past_7fff"] = (blocks_table([a, big, z]),
                                [k for k, _ in big] + [b"big0004\0", b"big9", b"a001", b"z003"])
    out["long_key"] = (blocks_table([a, [(LONG, b"long-value")], z],
                                    bloom=M.bloom_of([k for k, _ in a + z] + [LONG], 0.1)),
                       [LONG, LONG[:-1] + b"\x00", LONG[:-1] + b"\xff", LONG[:-1], LONG + b"\0",
                        LONG[:30000], b"a003", b"z001"])
    # an empty key inside a block: a seek that lands on it is invalid and tries the next block
    out["empty_key"] = (blocks_table([[(b"", b"e"), (b"b", b"1")], [(b"c", b"2")]], [b"", b"c"]),
                        [b"", b"a", b"b", b"b\0", b"c", b"d"])
    lens = [0, 1, 255, 256, 257, 5000]
    vals = [(b"v%04d" % n, bytes([n % 250 + 1]) * n) for n in lens]
    out["values"] = (blocks_table([vals[:3], vals[3:]]),
                     [k for k, _ in vals] * 3 + [b"v0256\0"])
    return out


EDGES = edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_shape_edges(ctx, name):
    p, qs = EDGES[name]
    pieces = [[], [p]] if name in ("n1", "values") else [[p]]
    model = model_of(pieces, qs)
    blk = [p.region[int(p.ext[b]):int(p.ext[b + 1])] for b in range(len(p.ext) - 1)]
    ns = [int.from_bytes(b[:2], "big") for b in blk]
    if name == "n0":
        assert 0 in ns and any(g.block == 2 and g.entry == 0 for g in model)
    elif name == "n1":
        assert ns == [1, 1, 1] and [g.result for g in model] == [
            M.ABSENT, M.FOUND, M.ABSENT, M.FOUND, M.ABSENT, M.DELETED, M.ABSENT]
    elif name == "n300":
        assert ns[0] == 300 and sum(1 for g in model if g.entry > 255 and g.result == M.FOUND) >= 40
    elif name == "offsets_past_7fff":
        assert len(blk[1]) > 32768 and int.from_bytes(blk[1][2 + 2 * 8:4 + 2 * 8], "big") > 0x7FFF
        assert sum(1 for g in model if g.result == M.FOUND and g.block == 1 and g.entry >= 7) >= 2
    elif name == "long_key":
        assert [g.result for g in model[:6]] == [M.FOUND] + [M.ABSENT] * 5
    elif name == "empty_key":
        # b"" lands on the empty key of block 0 (an invalid cursor), steps to block 1 and finds
        # b"c" there: not its key
        assert model[0].result == M.ABSENT and model[2].result == M.FOUND
        assert model[4].result == M.FOUND and model[4].block == 1
    else:
        assert sorted({len(g.value) for g in model}) == [0, 1, 255, 256, 257, 5000]
        assert any(g.result == M.DELETED for g in model)
    odd_starts(pieces)
    check(ctx, pieces, qs, model)


def test_val_cap_smaller_than_the_total(ctx):
    """Nothing is written at or past val_cap: inside a lane-copied value, inside a wave-copied
    one, and at 0."""
    p, qs = EDGES["values"]
    pieces = [[p]]
    model = model_of(pieces, qs)
    want = expected_arrays(model)
    total = len(want["values"])
    rl = raw_levels(ctx, pieces)
    w = rl.walk(qs)
    torch.cuda.synchronize()
    assert int(w["val_pos"][len(qs)]) == total
    i5000 = max(i for i, g in enumerate(model) if len(g.value) == 5000)
    i257 = next(i for i, g in enumerate(model) if len(g.value) == 257)
    i255 = next(i for i, g in enumerate(model) if len(g.value) == 255)
    guard = 256
    for cap in (total, int(want["val_pos"][i5000]) + 2999, int(want["val_pos"][i257]) + 100,
                int(want["val_pos"][i255]) + 20, 0):
        buf = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=rl.dev)
        ctx.raw_get_values_ptrs(rl.d_tables.data_ptr(), rl.n_tables, len(qs),
                                w["result"].data_ptr(), w["table"].data_ptr(),
                                w["block"].data_ptr(), w["entry"].data_ptr(),
                                w["val_pos"].data_ptr(), buf.data_ptr(), cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tobytes()
        assert out[:cap] == want["values"][:cap], cap
        assert out[cap:] == b"\xa5" * (total + guard - cap), cap


# ------------------------------------------------------------------------------- codecs
@pytest.mark.parametrize("name", ["sst_snappy_4k", "sst_lz4_4k", "sst_snappy_bench", "sst_lz4_bench"])
def test_golden_codec_tables(ctx, name):
    p = M.Pieces.from_image(open(os.path.join(GOLDEN, name + ".sst"), "rb").read())
    assert {p.region[int(e) - 1] for e in p.ext[1:]} == {2 if "snappy" in name else 3}
    host = p.host_table()
    held = [blk.key_at(i) for blk in host._blocks for i in range(blk.num_entries)]
    qs = list(held)
    for k in held:
        qs += neighbours(k)
    pieces = [[p]]
    rl = raw_levels(ctx, pieces)
    assert rl.tables[0].codec is not None
    got = rl.get_batch(qs)
    assert_same(got, device_levels(ctx, pieces).get_batch(qs))
    # (the bench tables' keys are not in byte order, so a bisection misses some held keys: in the
    # reference, the model and on both device routes alike)
    assert_equal(got, model_of(pieces, qs), qs)
    assert (got["result"][:len(held)] == M.FOUND).sum() >= len(held) // 2
    assert (got["result"] != M.ERROR).all()
    assert rl.tables[0].last_key() == held[-1]


# ------------------------------------------------------------------------------- positions
def test_image_past_4_gib_of_its_arena(ctx):
    """A small table whose blocks lie past byte 2^32 of the buffer its extents index: the same
    answers as the table at offset 0. The buffer is uninitialised apart from the blocks, with 2^31
    bytes below the base, so that an extent truncated to 32 bits or sign-extended from them reads
    other bytes of the same allocation (a wrong answer here, not a fault). The 6 GiB go back to
    the device afterwards, as the other big-buffer tests leave it (tests/test_gpu_positions.py):
    no later test's tensors are carved out of that buffer."""
    ents, pieces, qs, model = random_set(3)
    p = next(x for x in flat(pieces) if x.bloom is not None)
    qs = qs[::4]
    base_answers = raw_levels(ctx, [[p]]).get_batch(qs)
    try:
        past_4_gib(ctx, p, qs, base_answers)
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def past_4_gib(ctx, p, qs, base_answers):
    dev = torch.device("cuda", ctx.device)
    free, _ = torch.cuda.mem_get_info()
    porch, at = 1 << 31, (1 << 32) + 4099
    need = porch + at + len(p.region) + 4096
    assert free >= need + (1 << 30), f"{free >> 20} MiB free, the buffer needs {need >> 20} MiB"
    buf = torch.empty(need, dtype=torch.uint8, device=dev)
    view = buf[porch:]
    view[at:at + len(p.region)].copy_(torch.from_numpy(np.frombuffer(p.region, np.uint8).copy()))
    ext = torch.from_numpy((p.ext.astype(np.int64) + at)).to(dev)
    assert int(ext[0]) > 1 << 32 and int(ext[0]) % 2 == 1
    plain = raw_table(ctx, p)
    t = RawTable.from_resident(ctx, view, ext, plain.first_keys, plain.first_pos, plain.bloom,
                               plain.bloom_len, False)
    assert t.status[:t.n_blocks].cpu().tolist() == [_lib.BLOCK_OK] * t.n_blocks
    assert np.array_equal(t.crc.cpu().numpy(), plain.crc.cpu().numpy())
    got = DeviceLevels(ctx, [[t]]).get_batch(qs)
    assert_same(got, base_answers)
    assert (got["result"] == M.FOUND).sum() >= 20
    sk, sk0 = t.seek_keys(qs), plain.seek_keys(qs)
    for k in sk:
        assert np.array_equal(sk[k], sk0[k]), k


# ------------------------------------------------------------------------------- counts, refusals
def test_no_keys_and_no_tables(ctx):
    qs = [b"a", b"", b"key_0001"]
    for levels in ([], [[] for _ in range(6)]):
        dl = DeviceLevels(ctx, levels)
        w = {k: torch.full((4,), 0x5A, dtype=t, device=dl.dev) for k, t in
             (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
              ("block", torch.int32), ("entry", torch.int32), ("val_pos", torch.int64))}
        buf, pos = np.frombuffer(b"akey_0001", np.uint8), np.array([0, 1, 1, 9], np.int64)
        q, qp = torch.from_numpy(buf.copy()).to(dl.dev), torch.from_numpy(pos).to(dl.dev)
        ctx.raw_get_keys_ptrs(0, 0, dl.level_first.ctypes.data, dl.n_levels, q.data_ptr(),
                              qp.data_ptr(), 3, *(w[k].data_ptr() for k in w))
        torch.cuda.synchronize()
        assert w["result"].tolist() == [M.ABSENT] * 3 + [0x5A] and w["val_pos"].tolist() == [0] * 4
        assert w["table"][:3].cpu().numpy().view(np.uint32).tolist() == [M.NONE] * 3
    p = M.build_pieces([(b"a", b"1"), (b"b", b"22"), (b"c", b"")], 64)
    rl = raw_levels(ctx, [[p]])
    assert_equal(rl.get_batch([]), [], [])
    cols = {k: torch.full((2,), 0x5A, dtype=t, device=rl.dev) for k, t in
            (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
             ("block", torch.int32), ("entry", torch.int32), ("val_pos", torch.int64))}
    qp = torch.zeros(1, dtype=torch.int64, device=rl.dev)
    ctx.raw_get_keys_ptrs(rl.d_tables.data_ptr(), rl.n_tables, rl.level_first.ctypes.data,
                          rl.n_levels, 0, qp.data_ptr(), 0, *(cols[k].data_ptr() for k in cols))
    torch.cuda.synchronize()
    assert cols["val_pos"].tolist() == [0, 0x5A]
    for k in ("result", "status", "table", "block", "entry"):
        assert cols[k].tolist() == [0x5A, 0x5A], k
    assert rl.get(b"b") == b"22" and rl.get(b"c") is None and rl.get(b"bb") is None


def test_mixed_sets_and_scans_are_refused(ctx):
    p = M.build_pieces([(b"a", b"1"), (b"b", b"22")], 64)
    raw, dec = raw_table(ctx, p), DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom)
    with pytest.raises(TypeError):
        DeviceLevels(ctx, [[raw, dec]])
    rl = DeviceLevels(ctx, [[raw]])
    with pytest.raises(ValueError, match="in-place tables answer gets; scans need DeviceTables"):
        rl.scan_batch([(None, None)], 4)
    with pytest.raises(ValueError, match="in-place tables answer gets; scans need DeviceTables"):
        rl.scan()
    from topazdb_amd.compact import entries_from_tables
    with pytest.raises(ValueError, match="in-place tables answer gets"):
        entries_from_tables(ctx, [raw])
    assert raw.resident_bytes <= len(p.region) + 64 * raw.n_blocks + sum(map(len, p.first_keys)) \
        + len(p.bloom)
    torch.cuda.synchronize()          # (the tables' verify and decode launches end here)

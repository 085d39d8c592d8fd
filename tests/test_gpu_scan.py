"""tpz_scan_ranges / tpz_scan_entries (LsmStorage::scan's SST half for batches of ranges over
resident tables, src/lsm_storage.rs:335-374) against the line-by-line model of
tests/_scan_model.py, which tests/test_scan_model.py ties to the closed form and to the
reference's own scan tests.

Every case compares d_result, d_status, d_where, the hit columns up to each scan's count, the
three prefix arrays, d_kpos, d_vpos and the key and value bytes with the model, exactly, and first
asserts from the model alone that its inputs reach what the case names.
"""
import functools

import numpy as np
import pytest
import torch

import _get_model as G
import _scan_cases as K
import _scan_model as S
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels, _bound
from topazdb_amd.table import BlockError, DeviceTable, FileObject, SsTable, _pack

pytestmark = pytest.mark.gpu

NONE3 = (G.NONE,) * 3


# ------------------------------------------------------------------------------- harness
def device_levels(ctx, pieces) -> DeviceLevels:
    return DeviceLevels(ctx, [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom)
                               for p in lv] for lv in pieces])


def assert_equal(got, models, limit, ranges):
    want = K.expected(models, limit)
    for k in ("result", "status", "where", "first", "key_first", "val_first", "kpos", "vpos"):
        g, w = np.asarray(got[k]), want[k]
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (k, bad[0], ranges[min(int(bad[0][0]), len(ranges) - 1)],
                               g[tuple(bad[0])], w[tuple(bad[0])])
    for i, h in enumerate(want["hits"]):
        for c, k in enumerate(("hit_table", "hit_block", "hit_entry")):
            assert np.array_equal(got[k][i, :len(h)], h[:, c]), (k, i, ranges[i])
    assert got["keys"] == want["keys"] and got["values"] == want["values"]


def check(ctx, case: K.Case, limit, idx=None, dl=None) -> DeviceLevels:
    idx = list(range(len(case.ranges))) if idx is None else idx
    dl = dl or device_levels(ctx, case.pieces)
    ranges = [case.ranges[r] for r in idx]
    assert_equal(dl.scan_batch(ranges, limit), case.models(limit, idx), limit, ranges)
    return dl


def drain(it) -> list:
    out = []
    while it.is_valid():
        out.append((it.key(), it.value()))
        it.next()
    it.next()                                   # FusedIterator: a no-op once invalid
    assert not it.is_valid()
    return out


def small_case(level_ents, ranges, block_size=64) -> K.Case:
    return K.Case(level_ents, K.pieces_of(level_ents, block_size), ranges)


# ------------------------------------------------------------------------------- 1. reference cases
def test_reference_scan_cases(ctx, tmp_path):
    """src/tests/storage.rs:110-246 through SsTable.open and DeviceLevels: scan_batch and the
    scan() iterator."""
    for name, (l0, scans) in S.reference_cases().items():
        pieces = K.pieces_of([l0], 64)
        tables = []
        for j, p in enumerate(pieces[0]):
            path = tmp_path / f"{name}_{j}.sst"
            path.write_bytes(p.image())
            tables.append(SsTable.open(j, FileObject.open(str(path), ctx), ctx))
        ranges = [(lo, hi) for lo, hi, _ in scans]
        host = K.host_levels(pieces)
        models = [S.lsm_scan(host, lo, hi, 16) for lo, hi in ranges]
        assert [m.entries for m in models] == [w for _, _, w in scans], name
        for levels in ([tables], [tables] + [[] for _ in range(5)]):     # MAX_LEVEL 6
            dl = DeviceLevels(ctx, levels)
            assert_equal(dl.scan_batch(ranges, 16), models, 16, ranges)
            for lo, hi, want in scans:
                assert drain(dl.scan(lo, hi)) == want, (name, lo, hi)
                assert drain(dl.scan(lo, hi, page=1)) == want, (name, lo, hi)


# ------------------------------------------------------------------------------- 2. random sets
@functools.lru_cache(maxsize=None)
def coverage() -> dict:
    """What the random sets' scans meet, over all cases and limits, from the model alone."""
    seen = dict.fromkeys(("done", "more", "nothing", "tombstone", "tie", "crossing", "dropped_lo",
                          "dropped_hi", "quirk"), 0)
    for i in range(len(K.RANDOM_IDS)):
        case = K.random_case(i)
        for limit in K.LIMITS:
            for m in case.models(limit):
                assert m.result != S.ERROR
                seen["done"] += m.result == S.DONE
                seen["more"] += m.result == S.MORE
                seen["nothing"] += not m.hits
                seen["tombstone"] += m.stats["tombstones"] > 0
                seen["tie"] += m.stats["ties"] > 0
                seen["crossing"] += m.stats["crossings"] > 0
                seen["dropped_lo"] += m.stats["dropped_lo"] > 0
                seen["dropped_hi"] += m.stats["dropped_hi"] > 0
                seen["quirk"] += m.stats["quirk"]
    return seen


@pytest.mark.parametrize("limit", K.LIMITS)
@pytest.mark.parametrize("i", range(len(K.RANDOM_IDS)), ids=K.RANDOM_IDS)
def test_random_sets(ctx, i, limit):
    """Every bound-kind pair over bounds drawn from the keys, their neighbours and absent keys."""
    seen = coverage()
    assert min(v for k, v in seen.items() if k != "quirk") >= 50 and seen["quirk"] >= 10, seen
    case = K.random_case(i)
    kinds = {(lo and lo[0], hi and hi[0]) for lo, hi in case.ranges}
    assert kinds == set(K.KIND_PAIRS)
    sizes = [len(e) for lv in case.ents for e in lv]
    assert 1 <= min(sizes) and max(sizes) <= 200
    assert max(p.ext.size - 1 for p in K.flat(case.pieces)) >= 2          # blocks to cross
    if i == len(K.RANDOM):      # the long keys: all tie on the merge's 8-byte prefix
        keys = {k for lv in case.ents for e in lv for k, _ in e}
        assert len({k[:8] for k in keys}) == 1 and len({k[:32] for k in keys}) == 3
        assert all(len(k) == 40 for k in keys)
    check(ctx, case, limit)


# ------------------------------------------------------------------------------- 3. scan counts
@pytest.mark.parametrize("n", [1, 5, 257, 2049])
def test_scan_counts(ctx, n):
    """A partial wave's worth, a partial workgroup and more than one workgroup of the
    wave-per-scan kernels (4 scans per workgroup), and of the seek's thread per (scan, table)."""
    case = K.random_case(0)
    idx = [(7 * j) % len(case.ranges) for j in range(n)]
    models = case.models(3, idx)
    if n >= 257:
        assert len({m.result for m in models}) == 2 and sum(1 for m in models if not m.hits) >= 5
    check(ctx, case, 3, idx)


# ------------------------------------------------------------------------------- 4. boundaries
B, D, F = (b"b", b"1"), (b"d", b"4"), (b"f", b"6")
T = [B, D, F]
BOUNDARIES = [
    # name, levels as entry lists, lower, upper, the entries yielded
    ("lower_equals_key_included", [[T]], ("in", b"d"), None, [D, F]),
    ("lower_equals_key_excluded", [[T]], ("ex", b"d"), None, [F]),
    ("lower_equals_last_key_excluded", [[T]], ("ex", b"f"), None, []),
    ("lower_past_every_key", [[T]], ("in", b"g"), None, []),
    ("upper_before_every_key", [[T]], None, ("in", b"a"), []),
    ("upper_before_the_range_straddled", [[[(b"a", b"0"), D]]], ("in", b"b"), ("in", b"c"), [D]),
    ("upper_before_the_range_not_straddled", [[[D, F]]], ("in", b"b"), ("in", b"c"), []),
    ("upper_equals_key_included", [[T]], None, ("in", b"d"), [B, D]),
    ("upper_equals_key_excluded", [[T]], None, ("ex", b"d"), [B]),
    ("tombstone_as_e0", [[[(b"b", b""), D, F]]], None, None, [D, F]),
    ("tombstone_as_e0_past_the_end", [[[(b"a", b"0"), (b"b", b""), D, F]]], ("in", b"b"),
     ("in", b"a\xff"), []),
    ("tombstone_equal_to_upper", [[[B, (b"d", b""), F]]], None, ("in", b"d"), [B]),
    ("all_tombstone_range", [[[(b"b", b""), (b"d", b""), F]]], ("in", b"b"), ("in", b"d"), []),
    ("newer_tombstone_hides_older_value", [[T, [(b"d", b"")]]], None, None, [B, F]),
    ("empty_l0", [[], [T]], None, None, T),
    ("empty_levels_in_between", [[[B]], [], [], [[D, F]]], None, None, T),
    ("after_checks_e0", [[[(b"a", b"0"), D]]], ("after", b"b"), ("in", b"c"), []),
    ("after_is_excluded", [[T]], ("after", b"b"), ("in", b"f"), [D, F]),
]


@pytest.mark.parametrize("name,ents,lo,hi,want", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_boundaries_and_the_quirk(ctx, name, ents, lo, hi, want):
    case = small_case(ents, [(lo, hi)])
    m = case.model(0, 8)
    assert (m.result, m.entries) == (S.DONE, want)
    if name == "upper_before_the_range_straddled":
        assert m.stats["quirk"] == 1 and m.stats["dropped_hi"] == 0
    if name in ("upper_before_the_range_not_straddled", "upper_before_every_key"):
        assert m.stats["dropped_hi"] == 1 and m.stats["cursors"] == 0
    if name == "lower_past_every_key":
        assert m.stats["dropped_lo"] == 1
    if name.startswith("tombstone") or name.startswith("all_tombstone"):
        assert m.stats["tombstones"] >= 1
    dl = check(ctx, case, 8)
    if lo is None or lo[0] != "after":
        assert drain(dl.scan(lo, hi, page=1)) == want


def test_no_tables_and_no_levels(ctx):
    ranges = [(None, None), (("in", b"a"), ("ex", b"b")), (("ex", b""), None)]
    for levels in ([], [[] for _ in range(6)]):
        dl = DeviceLevels(ctx, levels)
        models = [S.lsm_scan([], lo, hi, 4) for lo, hi in ranges]
        assert all((m.result, m.where, m.hits) == (S.DONE, NONE3, []) for m in models)
        assert_equal(dl.scan_batch(ranges, 4), models, 4, ranges)
        assert_equal(dl.scan_batch([], 4), [], 4, [])               # n_scans == 0
        assert drain(dl.scan()) == []


# ------------------------------------------------------------------------------- 5. the maximum
def max_case() -> K.Case:
    l0 = [[(b"m%02d" % ((t + j) % 50), b"" if (t + j) % 7 == 0 else b"%d:%d" % (t, j))
           for j in range(1 + t % 4)] for t in range(60)]
    l0 = [sorted(set(e)) for e in l0]
    low = [[(b"z%d%d" % (t, j), b"low") for j in range(3)] for t in range(4)]
    return small_case([l0, low], [(None, None), (("in", b"m10"), ("ex", b"z2"))])


def test_sixty_four_tables(ctx):
    """60 tables in L0 and 4 below, every one with a cursor in the unbounded scan: all 64 lanes
    of the merge wave are live."""
    case = max_case()
    assert sum(len(lv) for lv in case.pieces) == _lib.SCAN_MAX_TABLES
    m, full = case.model(0, 16), case.model(0, 1 << 10)
    assert m.stats["cursors"] == 64 and m.stats["ties"] > 0 and full.stats["tombstones"] > 0
    assert (m.result, full.result) == (S.MORE, S.DONE) and len(full.hits) > 16
    assert {t for t, _, _ in full.hits} >= {59, 60, 63}      # the newest of L0, the level below
    dl = check(ctx, case, 16)
    check(ctx, case, 1 << 10, dl=dl)
    assert drain(dl.scan(page=7)) == full.entries
    with pytest.raises(_lib.TpzError):           # 65 tables: refused, nothing falls back
        DeviceLevels(ctx, [dl.tables + dl.tables[:1]]).scan_batch([(None, None)], 4)


# ------------------------------------------------------------------------------- 6. errors
def corrupt(p, block):
    region = bytearray(p.region)
    region[int(p.ext[block]) + 7] ^= 0x80                      # the block's CRC no longer matches
    p.region = bytes(region)


@functools.lru_cache(maxsize=None)
def corrupt_case(bad=3):
    keys = [b"ek%04d" % i for i in range(300)]
    old = [(k, b"old:" + k) for k in keys]
    mid = [(k, b"mid:" + k) for k in keys[::3]]
    pieces = K.pieces_of([[old, mid]], 256)
    p = pieces[0][1]
    nb = len(p.first_keys)
    bad = bad if bad >= 0 else nb + bad
    assert nb >= 6 and bad < nb
    corrupt(p, bad)
    fk = p.first_keys
    last_before = max(k for k, _ in mid if k < fk[bad])         # the last key of block bad - 1
    ranges = [
        (("in", fk[bad]), None),                # 0: the seek reads the bad block
        (("in", fk[bad - 1]), None),            # 1: a block crossing mid-scan reads it
        (("ex", last_before), None),            # 2: the Excluded step crosses into it
        (None, None),                           # 3: the whole range runs into it
        (("in", fk[0]), ("in", fk[1])),         # 4: ends before it
        (("in", fk[bad + 1]), None) if bad + 1 < nb else (("in", b"zz"), None),   # 5: starts past it
        (("in", fk[bad - 1]), ("ex", last_before)),   # 6: stops one key short of the crossing
    ]
    return K.Case([[old, mid]], pieces, ranges), bad


def test_errors_end_the_scan(ctx):
    case, bad = corrupt_case()
    cs = _lib.BLOCK_CHECKSUM_MISMATCH
    m = case.models(64)
    assert (m[0].result, m[0].status, m[0].where, m[0].hits) == (S.ERROR, cs, (1, bad, 0), [])
    assert (m[1].result, m[1].status, m[1].where) == (S.ERROR, cs, (1, bad, 0))
    assert 10 <= len(m[1].hits) < 64 and {t for t, _, _ in m[1].hits} == {0, 1}
    assert (m[2].result, m[2].status, m[2].where, m[2].hits) == (S.ERROR, cs, (1, bad, 0), [])
    assert m[3].result == S.MORE                     # 64 entries come before the crossing
    assert case.model(3, 1 << 10).result == S.ERROR and len(case.model(3, 1 << 10).hits) > 64
    for r in (4, 5, 6):                              # the bad block lies outside these ranges
        x = case.model(r, 1 << 10)
        assert x.result == S.DONE and x.hits and m[r].result != S.ERROR, r
    assert {t for t, _, _ in case.model(5, 1 << 10).hits} == {0, 1}
    assert case.model(1, 5).result == S.MORE         # a page that ends before the failure
    dl = check(ctx, case, 64)
    check(ctx, case, 5, dl=dl)
    check(ctx, case, 1 << 10, dl=dl)
    # the iterator yields the entries before the failure, then raises the reference's Err
    it = dl.scan(*case.ranges[1], page=7)
    got = []
    with pytest.raises(BlockError, match=r"checksum: expected \d+, actual \d+"):
        while it.is_valid():
            got.append((it.key(), it.value()))
            it.next()
    assert got == m[1].entries
    with pytest.raises(BlockError, match=r"checksum: expected"):
        dl.scan(*case.ranges[0])
    assert drain(dl.scan(*case.ranges[6])) == m[6].entries


def test_a_table_that_could_not_be_opened(ctx):
    """The last block unreadable: biggest_key cannot be read, SsTable::open fails in the
    reference, and every scan is an ERROR at that table, whatever its range."""
    case, bad = corrupt_case(-1)
    m = case.models(64)
    want = (S.ERROR, _lib.BLOCK_CHECKSUM_MISMATCH, (1, bad, G.NONE), [])
    assert all((x.result, x.status, x.where, x.hits) == want for x in m)
    check(ctx, case, 64)
    # ... and a table without blocks
    empty = G.Pieces(b"", np.zeros(1, np.uint64), [], None)
    c2 = K.Case([[T], [[]]], [K.pieces_of([[T]], 64)[0], [empty]], [(None, None), (("in", b"x"), None)])
    for x in c2.models(4):
        assert (x.result, x.status, x.where) == (S.ERROR, _lib.BLOCK_MALFORMED, (1, G.NONE, G.NONE))
    check(ctx, c2, 4)


def repeated_case() -> K.Case:
    """A table whose blocks repeat every entry 4 or 7 times (kept in spill records,
    tests/test_gpu_get.py spilled_pieces) between an older and a newer honest table."""
    from test_gpu_get import spilled_pieces
    sp, keys = spilled_pieces()
    older = sorted([(k, b"old:" + k) for k in keys[::2]] + [(b"sp9", b"tail")])
    newer = [(k, b"" if i % 3 == 0 else b"new:" + k) for i, k in enumerate(keys[::5])]
    pieces = [[G.build_pieces(older, 256, None), sp, G.build_pieces(newer, 256, None)]]
    ranges = [(None, None), (("in", keys[10]), ("ex", keys[100])), (("ex", keys[39]), None),
              (("in", keys[41] + b"\0"), ("in", keys[150]))]
    return K.Case(None, pieces, ranges)


def test_repeated_keys_within_a_table(ctx):
    """MergeIterator::next moves every other cursor at the current key on until its key differs
    (merge_iterator.rs:76-88) but the current one a single step: a key the newest table holds
    once is yielded once although the table below repeats it, and a key only the repeating table
    holds is yielded once per copy. The repeating table's blocks are read from spill records."""
    case = repeated_case()
    big = 1 << 12
    m = case.model(0, big)
    copies = {}
    for (t, _, _), (k, _) in zip(m.hits, m.entries):
        copies.setdefault(k, []).append(t)
    assert m.result == S.DONE and m.stats["ties"] > 100 and m.stats["crossings"] > 10
    assert sum(1 for c in copies.values() if c == [2]) >= 10           # held once by the newest
    assert {len(c) for c in copies.values() if set(c) == {1}} == {4, 7}
    assert copies[b"sp9"] == [0]
    dl = check(ctx, case, big)
    check(ctx, case, 5, dl=dl)
    st = dl.tables[1].cols.status[:4].cpu().numpy()
    assert (st == _lib.BLOCK_OK_SPILLED).all()


# ------------------------------------------------------------------------------- 7. capacity
LENGTHS = [1, 15, 16, 17, 31, 33, 255, 256, 257, 1000]


@functools.lru_cache(maxsize=None)
def length_case() -> K.Case:
    """Keys and values of every length class of the copies (below 16 bytes, lane-copied,
    wave-copied), at varying destination offsets."""
    import random
    rng = random.Random(61)
    ents = sorted((b"k%04d" % n + b"x" * (n if n > 250 else n % 19),
                   bytes(rng.getrandbits(8) for _ in range(n))) for n in LENGTHS)
    other = sorted((b"k%04d" % n + b"y" * (n % 5), b"v" * (1 + n % 40)) for n in range(0, 1100, 37))
    keys = [k for k, _ in ents]
    ranges = [(None, None)] + [(("in", k), None) for k in keys] + [(("ex", keys[2]), ("in", keys[-2]))]
    return K.Case([[ents], [other]], K.pieces_of([[ents], [other]], 4096), ranges)


def raw_inputs(dl, ranges):
    cols = []
    for side, lower in ((0, True), (1, False)):
        b = [_bound(r[side], lower) for r in ranges]
        buf, pos = _pack([k for _, k in b])
        cols += [torch.from_numpy(buf.copy()).to(dl.dev), torch.from_numpy(pos).to(dl.dev),
                 torch.from_numpy(np.array([k for k, _ in b], np.uint8)).to(dl.dev)]
    return cols


RANGE_OUT = (("result", torch.uint8, 1), ("status", torch.uint8, 1), ("where", torch.int32, 3),
             ("hit_table", torch.int32, None), ("hit_block", torch.int32, None),
             ("hit_entry", torch.int32, None), ("first", torch.int64, -1),
             ("key_first", torch.int64, -1), ("val_first", torch.int64, -1), ("info", torch.int64, 0))
GUARD = 64


def raw_outputs(dl, n, limit):
    """tpz_scan_ranges' output columns, each followed by GUARD elements, all bytes 0xA5."""
    out, sizes = {}, {}
    for k, dt, per in RANGE_OUT:
        sizes[k] = 3 if per == 0 else n + 1 if per == -1 else n * (limit if per is None else per)
        out[k] = torch.empty(sizes[k] + GUARD, dtype=dt, device=dl.dev)
        out[k].view(torch.uint8).fill_(0xA5)
    return out, sizes


def run_ranges(dl, cols, out, n, limit, stream=0):
    dl.ctx.scan_ranges_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data,
                            dl.n_levels, *(c.data_ptr() for c in cols), n, limit,
                            *(out[k].data_ptr() for k, _, _ in RANGE_OUT), stream)


def test_capacities_are_respected(ctx):
    case = length_case()
    limit = 8
    models = case.models(limit)
    want = K.expected(models, limit)
    seen = {len(k) for m in models for k, _ in m.entries} | {len(v) for m in models for _, v in m.entries}
    assert any(x < 16 for x in seen) and any(16 <= x <= 256 for x in seen) and any(x > 256 for x in seen)
    assert len({int(p) % 16 for p in want["vpos"][:-1]}) >= 8       # destination offsets
    assert {m.result for m in models} == {S.DONE, S.MORE}
    dl = check(ctx, case, limit)
    n = len(case.ranges)
    out, sizes = raw_outputs(dl, n, limit)
    cols = raw_inputs(dl, case.ranges)
    run_ranges(dl, cols, out, n, limit)
    torch.cuda.synchronize()
    for k, _, _ in RANGE_OUT:                      # nothing is written past a column's end
        tail = out[k][sizes[k]:].view(torch.uint8).cpu().numpy()
        assert (tail == 0xA5).all(), k
    hits = out["hit_table"][:n * limit].cpu().numpy().view(np.uint32).reshape(n, limit)
    for i, m in enumerate(models):                 # ... nor past a scan's count in its hit row
        assert (hits[i, len(m.hits):] == 0xA5A5A5A5).all(), i
    info = out["info"][:3].cpu().numpy()
    n_ent, kbytes, vbytes = (int(x) for x in info)
    assert (n_ent, kbytes, vbytes) == (len(want["kpos"]) - 1, len(want["keys"]), len(want["values"]))

    def gather(key_cap, val_cap):
        kp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
        vp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
        kb = torch.full((kbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        vb = torch.full((vbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        dl.ctx.scan_entries_ptrs(dl.d_tables.data_ptr(), dl.n_tables, n, limit,
                                 out["hit_table"].data_ptr(), out["hit_block"].data_ptr(),
                                 out["hit_entry"].data_ptr(), out["first"].data_ptr(),
                                 kb.data_ptr(), key_cap, kp.data_ptr(), vb.data_ptr(), val_cap,
                                 vp.data_ptr())
        torch.cuda.synchronize()
        assert (kp[n_ent + 1:] == -1).all() and (vp[n_ent + 1:] == -1).all()
        assert np.array_equal(kp[:n_ent + 1].cpu().numpy().astype(np.uint64), want["kpos"])
        assert np.array_equal(vp[:n_ent + 1].cpu().numpy().astype(np.uint64), want["vpos"])
        return kb.cpu().numpy().tobytes(), vb.cpu().numpy().tobytes()

    k, v = gather(kbytes, vbytes)
    assert k[:kbytes] == want["keys"] and k[kbytes:] == b"\xa5" * 256
    assert v[:vbytes] == want["values"] and v[vbytes:] == b"\xa5" * 256
    # capacities inside a wave-copied value / key, inside a lane-copied one, and at 0
    e1000 = next(j for j in range(n_ent) if want["vpos"][j + 1] - want["vpos"][j] == 1000)
    e33 = next(j for j in range(n_ent) if want["vpos"][j + 1] - want["vpos"][j] == 33)
    e300 = next(j for j in range(n_ent) if want["kpos"][j + 1] - want["kpos"][j] > 256)
    for kc, vc in ((int(want["kpos"][e300]) + 100, int(want["vpos"][e1000]) + 499),
                   (int(want["kpos"][e300]) - 3, int(want["vpos"][e33]) + 20), (0, 0)):
        k, v = gather(kc, vc)
        assert k[:kc] == want["keys"][:kc] and k[kc:] == b"\xa5" * (kbytes + 256 - kc), kc
        assert v[:vc] == want["values"][:vc] and v[vc:] == b"\xa5" * (vbytes + 256 - vc), vc


# ------------------------------------------------------------------------------- 8. paging
@pytest.mark.parametrize("i", [0, 4], ids=[K.RANDOM_IDS[0], K.RANDOM_IDS[4]])
def test_pages_of_three(ctx, i):
    """The scan() iterator with page=3 over whole-range scans: the model's unpaged sequence."""
    case = K.random_case(i)
    dl = device_levels(ctx, case.pieces)
    held = sorted({k for lv in case.ents for e in lv for k, _ in e})
    for lo, hi in ((None, None), (("in", held[3]), ("ex", held[-3])), (("ex", held[0]), None)):
        want = S.lsm_scan(case.host, lo, hi, 1 << 20)
        assert want.result == S.DONE and len(want.entries) >= 12 and want.stats["tombstones"] > 0
        assert S.paged_scan(case.host, lo, hi, 3)[0] == want.entries
        assert drain(dl.scan(lo, hi, page=3)) == want.entries


def test_kinds_the_device_cannot_read(ctx):
    """Kinds live in device memory: an out-of-range one gives that scan ERROR / MALFORMED with
    d_where all 0xFFFFFFFF, and its neighbours their answers."""
    case = small_case([[T]], [(None, None)] * 4)
    dl = device_levels(ctx, case.pieces)
    cols = raw_inputs(dl, case.ranges)
    cols[2][1] = 4                               # lower kind past AFTER
    cols[5][2] = _lib.BOUND_AFTER                # AFTER as an upper kind
    out, _ = raw_outputs(dl, 4, 4)
    run_ranges(dl, cols, out, 4, 4)
    torch.cuda.synchronize()
    assert out["result"][:4].tolist() == [S.DONE, S.ERROR, S.ERROR, S.DONE]
    assert out["status"][:4].tolist() == [0, _lib.BLOCK_MALFORMED, _lib.BLOCK_MALFORMED, 0]
    assert (out["where"][:12].cpu().numpy().view(np.uint32) == G.NONE).all()
    assert out["first"][:5].tolist() == [0, 3, 3, 3, 6]


# ------------------------------------------------------------------------------- 9. graph capture
def test_scan_ranges_in_a_graph(ctx):
    """tpz_scan_ranges captured and replayed (tests/test_gpu_graph.py's pattern): an uncaptured
    first call grows the stream's workspace, so the captured one allocates nothing."""
    case = K.random_case(1)
    limit, n = 3, len(case.ranges)
    want = K.expected(case.models(limit), limit)
    dl = device_levels(ctx, case.pieces)
    cols = raw_inputs(dl, case.ranges)
    out, sizes = raw_outputs(dl, n, limit)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run_ranges(dl, cols, out, n, limit, s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            run_ranges(dl, cols, out, n, limit, s.cuda_stream)
    for _ in range(2):
        for k, _, _ in RANGE_OUT:
            out[k].view(torch.uint8).fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        for k in ("result", "status"):
            assert np.array_equal(out[k][:n].cpu().numpy(), want[k]), k
        assert np.array_equal(out["where"][:3 * n].cpu().numpy().view(np.uint32).reshape(n, 3),
                              want["where"])
        for k in ("first", "key_first", "val_first"):
            assert np.array_equal(out[k][:n + 1].cpu().numpy().astype(np.uint64), want[k]), k
        hits = [out[k][:n * limit].cpu().numpy().view(np.uint32).reshape(n, limit)
                for k in ("hit_table", "hit_block", "hit_entry")]
        for i, h in enumerate(want["hits"]):
            for c in range(3):
                assert np.array_equal(hits[c][i, :len(h)], h[:, c]), (i, c)
        assert out["info"][:3].tolist() == [int(want[k][n]) for k in ("first", "key_first", "val_first")]

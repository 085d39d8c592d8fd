"""tpz_get_keys / tpz_get_values (LevelController::get for batches of keys over resident tables,
src/level.rs:427-465) against the line-by-line model of tests/_get_model.py, which
tests/test_get_model.py ties to the closed form and to the reference's own get tests.

Every case compares d_result, d_status, d_table, d_block, d_entry, d_val_pos and the value bytes
with the model, exactly, and first asserts from the model alone that its inputs reach what the
case names. The `*_case` functions build the inputs and the model's answers on the host; the
tests then run the device over them.
"""
import random

import numpy as np
import pytest
import torch

import _get_model as M
import badentry_util as U
from test_bad_entry import TABLES
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels
from topazdb_amd.table import BlockError, DeviceTable, FileObject, ReferencePanic, SsTable

pytestmark = pytest.mark.gpu

ALPHABET = b"ab\x00\xff"


# ------------------------------------------------------------------------------- harness
def flat(levels):
    return [t for lv in levels for t in lv]


def host_levels(pieces):
    out, tid = [], 0
    for lv in pieces:
        out.append([p.host_table(tid + j) for j, p in enumerate(lv)])
        tid += len(lv)
    return out


def device_levels(ctx, pieces, exact_ends=True) -> DeviceLevels:
    return DeviceLevels(ctx, [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom, exact_ends)
                               for p in lv] for lv in pieces])


def model_of(pieces, queries):
    host = host_levels(pieces)
    return [M.level_get(host, q) for q in queries]


def expected_arrays(model):
    n = len(model)
    vpos = np.zeros(n + 1, np.uint64)
    np.cumsum([len(g.value) for g in model], out=vpos[1:])
    return {"result": np.array([g.result for g in model], np.uint8),
            "status": np.array([g.status for g in model], np.uint8),
            "table": np.array([g.table for g in model], np.uint32),
            "block": np.array([g.block for g in model], np.uint32),
            "entry": np.array([g.entry for g in model], np.uint32),
            "val_pos": vpos, "values": b"".join(g.value for g in model)}


def assert_equal(got, model, queries):
    want = expected_arrays(model)
    for k in ("result", "status", "table", "block", "entry", "val_pos"):
        bad = np.nonzero(np.asarray(got[k]) != want[k][:len(got[k])])[0]
        assert len(got[k]) == len(want[k]) and bad.size == 0, \
            (k, int(bad[0]), queries[min(int(bad[0]), len(queries) - 1)] if queries else None,
             got[k][bad[:4]], want[k][bad[:4]])
    assert got["values"] == want["values"]


def check(ctx, pieces, queries, model=None, exact_ends=True) -> DeviceLevels:
    model = model if model is not None else model_of(pieces, queries)
    dl = device_levels(ctx, pieces, exact_ends)
    assert_equal(dl.get_batch(queries), model, queries)
    return dl


def neighbours(k: bytes) -> list[bytes]:
    return [k[:-1] + bytes([(k[-1] + 1) & 0xFF]), k[:-1] + bytes([(k[-1] - 1) & 0xFF]),
            k + b"\0", k[:-1]]


def count(model, result):
    return sum(1 for g in model if g.result == result)


# ------------------------------------------------------------------------------- 1. reference cases
def test_reference_get_cases(ctx, tmp_path):
    """src/level/test.rs:117-183 through SsTable.open and DeviceLevels: get() and get_batch()."""
    for name, (l0, asks) in M.reference_cases().items():
        pieces = [[M.build_pieces(ents, 64) for ents in l0]]
        tables = []
        for j, p in enumerate(pieces[0]):
            path = tmp_path / f"{name}_{j}.sst"
            path.write_bytes(p.image())
            tables.append(SsTable.open(j, FileObject.open(str(path), ctx), ctx))
            assert tables[-1].num_of_blocks() > 1 and tables[-1].bloom is not None
        queries = [k for k, _ in asks]
        model = model_of(pieces, queries)
        assert [(g.value if g.result == M.FOUND else None) for g in model] == [w for _, w in asks]
        dl = DeviceLevels(ctx, [tables])
        assert_equal(dl.get_batch(queries), model, queries)
        for k, want in asks:
            assert dl.get(k) == want, (name, k)
        # the levels below L0 empty, as LevelController::open leaves them (MAX_LEVEL 6)
        dl6 = DeviceLevels(ctx, [tables] + [[] for _ in range(5)])
        assert_equal(dl6.get_batch(queries), model, queries)


# ------------------------------------------------------------------------------- 2. random sets
#          seed, L0, lower levels, block size, tables without a filter (level, table)
RANDOM = [(11, 5, [4, 0, 1], 64, {(0, 1), (1, 2), (3, 0)}),
          (12, 3, [1, 2, 0], 256, {(0, 0), (2, 1)}),
          (13, 0, [0, 1, 4], 64, {(2, 0), (3, 3)}),
          (14, 1, [2, 1, 0], 256, {(0, 0)})]


def random_case(seed, l0, lower, block_size, no_filter):
    rng = random.Random(seed)
    ents = M.random_set(rng, l0, lower, 150, ALPHABET, 12, 0.2, pool=500, min_keys=120)
    pieces = [[M.build_pieces(e, block_size, None if (lv, t) in no_filter else 0.1)
               for t, e in enumerate(tabs)] for lv, tabs in enumerate(ents)]
    held = sorted({k for lv in ents for tab in lv for k, _ in tab})
    qs = list(held)
    for k in held:
        qs += neighbours(k)
    for p in flat(pieces):
        qs += p.first_keys
    qs += [p.first_keys[0] for p in flat(pieces)]            # every table's smallest key
    qs += [b"\x00", b"\xff" * 13, b""]                       # below all, above all, empty
    qs += [bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 14))) for _ in range(100)]
    model = model_of(pieces, qs)
    return ents, pieces, qs, model


@pytest.mark.parametrize("seed,l0,lower,block_size,no_filter", RANDOM,
                         ids=[f"l0_{c[1]}_b{c[3]}" for c in RANDOM])
def test_random_sets(ctx, seed, l0, lower, block_size, no_filter):
    ents, pieces, qs, model = random_case(seed, l0, lower, block_size, no_filter)
    assert 1500 <= len(qs) <= 3500
    assert min(p.ext.size - 1 for p in flat(pieces)) >= (9 if block_size == 256 else 19)
    assert min(count(model, r) for r in (M.FOUND, M.DELETED, M.ABSENT)) >= 50
    first = np.cumsum([0] + [len(lv) for lv in pieces])
    hit_level = {int(np.searchsorted(first, g.table, "right")) - 1 for g in model
                 if g.result in (M.FOUND, M.DELETED)}
    assert hit_level == {lv for lv, tabs in enumerate(pieces) if tabs}
    assert sorted(len(lv) for lv in pieces[1:])[:2] == [0, 1]     # an empty level, a single table
    if l0 >= 2:
        assert sum(1 for g in model if g.result == M.FOUND and g.table < l0 - 1) >= 20
        shadowed = 0                  # newest copy a tombstone, a live value in an older table
        for q, g in zip(qs, model):
            if g.result == M.DELETED:
                order = list(reversed(ents[0])) + [t for lv in ents[1:] for t in lv]
                copies = [dict(t).get(q) for t in order if q in dict(t)]
                shadowed += copies[0] == b"" and any(copies[1:])
        assert shadowed >= 20
    check(ctx, pieces, qs, model)


# ------------------------------------------------------------------------------- 3. filters
def filter_case():
    keys = [b"fk%04d" % i for i in range(400)]
    old = [(k, b"old:" + k) for k in keys[:200]]
    new = [(k, b"new:" + k) for k in keys[:200:2]]              # holds every second key of old
    low = [(k, b"low:" + k) for k in keys[200:300]]
    pieces = [[M.build_pieces(old, 256), M.build_pieces(new, 256)], [M.build_pieces(low, 256)]]
    foreign = M.bloom_of(keys[300:], 0.1)                       # another table's filter
    pieces[0][1].bloom = foreign
    pieces[1][0].bloom = foreign
    return keys, pieces


def test_filter_is_obeyed(ctx):
    keys, pieces = filter_case()
    qs = keys[:300]
    model = model_of(pieces, qs)
    f = M.Bloom(pieces[0][1].bloom)
    rejected = [k for k in keys[:200:2] if not f.may_contain(_lib.xxh3_64(k))]
    assert len(rejected) >= 20                       # held by the newest table, its filter says no
    for k in rejected:                               # ... so the older table answers
        g = model[qs.index(k)]
        assert (g.result, g.table, g.value) == (M.FOUND, 0, b"old:" + k)
    low_rejected = [k for k in keys[200:300] if not f.may_contain(_lib.xxh3_64(k))]
    assert len(low_rejected) >= 20 and all(model[qs.index(k)].result == M.ABSENT for k in low_rejected)
    assert any(g.table == 1 for g in model) and any(g.table == 2 for g in model)   # false positives
    check(ctx, pieces, qs, model)


@pytest.mark.parametrize("filt", [b"", b"\x03"], ids=["empty", "k3_no_bits"])
def test_degenerate_filters(ctx, filt):
    """bloom_kernel's panics: an empty filter; no bit array with k > 0. Every query that reaches
    the table is ERROR with MALFORMED, whatever an older table holds."""
    keys, pieces = filter_case()
    pieces[0][1].bloom = M.bloom_of(keys[:200:2], 0.1)          # honest again
    pieces[0][0].bloom = filt                                   # the older L0 table
    qs = keys[:300]
    model = model_of(pieces, qs)
    errors = [g for g in model if g.result == M.ERROR]
    assert len(errors) >= 100 and count(model, M.FOUND) >= 90   # hits in the newer table stand
    assert all((g.status, g.table, g.block, g.entry) == (_lib.BLOCK_MALFORMED, 0, M.NONE, M.NONE)
               for g in errors)
    dl = check(ctx, pieces, qs, model)
    with pytest.raises(ReferencePanic, match="unwrap" if filt == b"" else "remainder"):
        dl.get(qs[model.index(errors[0])])      # filter.last().unwrap() / `% 0` (bloom.rs:72-84)


def test_zero_probe_filter(ctx):
    """k == 0 with no bit array: may_contain is true (bloom_kernel's 1)."""
    keys, pieces = filter_case()
    pieces[0][1].bloom = b"\x00"
    qs = keys[:200]
    model = model_of(pieces, qs)
    assert count(model, M.ERROR) == 0 and sum(1 for g in model if g.table == 1) == 100
    check(ctx, pieces, qs, model)


# ------------------------------------------------------------------------------- 4. errors
def corrupt_case():
    keys = [b"ek%04d" % i for i in range(300)]
    old = [(k, b"old:" + k) for k in keys]
    mid = [(k, b"mid:" + k) for k in keys[::3]]
    new = [(k, b"new:" + k) for k in keys[::5]]
    pieces = [[M.build_pieces(old, 256), M.build_pieces(mid, 256), M.build_pieces(new, 256)]]
    p = pieces[0][1]
    bad = 3
    region = bytearray(p.region)
    region[int(p.ext[bad]) + 7] ^= 0x80                        # the block's CRC no longer matches
    p.region = bytes(region)                                   # (Pieces.image redoes the file CRC)
    # the seeks that read it: keys of its range, and keys past the last key of the block before
    # it (that block's iterator ends invalid and the seek steps on, table/iterator.rs:62-68)
    lo, hi = max(k for k, _ in mid if k < p.first_keys[bad]), p.first_keys[bad + 1]
    return keys, pieces, bad, lo, hi


def test_errors_end_the_walk(ctx, tmp_path):
    keys, pieces, bad, lo, hi = corrupt_case()
    qs = keys + [k + b"\0" for k in keys]
    model = model_of(pieces, qs)
    f = M.Bloom(pieces[0][1].bloom)
    in_bad = [q for q in qs if lo < q < hi]
    reach = [q for q in in_bad if f.may_contain(_lib.xxh3_64(q))]
    n_err = n_newer = n_rejected = 0
    for q in in_bad:
        g = model[qs.index(q)]
        newer = q in keys[::5]
        if newer:                                   # the newest table answers first
            assert (g.result, g.table) == (M.FOUND, 2)
            n_newer += 1
        elif q in reach:                            # the walk reads the corrupted block
            assert (g.result, g.status, g.table, g.block, g.entry) == \
                (M.ERROR, _lib.BLOCK_CHECKSUM_MISMATCH, 1, bad, 0)
            n_err += 1
        else:                                       # the filter keeps the walk out of it
            assert g.result == (M.FOUND if q in keys else M.ABSENT) and g.table in (0, M.NONE)
            n_rejected += 1
    assert n_err >= 10 and n_newer >= 3 and n_rejected >= 10
    assert sum(1 for q in reach if q in keys and q not in keys[::5]) >= 10   # old holds them
    assert count(model, M.ERROR) == n_err           # ... and no other query errs
    check(ctx, pieces, qs, model)
    # the facade raises the reference's Err for it
    tables = []
    for j, p in enumerate(pieces[0]):
        path = tmp_path / f"c{j}.sst"
        path.write_bytes(p.image())
        tables.append(SsTable.open(j, FileObject.open(str(path), ctx), ctx))
    dl = DeviceLevels(ctx, [tables])
    q = next(q for q in reach if q not in keys[::5])
    with pytest.raises(BlockError, match=r"checksum: expected \d+, actual \d+"):
        dl.get(q)
    assert dl.get(keys[0]) == b"new:" + keys[0] and dl.get(b"zz") is None


def bad_entry_case(spec):
    f, ents = U.table(spec)
    n = sum(m for m, *_ in spec)
    older = [(U.key(i), b"older_%d" % i) for i in range(n)]
    pieces = [[M.build_pieces(older, 128), M.Pieces.from_image(f)]]
    qs = U.probe_keys(n)
    return pieces, qs, model_of(pieces, qs)


@pytest.mark.parametrize("name,spec", TABLES, ids=[t[0] for t in TABLES])
def test_bad_entry_panics_come_through(ctx, name, spec):
    """The seek's panic classes (a BAD_KEY entry read by the bisection, a landing on a BAD_KEY or
    BAD_VALUE entry) in the newest table: ERROR with MALFORMED at that block and entry, although
    the older table holds every key."""
    pieces, qs, model = bad_entry_case(spec)
    errors = [g for g in model if g.result == M.ERROR]
    assert errors and all((g.status, g.table) == (_lib.BLOCK_MALFORMED, 1) for g in errors)
    bad_blocks = {b for b, s in enumerate(spec) if s[1] is not None}
    assert {g.block for g in errors} <= bad_blocks
    assert any(g.result == M.FOUND and g.table == 1 for g in model)     # the other seeks stand
    check(ctx, pieces, qs, model)


# ------------------------------------------------------------------------------- 5. layouts, codecs
def spilled_pieces():
    """Blocks that repeat their sorted entries (each 4 or 7 times): the device keeps them in spill
    records (tests/test_gpu_spill.py test_seek_and_iterate_spilled_blocks)."""
    blocks, fks, keys = [], [], []
    for b in range(4):
        ks = [b"sp%d-key%04d" % (b, i) for i in range(40)]
        ents = [(k, b"" if i % 7 == 3 else b"S" * (50 + i)) for i, k in enumerate(ks)]
        offs, data = U.entries_block(ents)
        rep = [o for o in offs for _ in range(4 + 3 * (b % 2))]
        blocks.append(U.raw_block(rep, bytes(data)))
        fks.append(ks[0])
        keys += ks
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    return M.Pieces(b"".join(blocks), ext, fks, M.bloom_of(keys, 0.1)), keys


def layout_case(codec):
    rng = random.Random(31)
    ents = M.random_set(rng, 2, [2, 1], 120, ALPHABET, 10, 0.2, pool=260)
    pieces = [[M.build_pieces(e, 256, 0.1, codec if (lv + t) % 2 == 0 else None)
               for t, e in enumerate(tabs)] for lv, tabs in enumerate(ents)]
    sp, sp_keys = spilled_pieces()
    pieces[0].insert(1, sp)                                   # L0: oldest, spilled, newest
    qs = sorted({k for lv in ents for tab in lv for k, _ in tab}) + sp_keys
    qs += [k + b"\0" for k in sp_keys[::3]] + [b"", b"sp", b"sp9"]
    return pieces, qs, model_of(pieces, qs)


@pytest.mark.parametrize("codec", [None, "snappy", "lz4"])
@pytest.mark.parametrize("exact_ends", [True, False], ids=["exact", "slotted"])
def test_layouts_and_codecs(ctx, codec, exact_ends):
    pieces, qs, model = layout_case(codec)
    if codec:
        tag = {"snappy": 2, "lz4": 3}[codec]
        assert sum(1 for p in flat(pieces) if p.region[int(p.ext[1]) - 1] == tag) >= 2
    in_sp = [g for g in model if g.table == 1]
    assert sum(1 for g in in_sp if g.result == M.FOUND) >= 100
    assert sum(1 for g in in_sp if g.result == M.DELETED) >= 10
    assert min(count(model, r) for r in (M.FOUND, M.DELETED, M.ABSENT)) >= 10
    dl = check(ctx, pieces, qs, model, exact_ends)
    st = dl.tables[1].cols.status[:4].cpu().numpy()
    assert (st == _lib.BLOCK_OK_SPILLED).all()                # the hits above lie in spill records
    assert (dl.tables[0].cols.entry_first is not None) == exact_ends


# ------------------------------------------------------------------------------- 6. values
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1000, 4000]


def value_case():
    rng = random.Random(61)
    keys = {n: b"len%05d" % n for n in LENGTHS}
    vals = {n: bytes(rng.getrandbits(8) for _ in range(n)) for n in LENGTHS}
    pad = (b"pad", b"\x5a")
    l0 = sorted([(keys[n], vals[n]) for n in LENGTHS[::2]] + [pad])
    l1 = sorted((keys[n], vals[n]) for n in LENGTHS[1::2])
    pieces = [[M.build_pieces(l0, 8192)], [M.build_pieces(l1, 8192, None)]]
    qs, off = [], 0
    for n in LENGTHS:                 # every length at every destination offset mod 16
        for o in range(16):
            while off % 16 != o:
                qs.append(pad[0])
                off += 1
            qs.append(keys[n])
            off += n
    qs += [b"nokey", keys[4000]]
    return pieces, qs, model_of(pieces, qs), keys


def test_values_every_length_and_offset(ctx):
    pieces, qs, model, keys = value_case()
    want = expected_arrays(model)
    seen = {(len(g.value), int(want["val_pos"][i]) % 16) for i, g in enumerate(model)
            if g.result == M.FOUND}
    assert {(n, o) for n in LENGTHS for o in range(16)} <= seen
    dl = check(ctx, pieces, qs, model)
    total = len(want["values"])
    guard = 256
    w = dl.walk(qs)
    torch.cuda.synchronize()
    assert int(w["val_pos"][len(qs)]) == total

    def gather(cap):
        buf = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=dl.dev)
        dl.ctx.get_values_ptrs(dl.d_tables.data_ptr(), dl.n_tables, len(qs), w["result"].data_ptr(),
                               w["table"].data_ptr(), w["block"].data_ptr(), w["entry"].data_ptr(),
                               w["val_pos"].data_ptr(), buf.data_ptr(), cap)
        torch.cuda.synchronize()
        return buf.cpu().numpy().tobytes()

    out = gather(total)
    assert out[:total] == want["values"] and out[total:] == b"\xa5" * guard
    # a capacity inside a lane-copied value, inside a wave-copied one, and at 0
    i4000 = max(i for i, g in enumerate(model) if len(g.value) == 4000 and i < len(qs) - 2)
    i33 = next(i for i, g in enumerate(model) if len(g.value) == 33)
    for cap in (int(want["val_pos"][i4000]) + 1999, int(want["val_pos"][i33]) + 20, 0):
        out = gather(cap)
        assert out[:cap] == want["values"][:cap], cap
        assert out[cap:] == b"\xa5" * (total + guard - cap), cap


# ------------------------------------------------------------------------------- 7. counts, streams
def count_case():
    rng = random.Random(71)
    ents = M.random_set(rng, 3, [3, 2], 60, ALPHABET, 8, 0.2, pool=200)
    pieces = [[M.build_pieces(e, 128) for e in tabs] for tabs in ents]
    held = sorted({k for lv in ents for tab in lv for k, _ in tab})
    qs = [held[rng.randrange(len(held))] if rng.random() < 0.7 else M.random_key(rng, ALPHABET, 8)
          for _ in range(2000)]
    return pieces, qs, model_of(pieces, qs)


def test_query_counts_and_two_streams(ctx):
    pieces, qs, model = count_case()
    assert min(count(model, r) for r in (M.FOUND, M.DELETED, M.ABSENT)) >= 100
    dl = device_levels(ctx, pieces)
    for n in (0, 1, 63, 64, 65, 257, 2000):
        got = dl.get_batch(qs[:n])
        assert_equal(got, model[:n], qs[:n])
        assert len(got["val_pos"]) == n + 1 and got["val_pos"][0] == 0
    # two streams at once, different query sets: the same answers as alone (both walks are in
    # flight before anything is read back, then both gathers)
    sets = [(qs[:1100], model[:1100]), (qs[900:], model[900:])]
    streams = [torch.cuda.Stream(dl.dev) for _ in sets]
    torch.cuda.synchronize()
    walks = []
    for s, (q, _) in zip(streams, sets):
        with torch.cuda.stream(s):
            walks.append(dl.walk(q))
    torch.cuda.synchronize()
    totals = [int(w["val_pos"][w["n"]].item()) for w in walks]
    vals = []
    for s, w, total in zip(streams, walks, totals):
        with torch.cuda.stream(s):
            vals.append(dl.values(w, total))
    torch.cuda.synchronize()
    for w, v, (q, m) in zip(walks, vals, sets):
        got = {k: w[k][:w["n"]].cpu().numpy() for k in ("result", "status")}
        for k in ("table", "block", "entry"):
            got[k] = w[k][:w["n"]].cpu().numpy().view(np.uint32)
        got["val_pos"] = w["val_pos"].cpu().numpy().astype(np.uint64)
        got["values"] = v.cpu().numpy().tobytes()
        assert_equal(got, m, q)


def mixed_filter_case():
    """Table 0 (the oldest of L0) without a filter, every later table with one; the queries are
    keys that only filtered tables hold, so a probe with a wrong hash loses them."""
    keys = [b"mx%04d" % i for i in range(240)]
    old = [(k, b"old:" + k) for k in keys[:40]]
    mid = [(k, b"mid:" + k) for k in keys[40:120]]
    new = [(k, b"new:" + k) for k in keys[120:160]]
    low = [(k, b"low:" + k) for k in keys[160:240]]
    pieces = [[M.build_pieces(old, 128, None), M.build_pieces(mid, 128), M.build_pieces(new, 128)],
              [M.build_pieces(low, 128)]]
    qs = (keys[40:160:2] + keys[160:240:8])[:65]
    return pieces, qs, model_of(pieces, qs)


def test_partial_wave_over_mixed_filters(ctx):
    """Whether the key gets hashed must not depend on the number of queries in a wave: with 1 or
    65 queries the last wave holds one, and the only table that lane would look at has no
    filter."""
    pieces, qs, model = mixed_filter_case()
    assert len(qs) == 65 and all(g.result == M.FOUND and g.table >= 1 for g in model)
    assert pieces[0][0].bloom is None and all(p.bloom for p in flat(pieces)[1:])
    assert model[0].table != model[64].table          # the single lanes' keys: L0 and level 1
    dl = device_levels(ctx, pieces)
    for n in (1, 65, 2, 64):
        assert_equal(dl.get_batch(qs[:n]), model[:n], qs[:n])
    assert_equal(dl.get_batch(qs[64:]), model[64:], qs[64:])
    for q, g in list(zip(qs, model))[::8]:
        assert dl.get(q) == g.value


def test_no_tables_and_no_levels(ctx):
    """With no tables every query is ABSENT: no level at all, and six empty levels."""
    qs = [b"a", b"", b"key_0001"]
    for levels in ([], [[] for _ in range(6)]):
        got = DeviceLevels(ctx, levels).get_batch(qs)
        assert_equal(got, [M.Get(M.ABSENT, 0, M.NONE, M.NONE, M.NONE, b"")] * 3, qs)
        assert DeviceLevels(ctx, levels).get(b"a") is None


def test_no_keys(ctx):
    """n_keys == 0 over one small table: tpz_get_keys zeroes the 8 bytes at d_val_pos and writes
    nothing else; tpz_get_values succeeds without touching d_vals (also with val_cap == 0 and
    keys to gather)."""
    ents = [(b"a", b"1"), (b"b", b"22"), (b"c", b"")]
    dl = device_levels(ctx, [[M.build_pieces(ents, 64)]])
    assert_equal(dl.get_batch([]), [], [])
    dev, stream = dl.dev, torch.cuda.current_stream(dl.dev).cuda_stream
    cols = {k: torch.full((2,), 0x5A, dtype=t, device=dev) for k, t in
            (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
             ("block", torch.int32), ("entry", torch.int32), ("val_pos", torch.int64))}
    qp = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.get_keys_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
                      0, qp.data_ptr(), 0, *(cols[k].data_ptr() for k in cols), stream)
    vals = torch.full((16,), 0x5A, dtype=torch.uint8, device=dev)
    args = [cols[k].data_ptr() for k in ("result", "table", "block", "entry", "val_pos")]
    ctx.get_values_ptrs(dl.d_tables.data_ptr(), dl.n_tables, 0, *args, vals.data_ptr(), 16, stream)
    ctx.get_values_ptrs(dl.d_tables.data_ptr(), dl.n_tables, 2, *args, vals.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert cols["val_pos"].tolist() == [0, 0x5A]
    for k in ("result", "status", "table", "block", "entry"):
        assert cols[k].tolist() == [0x5A, 0x5A], k
    assert vals.tolist() == [0x5A] * 16

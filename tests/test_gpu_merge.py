"""tpz_merge_runs (compaction's MergeIterator on the device) against the closed-form rule of
tests/_merge_model.py (which tests/test_merge_model.py pins to the reference's create / next):
n_out, every key byte, every value byte, every position and d_src_entry, exactly. Cases: run
counts up to TPZ_MERGE_MAX_RUNS (odd tree levels included), empty runs, run lengths around the
tile of the tile-merge kernel, key shapes that defeat the 8-byte prefix, every run shape of the
tie rule, tombstones, empty keys, argument checks, and the merged entries fed to the write side.
"""
import random

import numpy as np
import pytest
import torch

from _merge_model import merge_rule
from test_encode_host import pack
from topazdb_amd import _lib, synth
from topazdb_amd.compact import merge_runs
from topazdb_amd.encode import DeviceEntries, EntryError, encode_blocks_async, plan_blocks_async

pytestmark = pytest.mark.gpu

T = _lib.MERGE_TILE   # entries per tile-merge workgroup


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def value_for(rng: random.Random, r: int, j: int) -> bytes:
    """A value that names its entry, 0..300 bytes; about one in six is a tombstone."""
    if rng.random() < 0.16:
        return b""
    tag = b"%d:%d|" % (r, j)
    return (tag * (300 // len(tag) + 1))[:rng.randint(1, 300)]


def make_runs(rng: random.Random, key_lists) -> list:
    """Runs from lists of keys: each sorted, with values."""
    return [[(k, value_for(rng, r, j)) for j, k in enumerate(sorted(keys))]
            for r, keys in enumerate(key_lists)]


def assert_merge(ctx, runs):
    """The device's merge of `runs` equals the rule; returns (merged DeviceEntries, wanted kvs)."""
    flat = [kv for run in runs for kv in run]
    run_first = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    merged, src, info = merge_runs(ctx, DeviceEntries(*pack(flat)), run_first)
    rj = merge_rule(runs)
    want = [runs[r][j] for r, j in rj]
    wk, wkpos, wv, wvpos = pack(want)
    assert int(info[0]) == len(want) == merged.n
    assert int(info[1]) == len(wk) and int(info[2]) == len(wv) and int(info[3]) == 2**64 - 1
    assert src.cpu().numpy().tolist() == [int(run_first[r]) + j for r, j in rj]
    np.testing.assert_array_equal(merged.kpos.cpu().numpy().view(np.uint64), wkpos)
    np.testing.assert_array_equal(merged.vpos.cpu().numpy().view(np.uint64), wvpos)
    assert merged.keys[:len(wk)].cpu().numpy().tobytes() == wk.tobytes()
    assert merged.vals[:len(wv)].cpu().numpy().tobytes() == wv.tobytes()
    return merged, want


def random_keys(rng: random.Random, n: int, space: int, kmax: int = 12) -> list:
    """n keys drawn (with repeats) from a space of `space` keys of 1..kmax bytes."""
    pool_rng = random.Random(space * 7919 + kmax)
    pool = [bytes(pool_rng.getrandbits(8) for _ in range(pool_rng.randint(1, kmax)))
            for _ in range(space)]
    return [rng.choice(pool) for _ in range(n)]


@pytest.mark.parametrize("n_runs", [0, 1, 2, 3, 5, 8, _lib.MERGE_MAX_RUNS])
def test_run_counts(ctx, n_runs):
    """R = 3 and 5 leave an odd list at a tree level (copied through); R = 256 runs all 8 levels."""
    rng = random.Random(n_runs)
    per = 60 if n_runs > 8 else 900
    runs = make_runs(rng, [random_keys(rng, rng.randint(per // 2, per), 4 * per)
                           for _ in range(n_runs)])
    assert_merge(ctx, runs)


def test_too_many_runs_and_bad_run_tables(ctx):
    kvs = [(b"k%03d" % i, b"v") for i in range(10)]
    ent = DeviceEntries(*pack(kvs))
    with pytest.raises(_lib.TpzError):
        merge_runs(ctx, ent, [0] * _lib.MERGE_MAX_RUNS + [10, 10])      # 257 runs
    for rf in ([1, 10], [0, 7, 5, 10], [0, 4, 9], [0, 4, 11]):
        with pytest.raises(_lib.TpzError):
            merge_runs(ctx, ent, rf)
    merged, src, info = merge_runs(ctx, ent, [0, 4, 10])                 # (the table itself is fine)
    assert merged.n == 10


def test_misaligned_outputs_and_optional_source_column(ctx):
    runs = make_runs(random.Random(5), [[b"a", b"c"], [b"b", b"c"]])
    flat = [kv for run in runs for kv in run]
    ent = DeviceEntries(*pack(flat))
    rf = np.array([0, 2, 4], np.uint32)
    dev = torch.device("cuda", 0)
    ok = torch.empty(64, dtype=torch.uint8, device=dev)
    ov = torch.empty(2048, dtype=torch.uint8, device=dev)
    kp = torch.empty(5, dtype=torch.int64, device=dev)
    vp = torch.empty(5, dtype=torch.int64, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    for dk, dv in ((1, 0), (0, 8)):
        with pytest.raises(_lib.TpzError):
            ctx.merge_runs_ptrs(ent.struct(), rf.ctypes.data, 2, ok.data_ptr() + dk, kp.data_ptr(),
                                ov.data_ptr() + dv, vp.data_ptr(), 0, info.data_ptr(), 0)
    ctx.merge_runs_ptrs(ent.struct(), rf.ctypes.data, 2, ok.data_ptr(), kp.data_ptr(),
                        ov.data_ptr(), vp.data_ptr(), 0, info.data_ptr(), 0)     # d_src_entry NULL
    torch.cuda.synchronize()
    assert int(info[0]) == 3 and ok[:3].cpu().numpy().tobytes() == b"abc"


@pytest.mark.parametrize("empty", [[0], [2], [4], [0, 1, 4], [0, 1, 2, 3, 4]])
def test_empty_runs(ctx, empty):
    """Empty runs first, in the middle, last, and nothing but empty runs."""
    rng = random.Random(len(empty) * 10 + empty[0])
    runs = make_runs(rng, [[] if r in empty else random_keys(rng, 300, 500) for r in range(5)])
    assert_merge(ctx, runs)


@pytest.mark.parametrize("la,lb", [(T - 1, T - 1), (T - 1, T), (T, T), (T + 1, T), (T + 1, T + 1),
                                   (T + 5, T + 7), (1, 2 * T), (2 * T + 1, 1), (T, 0)])
def test_run_lengths_around_the_tile(ctx, la, lb):
    """Pairs of runs of T - 1, T and T + 1 entries; T + 5 with T + 7 crosses two tile boundaries.
    Keys interleave (even / odd counters) with a shared stretch in the middle."""
    rng = random.Random(la * 31 + lb)
    a = [b"%08d" % (2 * i) for i in range(la)]
    b = [b"%08d" % (2 * i + (0 if la // 3 < i < la // 2 else 1)) for i in range(lb)]
    assert_merge(ctx, make_runs(rng, [a, b]))
    assert_merge(ctx, make_runs(rng, [b, a, a[: T // 2]]))


def test_key_shapes(ctx):
    """Lengths 1..40 and 65,535; keys equal in their first 8, 16 and 17 bytes that differ later or
    only in length; bytes >= 0x80 (the compare is unsigned)."""
    rng = random.Random(77)
    fam = []
    for plen in (8, 16, 17):
        p = bytes(range(0x41, 0x41 + plen))
        fam += [p, p + b"\x00", p + b"\x00\x00", p + b"\x01", p + b"\xff", p + b"a" * 7 + b"b",
                p + b"a" * 7 + b"c", p + b"a" * 8, p[:-1], p[:-1] + b"\x80"]
    fam += [b"a", b"a\x00", b"a\x00\x00", b"\x00", b"\x00\x00", b"\x7f", b"\x80", b"\xff" * 9,
            b"\xff" * 8, b"\x80" * 8 + b"\x7f", b"\x80" * 8 + b"\x80"]
    long_a = bytes(rng.getrandbits(8) for _ in range(65534))
    fam += [long_a + b"\x01", long_a + b"\x02", long_a]
    lens = [bytes(rng.getrandbits(8) for _ in range(n)) for n in range(1, 41) for _ in range(3)]
    allk = fam + lens
    key_lists = [[k for k in allk if rng.random() < 0.6] for _ in range(4)]
    key_lists[2].append(long_a + b"\x01")     # the longest key in two runs at least
    key_lists[3].append(long_a + b"\x01")
    assert_merge(ctx, make_runs(rng, key_lists))


def test_run_shapes(ctx):
    rng = random.Random(9)
    # every key equal across all runs (one group of 8 x 40 entries: one winner run)
    assert_merge(ctx, make_runs(rng, [[b"same-key-0123"] * 40 for _ in range(8)]))
    # every run holds the same key set
    keys = [b"key%05d" % i for i in range(700)]
    assert_merge(ctx, make_runs(rng, [list(keys) for _ in range(5)]))
    # two one-entry runs with the same key
    merged, want = assert_merge(ctx, [[(b"k", b"first")], [(b"k", b"second")]])
    assert want == [(b"k", b"first")]
    # disjoint runs, in and against run order
    assert_merge(ctx, make_runs(rng, [[b"%d%04d" % (r, i) for i in range(1500)] for r in range(3)]))
    assert_merge(ctx, make_runs(rng, [[b"%d%04d" % (9 - r, i) for i in range(1500)] for r in range(3)]))
    # fully interleaved runs
    assert_merge(ctx, make_runs(rng, [[b"%06d" % (4 * i + r) for i in range(1300)] for r in range(4)]))
    # a key repeated inside the winning run (all copies stay) and inside a losing run (all go),
    # the repeats longer than a tile
    runs = make_runs(rng, [[b"a"] + [b"dup"] * (T + 3) + [b"z"],
                           [b"b"] + [b"dup"] * (T + 9) + [b"lose"] * 3 + [b"y"],
                           [b"lose"] * 5 + [b"dup"] * 2])
    merged, want = assert_merge(ctx, runs)
    assert [k for k, _ in want].count(b"dup") == T + 3 and [k for k, _ in want].count(b"lose") == 3


def test_tombstones_survive(ctx):
    runs = [[(b"a", b""), (b"c", b"")], [(b"a", b"old"), (b"b", b""), (b"c", b"old")]]
    merged, want = assert_merge(ctx, runs)
    assert want == [(b"a", b""), (b"b", b""), (b"c", b"")]


def test_empty_key_is_reported(ctx):
    kvs0 = [(b"a", b"1"), (b"b", b"2")]
    kvs1 = [(b"", b"x"), (b"", b"y"), (b"c", b"3")]
    ent = DeviceEntries(*pack(kvs0 + kvs1))
    with pytest.raises(EntryError) as e:
        merge_runs(ctx, ent, [0, 2, 5])
    assert e.value.index == 2                 # d_info[3]: the first input entry with an empty key


@pytest.mark.parametrize("block_size", [256, 4096])
def test_merged_entries_feed_the_write_side(ctx, block_size):
    """tpz_merge_runs' output is a tpz_entries: plan + encode it on the device, and the region is
    the host builder's over the model's entries."""
    rng = random.Random(block_size)
    runs = make_runs(rng, [random_keys(rng, 2500, 6000, kmax=24) for _ in range(3)])
    runs = [[(k, v[:150]) for k, v in run] for run in runs]
    merged, want = assert_merge(ctx, runs)
    first, ext, info = plan_blocks_async(ctx, merged, block_size)
    out = encode_blocks_async(ctx, merged, first, ext, info)
    torch.cuda.synchronize()
    o_region, o_ext = synth.build_blocks(*pack(want), block_size)
    _, bad, nb = info[:3].cpu().numpy().view(np.uint32).tolist()
    assert bad == 0xFFFFFFFF and nb == len(o_ext) - 1
    assert ext[:nb + 1].cpu().numpy().view(np.uint64).tolist() == o_ext.tolist()
    assert out[:int(o_ext[-1])].cpu().numpy().tobytes() == o_region.tobytes()

"""The closed-form rules of tpz_mem_build (tests/_membuild_model.py: closed_replay, closed_put)
equal the line-by-line restatement of WalIterator, MemTable::open and do_mem_put on random batches
with duplicate keys and versions in blocks. No GPU needed."""
import random

import pytest

import _membuild_model as M
from topazdb_amd.memtable import wal_encode


def random_entries(rng, n, n_keys, empty_keys=False, max_val=40):
    keys = [bytes(rng.randrange(256) for _ in range(rng.randrange(0 if empty_keys else 1, 12)))
            for _ in range(n_keys)]
    return [(rng.choice(keys), bytes(rng.randrange(256) for _ in range(rng.randrange(max_val))))
            for _ in range(n)]


def block_versions(rng, n, lo=1, hi=50):
    out, v = [], 0
    while len(out) < n:
        v += rng.randrange(1, 4)
        out += [v] * rng.randrange(lo, hi + 1)
    return out[:n]


def as_map(entries, win, versions=None):
    return {entries[i][0]: (entries[i][1], 0 if versions is None else versions[i]) for i in win}


@pytest.mark.parametrize("seed", range(12))
def test_closed_put_equals_do_mem_put(seed):
    rng = random.Random(seed)
    n = rng.randrange(1, 600)
    ent = random_entries(rng, n, rng.randrange(1, 80), empty_keys=True)
    ver = block_versions(rng, n)
    m, size = M.model_put(ent, ver)
    win, csize, stop, used = M.closed_put(ent, ver)
    assert as_map(ent, win, ver) == m
    assert [ent[i][0] for i in win] == sorted(m)
    assert csize == size and used == n
    assert stop == next((i for i, (k, _) in enumerate(ent) if not k), M.NONE)


@pytest.mark.parametrize("seed", range(12))
def test_closed_replay_equals_open(seed):
    rng = random.Random(100 + seed)
    n = rng.randrange(1, 600)
    ent = random_entries(rng, n, rng.randrange(1, 80), empty_keys=seed % 3 == 0)
    m, size = M.mem_open(wal_encode(ent))
    win, csize, stop, used = M.closed_replay(ent)
    assert as_map(ent, win) == m and csize == size
    assert used == (n if stop == M.NONE else stop)
    assert all(ent[i][0] for i in win)


def test_one_batch_first_wins_replay_last_wins():
    batch = [(b"k", b"first"), (b"j", b"x"), (b"k", b"second!"), (b"k", b"3")]
    m, size = M.model_put(batch, [7] * 4)
    assert m[b"k"] == (b"first", 7)
    # the turned-away duplicates still move size (compare_insert returns the entry it kept, whose
    # version equals theirs): +6, +2, then "second!" >= "first": +2, then "3" < "first": -(5 + 1)
    assert size == 6 + 2 + 2 - 6
    assert M.closed_put(batch, [7] * 4)[:2] == ([1, 0], size)
    r, rsize = M.mem_open(wal_encode(batch))
    assert r[b"k"] == (b"3", 0)
    assert rsize == sum(len(k) + len(v) for k, v in batch)
    assert M.closed_replay(batch)[:2] == ([1, 3], rsize)


def test_a_later_version_replaces():
    ent = [(b"k", b"aaaa"), (b"k", b"bb"), (b"k", b"cccccc"), (b"k", b"d")]
    ver = [1, 1, 2, 3]
    m, size = M.model_put(ent, ver)
    assert m[b"k"] == (b"d", 3)
    assert M.closed_put(ent, ver) == ([3], size, M.NONE, 4)


def test_size_underflows_when_a_long_value_is_replaced_by_a_short_one():
    ent = [(b"key", b"v" * 100), (b"key", b"w")]
    m, size = M.model_put(ent, [1, 2])
    # :193: sub = old_size - klen + vlen = 103 - 3 + 1 = 101; 103 - 101 = 2 (the map holds 4 bytes)
    assert m[b"key"] == (b"w", 2) and size == 2
    ent = [(b"key", b"v" * 10), (b"key", b"w" * 9), (b"key", b""), (b"key", b"")]
    m, size = M.model_put(ent, [1, 2, 3, 4])
    # 13, then -(10 + 9) wraps below zero, then -(9 + 0), then +0
    assert size == (13 - 19 - 9) % 2**64 and size > 2**63
    assert M.closed_put(ent, [1, 2, 3, 4])[1] == size


def test_wal_walk_follows_the_iterator():
    ent = [(b"a", b"1"), (b"", b"zz"), (b"b", b"2")]
    img = wal_encode(ent)
    assert M.wal_walk(img) == ([0, 6, 12], 1, M.NONE)
    assert M.wal_walk(img[:5]) == ([0], 2, 0)
    assert M.wal_walk(b"") == ([0], 0, M.NONE)
    assert M.wal_walk(img[:6]) == ([0, 6], 0, M.NONE)

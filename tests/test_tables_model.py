"""tests/_tables_model.py pinned on cases worked out by hand from src/table/builder.rs and
src/level.rs:206-220 (CPU only).

The shape: keys and values of 4 bytes, so Entry::encode is 12 bytes; block_size 30 takes two
entries (24 + 2 <= 30) and refuses the third (36 + 2 > 30). A stored block is 2 + 24 + 2 * 2 + 4 + 1
= 35 bytes. estimated_size() after block j is built is 35 (j + 1) + 2 (j + 1) = 37 (j + 1): 37, 74,
111, ... It only changes inside the add() that builds a block, and that add() puts its entry into a
fresh block before the loop tests reach_capacity() again."""
import pytest

import _tables_model as M
from _tables_model import sub_compact, task_tables

BS = 30


def ents(n: int, lo: int = 0):
    return [(b"k%03d" % i, b"v%03d" % i) for i in range(lo, lo + n)]


def test_the_shape_is_what_the_docstring_says():
    assert M.stored_plain(ents(2)) == 35
    assert sub_compact(ents(5), BS) == [[[0, 1], [2, 3], [4]]]
    assert M.cumulative_sizes(ents(6), BS) == [37, 74, 111]


def test_capacity_equal_to_the_size_at_block_1_cuts_there():
    """74 >= 74: the add of entry 4 built block 1, entry 4 sits alone in block 2, the table ends."""
    assert sub_compact(ents(10), BS, capacity=74) == [[[0, 1], [2, 3], [4]], [[5, 6], [7, 8], [9]]]


def test_capacity_one_more_cuts_a_block_later():
    """74 < 75 (`>=`, not `>`): the cut comes when block 2 is built (111), entry 6 alone after it."""
    assert sub_compact(ents(10), BS, capacity=75) == [[[0, 1], [2, 3], [4, 5], [6]], [[7, 8], [9]]]


def test_the_singleton_is_the_ranges_last_entry():
    """No empty table follows: the outer loop tests is_valid() first (level.rs:206)."""
    assert sub_compact(ents(5), BS, capacity=74) == [[[0, 1], [2, 3], [4]]]


def test_a_range_ending_on_a_block_boundary():
    """Block 1 is only built by build(): no add() follows it, so the size is never tested at 74."""
    assert sub_compact(ents(4), BS, capacity=74) == [[[0, 1], [2, 3]]]
    assert sub_compact(ents(6), BS, capacity=74) == [[[0, 1], [2, 3], [4]], [[5]]]


def test_capacity_1():
    """Every table is one full block and the entry that built it."""
    assert sub_compact(ents(10), BS, capacity=1) == [
        [[0, 1], [2]], [[3, 4], [5]], [[6, 7], [8]], [[9]]]
    assert sub_compact(ents(1), BS, capacity=1) == [[[0]]]
    assert sub_compact([], BS, capacity=1) == []


def test_the_stored_length_is_what_counts():
    """With a codec that stores every block in 10 bytes the size after block j is 12 (j + 1)."""
    got = sub_compact(ents(12), BS, capacity=36, stored_len=lambda b: 10)
    assert got == [[[0, 1], [2, 3], [4, 5], [6]], [[7, 8], [9, 10], [11]]]


def test_an_entry_no_block_holds():
    with pytest.raises(ValueError) as e:
        sub_compact(ents(3) + [(b"k", b"v" * 30)], BS)
    assert e.value.args[0] == 3


def test_task_tables_bounds_and_order():
    """Two runs (run 0 wins k002), ranges [k001, k004) and [k004, k006]: k000 and k007 are outside
    every range, each range starts a table of its own."""
    runs = [ents(3, 1), [(b"k%03d" % i, b"w%03d" % i) for i in (0, 2, 4, 5, 6, 7)]]
    bounds = [(b"k004", (b"k006", True)), (b"k001", (b"k004", False))]
    merged, tables = task_tables(runs, bounds, BS)
    assert [k for k, _ in merged] == [b"k%03d" % i for i in range(8)]
    assert merged[2] == (b"k002", b"v002")
    assert tables == [(1, 3, [1, 3]), (4, 3, [4, 6])]
    assert all(M.blocks_are_greedy_plan(merged, t, BS) for t in tables)
    assert M.in_bounds(merged, b"k0035", (b"k0035", True)) == (4, 4)        # between keys: empty
    assert M.in_bounds(merged, b"k009", (b"k001", True)) == (8, 8)         # upper below lower


@pytest.mark.parametrize("capacity", [1, 74, 75, 200, 1 << 26])
def test_every_table_is_the_greedy_plan_of_its_own_entries(capacity):
    """The singleton did not fit the block before it, so cutting the table there changes no block
    boundary: the cut positions are the only new thing (entries of mixed sizes)."""
    kvs = [(b"k%04d" % i, b"v" * (i * 7 % 23)) for i in range(300)]
    merged, tables = task_tables([kvs], [(b"k", (b"l", False))], 64, capacity)
    assert sum(t[1] for t in tables) == 300 and tables[0][0] == 0
    assert all(M.blocks_are_greedy_plan(merged, t, 64) for t in tables)
    if capacity == 1 << 26:
        assert len(tables) == 1

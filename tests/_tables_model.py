"""What a compaction task's sub-compactions write, restated (test infrastructure, CPU only).

`sub_compact` follows the two loops of the reference's sub_compact (src/level.rs:206-220) and the
SsTableBuilder they drive (src/table/builder.rs:49-94, BlockBuilder::add src/block/builder.rs:26-41)
over a list of merged entries that already lie inside the range's bounds. The table capacity is a
parameter (TABLE_CAPACITY, builder.rs:27) and so is the length a block has once it is stored (the
codec's output): the builder's estimated size only grows by that when add() builds a block.

`task_tables` applies it to a whole task: the merge model's entries (tests/_merge_model.py), cut at
the ranges' bounds as sub_compact's seek (level.rs:188-195) and key_vaild (:199-205) do, one
sub_compact per range, the tables sorted by smallest key (do_compact, :167).
`blocks_are_greedy_plan` checks a table's blocks against the write side's oracle
(_oracle.build_blocks): a table's blocks are the greedy plan of the table's own entries.
"""
from __future__ import annotations

import numpy as np

from _merge_model import merged_entries

TABLE_CAPACITY = 64 * 1024 * 1024      # src/table/builder.rs:27


def stored_plain(block) -> int:
    """A block's length under CompressOptions::Uncompress: n, the entries (Entry::encode: two
    u16 lengths, key, value), n u16 offsets, the CRC and the tag (src/block.rs:31-44,
    src/block/compress.rs:85-89)."""
    return 2 + sum(4 + len(k) + len(v) for k, v in block) + 2 * len(block) + 4 + 1


def sub_compact(entries, block_size: int, capacity: int = TABLE_CAPACITY,
                stored_len=stored_plain):
    """The tables one sub_compact builds from `entries` [(key, value)]: a list of tables, each a
    list of blocks, each a list of entry indices."""
    tables, i, n = [], 0, len(entries)
    while i < n:                                   # level.rs:206  iter.is_valid() && key_vaild
        blocks, cur, size, data_len = [], [], 0, 0          # SsTableBuilder::new
        # :209  !build.reach_capacity(): data.len() + meta.len() * 2 >= TABLE_CAPACITY
        while i < n and not data_len + 2 * len(blocks) >= capacity:
            k, v = entries[i]
            assert k, "key must not be empty"                          # block/builder.rs:27
            el = 4 + len(k) + len(v)
            if el + size + 2 > block_size:         # BlockBuilder::add refuses: block_build, add again
                if not cur:
                    raise ValueError(i)            # no block holds it: add recurses without end
                data_len += stored_len([entries[j] for j in cur])     # builder.rs:74-84
                blocks.append(cur)
                cur, size = [], 0
                if el + 2 > block_size:
                    raise ValueError(i)
            cur.append(i)
            size += el
            i += 1                                 # :211 iter.next()
        blocks.append(cur)                         # build(): block_build of the open block
        tables.append(blocks)
    return tables


def in_bounds(entries, lower: bytes, upper):
    """[lo, hi): the entries sub_compact(lower, upper) reads: from the first key >= lower up to the
    last key <= upper (Included) or < upper (Excluded)."""
    key, inclusive = upper
    lo = sum(1 for k, _ in entries if k < lower)
    hi = sum(1 for k, _ in entries if (k <= key if inclusive else k < key))
    return lo, max(hi, lo)


def task_tables(runs, bounds, block_size: int, capacity: int = TABLE_CAPACITY,
                stored_len=stored_plain):
    """(merged, tables): the merged entries of `runs` and the task's output tables in key order,
    each (first entry, entry count, [each block's first entry]) in merged indices."""
    merged = merged_entries(runs)
    out = []
    for lower, upper in bounds:
        lo, hi = in_bounds(merged, lower, upper)
        for blocks in sub_compact(merged[lo:hi], block_size, capacity, stored_len):
            out.append((lo + blocks[0][0], sum(map(len, blocks)), [lo + b[0] for b in blocks]))
    out.sort(key=lambda t: t[0])
    return merged, out


def pack(kvs):
    kl = np.array([len(k) for k, _ in kvs], np.uint64)
    vl = np.array([len(v) for _, v in kvs], np.uint64)
    kpos = np.zeros(len(kvs) + 1, np.uint64)
    vpos = np.zeros(len(kvs) + 1, np.uint64)
    np.cumsum(kl, out=kpos[1:])
    np.cumsum(vl, out=vpos[1:])
    return (np.frombuffer(b"".join(k for k, _ in kvs) or b"\0", np.uint8), kpos,
            np.frombuffer(b"".join(v for _, v in kvs) or b"\0", np.uint8), vpos)


def blocks_are_greedy_plan(merged, table, block_size: int) -> bool:
    """The table's block starts equal the oracle builder's over the table's own entries."""
    import _oracle as O
    t0, n, firsts = table
    _, _, first = O.build_blocks(*pack(merged[t0:t0 + n]), block_size)
    return [t0 + int(f) for f in first[:-1]] == firsts


def cumulative_sizes(entries, block_size: int):
    """estimated_size() after each block of one unbounded table over `entries`: ext[j + 1] +
    2 (j + 1) for j = 0.. (the values a capacity is compared with)."""
    import _oracle as O
    _, ext, _ = O.build_blocks(*pack(entries), block_size)
    return [int(ext[j + 1]) + 2 * (j + 1) for j in range(len(ext) - 1)]

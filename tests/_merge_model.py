"""What compaction's MergeIterator yields, restated twice (test infrastructure, CPU only).

`merge_iterator` follows MergeIterator::create / next of the reference line by line
(src/iterators/merge_iterator.rs:46-105) over plain lists; `merge_rule` is the closed form the
device merge implements (include/tpz_gpu.h, tpz_merge_runs). tests/test_merge_model.py checks
that the two agree; the GPU tests compare the device against `merge_rule`.

A run is a list of (key, value) pairs sorted non-decreasing by key (bytes compare as Rust's [u8]
Ord does: bytewise, unsigned, a proper prefix is smaller). Both functions return the yielded
entries as (run, position) pairs in yield order.
"""
from __future__ import annotations


class _Iter:
    """A run as a StorageIterator: key() / next() / is_valid()."""

    def __init__(self, run: int, entries):
        self.run, self.entries, self.pos = run, entries, 0

    def is_valid(self) -> bool:
        return self.pos < len(self.entries)

    def key(self) -> bytes:
        return self.entries[self.pos][0]

    def next(self) -> None:
        self.pos += 1


def merge_iterator(runs) -> list[tuple[int, int]]:
    """MergeIterator::create (:46-57) and the loop `while iter.is_valid() { add; iter.next() }`
    of sub_compact (src/level.rs:201-212). The BinaryHeap of HeapWrapper(index, iter) is a list
    whose top is the minimum of (key, index): HeapWrapper's ordering reversed (:21-29)."""
    # :47-52  filter(is_valid) -> enumerate -> heap: the index counts the non-empty iterators
    heap = [[idx, it] for idx, it in
            enumerate(it for it in (_Iter(r, e) for r, e in enumerate(runs)) if it.is_valid())]

    def top():
        return min(heap, key=lambda w: (w[1].key(), w[0])) if heap else None

    def pop():
        w = top()
        if w is not None:
            heap.remove(w)
        return w

    current = pop()                                            # :54
    out = []
    while current is not None:                                 # is_valid, :71-73
        out.append((current[1].run, current[1].pos))           # key() / value(), :63-69
        key = current[1].key()                                 # :76
        while True:                                            # :78-88
            inner = top()
            if inner is None or key != inner[1].key():
                break
            inner[1].next()
            if not inner[1].is_valid():
                heap.remove(inner)
        current[1].next()                                      # :91
        if not current[1].is_valid():                          # :93-96
            current = pop()
            continue
        it = top()                                             # :98-102
        if it is not None and (it[1].key(), it[0]) < (current[1].key(), current[0]):
            heap.remove(it)
            heap.append(current)
            current = it
    return out


def merge_rule(runs) -> list[tuple[int, int]]:
    """Entry (r, j) is yielded iff no run with a lower index holds an equal key; the yielded
    entries are ordered by (key, r, j)."""
    winner: dict[bytes, int] = {}
    for r, run in enumerate(runs):
        for k, _ in run:
            winner.setdefault(k, r)
    kept = [(k, r, j) for r, run in enumerate(runs) for j, (k, _) in enumerate(run)
            if winner[k] == r]
    kept.sort()
    return [(r, j) for _, r, j in kept]


def merged_entries(runs) -> list[tuple[bytes, bytes]]:
    """The (key, value) pairs compaction adds to the builder, in order."""
    return [runs[r][j] for r, j in merge_rule(runs)]

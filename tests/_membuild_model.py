"""What the reference does with a WAL image and with puts, restated line by line in Python, and the
closed-form rules the device build implements (include/tpz_gpu.h, tpz_mem_build / tpz_wal_index).
tests/test_membuild_model.py checks the closed forms against the line-by-line model.

Line by line:
  WalIterator   src/wal/iterator.rs:10-45 (create, is_valid, next) over `bytes`
  mem_open      MemTable::open, src/mem_table.rs:119-143
  MemTable      do_mem_put, src/mem_table.rs:169-196, over a dict {key: (value, version)}.
                compare_insert(k, v, |x| x.version < version) replaces the entry iff the closure
                holds for the one it finds and returns the entry the map holds afterwards: the new
                one, or the one it kept.
usize is 64 bits: `size` wraps at 2^64 (fetch_add / fetch_sub wrap).
"""
from __future__ import annotations

U64 = (1 << 64) - 1
NONE = U64


class Panic(Exception):
    """A Rust panic (get_u16 on a short buffer, a slice out of range)."""


class WalIterator:
    def __init__(self, buf: bytes):            # create (:10-18)
        self.data = bytes(buf)
        self.key = b""
        self.value = b""
        self.at = 0                            # bytes consumed so far (not in the reference)
        self.next()

    def is_valid(self) -> bool:                # :30-32
        return len(self.key) != 0

    def _get_u16(self) -> int:
        if len(self.data) < 2:
            raise Panic(f"get_u16 at byte {self.at}")
        v = (self.data[0] << 8) | self.data[1]
        self._advance(2)
        return v

    def _advance(self, k: int) -> None:
        self.data = self.data[k:]
        self.at += k

    def next(self) -> None:                    # :34-45
        if len(self.data) == 0:
            self.key = b""
            return
        klen = self._get_u16()
        if klen > len(self.data):
            raise Panic(f"key slice at byte {self.at}")
        self.key = self.data[:klen]
        self._advance(klen)
        vlen = self._get_u16()
        if vlen > len(self.data):
            raise Panic(f"value slice at byte {self.at}")
        self.value = self.data[:vlen]
        self._advance(vlen)


def mem_open(image: bytes):
    """MemTable::open (:119-143): (map {key: (value, version 0)}, size)."""
    it = WalIterator(image)
    m: dict = {}
    size = 0
    while it.is_valid():
        size = (size + len(it.key) + len(it.value)) & U64
        m[it.key] = (it.value, 0)              # map.insert replaces
        it.next()
    return m, size


def wal_walk(image: bytes):
    """What tpz_wal_index reports, from WalIterator: (record starts + the end, how it ended:
    0 the image's end / 1 an empty key / 2 a panic, the failing record's offset or NONE)."""
    rec = []
    at = 0
    try:
        it = WalIterator(b"")
        it.data = bytes(image)
        while True:
            if len(it.data) == 0:
                return rec + [at], 0, NONE
            it.next()
            rec.append(at)
            at = it.at
            if not it.is_valid():
                return rec + [at], 1, NONE
    except Panic:
        return rec + [at], 2, at


class MemTable:
    def __init__(self):
        self.map: dict = {}
        self.size = 0

    def do_mem_put(self, key: bytes, value: bytes, version: int) -> None:     # :169-196
        held = self.map.get(key)
        old_size = len(key) + len(held[0]) if held is not None else 0          # :170-174
        if held is None or held[1] < version:                                  # compare_insert
            self.map[key] = (value, version)
        insert_version = self.map[key][1]                                      # :182-183
        if version != insert_version:                                          # :185-187
            return
        if len(key) + len(value) >= old_size:                                  # :189-191
            self.size = (self.size + len(key) + len(value) - old_size) & U64
        else:                                                                  # :193-194
            sub = old_size - len(key) + len(value)
            self.size = (self.size - sub) & U64

    def put_entries(self, entries, version: int) -> None:                      # :161-167
        for k, v in entries:
            self.do_mem_put(k, v, version)


def model_put(entries, versions):
    """Line by line: (map {key: (value, version)}, size)."""
    t = MemTable()
    for (k, v), ver in zip(entries, versions):
        t.do_mem_put(bytes(k), bytes(v), int(ver))
    return t.map, t.size


# ---- the closed forms ---------------------------------------------------------------------------
def closed_replay(entries):
    """(winner ids in key order, size, first empty key or NONE, consumed)."""
    n = len(entries)
    stop = next((i for i, (k, _) in enumerate(entries) if len(k) == 0), None)
    live = n if stop is None else stop
    last = {}
    size = 0
    for i in range(live):
        k, v = entries[i]
        last[bytes(k)] = i                      # the last record of a key wins
        size = (size + len(k) + len(v)) & U64
    win = [last[k] for k in sorted(last)]
    return win, size, NONE if stop is None else stop, live


def closed_put(entries, versions):
    """(winner ids in key order, size, first empty key or NONE, consumed). Versions non-decreasing.
    Per key, its entries in arrival order fall into version subgroups; the winner is the head of
    the last subgroup. Entry e's size term uses h = the entry the map held before it: the head of
    e's subgroup if e is not that head, else the head of the previous subgroup (none: an insert)."""
    n = len(entries)
    groups: dict = {}
    for i, (k, _) in enumerate(entries):
        groups.setdefault(bytes(k), []).append(i)
    size = 0
    win = {}
    for k, ids in groups.items():
        heads = [ids[0]] + [b for a, b in zip(ids, ids[1:]) if versions[a] != versions[b]]
        win[k] = heads[-1]
        head_of = {}
        prev_head = {}
        cur = None
        for i in ids:
            if i in heads:
                prev_head[i] = cur
                cur = i
            head_of[i] = cur
        for i in ids:
            vlen = len(entries[i][1])
            h = prev_head[i] if i in prev_head else head_of[i]
            if h is None:
                size += len(k) + vlen
            else:
                hl = len(entries[h][1])
                size += vlen - hl if vlen >= hl else -(hl + vlen)
        size &= U64
    stop = next((i for i, (k, _) in enumerate(entries) if len(k) == 0), None)
    return [win[k] for k in sorted(win)], size, NONE if stop is None else stop, n


def prefix_of(key: bytes) -> int:
    """tpz_mem_prefix: the first 8 bytes, big-endian, zero padded."""
    return int.from_bytes(bytes(key[:8]).ljust(8, b"\0"), "big")


def expect(entries, versions=None):
    """Everything tpz_mem_build writes for `entries` (REPLAY without versions, PUT with):
    dict(src, keys, vals, prefix, version, info[0..5])."""
    entries = [(bytes(k), bytes(v)) for k, v in entries]
    if versions is None:
        win, size, stop, used = closed_replay(entries)
        over = [0] * len(win)
    else:
        win, size, stop, used = closed_put(entries, versions)
        over = [int(versions[i]) for i in win]
    keys = [entries[i][0] for i in win]
    vals = [entries[i][1] for i in win]
    return dict(src=win, keys=keys, vals=vals, prefix=[prefix_of(k) for k in keys], version=over,
                info=[len(win), sum(map(len, keys)), sum(map(len, vals)), stop, size, used])

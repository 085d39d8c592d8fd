"""LevelController::get (src/level.rs:427-465) and the SST half of LsmStorage::scan
(src/lsm_storage.rs:335-374) for batches of keys and ranges over tables resident in HBM.

`DeviceLevels(ctx, levels)` takes the level lists of a LevelController (`levels[0]` is L0 in push
order, oldest first; every level below is sorted by smallest key) whose tables were opened with
`SsTable.open` (their `.device` is the resident `DeviceTable`), uploads one tpz_get_table
descriptor per table once, and answers

  get_batch(keys)   one tpz_get_keys (the walk over L0 and the levels: bloom probe, seek, equality,
                    tombstone rule), one read-back of the total value bytes, one tpz_get_values
  get(key)          the reference's Result<Option<Bytes>>: bytes, None, or the reference's error
                    (BlockError) / panic (ReferencePanic)

  scan_batch(ranges, limit)
                    one tpz_scan_ranges (the table filter, one cursor per table, MergeIterator,
                    the end bound and the tombstone rule, at most `limit` entries per range), one
                    read-back of the totals, one tpz_scan_entries
  scan(lower, upper)
                    the reference's FusedIterator<LsmIterator>, pulled page by page

A set of more than 64 tables (runs included) is scanned with tpz_level_scan_ranges /
tpz_level_scan_entries instead: one merge cursor per run, per L0 table and per non-empty level below
L0, so a level may hold any number of tables; runs + L0 tables + non-empty lower levels <= 64.
`by_level=True` on scan_ranges / scan_batch takes that path for a smaller set too.

`DeviceRun(ctx, entries)` is one memtable's sorted snapshot in HBM (a tpz_mem_run, with its prefix
column), and `DeviceLsm(ctx, runs, levels)` answers LsmStorage::get (src/lsm_storage.rs:198-213)
and LsmStorage::scan (:335-374, the memtables merged in with TwoMergeIterator) over runs plus
tables: `get_batch`, `get`, `scan_batch` and `scan` shaped exactly like DeviceLevels'.

There is no CPU fallback: the walk, the merge and the gathers are the kernels of csrc/tpz_get.hip,
csrc/tpz_scan.hip, csrc/tpz_mem.hip and csrc/tpz_levelscan.hip.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (BLOCK_MALFORMED, BOUND_AFTER, BOUND_EXCLUDED, BOUND_INCLUDED, BOUND_UNBOUNDED,
                   GET_ABSENT, GET_DELETED, GET_ERROR, GET_FOUND, GET_NONE, SCAN_ERROR, SCAN_MORE,
                   Context, Entries, GetTable, MemRun)
from .table import RAW_SCAN_ERROR, DeviceTable, RawTable, ReferencePanic, _pack


def _device_table(t):
    return t if isinstance(t, (DeviceTable, RawTable)) else t.device


_KINDS = {"in": BOUND_INCLUDED, "ex": BOUND_EXCLUDED, "after": BOUND_AFTER}


def _bound(b, lower: bool) -> tuple[int, bytes]:
    """None / ("in", key) / ("ex", key) / ("after", key) -> (TPZ_BOUND_*, key)."""
    if b is None:
        return BOUND_UNBOUNDED, b""
    kind, key = b
    if kind not in _KINDS or (kind == "after" and not lower):
        raise ValueError(f"bound kind {kind!r}")
    return _KINDS[kind], bytes(key)


class ScanIterator:
    """FusedIterator<LsmIterator> (src/lsm_iterator.rs) over DeviceLevels.scan_batch pages: a
    page that reported MORE is continued from its last key with ("after", key); a page that
    reported ERROR raises the reference's error once the entries before the failure are
    consumed."""

    def __init__(self, levels: "DeviceLevels", lower, upper, page: int):
        self._levels, self._upper, self._page = levels, upper, page
        self._pull(lower)

    def _pull(self, lower) -> None:
        r = self._levels.scan_batch([(lower, self._upper)], self._page)
        kp, vp = r["kpos"].astype(np.int64), r["vpos"].astype(np.int64)
        self._ents = [(r["keys"][kp[j]:kp[j + 1]], r["values"][vp[j]:vp[j + 1]])
                      for j in range(int(r["first"][1]))]
        self._j = 0
        self._result = int(r["result"][0])
        self._fail = (int(r["status"][0]), *(int(x) for x in r["where"][0]))
        if not self._ents:
            self._end()

    def _end(self) -> None:
        """The page is used up: the next one, the reference's error, or the end."""
        if self._result == SCAN_ERROR:
            self._result = None
            if self._fail[2] == GET_NONE:        # a table without blocks: block_metas[0]
                raise ReferencePanic("index out of bounds: the len is 0 but the index is 0")
            raise self._levels.error(*self._fail)
        if self._result == SCAN_MORE:
            self._pull(("after", self._ents[-1][0]))

    def is_valid(self) -> bool:
        return self._j < len(self._ents)

    def key(self) -> bytes:
        return self._ents[self._j][0]

    def value(self) -> bytes:
        return self._ents[self._j][1]

    def next(self) -> None:
        if not self.is_valid():              # FusedIterator::next
            return
        self._j += 1
        if self._j == len(self._ents):
            self._end()


class DeviceLevels:
    """The tables of a LevelController as one tpz_get_table array in HBM."""

    def __init__(self, ctx: Context, levels: list[list]):
        if len(levels) > _lib.GET_MAX_LEVELS:
            raise ValueError(f"{len(levels)} levels: at most {_lib.GET_MAX_LEVELS}")
        self.ctx = ctx
        self.dev = torch.device("cuda", ctx.device)
        self.levels = [list(lv) for lv in levels]
        self.tables = [t for lv in self.levels for t in lv]      # descriptor order
        self.level_first = np.zeros(len(self.levels) + 1, np.uint32)
        np.cumsum([len(lv) for lv in self.levels], out=self.level_first[1:])
        self.n_tables = len(self.tables)
        self.n_levels = len(self.levels)
        # the level scan's cursors: one per L0 table and per non-empty level below L0
        self.n_cursors = sum(len(lv) if i == 0 else bool(lv) for i, lv in enumerate(self.levels))
        # a set of in-place tables (RawTable) answers gets with the tpz_raw_* calls
        kinds = {isinstance(_device_table(t), RawTable) for t in self.tables}
        if len(kinds) > 1:
            raise TypeError("a level set holds DeviceTables or RawTables, not both")
        self.raw = kinds == {True}
        desc = ((_lib.RawTable if self.raw else GetTable) * max(self.n_tables, 1))()
        for i, t in enumerate(self.tables):
            dt = _device_table(t)
            if dt is None:
                raise ValueError(f"table {i} has no resident DeviceTable (SsTable.open keeps one)")
            desc[i] = dt.raw_table() if self.raw else GetTable(
                dt.table(), dt.bloom.data_ptr() if dt.bloom is not None else None, dt.bloom_len)
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        self.d_tables = torch.from_numpy(raw).to(self.dev)       # uploaded once

    # What DeviceLsm adds: the ABI family of its calls, and its memtable runs.
    _family = ""                # tpz_get_* / tpz_scan_*
    n_runs = 0

    def _runs(self) -> tuple:
        """(d_runs pointer, n_runs) for the calls that take memtable runs."""
        return 0, 0

    def _call(self, op: str, by_level: bool, *args) -> None:
        """tpz_<family><op> over the tables (the lsm family: the runs in front), or with
        by_level (scans only) tpz_level_<op> over the runs and the tables. Over in-place tables
        the gets are tpz_raw_<family><op>; the scans need DeviceTables."""
        if self.raw:
            if not op.startswith("get_"):
                raise ValueError(RAW_SCAN_ERROR)
            getattr(self.ctx, f"raw_{self._family}{op}_ptrs")(
                *(self._runs() if self._family else ()), *args)
        elif by_level:
            getattr(self.ctx, f"level_{op}_ptrs")(*self._runs(), *args)
        elif self._family:
            getattr(self.ctx, f"{self._family}{op}_ptrs")(*self._runs(), *args)
        else:
            getattr(self.ctx, f"{op}_ptrs")(*args)

    def walk(self, keys: list[bytes]) -> dict:
        """tpz_get_keys (DeviceLsm: tpz_lsm_get_keys) on the current stream: device tensors
        result, status (uint8), table, block, entry (int32 holding the u32 values), val_pos
        (int64, n + 1), and n."""
        n = len(keys)
        buf, pos = _pack(keys)
        q = torch.from_numpy(buf.copy()).to(self.dev)
        qp = torch.from_numpy(pos).to(self.dev)
        out = {k: torch.empty(max(n, 1), dtype=t, device=self.dev) for k, t in
               (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
                ("block", torch.int32), ("entry", torch.int32))}
        out["val_pos"] = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        self._call("get_keys", False, self.d_tables.data_ptr(), self.n_tables,
                   self.level_first.ctypes.data, self.n_levels, q.data_ptr(), qp.data_ptr(), n,
                   out["result"].data_ptr(), out["status"].data_ptr(), out["table"].data_ptr(),
                   out["block"].data_ptr(), out["entry"].data_ptr(), out["val_pos"].data_ptr(),
                   torch.cuda.current_stream(self.dev).cuda_stream)
        out["n"] = n
        out["_keys"] = (q, qp)      # alive until the stream has run the walk
        return out

    def values(self, w: dict, total: int) -> torch.Tensor:
        """tpz_get_values (DeviceLsm: tpz_lsm_get_values) on the current stream: the packed
        values (uint8, `total` bytes)."""
        vals = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        self._call("get_values", False, self.d_tables.data_ptr(), self.n_tables, w["n"],
                   w["result"].data_ptr(), w["table"].data_ptr(), w["block"].data_ptr(),
                   w["entry"].data_ptr(), w["val_pos"].data_ptr(), vals.data_ptr(), total,
                   torch.cuda.current_stream(self.dev).cuda_stream)
        return vals[:total]

    def get_batch(self, keys: list[bytes]) -> dict:
        """LevelController::get for every key. Numpy arrays, one entry per key: result
        (GET_ABSENT / GET_FOUND / GET_DELETED / GET_ERROR), status, table, block, entry (uint32,
        GET_NONE where the walk ended nowhere); val_pos (n + 1) and values: key i's value is
        values[val_pos[i]:val_pos[i + 1]] (empty unless FOUND)."""
        w = self.walk(keys)
        n = w["n"]
        total = int(w["val_pos"][n].item())          # the one read-back between the two calls
        vals = self.values(w, total)
        out = {k: w[k][:n].cpu().numpy() for k in ("result", "status")}
        for k in ("table", "block", "entry"):
            out[k] = w[k][:n].cpu().numpy().view(np.uint32)
        out["val_pos"] = w["val_pos"].cpu().numpy().astype(np.uint64)
        out["values"] = vals.cpu().numpy().tobytes()
        return out

    def scan_ranges(self, ranges: list, limit: int, by_level: bool = False) -> dict:
        """tpz_scan_ranges (DeviceLsm: tpz_lsm_scan_ranges) on the current stream: device tensors
        result, status (uint8), where (int32, n x 3), hit_table, hit_block, hit_entry (int32,
        n x limit), first, key_first, val_first (int64, n + 1), info (int64, 3), and n, limit.
        More than SCAN_MAX_TABLES runs plus tables, or by_level: tpz_level_scan_ranges (one cursor
        per level below L0)."""
        by_level = by_level or self.n_runs + self.n_tables > _lib.SCAN_MAX_TABLES
        n = len(ranges)
        lo = [_bound(r[0], True) for r in ranges]
        hi = [_bound(r[1], False) for r in ranges]
        dev = self.dev
        cols = []
        for side in (lo, hi):
            buf, pos = _pack([k for _, k in side])
            cols += [torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(pos).to(dev),
                     torch.from_numpy(np.array([k for k, _ in side] or [0], np.uint8)).to(dev)]
        out = {k: torch.empty(max(n, 1), dtype=torch.uint8, device=dev) for k in ("result", "status")}
        out["where"] = torch.empty((max(n, 1), 3), dtype=torch.int32, device=dev)
        for k in ("hit_table", "hit_block", "hit_entry"):
            out[k] = torch.empty(max(n * limit, 1), dtype=torch.int32, device=dev)
        for k in ("first", "key_first", "val_first"):
            out[k] = torch.empty(n + 1, dtype=torch.int64, device=dev)
        out["info"] = torch.empty(3, dtype=torch.int64, device=dev)
        self._call("scan_ranges", by_level, self.d_tables.data_ptr(), self.n_tables,
                   self.level_first.ctypes.data, self.n_levels, *(c.data_ptr() for c in cols), n,
                   limit,
                   *(out[k].data_ptr() for k in
                     ("result", "status", "where", "hit_table", "hit_block", "hit_entry", "first",
                      "key_first", "val_first", "info")),
                   torch.cuda.current_stream(dev).cuda_stream)
        out["n"], out["limit"], out["by_level"] = n, limit, by_level
        out["_bounds"] = cols        # alive until the stream has run the scan
        return out

    def scan_entries(self, s: dict, totals) -> dict:
        """tpz_scan_entries (DeviceLsm: tpz_lsm_scan_entries; by_level: tpz_level_scan_entries) on
        the current stream over scan_ranges' outputs: device tensors kpos, vpos (int64, entries +
        1), keys, values (uint8). totals = the three numbers of info."""
        n_ent, kbytes, vbytes = (int(x) for x in totals)
        dev = self.dev
        out = {"kpos": torch.empty(n_ent + 1, dtype=torch.int64, device=dev),
               "vpos": torch.empty(n_ent + 1, dtype=torch.int64, device=dev),
               "keys": torch.empty(max(kbytes, 1), dtype=torch.uint8, device=dev),
               "values": torch.empty(max(vbytes, 1), dtype=torch.uint8, device=dev)}
        self._call("scan_entries", bool(s.get("by_level")), self.d_tables.data_ptr(),
                   self.n_tables, s["n"], s["limit"], s["hit_table"].data_ptr(),
                   s["hit_block"].data_ptr(), s["hit_entry"].data_ptr(), s["first"].data_ptr(),
                   out["keys"].data_ptr(), kbytes, out["kpos"].data_ptr(),
                   out["values"].data_ptr(), vbytes, out["vpos"].data_ptr(),
                   torch.cuda.current_stream(dev).cuda_stream)
        out["keys"], out["values"] = out["keys"][:kbytes], out["values"][:vbytes]
        return out

    def scan_batch(self, ranges: list, limit: int, by_level: bool = False) -> dict:
        """LsmStorage::scan's SST half for every (lower, upper) of `ranges`, at most `limit`
        entries each; a bound is None (Unbounded), ("in", key), ("ex", key) or, as a lower bound
        only, ("after", key). Numpy arrays: result (SCAN_DONE / SCAN_MORE / SCAN_ERROR), status,
        where (n x 3 uint32: table, block, entry of a failure, GET_NONE otherwise), hit_table,
        hit_block, hit_entry (n x limit uint32; a row is defined up to the scan's count), first,
        key_first, val_first (n + 1 uint64); kpos, vpos (entries + 1 uint64) and keys, values
        (bytes): scan i owns entries [first[i], first[i + 1]) in iterator order, entry j's key
        is keys[kpos[j]:kpos[j + 1]]. by_level: as for scan_ranges."""
        s = self.scan_ranges(ranges, limit, by_level)
        n = s["n"]
        totals = s["info"].cpu().numpy()             # the one read-back between the two calls
        e = self.scan_entries(s, totals)
        out = {k: s[k][:n].cpu().numpy() for k in ("result", "status")}
        out["where"] = s["where"][:n].cpu().numpy().view(np.uint32)
        for k in ("hit_table", "hit_block", "hit_entry"):
            out[k] = s[k][:n * limit].cpu().numpy().view(np.uint32).reshape(n, limit)
        for k in ("first", "key_first", "val_first"):
            out[k] = s[k].cpu().numpy().astype(np.uint64)
        for k in ("kpos", "vpos"):
            out[k] = e[k].cpu().numpy().astype(np.uint64)
        out["keys"] = e["keys"].cpu().numpy().tobytes()
        out["values"] = e["values"].cpu().numpy().tobytes()
        return out

    def scan(self, lower=None, upper=None, page: int = 256) -> ScanIterator:
        """lsm_storage.rs:335-374 without memtables: is_valid() / key() / value() / next()."""
        return ScanIterator(self, lower, upper, page)

    def _host_block(self, table: int, block: int):
        t = self.tables[table]
        blocks = t.host_blocks() if isinstance(t, DeviceTable) else t._blocks
        return blocks[block]

    def error(self, status: int, table: int, block: int, entry: int) -> Exception:
        """The reference's Err / panic for a GET_ERROR query, with the texts table.py raises."""
        if block == GET_NONE:                        # Bloom::may_contain (bloom.rs:72-84)
            if _device_table(self.tables[table]).bloom_len == 0:      # filter.last().unwrap()
                return ReferencePanic("called `Option::unwrap()` on a `None` value")
            return ReferencePanic("attempt to calculate the remainder with a divisor of zero")
        if _device_table(self.tables[table]).n_blocks == 0:       # block_metas[0]
            return ReferencePanic("index out of bounds: the len is 0 but the index is 0")
        t = _device_table(self.tables[table])
        r = t.block_error(block) if self.raw else self._host_block(table, block)
        if isinstance(r, Exception):                 # read_block_cached's Err / decode's panic
            return r
        assert status == BLOCK_MALFORMED, status
        return ReferencePanic(f"entry {entry} of the block is out of range")    # iterator.rs:74-98

    def get(self, key: bytes) -> bytes | None:
        """level.rs:427-465: the value, None (absent or deleted), or the reference's error."""
        r = self.get_batch([key])
        res = int(r["result"][0])
        if res == GET_FOUND:
            return r["values"]
        if res in (GET_ABSENT, GET_DELETED):
            return None
        assert res == GET_ERROR, res
        raise self.error(int(r["status"][0]), int(r["table"][0]), int(r["block"][0]),
                         int(r["entry"][0]))


class DeviceRun:
    """One memtable's SkipMap as a tpz_mem_run in HBM: `entries` is its (key, value) list in key
    order (keys strictly increasing, an empty value a tombstone), or a dict of device columns
    keys, kpos, vals, vpos (uint8 / int64 tensors; kpos and vpos hold n + 1 positions). With
    `prefix` the prefix column is built on the device (tpz_mem_prefix); without it the lookups
    bisect on the keys, with the same answers."""

    def __init__(self, ctx: Context, entries, prefix: bool = True):
        self.ctx = ctx
        self.dev = torch.device("cuda", ctx.device)
        if isinstance(entries, dict):
            self.keys, self.kpos, self.vals, self.vpos = (entries[k] for k in
                                                          ("keys", "kpos", "vals", "vpos"))
            self.n = int(self.kpos.numel()) - 1
            self.key_bytes, self.val_bytes = int(self.kpos[-1].item()), int(self.vpos[-1].item())
        else:
            entries = [(bytes(k), bytes(v)) for k, v in entries]
            self.n = len(entries)
            cols = []
            for side in ([k for k, _ in entries], [v for _, v in entries]):
                buf, pos = _pack(side)
                cols += [torch.from_numpy(buf.copy()).to(self.dev), torch.from_numpy(pos).to(self.dev),
                         int(pos[-1])]
            self.keys, self.kpos, self.key_bytes, self.vals, self.vpos, self.val_bytes = cols
        self.prefix = None
        if prefix:
            self.prefix = torch.empty(max(self.n, 1), dtype=torch.int64, device=self.dev)
            ctx.mem_prefix_ptrs(self.entries(), self.prefix.data_ptr(),
                                torch.cuda.current_stream(self.dev).cuda_stream)

    @classmethod
    def build(cls, ctx: Context, entries, versions=None, mode=None, prefix: bool = True):
        """From entries in ARRIVAL order, sorted and deduplicated on the device with the reference's
        rules (memtable.build_run: tpz_mem_build)."""
        from .memtable import build_run
        return build_run(ctx, entries, versions=versions, mode=mode, prefix=prefix)

    @classmethod
    def from_wal(cls, ctx: Context, image: bytes, prefix: bool = True):
        """MemTable::open over a WAL image (memtable.replay_wal)."""
        from .memtable import replay_wal
        return replay_wal(ctx, image, prefix=prefix)

    def entries(self) -> Entries:
        return Entries(self.keys.data_ptr(), self.kpos.data_ptr(), self.vals.data_ptr(),
                       self.vpos.data_ptr(), self.n, self.key_bytes, self.val_bytes)

    def run(self) -> MemRun:
        return MemRun(self.entries(), None if self.prefix is None else self.prefix.data_ptr())


class DeviceLsm(DeviceLevels):
    """LsmStorage::get and LsmStorage::scan over memtable runs plus the tables of a
    LevelController: `runs` are DeviceRuns in MemTables::view() order (src/mem_table.rs:74-81: the
    immutable memtables oldest first, the mutable one last; the last run has the highest
    priority), `levels` as for DeviceLevels. A hit in run r is reported as table = HIT_MEM | r,
    block 0, entry = its index in the run."""

    def __init__(self, ctx: Context, runs: list, levels: list[list]):
        if len(runs) > _lib.MEM_MAX_RUNS:
            raise ValueError(f"{len(runs)} runs: at most {_lib.MEM_MAX_RUNS}")
        super().__init__(ctx, levels)
        if len(runs) + self.n_cursors > _lib.LEVEL_SCAN_MAX_CURSORS:
            raise ValueError(f"{len(runs)} runs and {self.n_cursors} table cursors (L0 tables plus "
                             f"non-empty lower levels): at most {_lib.LEVEL_SCAN_MAX_CURSORS}")
        self.runs = list(runs)
        self.n_runs = len(self.runs)
        desc = (MemRun * max(self.n_runs, 1))()
        for i, r in enumerate(self.runs):
            desc[i] = r.run()
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        self.d_runs = torch.from_numpy(raw).to(self.dev)         # uploaded once

    _family = "lsm_"            # tpz_lsm_get_* / tpz_lsm_scan_*

    def _runs(self) -> tuple:
        return self.d_runs.data_ptr(), self.n_runs

    def scan(self, lower=None, upper=None, page: int = 256) -> ScanIterator:
        """lsm_storage.rs:335-374: is_valid() / key() / value() / next(). A page that reported
        MORE is continued with ("after", its last key) over the same runs."""
        return ScanIterator(self, lower, upper, page)

    def error(self, status: int, table: int, block: int, entry: int) -> Exception:
        if table == GET_NONE:                        # assert!(!key.is_empty()) (lsm_storage.rs:199)
            return ReferencePanic("key cannot be empty")
        return super().error(status, table, block, entry)

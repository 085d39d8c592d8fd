"""LevelController::get (src/level.rs:427-465) for batches of keys over tables resident in HBM.

`DeviceLevels(ctx, levels)` takes the level lists of a LevelController (`levels[0]` is L0 in push
order, oldest first; every level below is sorted by smallest key) whose tables were opened with
`SsTable.open` (their `.device` is the resident `DeviceTable`), uploads one tpz_get_table
descriptor per table once, and answers

  get_batch(keys)   one tpz_get_keys (the walk over L0 and the levels: bloom probe, seek, equality,
                    tombstone rule), one read-back of the total value bytes, one tpz_get_values
  get(key)          the reference's Result<Option<Bytes>>: bytes, None, or the reference's error
                    (BlockError) / panic (ReferencePanic)

There is no CPU fallback: the walk and the gather are the kernels of csrc/tpz_get.hip.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (BLOCK_MALFORMED, GET_ABSENT, GET_DELETED, GET_ERROR, GET_FOUND, GET_NONE,
                   Context, GetTable)
from .table import DeviceTable, ReferencePanic, _pack


def _device_table(t) -> DeviceTable:
    return t if isinstance(t, DeviceTable) else t.device


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
        desc = (GetTable * max(self.n_tables, 1))()
        for i, t in enumerate(self.tables):
            dt = _device_table(t)
            if dt is None:
                raise ValueError(f"table {i} has no resident DeviceTable (SsTable.open keeps one)")
            desc[i] = GetTable(dt.table(), dt.bloom.data_ptr() if dt.bloom is not None else None,
                               dt.bloom_len)
        raw = np.frombuffer(bytes(desc), np.uint8).copy()
        self.d_tables = torch.from_numpy(raw).to(self.dev)       # uploaded once

    def walk(self, keys: list[bytes]) -> dict:
        """tpz_get_keys on the current stream: device tensors result, status (uint8), table,
        block, entry (int32 holding the u32 values), val_pos (int64, n + 1), and n."""
        n = len(keys)
        buf, pos = _pack(keys)
        q = torch.from_numpy(buf.copy()).to(self.dev)
        qp = torch.from_numpy(pos).to(self.dev)
        out = {k: torch.empty(max(n, 1), dtype=t, device=self.dev) for k, t in
               (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
                ("block", torch.int32), ("entry", torch.int32))}
        out["val_pos"] = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        self.ctx.get_keys_ptrs(self.d_tables.data_ptr(), self.n_tables,
                               self.level_first.ctypes.data, self.n_levels, q.data_ptr(),
                               qp.data_ptr(), n, out["result"].data_ptr(),
                               out["status"].data_ptr(), out["table"].data_ptr(),
                               out["block"].data_ptr(), out["entry"].data_ptr(),
                               out["val_pos"].data_ptr(),
                               torch.cuda.current_stream(self.dev).cuda_stream)
        out["n"] = n
        out["_keys"] = (q, qp)      # alive until the stream has run the walk
        return out

    def values(self, w: dict, total: int) -> torch.Tensor:
        """tpz_get_values on the current stream: the packed values (uint8, `total` bytes)."""
        vals = torch.empty(max(total, 1), dtype=torch.uint8, device=self.dev)
        self.ctx.get_values_ptrs(self.d_tables.data_ptr(), self.n_tables, w["n"],
                                 w["result"].data_ptr(), w["table"].data_ptr(),
                                 w["block"].data_ptr(), w["entry"].data_ptr(),
                                 w["val_pos"].data_ptr(), vals.data_ptr(), total,
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
        r = self._host_block(table, block)
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

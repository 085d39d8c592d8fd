#!/usr/bin/env python3
"""tpz_level_scan_ranges beside tpz_scan_ranges, and on a set only it can scan (diagnostic, GPU
box). tools/scan_probe.py's conventions: one process, HIP events, 0.3 s of untimed launches before
every timing (bench.settle), 20 timed repetitions, 2^16 scans whose lower bounds (Included) are
keys of the set drawn uniformly, upper bound Unbounded, limits 10 and 100.

  shape (a)  scan_probe's set: 4 overlapping L0 tables and 3 levels of 8 disjoint tables of the
             "4k" synth shape (28 tables). The level path (7 cursors) and the per-table path (28),
             interleaved, five repeats each: the medians and the spread (max - min) of each.
  shape (b)  4 L0 tables, 40 tables in L1 and 400 in L2 (the reference's default widths,
             src/opt.rs:31-54), the same entry shape, small tables: 444 tables under 6 cursors,
             which tpz_scan_ranges refuses. The level path alone, and the per-call index and links
             passes as lines of their own (the library's diagnostic tpz_debug_level_scan).
The answers are checked first: both paths agree byte for byte on shape (a); every scan starts at
its lower bound and yields ascending keys on both shapes.
Prints one JSON line per shape and, with --out, writes both to a file
(profiles/levelscan/probe.json).

    python3 tools/levelscan_probe.py [--blocks 2048] [--wide-blocks 64] [--scans 65536] [--out F]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from get_probe import KLEN, PER_BLOCK, VLEN, make_table, timed  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.levels import DeviceLevels  # noqa: E402

WHAT = ("tools/levelscan_probe.py: the level scan (one merge cursor per level below L0) on (a) "
        "scan_probe's 28 tables beside the per-table path and (b) 4 L0 + 40 L1 + 400 L2 tables; "
        "lower bounds drawn from the keys, upper unbounded; HIP-event ms per call on one MI355X, "
        "one box, one run")
OUT = ("result", "status", "where", "hit_table", "hit_block", "hit_entry", "first", "key_first",
       "val_first", "info")


class Bench:
    """A table set, 2^16 lower bounds and the two calls over them."""

    def __init__(self, ctx, levels, k2, n_s: int):
        self.ctx, self.k2, self.n_s = ctx, k2, n_s
        self.dl = DeviceLevels(ctx, levels)
        self.dev = self.dl.dev
        self.stream = torch.cuda.current_stream(self.dev)
        dev = self.dev
        rng = np.random.default_rng(7)
        self.pick = rng.integers(0, len(k2), n_s)
        self.lo = torch.from_numpy(k2[self.pick].reshape(-1).copy()).to(dev)
        self.lo_pos = torch.arange(n_s + 1, device=dev, dtype=torch.int64) * KLEN
        self.lo_kind = torch.full((n_s,), _lib.BOUND_INCLUDED, dtype=torch.uint8, device=dev)
        self.hi = torch.zeros(16, dtype=torch.uint8, device=dev)
        self.hi_pos = torch.zeros(n_s + 1, dtype=torch.int64, device=dev)
        self.hi_kind = torch.full((n_s,), _lib.BOUND_UNBOUNDED, dtype=torch.uint8, device=dev)

    def outputs(self, limit: int) -> dict:
        n_s, dev = self.n_s, self.dev
        out = {k: torch.empty(n_s, dtype=torch.uint8, device=dev) for k in ("result", "status")}
        out["where"] = torch.empty(3 * n_s, dtype=torch.int32, device=dev)
        for k in ("hit_table", "hit_block", "hit_entry"):
            out[k] = torch.empty(n_s * limit, dtype=torch.int32, device=dev)
        for k in ("first", "key_first", "val_first"):
            out[k] = torch.empty(n_s + 1, dtype=torch.int64, device=dev)
        out["info"] = torch.empty(3, dtype=torch.int64, device=dev)
        return out

    def args(self, out: dict, limit: int) -> tuple:
        dl = self.dl
        return (dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
                self.lo.data_ptr(), self.lo_pos.data_ptr(), self.lo_kind.data_ptr(),
                self.hi.data_ptr(), self.hi_pos.data_ptr(), self.hi_kind.data_ptr(), self.n_s,
                limit, *(out[k].data_ptr() for k in OUT), self.stream.cuda_stream)

    def by_level(self, out, limit):
        return lambda: self.ctx.level_scan_ranges_ptrs(0, 0, *self.args(out, limit))

    def by_table(self, out, limit):
        return lambda: self.ctx.scan_ranges_ptrs(*self.args(out, limit))

    def cut_short(self, out, limit, stop_after: int):
        a = self.args(out, limit)
        ptr = [C.c_void_p(x) for x in a]
        call = (self.ctx.handle, C.c_void_p(0), 0, ptr[0], a[1], ptr[2], a[3], *ptr[4:10], a[10],
                a[11], *ptr[12:], stop_after)
        return lambda: _lib.check(_lib.lib().tpz_debug_level_scan(*call), "tpz_debug_level_scan")

    def gather(self, out, limit):
        """tpz_level_scan_entries over `out`; returns the key rows and the call."""
        dl, dev = self.dl, self.dev
        n_ent, kbytes, vbytes = (int(x) for x in out["info"].cpu().numpy())
        kpos = torch.empty(n_ent + 1, dtype=torch.int64, device=dev)
        vpos = torch.empty(n_ent + 1, dtype=torch.int64, device=dev)
        keys = torch.empty(max(kbytes, 1), dtype=torch.uint8, device=dev)
        vals = torch.empty(max(vbytes, 1), dtype=torch.uint8, device=dev)

        def call():
            self.ctx.level_scan_entries_ptrs(0, 0, dl.d_tables.data_ptr(), dl.n_tables, self.n_s,
                                             limit, out["hit_table"].data_ptr(),
                                             out["hit_block"].data_ptr(),
                                             out["hit_entry"].data_ptr(), out["first"].data_ptr(),
                                             keys.data_ptr(), kbytes, kpos.data_ptr(),
                                             vals.data_ptr(), vbytes, vpos.data_ptr(),
                                             self.stream.cuda_stream)
        call()
        torch.cuda.synchronize(dev)
        assert kbytes == n_ent * KLEN and vbytes == n_ent * VLEN
        return keys.cpu().numpy().reshape(n_ent, KLEN), call, (keys, vals, kpos, vpos)

    def check(self, out, limit):
        """No scan fails; scan j starts at its lower bound and its keys ascend."""
        res = out["result"].cpu().numpy()
        assert (res != _lib.SCAN_ERROR).all() and (out["status"].cpu().numpy() == 0).all()
        first = out["first"].cpu().numpy()
        counts = np.diff(first)
        assert ((counts == limit) | (res == _lib.SCAN_DONE)).all() and counts.min() >= 1
        got, call, keep = self.gather(out, limit)
        assert (got[first[:-1]] == self.k2[self.pick]).all()
        void = got.view(f"S{KLEN}").reshape(-1)
        inner = np.ones(len(got), bool)
        inner[first[:-1]] = False
        assert (void[1:][inner[1:]] > void[:-1][inner[1:]]).all()
        return call, keep, int(first[-1]), int((res == _lib.SCAN_MORE).sum())


def stream_of(n: int):
    keys, _, vals, _ = synth.entries("4k", n)
    return keys.reshape(n, KLEN), vals.reshape(n, VLEN)


def shape_a(ctx, blocks: int, n_s: int, steps: int, repeats: int) -> dict:
    n = 3 * 8 * blocks * PER_BLOCK
    k2, v2 = stream_of(n)
    i = np.arange(n)
    levels = [[make_table(ctx, k2, v2, np.nonzero(i % 16 == r)[0]) for r in range(4)]]
    for lv in range(3):
        own = np.nonzero(i % 3 == lv)[0]
        levels.append([make_table(ctx, k2, v2, c) for c in np.array_split(own, 8)])
    b = Bench(ctx, levels, k2, n_s)
    row = {"tables": b.dl.n_tables, "cursors_level_path": b.dl.n_cursors,
           "cursors_table_path": b.dl.n_tables, "blocks_per_level_table": blocks,
           "entries": int(sum(t.n_blocks for t in b.dl.tables)) * PER_BLOCK, "scans": n_s,
           "steps": steps, "repeats": repeats}
    for limit in (10, 100):
        lvl, tab = b.outputs(limit), b.outputs(limit)
        f_lvl, f_tab = b.by_level(lvl, limit), b.by_table(tab, limit)
        f_lvl()
        f_tab()
        torch.cuda.synchronize(b.dev)
        for k in ("result", "status", "where", "first", "key_first", "val_first", "info"):
            assert torch.equal(lvl[k], tab[k]), k
        first = lvl["first"].cpu().numpy()
        used = torch.from_numpy((np.arange(n_s * limit) % limit) <
                                np.repeat(np.diff(first), limit)).to(b.dev)
        for k in ("hit_table", "hit_block", "hit_entry"):
            assert torch.equal(lvl[k][used], tab[k][used]), k
        _, _, n_ent, more = b.check(lvl, limit)
        ms = {"level": [], "table": []}
        for _ in range(repeats):                             # interleaved
            ms["level"].append(timed(f_lvl, b.stream, steps, b.dev))
            ms["table"].append(timed(f_tab, b.stream, steps, b.dev))
        row[f"limit_{limit}"] = {
            "entries_yielded": n_ent, "scans_more": more,
            "ms_level_path": [round(x, 4) for x in ms["level"]],
            "ms_table_path": [round(x, 4) for x in ms["table"]],
            "ms_level_path_median": round(float(np.median(ms["level"])), 4),
            "ms_table_path_median": round(float(np.median(ms["table"])), 4),
            "spread_level_path": round(max(ms["level"]) - min(ms["level"]), 4),
            "spread_table_path": round(max(ms["table"]) - min(ms["table"]), 4)}
    return row


def shape_b(ctx, blocks: int, n_s: int, steps: int) -> dict:
    n = 2 * 400 * blocks * PER_BLOCK
    k2, v2 = stream_of(n)
    i = np.arange(n)
    levels = [[make_table(ctx, k2, v2, np.nonzero(i % 64 == r)[0]) for r in range(4)],
              [make_table(ctx, k2, v2, c) for c in np.array_split(np.nonzero(i % 2 == 1)[0], 40)],
              [make_table(ctx, k2, v2, c) for c in np.array_split(np.nonzero(i % 2 == 0)[0], 400)]]
    b = Bench(ctx, levels, k2, n_s)
    n_blocks = [int(sum(t.n_blocks for t in lv)) for lv in levels]
    row = {"tables": b.dl.n_tables, "tables_per_level": [4, 40, 400], "cursors": b.dl.n_cursors,
           "blocks_per_l2_table": blocks, "blocks_per_level": n_blocks,
           "entries": sum(n_blocks) * PER_BLOCK,
           "raw_bytes": sum(n_blocks) * PER_BLOCK * (KLEN + VLEN), "scans": n_s, "steps": steps}
    for limit in (10, 100):
        out = b.outputs(limit)
        f = b.by_level(out, limit)
        f()
        call, keep, n_ent, more = b.check(out, limit)
        ms_r = timed(f, b.stream, steps, b.dev)
        ms_e = timed(call, b.stream, steps, b.dev)
        ms_1 = timed(b.cut_short(out, limit, 1), b.stream, steps, b.dev)
        ms_2 = timed(b.cut_short(out, limit, 2), b.stream, steps, b.dev)
        row[f"limit_{limit}"] = {
            "entries_yielded": n_ent, "scans_more": more,
            "ms_level_scan_ranges": round(ms_r, 4), "ms_level_scan_entries": round(ms_e, 4),
            "ms_index_pass": round(ms_1, 4), "ms_index_and_links_passes": round(ms_2, 4),
            "scans_per_s": round(n_s / ((ms_r + ms_e) * 1e-3)),
            "entries_per_s": round(n_ent / ((ms_r + ms_e) * 1e-3))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048, help="shape (a): blocks per table of levels 1-3")
    ap.add_argument("--wide-blocks", type=int, default=64, help="shape (b): blocks per L2 table")
    ap.add_argument("--scans", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    doc = {"what": WHAT}
    doc["shape_a"] = shape_a(ctx, a.blocks, a.scans, a.steps, a.repeats)
    print(json.dumps(doc["shape_a"]), flush=True)
    doc["shape_b"] = shape_b(ctx, a.wide_blocks, a.scans, a.steps)
    print(json.dumps(doc["shape_b"]), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

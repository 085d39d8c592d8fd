#!/usr/bin/env python3
"""tpz_scan_ranges / tpz_scan_entries beside two yardsticks (diagnostic, GPU box).

The table set of tools/get_probe.py: 4 overlapping L0 tables and 3 levels of 8 disjoint tables
each of the "4k" synth shape (16-B keys, 100-B values, 34 entries per 4 KiB block). 2^16 scans
whose lower bounds (Included) are keys of the set drawn uniformly, upper bound Unbounded, with
limits 10 and 100 (YCSB-E style short range scans).

In one process, after 0.3 s of untimed launches each (bench.settle), HIP events around, per limit:
  scan_ranges     one tpz_scan_ranges over all scans
  scan_entries    one tpz_scan_entries over its output (buffers sized beforehand)
and the yardsticks
  seek_floor      one tpz_seek_keys per table over the scans' lower bounds (n_scans x n_tables
                  seeks: what the seek phase cannot beat)
  copy            a plain device copy of as many bytes as the gather writes
The answers are checked first: every scan starts at its lower bound and yields ascending keys.
Prints one JSON line and, with --out, writes it to a file (profiles/scan/probe.json).

    python3 tools/scan_probe.py [--blocks 2048] [--scans 65536] [--steps 20] [--out FILE]

For the per-kernel shares run it under `rocprofv3 --kernel-trace --stats` in a run of its own and
fold the kernel_stats CSV into the file with --shares CSV --out FILE (no GPU work).
"""
from __future__ import annotations

import argparse
import csv
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

WHAT = ("tools/scan_probe.py: 4 L0 tables + 3 levels x 8 tables of the '4k' synth shape, lower "
        "bounds drawn from the keys, upper unbounded; HIP-event ms per step on one MI355X, one run")


def probe(ctx, blocks: int, n_s: int, steps: int) -> dict:
    dev = torch.device("cuda", ctx.device)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    n = 3 * 8 * blocks * PER_BLOCK
    keys, _, vals, _ = synth.entries("4k", n)
    k2, v2 = keys.reshape(n, KLEN), vals.reshape(n, VLEN)
    i = np.arange(n)
    levels = [[make_table(ctx, k2, v2, np.nonzero(i % 16 == r)[0]) for r in range(4)]]
    for lv in range(3):
        own = np.nonzero(i % 3 == lv)[0]
        levels.append([make_table(ctx, k2, v2, c) for c in np.array_split(own, 8)])
    dl = DeviceLevels(ctx, levels)
    tables = dl.tables

    rng = np.random.default_rng(7)
    pick = rng.integers(0, n, n_s)
    lo = torch.from_numpy(k2[pick].reshape(-1).copy()).to(dev)
    lo_pos = torch.arange(n_s + 1, device=dev, dtype=torch.int64) * KLEN
    lo_kind = torch.full((n_s,), _lib.BOUND_INCLUDED, dtype=torch.uint8, device=dev)
    hi = torch.zeros(16, dtype=torch.uint8, device=dev)
    hi_pos = torch.zeros(n_s + 1, dtype=torch.int64, device=dev)
    hi_kind = torch.full((n_s,), _lib.BOUND_UNBOUNDED, dtype=torch.uint8, device=dev)
    row = {"tables": len(tables), "l0_tables": 4, "levels_below": 3, "tables_per_level": 8,
           "blocks_per_level_table": blocks,
           "entries": int(sum(t.n_blocks for t in tables)) * PER_BLOCK, "scans": n_s, "steps": steps}

    for limit in (10, 100):
        out = {k: torch.empty(n_s, dtype=torch.uint8, device=dev) for k in ("result", "status")}
        out["where"] = torch.empty(3 * n_s, dtype=torch.int32, device=dev)
        for k in ("hit_table", "hit_block", "hit_entry"):
            out[k] = torch.empty(n_s * limit, dtype=torch.int32, device=dev)
        for k in ("first", "key_first", "val_first"):
            out[k] = torch.empty(n_s + 1, dtype=torch.int64, device=dev)
        out["info"] = torch.empty(3, dtype=torch.int64, device=dev)

        def scan_ranges():
            ctx.scan_ranges_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data,
                                 dl.n_levels, lo.data_ptr(), lo_pos.data_ptr(), lo_kind.data_ptr(),
                                 hi.data_ptr(), hi_pos.data_ptr(), hi_kind.data_ptr(), n_s, limit,
                                 *(out[k].data_ptr() for k in
                                   ("result", "status", "where", "hit_table", "hit_block",
                                    "hit_entry", "first", "key_first", "val_first", "info")), s)

        scan_ranges()
        n_ent, kbytes, vbytes = (int(x) for x in out["info"].cpu().numpy())
        kpos = torch.empty(n_ent + 1, dtype=torch.int64, device=dev)
        vpos = torch.empty(n_ent + 1, dtype=torch.int64, device=dev)
        d_keys = torch.empty(max(kbytes, 1), dtype=torch.uint8, device=dev)
        d_vals = torch.empty(max(vbytes, 1), dtype=torch.uint8, device=dev)

        def scan_entries():
            ctx.scan_entries_ptrs(dl.d_tables.data_ptr(), dl.n_tables, n_s, limit,
                                  out["hit_table"].data_ptr(), out["hit_block"].data_ptr(),
                                  out["hit_entry"].data_ptr(), out["first"].data_ptr(),
                                  d_keys.data_ptr(), kbytes, kpos.data_ptr(), d_vals.data_ptr(),
                                  vbytes, vpos.data_ptr(), s)

        # the answers: no scan fails; scan j starts at its lower bound (a key of the set) and its
        # keys ascend; a scan short of `limit` entries ran into the end of the key space
        scan_entries()
        torch.cuda.synchronize(dev)
        res = out["result"].cpu().numpy()
        assert (res != _lib.SCAN_ERROR).all() and (out["status"].cpu().numpy() == 0).all()
        first = out["first"].cpu().numpy()
        counts = np.diff(first)
        assert ((counts == limit) | (res == _lib.SCAN_DONE)).all() and counts.min() >= 1
        assert kbytes == n_ent * KLEN and vbytes == n_ent * VLEN
        got = d_keys.cpu().numpy().reshape(n_ent, KLEN)
        assert (got[first[:-1]] == k2[pick]).all()
        void = got.view(f"S{KLEN}").reshape(-1)     # bytewise order = key order
        inner = np.ones(n_ent, bool)
        inner[first[:-1]] = False
        assert (void[1:][inner[1:]] > void[:-1][inner[1:]]).all()

        src = torch.empty(kbytes + vbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms_r = timed(scan_ranges, stream, steps, dev)
        ms_e = timed(scan_entries, stream, steps, dev)
        ms_c = timed(lambda: dst.copy_(src), stream, steps, dev)
        row[f"limit_{limit}"] = {
            "entries_yielded": n_ent, "gathered_bytes": kbytes + vbytes,
            "scans_more": int((res == _lib.SCAN_MORE).sum()),
            "ms_scan_ranges": round(ms_r, 4), "ms_scan_entries": round(ms_e, 4),
            "ms_copy_of_gathered_bytes": round(ms_c, 4),
            "scans_per_s": round(n_s / ((ms_r + ms_e) * 1e-3)),
            "entries_per_s": round(n_ent / ((ms_r + ms_e) * 1e-3))}

    # the seek phase's floor: every lower bound sought in every table, a launch per table
    s_out = {k: torch.empty(n_s, dtype=t, device=dev) for k, t in
             (("block", torch.int32), ("entry", torch.int32), ("status", torch.uint8),
              ("valid", torch.uint8))}
    structs = [t.table() for t in tables]

    def seek_floor():
        for st in structs:
            ctx.seek_keys_ptrs(st, lo.data_ptr(), lo_pos.data_ptr(), n_s, s_out["block"].data_ptr(),
                               s_out["entry"].data_ptr(), s_out["status"].data_ptr(),
                               s_out["valid"].data_ptr(), s)

    row["ms_seek_floor_seek_keys_per_table"] = round(timed(seek_floor, stream, steps, dev), 4)
    row["seeks"] = n_s * len(tables)
    return row


def shares(path: str) -> dict:
    """Per-kernel shares of a rocprofv3 kernel_stats CSV: the scan's kernels and the rest."""
    rows = list(csv.DictReader(open(path)))
    ours = ("scan_seek_kernel", "scan_merge_kernel", "scan_entries_kernel", "scan_info_kernel",
            "flat_scan_")
    out = {}
    for r in rows:
        name = r["Name"]
        if any(o in name for o in ours):
            short = next(o for o in ours if o in name)
            if short == "scan_entries_kernel":
                short += "<copy>" if "Lb1" in name or "<true>" in name else "<lengths>"
            if short == "flat_scan_":
                short = "flat_scan_* (prefix sums)"
            d = out.setdefault(short, {"calls": 0, "total_ns": 0})
            d["calls"] += int(r["Calls"])
            d["total_ns"] += int(float(r["TotalDurationNs"]))
    total = sum(d["total_ns"] for d in out.values()) or 1
    for d in out.values():
        d["share_of_scan_kernels"] = round(d["total_ns"] / total, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048, help="blocks per table of levels 1-3")
    ap.add_argument("--scans", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shares", help="a rocprofv3 kernel_stats CSV to fold into --out (no GPU work)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.shares:
        doc = json.load(open(a.out))
        doc["kernel_shares"] = {"what": "rocprofv3 --kernel-trace --stats over another run of the "
                                        "probe (both limits, settle and checks included)",
                                "kernels": shares(a.shares)}
    else:
        ctx = _lib.Context(0)
        row = probe(ctx, a.blocks, a.scans, a.steps)
        print(json.dumps(row), flush=True)
        ctx.close()
        doc = {"what": WHAT, "row": row}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

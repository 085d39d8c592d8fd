#!/usr/bin/env python3
"""Resident tables as a compaction's inputs (diagnostic, GPU box): the task of DESIGN.md §3.13 and
tools/tables_probe.py (2^22 "4k" synth entries in 4 sorted runs, block size 4096), its four input
tables resident as DeviceTables. In one process, after untimed warm-up calls, the routes alternating
over the rounds so that all see the same clocks; HIP events on the stream unless it says wall:

  (a) the two new calls: tpz_table_runs_layout and tpz_table_runs_entries through the raw pointers
      (no read-back between them: the outputs are sized from the warm-up), each alone and together;
      the gather in both forms through the diagnostic export (copydev::wave_copy, which the product
      call launches, and aligned loads + funnel shift); and entries_from_tables as a caller sees it
      (events and wall)
  (b) the only device route the parent commit has from the same resident data: decode_flat of each
      table's kept batch plus entries_from_flat (events and wall; it synchronises per table)
  (c) a plain device copy of the gathered key and value bytes (the floor of the gather)
  (d) compact_task wall time over the DeviceTables against the same tables as host regions

Prints one JSON object and, with --out, writes it (profiles/runs/probe.json).

    python3 tools/runs_probe.py [--entries 4194304] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tables_probe import make_task  # noqa: E402
from topazdb_amd import _lib  # noqa: E402
from topazdb_amd.batch import decode_flat  # noqa: E402
from topazdb_amd.compact import compact_task, entries_from_flat, entries_from_tables  # noqa: E402
from topazdb_amd.table import DeviceTable  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3), "all": [round(x, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=64 << 20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.Context(0)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    regions, bounds = make_task(a.entries, a.runs)
    tables = [DeviceTable(ctx, src.tobytes(), ext) for src, ext in regions]
    n_runs = len(tables)

    # warm-up, the sizes of the outputs, and the two routes agree on the entries
    ent, run_first = entries_from_tables(ctx, tables)
    n, kb, vb = ent.n, int(ent.kpos[-1].cpu()), int(ent.vpos[-1].cpu())
    off = 0
    for t in tables:
        f = entries_from_flat(ctx, decode_flat(ctx, t.batch).complete())
        k1, v1 = int(f.kpos[-1].cpu()), int(f.vpos[-1].cpu())
        k0, v0 = int(ent.kpos[off].cpu()), int(ent.vpos[off].cpu())
        assert torch.equal(f.keys[:k1], ent.keys[k0:k0 + k1])
        assert torch.equal(f.vals[:v1], ent.vals[v0:v0 + v1])
        assert torch.equal(f.kpos + k0, ent.kpos[off:off + f.n + 1])
        off += f.n
        del f
    assert off == n

    bf = np.zeros(n_runs + 1, np.uint32)
    np.cumsum([t.n_blocks for t in tables], out=bf[1:])
    nb = int(bf[-1])
    descs = (_lib.Table * n_runs)(*[t.table() for t in tables])
    d_tabs = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(dev)
    first = torch.empty(3 * (nb + 1), dtype=torch.int64, device=dev)
    rf = torch.empty(n_runs + 1, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    keys = torch.empty(kb, dtype=torch.uint8, device=dev)
    vals = torch.empty(vb, dtype=torch.uint8, device=dev)
    kpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    vpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    keys2, vals2 = torch.empty_like(keys), torch.empty_like(vals)

    def layout():
        ctx.table_runs_layout_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                                   rf.data_ptr(), info.data_ptr(), s)

    def gather(aligned=None):
        ctx.table_runs_entries_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                                    keys.data_ptr(), kb, kpos.data_ptr(), vals.data_ptr(), vb,
                                    vpos.data_ptr(), n, s, aligned)

    def both():
        layout()
        gather()

    def flat_route():
        for t in tables:
            entries_from_flat(ctx, decode_flat(ctx, t.batch).complete())

    def copy():
        keys2.copy_(keys)
        vals2.copy_(vals)

    def timed(fn):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    layout()
    for al in (1, 0):       # both forms write the same bytes
        keys.zero_()
        gather(al)
        torch.cuda.synchronize(dev)
        assert torch.equal(keys, ent.keys[:kb]) and torch.equal(vals, ent.vals[:vb])
        assert torch.equal(kpos, ent.kpos)
    fns = {"a_layout": layout, "a_gather_aligned": lambda: gather(1),
           "a_gather_wave_copy": lambda: gather(0), "a_both_calls": both,
           "a_entries_from_tables": lambda: entries_from_tables(ctx, tables),
           "b_decode_flat_entries_from_flat": flat_route, "c_plain_copy": copy}
    ms = {k: ([], []) for k in fns}
    for k, fn in fns.items():
        fn()
    for _ in range(a.rounds):          # alternating, so that a drift hits all
        for k, fn in fns.items():
            w, e = timed(fn)
            ms[k][0].append(w)
            ms[k][1].append(e)
    del ent, keys2, vals2

    def task(inputs):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = compact_task(ctx, inputs, bounds, table_capacity=a.capacity)
        torch.cuda.synchronize(dev)
        w = (time.perf_counter() - t0) * 1e3
        n_out = (len(out), out.entries.n)
        del out
        return w, n_out

    assert task(tables)[1] == task(regions)[1]      # warm-up; same tables and entries out
    d_res, d_host = [], []
    for _ in range(a.rounds):
        d_res.append(task(tables)[0])
        d_host.append(task(regions)[0])

    row = {
        "what": "tools/runs_probe.py: resident tables gathered into merge runs vs the flat decode "
                "of their kept batches, one MI355X, one run; ms",
        "entries": n, "runs": n_runs, "block_size": 4096, "blocks": nb, "key_bytes": kb,
        "value_bytes": vb, "input_bytes": int(sum(int(ext[-1]) for _, ext in regions)),
        "rounds": a.rounds,
    }
    for k in fns:
        row[k + "_events_ms"] = spread(ms[k][1])
    for k in ("a_entries_from_tables", "b_decode_flat_entries_from_flat"):
        row[k + "_wall_ms"] = spread(ms[k][0])
    row["d_compact_task_resident_wall_ms"] = spread(d_res)
    row["d_compact_task_host_regions_wall_ms"] = spread(d_host)
    moved = 2 * (kb + vb) + 16 * n
    row["a_gather_aligned_tb_s"] = round(moved / row["a_gather_aligned_events_ms"]["median"] / 1e9, 3)
    row["a_gather_wave_copy_tb_s"] = round(moved / row["a_gather_wave_copy_events_ms"]["median"] / 1e9, 3)
    row["c_plain_copy_tb_s"] = round(2 * (kb + vb) / row["c_plain_copy_events_ms"]["median"] / 1e9, 3)
    row["b_over_a_events"] = round(row["b_decode_flat_entries_from_flat_events_ms"]["median"] /
                                   row["a_entries_from_tables_events_ms"]["median"], 2)
    row["host_regions_over_resident_wall"] = round(
        row["d_compact_task_host_regions_wall_ms"]["median"] /
        row["d_compact_task_resident_wall_ms"]["median"], 2)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

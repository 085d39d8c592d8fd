#!/usr/bin/env python3
"""compact_task beside compact() (diagnostic, GPU box): 2^22 "4k" synth entries in 4 sorted runs,
block size 4096, codec 1, fpp 0.1, the default 64 MiB table capacity (about 8 output tables), four
key ranges. In one process, after bench.settle, alternating the two so that they see the same
clocks:

  compact()        the parent path: one unbounded data region (upload, decode, merge, plan, encode)
  compact_task()   the same front, then per table plan window + cut + encode + bloom, and one
                   tpz_sst_finish: whole SST file images
  + d2h            each followed by the copies to the host a writer of files needs (the region;
                   every image)

both as host wall time around calls that end in a device read-back, and the new pieces alone with
HIP events on the task's own data: the bound search, one window plan + cut, one table's bloom
build, tpz_sst_finish over all images (run again: it rewrites the same bytes), and the
whole-range CRC over the same bytes (the finish's share that is FileObject::create's checksum).
The host copies go to pageable memory. Prints one JSON object and, with --out, writes it
(profiles/tables/probe.json).

    python3 tools/tables_probe.py [--entries 4194304] [--runs 4] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
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

from bench import settle  # noqa: E402
from merge_probe import make_runs  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.compact import compact, compact_task, entries_bound  # noqa: E402


def events(fn, stream, steps: int, dev) -> float:
    settle(fn, dev, 0.5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def wall(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def make_task(n_total: int, n_runs: int):
    """The runs' data regions and four key ranges of about equal entry counts that cover every
    key: the keys at the quartiles of the sorted stream."""
    runs = make_runs(n_total, n_runs, False)
    regions = [synth.build_blocks(*run, 4096) for run in runs]
    keys = np.sort(np.concatenate([r[0].reshape(-1, 16) for r in runs]).view("S16").reshape(-1))
    cuts = [bytes(keys[len(keys) * q // 4]) for q in (1, 2, 3)]
    bounds = [(b"", (cuts[0], False)), (cuts[0], (cuts[1], False)), (cuts[1], (cuts[2], False)),
              (cuts[2], (b"\xff" * 17, True))]
    return regions, bounds


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
    regions, bounds = make_task(a.entries, a.runs)

    def task():
        return compact_task(ctx, regions, bounds, table_capacity=a.capacity)

    def task_d2h():
        return [t.image.cpu() for t in task()]

    def parent():
        return compact(ctx, regions)

    def parent_d2h():
        return parent().region.cpu()

    out = task()
    assert sum(t.n_entries for t in out) == a.entries
    parent()                        # every shape once before the timed rounds
    settle(parent, dev, 1.0)
    ms = {"compact": [], "compact_task": [], "compact_d2h": [], "compact_task_d2h": []}
    for _ in range(a.rounds):       # alternating, so that a drift hits both
        ms["compact"].append(wall(parent, dev))
        ms["compact_task"].append(wall(task, dev))
        ms["compact_d2h"].append(wall(parent_d2h, dev))
        ms["compact_task_d2h"].append(wall(task_d2h, dev))

    # the new pieces alone, on the task's merged entries and its first table
    ent, t0 = out.entries, out[0]
    ment = ent.struct()
    probes = [p for lo, up in bounds for p in ((lo, False), up)]
    ms_bound = wall(lambda: entries_bound(ctx, ent, probes), dev)
    win = t0.n_entries
    went = _lib.Entries(ent.keys.data_ptr(), ent.kpos.data_ptr(), ent.vals.data_ptr(),
                        ent.vpos.data_ptr(), win, ent.keys.numel(), ent.vals.numel())
    first = torch.empty(win + 1, dtype=torch.int32, device=dev)
    ext = torch.empty(win + 1, dtype=torch.int64, device=dev)
    pinfo = torch.empty(4, dtype=torch.int32, device=dev)
    cut = torch.empty(8, dtype=torch.int64, device=dev)

    def do_plan():
        ctx.plan_blocks_async_ptrs(went, 4096, first.data_ptr(), ext.data_ptr(), pinfo.data_ptr(),
                                   stream.cuda_stream)

    def do_cut():
        ctx.table_cut_ptrs(ment, 0, win, win, first.data_ptr(), ext.data_ptr(), ext.data_ptr(),
                           pinfo.data_ptr(), 4096, a.capacity, cut.data_ptr(), stream.cuda_stream)

    do_plan()
    geo = _lib.bloom_geometry(win, 0.1)
    filt = torch.empty((geo[0] + 3) // 4, dtype=torch.int32, device=dev)

    def do_bloom():
        _lib.check(_lib.lib().tpz_bloom_build(ctx.handle, C.c_void_p(ent.keys.data_ptr()),
                                              C.c_void_p(ent.kpos.data_ptr()), win, 0.1,
                                              C.c_void_p(filt.data_ptr()),
                                              C.c_void_p(stream.cuda_stream)), "tpz_bloom_build")

    # the finish once more over the task's images (it rewrites the same bytes), and the
    # whole-range CRC over the same span
    d_desc, n_img, max_blocks, span = out.finish_args
    finfo = torch.empty((n_img, 4), dtype=torch.int64, device=dev)

    def do_finish():
        ctx.sst_finish_ptrs(ment, d_desc.data_ptr(), n_img, max_blocks, out.arena.data_ptr(), span,
                            finfo.data_ptr(), stream.cuda_stream)

    crc_ext = torch.tensor([0, span], dtype=torch.int64, device=dev)
    crc_out = torch.empty(1, dtype=torch.int32, device=dev)

    def do_crc():
        ctx.crc32_ptrs(out.arena.data_ptr(), crc_ext.data_ptr(), 1, span, crc_out.data_ptr(),
                       stream.cuda_stream)

    row = {
        "what": "tools/tables_probe.py: compact_task vs compact() on one MI355X, host wall ms per "
                "call (median of rounds, alternating) and HIP-event ms for the pieces",
        "entries": a.entries, "runs": a.runs, "block_size": 4096, "codec": 1, "fpp": 0.1,
        "table_capacity": a.capacity, "ranges": len(bounds), "tables": len(out),
        "image_bytes": int(sum(t.size for t in out)), "rounds": a.rounds,
        "ms_compact": round(statistics.median(ms["compact"]), 3),
        "ms_compact_task": round(statistics.median(ms["compact_task"]), 3),
        "ms_compact_plus_region_d2h": round(statistics.median(ms["compact_d2h"]), 3),
        "ms_compact_task_plus_images_d2h": round(statistics.median(ms["compact_task_d2h"]), 3),
        "ms_all_rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "ms_bound_search_8_probes_with_readback": round(ms_bound, 4),
        "ms_plan_one_table_window": round(events(do_plan, stream, 10, dev), 4),
        "ms_cut_one_table": round(events(do_cut, stream, 20, dev), 4),
        "ms_bloom_one_table": round(events(do_bloom, stream, 10, dev), 4),
        "ms_finish_all_images": round(events(do_finish, stream, 10, dev), 4),
        "ms_crc_all_images": round(events(do_crc, stream, 10, dev), 4),
        "first_table_entries": win,
    }
    row["task_over_compact"] = round(row["ms_compact_task"] / row["ms_compact"], 3)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

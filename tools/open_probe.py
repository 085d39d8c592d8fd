#!/usr/bin/env python3
"""Opening compact_task's output tables where they lie (diagnostic, GPU box): the task of
tools/tables_probe.py (2^22 "4k" synth entries in 4 sorted runs, block size 4096, codec 1, fpp
0.1, 64 MiB tables: about 8 images). In one process, after untimed warm-up calls, alternating over
the rounds so that both routes see the same clocks:

  (a) device open   TaskTables.open: tpz_open_index, the read-back of its totals and d_info,
                    tpz_open_metas, and per table the decode in place; by HIP events on the
                    stream and by host wall time ending in a synchronise
  (b) host route    what a caller had before: D2H of every image, the host parse of table.py
                    (SsTable._read_bloom, BlockMeta.decode_block_meta), and DeviceTable over the
                    region bytes (H2D, decode). SsTable.open itself goes on to build a host Block
                    per block (host_blocks), which the device open has no counterpart of: it is
                    left out of (b) so that both routes end with the same resident tables.
  (c) the two calls alone for the first table (HIP events): tpz_open_index (fill of the scratch,
      open_index_kernel, open_scan_kernel) and tpz_open_metas (open_metas_kernel,
      open_flags_kernel)
  (d) beside them, tpz_decode_blocks over the same table's data region into exact columns

Prints one JSON object and, with --out, writes it (profiles/open/probe.json).

    python3 tools/open_probe.py [--entries 4194304] [--rounds 5] [--out FILE]
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
from topazdb_amd.batch import DeviceBatch, decode_batch, exact_columns, open_index, open_metas  # noqa: E402
from topazdb_amd.compact import compact_task  # noqa: E402
from topazdb_amd.table import BlockMeta, DeviceTable, FileObject, SsTable  # noqa: E402


def host_route(ctx, out):
    tables = []
    for i, t in enumerate(out):
        f = FileObject(f"t{i}", t.image.cpu().numpy().tobytes())
        offset, bloom = SsTable._read_bloom(f)
        meta_offset = int.from_bytes(f.read(offset - 4, 4), "big")
        metas = BlockMeta.decode_block_meta(f.read(meta_offset, offset - 4 - meta_offset))
        ext = np.array([m.offset for m in metas] + [meta_offset], np.uint64)
        tables.append(DeviceTable(ctx, f.read(0, meta_offset), ext, [m.first_key for m in metas],
                                  None if bloom is None else bloom.filter))
    return tables


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
    regions, bounds = make_task(a.entries, a.runs)
    out = compact_task(ctx, regions, bounds, table_capacity=a.capacity)
    del regions

    def device_route():
        return out.open(ctx)

    def timed(fn):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        r = fn()
        e1.record(stream)
        torch.cuda.synchronize(dev)
        w = (time.perf_counter() - t0) * 1e3
        n = len(r)
        del r
        return w, e0.elapsed_time(e1), n

    opened = device_route()            # warm-up, and the two routes agree on what they opened
    hosted = host_route(ctx, out)
    for t, h in zip(opened, hosted):
        assert t.n_blocks == h.n_blocks and t.bloom_len == h.bloom_len
        assert torch.equal(t.first_keys[:h.first_keys.numel()], h.first_keys)
        assert torch.equal(t.batch.ext, h.batch.ext) and torch.equal(t.status, h.status)
    n_blocks = [t.n_blocks for t in opened]
    del opened, hosted
    ms = {"device_wall": [], "device_events": [], "host_wall": []}
    for _ in range(a.rounds):          # alternating, so that a drift hits both
        w, e, _n = timed(device_route)
        ms["device_wall"].append(w)
        ms["device_events"].append(e)
        ms["host_wall"].append(timed(lambda: host_route(ctx, out))[0])

    # (c) the two calls alone for the first table, (d) the decode of its data region
    t0 = out[0]
    img = t0.image
    idx = open_index(ctx, img, [(0, t0.size)])
    nb, kb = int(idx.file_block[1].cpu()), int(idx.file_key[1].cpu())
    ext, pos, keys = open_metas(ctx, idx, nb, kb)
    sb = _lib.open_scratch_bytes(idx.span_bytes, 1)
    s = stream.cuda_stream

    def do_index():
        ctx.open_index_ptrs(img.data_ptr(), idx.span_bytes, idx.span.data_ptr(), 1,
                            idx.info.data_ptr(), idx.file_block.data_ptr(),
                            idx.file_key.data_ptr(), idx.scratch.data_ptr(), sb, s)

    def do_metas():
        ctx.open_metas_ptrs(img.data_ptr(), idx.span_bytes, idx.span.data_ptr(), 1,
                            idx.info.data_ptr(), idx.file_block.data_ptr(),
                            idx.file_key.data_ptr(), idx.scratch.data_ptr(), sb, ext.data_ptr(),
                            pos.data_ptr(), keys.data_ptr(), nb, kb, s)

    batch = DeviceBatch(img, ext[:nb + 1], 0)
    cols = exact_columns(ctx, batch)

    def do_decode():
        decode_batch(ctx, batch, cols)

    def events(fn, steps=10):
        fn()
        torch.cuda.synchronize(dev)
        xs = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            xs.append(e0.elapsed_time(e1) / steps)
        return spread(xs)

    row = {
        "what": "tools/open_probe.py: opening compact_task's images in HBM vs the host route, one "
                "MI355X, one run; ms",
        "entries": a.entries, "runs": a.runs, "block_size": 4096, "codec": 1,
        "table_capacity": a.capacity, "tables": len(out), "blocks_per_table": n_blocks,
        "image_bytes": int(sum(t.size for t in out)), "rounds": a.rounds,
        "a_device_open_wall_ms": spread(ms["device_wall"]),
        "a_device_open_events_ms": spread(ms["device_events"]),
        "b_host_route_wall_ms": spread(ms["host_wall"]),
        "c_first_table_bytes": int(t0.size), "c_first_table_blocks": nb,
        "c_first_table_meta_bytes": int(idx.info[0, 3].cpu()),
        "c_open_index_ms": events(do_index),
        "c_open_metas_ms": events(do_metas),
        "d_decode_blocks_ms": events(do_decode, 5),
    }
    row["host_over_device_wall"] = round(row["b_host_route_wall_ms"]["median"] /
                                         row["a_device_open_wall_ms"]["median"], 2)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

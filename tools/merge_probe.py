#!/usr/bin/env python3
"""tpz_merge_runs beside the two steps it sits between (diagnostic, GPU box): R runs of the "4k"
synth entries, 2^22 entries in all, keys disjoint across runs or half of the keys held by two
runs. For the same entries, in one process, after bench.settle: the flat decode of the runs'
blocks, the merge, and the write side (tpz_plan_blocks_async + tpz_encode_blocks_async) over the
merged entries, each timed with HIP events. Prints one JSON line per (runs, shape) and, with
--out, writes them to a file (profiles/merge/probe.json).

    python3 tools/merge_probe.py [--entries 4194304] [--runs 4 8] [--steps 10] [--out FILE]

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats` with one --runs value.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import settle  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.batch import DeviceBatch, FlatColumns, decode_flat  # noqa: E402
from topazdb_amd.compact import entries_from_flat, merge_runs  # noqa: E402
from topazdb_amd.encode import (encode_blocks_async, encode_bound,  # noqa: E402
                                plan_blocks_async)


def make_runs(n_total: int, n_runs: int, overlap: bool):
    """Per run: (keys, kpos, vals, vpos) of sorted "4k" entries. Entry i of the generated stream
    belongs to run i % R; with `overlap` every second entry is also in the next run, so half of
    the keys are held by two runs (the lower run wins them)."""
    m = n_total * 2 // 3 if overlap else n_total
    keys, kpos, vals, vpos = synth.entries("4k", m)
    k2, v2 = keys.reshape(m, 16), vals.reshape(m, 100)
    i = np.arange(m)
    runs = []
    for r in range(n_runs):
        sel = i % n_runs == r
        if overlap:
            sel |= (i % 2 == 0) & ((i % n_runs + 1) % n_runs == r)
        idx = np.nonzero(sel)[0]
        n = len(idx)
        runs.append((k2[idx].reshape(-1), np.arange(n + 1, dtype=np.uint64) * 16,
                     v2[idx].reshape(-1), np.arange(n + 1, dtype=np.uint64) * 100))
    return runs


def timed(fn, stream, steps: int, dev) -> float:
    settle(fn, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def probe(ctx, n_total: int, n_runs: int, overlap: bool, steps: int) -> dict:
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    runs = make_runs(n_total, n_runs, overlap)
    srcs, exts, tblock, off = [], [np.zeros(1, np.uint64)], [0], 0
    for run in runs:
        src, ext = synth.build_blocks(*run, 4096)
        srcs.append(src)
        exts.append(ext[1:] + np.uint64(off))
        off += int(ext[-1])
        tblock.append(tblock[-1] + len(ext) - 1)
    batch = DeviceBatch(np.concatenate(srcs), np.concatenate(exts), 0)
    cols = FlatColumns(ctx, batch)
    decode_flat(ctx, batch, cols).complete()
    ent = entries_from_flat(ctx, cols)
    run_first = cols.first[0].cpu().numpy()[np.asarray(tblock)]
    rf = np.ascontiguousarray(run_first.astype(np.uint32))
    merged, src_entry, info = merge_runs(ctx, ent, run_first)
    n_in, n_out = ent.n, merged.n
    assert n_out == (n_total * 2 // 3 if overlap else n_total), (n_in, n_out)   # every key once
    scratch = torch.empty(4, dtype=torch.int64, device=dev)
    enc_out = torch.empty(encode_bound(merged), dtype=torch.uint8, device=dev)

    def do_decode():
        ctx.decode_flat_ptrs(batch.src.data_ptr(), batch.ext.data_ptr(), batch.n_blocks,
                             batch.src_bytes, cols.ptrs(), stream.cuda_stream)

    def do_merge():
        ctx.merge_runs_ptrs(ent.struct(), rf.ctypes.data, n_runs, merged.keys.data_ptr(),
                            merged.kpos.data_ptr(), merged.vals.data_ptr(), merged.vpos.data_ptr(),
                            src_entry.data_ptr(), scratch.data_ptr(), stream.cuda_stream)

    def do_encode():
        first, ext, pinfo = plan_blocks_async(ctx, merged, 4096, stream)
        encode_blocks_async(ctx, merged, first, ext, pinfo, out=enc_out, stream=stream)

    ms_decode = timed(do_decode, stream, steps, dev)
    ms_merge = timed(do_merge, stream, steps, dev)
    ms_encode = timed(do_encode, stream, steps, dev)
    assert int(scratch[0]) == n_out
    return {"runs": n_runs, "shape": "overlap50" if overlap else "disjoint", "entries_in": n_in,
            "entries_out": n_out, "ms_decode_flat": round(ms_decode, 4),
            "ms_merge": round(ms_merge, 4), "ms_plan_encode": round(ms_encode, 4),
            "merge_entries_per_s": round(n_in / (ms_merge * 1e-3)),
            "merge_over_decode_plus_encode": round(ms_merge / (ms_decode + ms_encode), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rows = []
    for n_runs in a.runs:
        for overlap in (False, True):
            rows.append(probe(ctx, a.entries, n_runs, overlap, a.steps))
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/merge_probe.py: 2^22 '4k' synth entries in R runs, HIP-event "
                               "ms per step on one MI355X", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

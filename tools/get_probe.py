#!/usr/bin/env python3
"""tpz_get_keys / tpz_get_values beside the route they replace (diagnostic, GPU box).

A LevelController's worth of resident tables of the "4k" synth shape (16-B keys, 100-B values, 34
entries per 4 KiB block): 4 overlapping L0 tables and 3 levels of 8 disjoint tables each, every
table with its bloom filter (fpp 0.1, built on the device). Entry i of the generated stream is in
level 1 + i % 3 (each level cut into 8 contiguous tables) and, for i % 16 < 4, also in L0 table
i % 16. 2^20 queries, half of them keys of the set (drawn uniformly), half the same keys with the
last byte changed (absent, but in range of the same tables).

In one process, after 0.3 s of untimed launches each (bench.settle), HIP events around:
  get_keys          one tpz_get_keys over all queries
  get_keys_values   tpz_get_keys + tpz_get_values (the value buffer sized beforehand; the read-back
                    of the total between the two calls is not in the device time)
  baseline          the per-table route of INTEGRATION.md before this call existed: one
                    tpz_bloom_may_contain and one tpz_seek_keys per table over all queries (2 T
                    launches; its host combine and value reads are not counted, which favours it)
The fused answers are checked against the generated entries first. Prints one JSON line and, with
--out, writes it to a file (profiles/get/probe.json).

    python3 tools/get_probe.py [--blocks 2048] [--queries 1048576] [--steps 10] [--out FILE]

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats` in a run of its own.
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
from topazdb_amd.encode import DeviceEntries, bloom_build  # noqa: E402
from topazdb_amd.levels import DeviceLevels  # noqa: E402
from topazdb_amd.table import DeviceTable  # noqa: E402

PER_BLOCK, KLEN, VLEN = 34, 16, 100


def make_table(ctx, k2, v2, idx):
    """A resident table of entries idx (sorted) of the stream."""
    n = len(idx)
    keys, vals = k2[idx].reshape(-1), v2[idx].reshape(-1)
    kpos = np.arange(n + 1, dtype=np.uint64) * KLEN
    vpos = np.arange(n + 1, dtype=np.uint64) * VLEN
    src, ext = synth.build_blocks(keys, kpos, vals, vpos, 4096)
    first = [k2[i].tobytes() for i in idx[::PER_BLOCK]]
    assert len(first) == len(ext) - 1
    bloom = bloom_build(ctx, DeviceEntries(keys, kpos, vals, vpos, ctx.device), 0.1)
    return DeviceTable(ctx, src.tobytes(), ext, first, bloom)


def timed(fn, stream, steps: int, dev) -> float:
    settle(fn, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def probe(ctx, blocks: int, n_q: int, steps: int) -> dict:
    dev = torch.device("cuda", ctx.device)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    n = 3 * 8 * blocks * PER_BLOCK                    # entries of the stream; a level holds a third
    keys, _, vals, _ = synth.entries("4k", n)
    k2, v2 = keys.reshape(n, KLEN), vals.reshape(n, VLEN)
    i = np.arange(n)
    l0 = [make_table(ctx, k2, v2, np.nonzero(i % 16 == r)[0]) for r in range(4)]
    levels = [l0]
    for lv in range(3):
        own = np.nonzero(i % 3 == lv)[0]
        levels.append([make_table(ctx, k2, v2, c) for c in np.array_split(own, 8)])
    dl = DeviceLevels(ctx, levels)
    tables = dl.tables

    rng = np.random.default_rng(7)
    pick = rng.integers(0, n, n_q)
    qk = k2[pick].copy()
    absent = np.arange(n_q) % 2 == 1
    qk[absent, KLEN - 1] ^= 0x55                      # the random tail: not a key of the set
    q = torch.from_numpy(qk.reshape(-1)).to(dev)
    qp = torch.arange(n_q + 1, device=dev, dtype=torch.int64) * KLEN
    out = {k: torch.empty(n_q, dtype=t, device=dev) for k, t in
           (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
            ("block", torch.int32), ("entry", torch.int32))}
    val_pos = torch.empty(n_q + 1, dtype=torch.int64, device=dev)

    def get_keys():
        ctx.get_keys_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data,
                          dl.n_levels, q.data_ptr(), qp.data_ptr(), n_q, out["result"].data_ptr(),
                          out["status"].data_ptr(), out["table"].data_ptr(),
                          out["block"].data_ptr(), out["entry"].data_ptr(), val_pos.data_ptr(), s)

    get_keys()
    total = int(val_pos[n_q].item())
    d_vals = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)

    def get_values():
        ctx.get_values_ptrs(dl.d_tables.data_ptr(), dl.n_tables, n_q, out["result"].data_ptr(),
                            out["table"].data_ptr(), out["block"].data_ptr(),
                            out["entry"].data_ptr(), val_pos.data_ptr(), d_vals.data_ptr(), total, s)

    def get_both():
        get_keys()
        get_values()

    # the answers: every present query FOUND with its entry's value, every other ABSENT; a key
    # of L0 table r comes from there (the newest table holding it), the others from their level
    get_both()
    torch.cuda.synchronize(dev)
    res = out["result"].cpu().numpy()
    assert (res[~absent] == _lib.GET_FOUND).all() and (res[absent] == _lib.GET_ABSENT).all()
    tab = out["table"].cpu().numpy()
    in_l0 = pick[~absent] % 16 < 4
    assert (tab[~absent][in_l0] == pick[~absent][in_l0] % 16).all()
    assert (tab[~absent][~in_l0] >= 4).all()
    assert total == VLEN * int((~absent).sum())
    got = d_vals.cpu().numpy().reshape(-1, VLEN)
    assert (got == v2[pick[~absent]]).all()

    # the baseline: every query against every table, one bloom and one seek launch per table
    b_out = torch.empty(n_q, dtype=torch.uint8, device=dev)
    s_out = {k: torch.empty(n_q, dtype=t, device=dev) for k, t in
             (("block", torch.int32), ("entry", torch.int32), ("status", torch.uint8),
              ("valid", torch.uint8))}
    structs = [t.table() for t in tables]

    def baseline():
        for t, st in zip(tables, structs):
            ctx.bloom_ptrs(t.bloom.data_ptr(), t.bloom_len, q.data_ptr(), qp.data_ptr(), n_q,
                           b_out.data_ptr(), s)
            ctx.seek_keys_ptrs(st, q.data_ptr(), qp.data_ptr(), n_q, s_out["block"].data_ptr(),
                               s_out["entry"].data_ptr(), s_out["status"].data_ptr(),
                               s_out["valid"].data_ptr(), s)

    ms_keys = timed(get_keys, stream, steps, dev)
    ms_both = timed(get_both, stream, steps, dev)
    ms_base = timed(baseline, stream, steps, dev)
    ms_keys2 = timed(get_keys, stream, steps, dev)    # again, after the baseline: the spread
    return {"tables": len(tables), "l0_tables": 4, "levels_below": 3, "tables_per_level": 8,
            "blocks_per_level_table": blocks, "entries": int(sum(t.n_blocks for t in tables)) * PER_BLOCK,
            "queries": n_q, "present": int((~absent).sum()), "value_bytes": total,
            "ms_get_keys": round(ms_keys, 4), "ms_get_keys_again": round(ms_keys2, 4),
            "ms_get_keys_values": round(ms_both, 4), "ms_baseline_bloom_seek_per_table": round(ms_base, 4),
            "get_keys_queries_per_s": round(n_q / (ms_keys * 1e-3)),
            "get_keys_values_queries_per_s": round(n_q / (ms_both * 1e-3)),
            "baseline_queries_per_s": round(n_q / (ms_base * 1e-3)),
            "baseline_over_get_keys": round(ms_base / ms_keys, 2),
            "baseline_over_get_keys_values": round(ms_base / ms_both, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048, help="blocks per table of levels 1-3")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    row = probe(ctx, a.blocks, a.queries, a.steps)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/get_probe.py: 4 L0 tables + 3 levels x 8 tables of the '4k' synth "
                               "shape, HIP-event ms per step on one MI355X, one run", "row": row},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

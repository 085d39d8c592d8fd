#!/usr/bin/env python3
"""tpz_lsm_get_keys and tpz_lsm_scan_ranges beside the calls they extend (diagnostic, GPU box).

The table set of tools/get_probe.py (4 overlapping L0 tables and 3 levels of 8 disjoint tables of
the "4k" synth shape: 16-B keys, 100-B values) under 5 memtable runs of 2^18 entries of the same
shape. A run's keys are keys of the stream with the last byte changed (^ 0xAA), so no table holds
them. 2^20 queries: half absent (a key of the set with the last byte ^ 0x55), half present, a
quarter of the present ones keys of a run. 2^16 scans as tools/scan_probe.py draws them, at limits
10 and 100.

In one process, after 0.3 s of untimed launches each (bench.settle), HIP events around `steps`
calls, every variant `repeats` times with the orders interleaved (a, b, c, .., a, b, c, ..):
  lsm_get_prefix      tpz_lsm_get_keys over the 5 runs with their prefix columns
  lsm_get_keys_only   the same with d_prefix = NULL (the bisections read the keys)
  lsm_get_no_runs     tpz_lsm_get_keys with n_runs = 0
  get_keys            tpz_get_keys (what lsm_get_no_runs must not be slower than)
  lsm_scan_*, scan_ranges likewise per limit.
The row holds each variant's median ms and its spread (max - min over the repeats) and, for the
comparison that matters, lsm_*_no_runs / the existing call. The answers are checked first.
Prints one JSON line and, with --out, writes it to a file (profiles/lsm/probe.json).

    python3 tools/lsm_probe.py [--blocks 2048] [--run-entries 262144] [--queries 1048576]
                               [--scans 65536] [--steps 10] [--repeats 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from get_probe import KLEN, PER_BLOCK, VLEN, make_table, timed  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.levels import DeviceLsm, DeviceRun  # noqa: E402

N_RUNS = 5


def make_run(ctx, k2, v2, idx, prefix: bool) -> tuple[DeviceRun, np.ndarray]:
    """A run of the entries idx of the stream, their keys' last byte changed; sorted by key."""
    keys = k2[idx].copy()
    keys[:, KLEN - 1] ^= 0xAA
    order = np.argsort(keys.view(f"S{KLEN}").reshape(-1), kind="stable")
    keys, vals = keys[order], v2[idx][order]
    void = keys.view(f"S{KLEN}").reshape(-1)
    assert (void[1:] > void[:-1]).all()
    dev = torch.device("cuda", ctx.device)
    n = len(idx)
    cols = {"keys": torch.from_numpy(keys.reshape(-1)).to(dev),
            "kpos": torch.arange(n + 1, device=dev, dtype=torch.int64) * KLEN,
            "vals": torch.from_numpy(vals.reshape(-1)).to(dev),
            "vpos": torch.arange(n + 1, device=dev, dtype=torch.int64) * VLEN}
    return DeviceRun(ctx, cols, prefix), keys


def interleaved(fns: dict, stream, steps: int, repeats: int, dev) -> dict:
    """name -> [ms per call] over `repeats` rounds, the variants taking turns within a round."""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn, stream, steps, dev))
    return ms


def summary(ms: dict) -> dict:
    return {k: {"ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4)}
            for k, v in ms.items()}


def probe(ctx, blocks: int, run_entries: int, n_q: int, n_s: int, steps: int, repeats: int) -> dict:
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
    rng = np.random.default_rng(11)
    run_entries = min(run_entries, n)
    made = [make_run(ctx, k2, v2, np.sort(rng.choice(n, run_entries, replace=False)), True)
            for _ in range(N_RUNS)]
    runs, run_keys = [m[0] for m in made], [m[1] for m in made]
    bare = []
    for r in runs:                               # the same columns without the prefix column
        b = DeviceRun(ctx, {"keys": r.keys, "kpos": r.kpos, "vals": r.vals, "vpos": r.vpos}, False)
        bare.append(b)
    with_prefix = DeviceLsm(ctx, runs, levels)
    keys_only = DeviceLsm(ctx, bare, levels)
    dl = with_prefix

    # ---- get
    pick = rng.integers(0, n, n_q)
    qk = k2[pick].copy()
    absent = np.arange(n_q) % 2 == 1
    qk[absent, KLEN - 1] ^= 0x55
    in_run = np.arange(n_q) % 8 == 0             # a quarter of the present ones
    which = rng.integers(0, N_RUNS, n_q)
    for r in range(N_RUNS):
        sel = np.nonzero(in_run & (which == r))[0]
        qk[sel] = run_keys[r][rng.integers(0, run_entries, len(sel))]
    q = torch.from_numpy(qk.reshape(-1)).to(dev)
    qp = torch.arange(n_q + 1, device=dev, dtype=torch.int64) * KLEN
    out = {k: torch.empty(n_q, dtype=t, device=dev) for k, t in
           (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
            ("block", torch.int32), ("entry", torch.int32))}
    val_pos = torch.empty(n_q + 1, dtype=torch.int64, device=dev)
    outs = [out[k].data_ptr() for k in ("result", "status", "table", "block", "entry")] + \
        [val_pos.data_ptr()]

    def lsm_get(lsm, n_runs):
        return lambda: ctx.lsm_get_keys_ptrs(lsm.d_runs.data_ptr(), n_runs, dl.d_tables.data_ptr(),
                                             dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
                                             q.data_ptr(), qp.data_ptr(), n_q, *outs, s)

    def get_keys():
        ctx.get_keys_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data,
                          dl.n_levels, q.data_ptr(), qp.data_ptr(), n_q, *outs, s)

    # the answers: a run's key comes from a run (the newest holding it), every other present key
    # from a table, the rest is absent; both forms of the bisection agree
    columns = []
    for lsm in (with_prefix, keys_only):
        lsm_get(lsm, N_RUNS)()
        torch.cuda.synchronize(dev)
        columns.append([out[k].cpu().numpy().copy() for k in ("result", "table", "entry")])
    assert all((a == b).all() for a, b in zip(*columns))
    res, tab, _ = columns[0]
    tab = tab.view(np.uint32)
    assert (res[absent & ~in_run] == _lib.GET_ABSENT).all() and (res[~absent | in_run] == _lib.GET_FOUND).all()
    assert ((tab[in_run] & _lib.HIT_MEM) != 0).all() and ((tab[~absent & ~in_run] & _lib.HIT_MEM) == 0).all()
    lsm_get(with_prefix, 0)()
    torch.cuda.synchronize(dev)
    a = [out[k].cpu().numpy().copy() for k in ("result", "table", "block", "entry")]
    get_keys()
    torch.cuda.synchronize(dev)
    assert all((x == out[k].cpu().numpy()).all() for x, k in zip(a, ("result", "table", "block", "entry")))

    get_ms = interleaved({"lsm_get_prefix": lsm_get(with_prefix, N_RUNS),
                          "lsm_get_keys_only": lsm_get(keys_only, N_RUNS),
                          "lsm_get_no_runs": lsm_get(with_prefix, 0), "get_keys": get_keys},
                         stream, steps, repeats, dev)
    row = {"box": socket.gethostname(), "tables": dl.n_tables, "runs": N_RUNS,
           "run_entries": run_entries, "blocks_per_level_table": blocks, "queries": n_q,
           "queries_answered_by_a_run": int(in_run.sum()), "scans": n_s, "steps": steps,
           "repeats": repeats, "get": summary(get_ms)}
    g = row["get"]
    row["get"]["no_runs_over_get_keys"] = round(g["lsm_get_no_runs"]["ms"] / g["get_keys"]["ms"], 4)
    row["get"]["prefix_over_keys_only"] = round(g["lsm_get_prefix"]["ms"] / g["lsm_get_keys_only"]["ms"], 4)

    # ---- scan
    pick = rng.integers(0, n, n_s)
    lo = torch.from_numpy(k2[pick].reshape(-1).copy()).to(dev)
    lo_pos = torch.arange(n_s + 1, device=dev, dtype=torch.int64) * KLEN
    lo_kind = torch.full((n_s,), _lib.BOUND_INCLUDED, dtype=torch.uint8, device=dev)
    hi = torch.zeros(16, dtype=torch.uint8, device=dev)
    hi_pos = torch.zeros(n_s + 1, dtype=torch.int64, device=dev)
    hi_kind = torch.full((n_s,), _lib.BOUND_UNBOUNDED, dtype=torch.uint8, device=dev)
    bounds = [x.data_ptr() for x in (lo, lo_pos, lo_kind, hi, hi_pos, hi_kind)]
    for limit in (10, 100):
        so = {k: torch.empty(n_s, dtype=torch.uint8, device=dev) for k in ("result", "status")}
        so["where"] = torch.empty(3 * n_s, dtype=torch.int32, device=dev)
        for k in ("hit_table", "hit_block", "hit_entry"):
            so[k] = torch.empty(n_s * limit, dtype=torch.int32, device=dev)
        for k in ("first", "key_first", "val_first"):
            so[k] = torch.empty(n_s + 1, dtype=torch.int64, device=dev)
        so["info"] = torch.empty(3, dtype=torch.int64, device=dev)
        sp = [so[k].data_ptr() for k in ("result", "status", "where", "hit_table", "hit_block",
                                         "hit_entry", "first", "key_first", "val_first", "info")]

        def lsm_scan(lsm, n_runs, sp=sp, limit=limit):
            return lambda: ctx.lsm_scan_ranges_ptrs(lsm.d_runs.data_ptr(), n_runs,
                                                    dl.d_tables.data_ptr(), dl.n_tables,
                                                    dl.level_first.ctypes.data, dl.n_levels,
                                                    *bounds, n_s, limit, *sp, s)

        def scan_ranges(sp=sp, limit=limit):
            ctx.scan_ranges_ptrs(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data,
                                 dl.n_levels, *bounds, n_s, limit, *sp, s)

        # the answers: no scan fails; with the runs every scan still yields `limit` entries or ends,
        # and some of them come from runs; without runs the two calls agree
        lsm_scan(with_prefix, N_RUNS)()
        torch.cuda.synchronize(dev)
        assert (so["result"].cpu().numpy() != _lib.SCAN_ERROR).all()
        first = so["first"].cpu().numpy()
        hit_tab = so["hit_table"].cpu().numpy().view(np.uint32).reshape(n_s, limit)
        from_runs = int(sum(((hit_tab[j, :first[j + 1] - first[j]] & _lib.HIT_MEM) != 0).sum()
                            for j in range(0, n_s, 64)))
        assert from_runs > 0
        lsm_scan(with_prefix, 0)()
        torch.cuda.synchronize(dev)
        a = [so[k].cpu().numpy().copy() for k in ("result", "first", "key_first", "val_first")]
        scan_ranges()
        torch.cuda.synchronize(dev)
        assert all((x == so[k].cpu().numpy()).all()
                   for x, k in zip(a, ("result", "first", "key_first", "val_first")))
        ms = interleaved({"lsm_scan_prefix": lsm_scan(with_prefix, N_RUNS),
                          "lsm_scan_keys_only": lsm_scan(keys_only, N_RUNS),
                          "lsm_scan_no_runs": lsm_scan(with_prefix, 0), "scan_ranges": scan_ranges},
                         stream, steps, repeats, dev)
        r = summary(ms)
        r["no_runs_over_scan_ranges"] = round(r["lsm_scan_no_runs"]["ms"] / r["scan_ranges"]["ms"], 4)
        r["prefix_over_keys_only"] = round(r["lsm_scan_prefix"]["ms"] / r["lsm_scan_keys_only"]["ms"], 4)
        row[f"scan_limit_{limit}"] = r
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048, help="blocks per table of levels 1-3")
    ap.add_argument("--run-entries", type=int, default=1 << 18)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--scans", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    row = probe(ctx, a.blocks, a.run_entries, a.queries, a.scans, a.steps, a.repeats)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/lsm_probe.py: tools/get_probe.py's 28 tables under 5 memtable "
                               "runs of the '4k' synth shape; HIP-event ms per call on one MI355X "
                               "(row.box), median and max - min over the interleaved repeats",
                       "row": row}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

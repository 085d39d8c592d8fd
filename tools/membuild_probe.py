#!/usr/bin/env python3
"""tpz_mem_build beside the merge the project already has (diagnostic, GPU box): 2^22 entries of
the "4k" synth shape (16-byte keys, 100-byte values) in random arrival order, with 0 %, 10 % and
100 % of the entries repeating a key (100 %: one key), under both rules. For the same entries, in
one process, after bench.settle, each timed with HIP events:
  - tpz_mem_build whole, and cut after the sort passes and after the pick + scan
    (tpz_debug_mem_build), which gives the sort passes, the pick and the gather separately;
  - tpz_merge_runs over the same entries pre-sorted on the host into 4 runs: the yardstick.
Prints one JSON line per (duplicates, mode) and, with --out, writes them to a file
(profiles/membuild/probe.json).

    python3 tools/membuild_probe.py [--entries 4194304] [--steps 10] [--out FILE]
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

from bench import settle  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.compact import merge_runs  # noqa: E402
from topazdb_amd.encode import DeviceEntries  # noqa: E402

KLEN, VLEN = 16, 100
BATCH = 4096          # entries per put_entries batch: one version each


def make_entries(n: int, dup_pct: int, seed: int = 1):
    """(keys n x 16, vals n x 100) in arrival order: n - d distinct keys and d = dup_pct % of n
    entries that repeat one of them, shuffled; 100 %: one key n times."""
    rng = np.random.default_rng(seed)
    distinct = 1 if dup_pct == 100 else n - n * dup_pct // 100
    keys, _, vals, _ = synth.entries("4k", distinct)
    k2, v2 = keys.reshape(distinct, KLEN), vals.reshape(distinct, VLEN)
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(pick)
    v = v2[pick].copy()
    v[:, :8] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)     # a value names its entry
    return np.ascontiguousarray(k2[pick]), v


def timed(fn, stream, steps: int, dev) -> float:
    settle(fn, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def probe(ctx, n: int, dup_pct: int, steps: int) -> list[dict]:
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    k2, v2 = make_entries(n, dup_pct)
    pos = lambda w: torch.from_numpy(np.arange(n + 1, dtype=np.int64) * w).to(dev)   # noqa: E731
    ent = DeviceEntries(torch.from_numpy(k2.reshape(-1)).to(dev), pos(KLEN),
                        torch.from_numpy(v2.reshape(-1)).to(dev), pos(VLEN), 0)
    ver = torch.from_numpy(1 + np.arange(n, dtype=np.int64) // BATCH).to(dev)
    out = {"keys": torch.empty(n * KLEN, dtype=torch.uint8, device=dev),
           "vals": torch.empty(n * VLEN, dtype=torch.uint8, device=dev)}
    for name, dt in (("kpos", torch.int64), ("vpos", torch.int64), ("pre", torch.int64),
                     ("over", torch.int64), ("src", torch.int32)):
        out[name] = torch.empty(n + 1, dtype=dt, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    L = _lib.lib()
    distinct = len(np.unique(k2.view("V16")))
    rows = []
    for mode, name in ((_lib.MEM_REPLAY, "replay"), (_lib.MEM_PUT, "put")):
        def build(stop: int):
            _lib.check(L.tpz_debug_mem_build(
                ctx.handle, C.byref(ent.struct()), mode, C.c_void_p(ver.data_ptr()),
                C.c_void_p(out["keys"].data_ptr()), C.c_void_p(out["kpos"].data_ptr()),
                C.c_void_p(out["vals"].data_ptr()), C.c_void_p(out["vpos"].data_ptr()),
                C.c_void_p(out["pre"].data_ptr()), C.c_void_p(out["src"].data_ptr()),
                C.c_void_p(out["over"].data_ptr()), C.c_void_p(info.data_ptr()),
                C.c_void_p(stream.cuda_stream), stop), "tpz_debug_mem_build")

        ms_sort = timed(lambda: build(1), stream, steps, dev)
        ms_pick = timed(lambda: build(2), stream, steps, dev)
        ms_all = timed(lambda: build(0), stream, steps, dev)
        h = info.cpu().numpy().view(np.uint64)
        assert int(h[0]) == distinct and int(h[5]) == n, (h, distinct)
        rows.append({"dup_pct": dup_pct, "mode": name, "entries_in": n, "entries_out": int(h[0]),
                     "ms_build": round(ms_all, 4), "ms_sort_passes": round(ms_sort, 4),
                     "ms_pick_scan": round(ms_pick - ms_sort, 4),
                     "ms_gather": round(ms_all - ms_pick, 4),
                     "build_entries_per_s": round(n / (ms_all * 1e-3))})
    # the yardstick: the same entries sorted on the host into 4 runs, merged by tpz_merge_runs
    n_runs = 4
    cut = [n * r // n_runs for r in range(n_runs + 1)]
    order = np.concatenate([cut[r] + np.argsort(k2[cut[r]:cut[r + 1]].view("V16").reshape(-1),
                                                kind="stable") for r in range(n_runs)])
    sent = DeviceEntries(torch.from_numpy(k2[order].reshape(-1)).to(dev), pos(KLEN),
                         torch.from_numpy(v2[order].reshape(-1)).to(dev), pos(VLEN), 0)
    rf = np.ascontiguousarray(np.asarray(cut, np.uint32))
    merged, src_entry, minfo = merge_runs(ctx, sent, cut)
    scratch = torch.empty(4, dtype=torch.int64, device=dev)

    def do_merge():
        ctx.merge_runs_ptrs(sent.struct(), rf.ctypes.data, n_runs, merged.keys.data_ptr(),
                            merged.kpos.data_ptr(), merged.vals.data_ptr(), merged.vpos.data_ptr(),
                            src_entry.data_ptr(), scratch.data_ptr(), stream.cuda_stream)

    ms_merge = timed(do_merge, stream, steps, dev)
    for r in rows:
        r["ms_merge_4_sorted_runs"] = round(ms_merge, 4)
        r["build_over_merge"] = round(r["ms_build"] / ms_merge, 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--dups", type=int, nargs="+", default=[0, 10, 100])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    rows = []
    for d in a.dups:
        for row in probe(ctx, a.entries, d, a.steps):
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/membuild_probe.py: '4k' synth entries in random arrival order, "
                               f"HIP-event ms per step, mean of {a.steps} steps after settle, one "
                               f"MI355X ({torch.cuda.get_device_name(0)}), one run",
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tpz_raw_get_keys / tpz_raw_get_values (gets served from the encoded blocks in place) beside
tpz_get_keys / tpz_get_values over the decoded columns of the same data (diagnostic, GPU box).

The workload of tools/get_probe.py: 4 overlapping L0 tables and 3 levels of 8 disjoint tables of
the "4k" synth shape (16-B keys, 100-B values, 34 entries per 4 KiB block), every table with its
bloom filter; 2^20 queries, half of them present. Both routes are built over the same regions in
one process; their answers are compared first. Then, after the settle launches of each, the two
routes are timed in turn, five repeats each, interleaved (decoded, in place, decoded, ...), HIP
events around `steps` calls a repeat. Reports per route the median, minimum and maximum ms of
get_keys and of get_keys + get_values, the device bytes each route holds (RawTable.resident_bytes
summed; the DeviceTables' encoded region plus their decoded columns), and the one-off cost of
tpz_raw_verify against tpz_decode_blocks over the tables' blocks in one batch.

    python3 tools/rawget_probe.py [--blocks 2048] [--queries 1048576] [--steps 5] [--out FILE]

Writes one JSON line and, with --out, profiles/rawget/probe.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import settle  # noqa: E402
from topazdb_amd import _lib, synth  # noqa: E402
from topazdb_amd.batch import DeviceBatch, decode_batch, exact_columns  # noqa: E402
from topazdb_amd.encode import DeviceEntries, bloom_build  # noqa: E402
from topazdb_amd.levels import DeviceLevels  # noqa: E402
from topazdb_amd.table import DeviceTable, RawTable  # noqa: E402

PER_BLOCK, KLEN, VLEN = 34, 16, 100
REPEATS = 5


def make_tables(ctx, k2, v2, idx):
    """The decoded and the in-place table of entries idx (sorted) of the stream."""
    n = len(idx)
    keys, vals = k2[idx].reshape(-1), v2[idx].reshape(-1)
    kpos = np.arange(n + 1, dtype=np.uint64) * KLEN
    vpos = np.arange(n + 1, dtype=np.uint64) * VLEN
    src, ext = synth.build_blocks(keys, kpos, vals, vpos, 4096)
    first = [k2[i].tobytes() for i in idx[::PER_BLOCK]]
    bloom = bloom_build(ctx, DeviceEntries(keys, kpos, vals, vpos, ctx.device), 0.1)
    region = src.tobytes()
    return (DeviceTable(ctx, region, ext, first, bloom), RawTable(ctx, region, ext, first, bloom),
            (src, ext))


def tensor_bytes(obj) -> int:
    return sum(v.numel() * v.element_size() for v in vars(obj).values() if torch.is_tensor(v))


def decoded_bytes(t: DeviceTable) -> dict:
    image = t.batch.src_bytes + 8 * (t.n_blocks + 1)
    meta = sum(x.numel() * x.element_size() for x in (t.first_keys, t.first_pos, t.status)) + \
        (t.bloom.numel() if t.bloom is not None else 0)
    return {"image": int(image), "columns": int(tensor_bytes(t.cols)), "meta": int(meta)}


def once(fn, stream, steps: int, dev) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def spread(xs) -> dict:
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def probe(ctx, blocks: int, n_q: int, steps: int) -> dict:
    dev = torch.device("cuda", ctx.device)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    n = 3 * 8 * blocks * PER_BLOCK
    keys, _, vals, _ = synth.entries("4k", n)
    k2, v2 = keys.reshape(n, KLEN), vals.reshape(n, VLEN)
    i = np.arange(n)
    built = [[make_tables(ctx, k2, v2, np.nonzero(i % 16 == r)[0]) for r in range(4)]]
    for lv in range(3):
        own = np.nonzero(i % 3 == lv)[0]
        built.append([make_tables(ctx, k2, v2, c) for c in np.array_split(own, 8)])
    routes = {"decoded": DeviceLevels(ctx, [[t[0] for t in lv] for lv in built]),
              "in_place": DeviceLevels(ctx, [[t[1] for t in lv] for lv in built])}
    assert routes["in_place"].raw and not routes["decoded"].raw

    rng = np.random.default_rng(7)
    pick = rng.integers(0, n, n_q)
    qk = k2[pick].copy()
    absent = np.arange(n_q) % 2 == 1
    qk[absent, KLEN - 1] ^= 0x55
    q = torch.from_numpy(qk.reshape(-1)).to(dev)
    qp = torch.arange(n_q + 1, device=dev, dtype=torch.int64) * KLEN

    calls, outs = {}, {}
    for name, dl in routes.items():
        out = {k: torch.empty(n_q, dtype=t, device=dev) for k, t in
               (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
                ("block", torch.int32), ("entry", torch.int32))}
        out["val_pos"] = torch.empty(n_q + 1, dtype=torch.int64, device=dev)
        kfn = ctx.raw_get_keys_ptrs if dl.raw else ctx.get_keys_ptrs
        vfn = ctx.raw_get_values_ptrs if dl.raw else ctx.get_values_ptrs

        def get_keys(dl=dl, out=out, kfn=kfn):
            kfn(dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
                q.data_ptr(), qp.data_ptr(), n_q, out["result"].data_ptr(),
                out["status"].data_ptr(), out["table"].data_ptr(), out["block"].data_ptr(),
                out["entry"].data_ptr(), out["val_pos"].data_ptr(), s)

        get_keys()
        total = int(out["val_pos"][n_q].item())
        out["vals"] = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)

        def get_both(dl=dl, out=out, vfn=vfn, get_keys=get_keys, total=total):
            get_keys()
            vfn(dl.d_tables.data_ptr(), dl.n_tables, n_q, out["result"].data_ptr(),
                out["table"].data_ptr(), out["block"].data_ptr(), out["entry"].data_ptr(),
                out["val_pos"].data_ptr(), out["vals"].data_ptr(), total, s)

        get_both()
        calls[name], outs[name] = (get_keys, get_both), out
    torch.cuda.synchronize(dev)
    a, b = outs["decoded"], outs["in_place"]
    for k in a:
        assert torch.equal(a[k], b[k]), k                      # the two routes answer alike
    res = a["result"].cpu().numpy()
    assert (res[~absent] == _lib.GET_FOUND).all() and (res[absent] == _lib.GET_ABSENT).all()
    assert (b["vals"].cpu().numpy().reshape(-1, VLEN) == v2[pick[~absent]]).all()

    ms = {name: {"get_keys": [], "get_keys_values": []} for name in routes}
    for name in routes:
        for fn in calls[name]:
            settle(fn, dev)
    for _ in range(REPEATS):                                    # interleaved
        for name in routes:
            ms[name]["get_keys"].append(once(calls[name][0], stream, steps, dev))
            ms[name]["get_keys_values"].append(once(calls[name][1], stream, steps, dev))

    # the one-off cost per table set: tpz_raw_verify against the decode, all blocks in one batch
    src = np.concatenate([t[2][0] for lv in built for t in lv])
    exts, at = [np.zeros(1, np.uint64)], 0
    for lv in built:
        for t in lv:
            exts.append(t[2][1][1:] + np.uint64(at))
            at += int(t[2][1][-1])
    batch = DeviceBatch(src, np.concatenate(exts), ctx.device)
    nb = batch.n_blocks
    st = torch.empty(nb, dtype=torch.uint8, device=dev)
    crc = torch.empty(nb, dtype=torch.int32, device=dev)
    cols = exact_columns(ctx, batch)

    def verify():
        ctx.raw_verify_ptrs(batch.src.data_ptr(), batch.ext.data_ptr(), nb, batch.src_bytes,
                            st.data_ptr(), crc.data_ptr(), s)

    def decode():
        decode_batch(ctx, batch, cols)

    one_off = {}
    for name, fn in (("raw_verify", verify), ("decode", decode)):
        settle(fn, dev)
        one_off[name] = []
    for _ in range(REPEATS):
        for name, fn in (("raw_verify", verify), ("decode", decode)):
            one_off[name].append(once(fn, stream, steps, dev))
    assert int((st != 0).sum()) == 0

    dec = [decoded_bytes(t) for t in routes["decoded"].tables]
    held = {"in_place": int(sum(t.resident_bytes for t in routes["in_place"].tables)),
            "decoded_image": sum(d["image"] for d in dec),
            "decoded_columns": sum(d["columns"] for d in dec),
            "decoded_meta": sum(d["meta"] for d in dec)}
    held["decoded"] = held["decoded_image"] + held["decoded_columns"] + held["decoded_meta"]
    held["in_place_over_decoded"] = round(held["in_place"] / held["decoded"], 3)
    row = {"tables": routes["decoded"].n_tables, "blocks_per_level_table": blocks, "blocks": nb,
           "encoded_bytes": int(batch.src_bytes), "queries": n_q, "present": int((~absent).sum()),
           "steps_per_repeat": steps, "repeats": REPEATS, "device_bytes": held,
           "ms": {name: {k: spread(v) for k, v in r.items()} for name, r in ms.items()},
           "one_off_ms": {k: spread(v) for k, v in one_off.items()}}
    for k in ("get_keys", "get_keys_values"):
        row["in_place_over_decoded_" + k] = round(
            row["ms"]["in_place"][k]["median"] / row["ms"]["decoded"][k]["median"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048, help="blocks per table of levels 1-3")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    row = probe(ctx, a.blocks, a.queries, a.steps)
    print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"what": "tools/rawget_probe.py: 4 L0 tables + 3 levels x 8 tables of the "
                               "'4k' synth shape; the decoded and the in-place route interleaved "
                               "in one process, HIP-event ms per call, median / min / max of 5 "
                               "repeats, on one MI355X, one run",
                       "row": row}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

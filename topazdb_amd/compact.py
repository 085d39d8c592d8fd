"""Compaction on the device: decode -> merge -> plan -> encode -> compress with the entries in HBM.

`compact` is sub_compact's loop (src/level.rs:178-222) for one output table: a MergeIterator over
one SsTableIterator per input table (src/iterators/merge_iterator.rs:41-106) feeding
SsTableBuilder::add (src/table/builder.rs:49-64). The read side (tpz_decode_blocks_flat) leaves
the inputs' entries as flat columns, `entries_from_flat` (tpz_flat_entry_pos) turns those into
the write side's tpz_entries, `merge_runs` (tpz_merge_runs) merges the tables' runs with the
iterator's tie rule, and the write side (tpz_plan_blocks_async, tpz_encode_blocks_async,
tpz_compress_blocks) writes the output blocks. Tombstones (empty values) are kept: only
LsmIterator drops them, and compaction does not use it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import Context
from .batch import DeviceBatch, FlatColumns, decode_flat, decompress_batch
from .encode import (DeviceEntries, EntryError, compress_blocks, encode_blocks_async,
                     plan_blocks_async)
from .table import BlockError


def _dev(device: int) -> torch.device:
    return torch.device("cuda", device)


def entries_from_flat(ctx: Context, cols: FlatColumns, check: bool = True,
                      stream: torch.cuda.Stream | None = None) -> DeviceEntries:
    """tpz_flat_entry_pos: the decoded flat columns as the write side's entries (the key and value
    columns themselves plus absolute entry positions), in SsTableIterator order. One read-back of
    the first block whose status is not OK (`.bad_block`, -1: none); with `check` that block
    raises BlockError, as sub_compact's `?` fails the compaction there."""
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    cols.complete()
    n = cols.n_pairs
    kpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    vpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ctx.flat_entry_pos_ptrs(cols.ptrs(), cols.n_blocks, kpos.data_ptr(), vpos.data_ptr(),
                            info.data_ptr(), s.cuda_stream)
    s.synchronize()
    bad = int(info.cpu().numpy().view(np.uint32)[0])
    ent = DeviceEntries(cols.keys, kpos, cols.values, vpos, ctx.device)
    ent.bad_block = -1 if bad == 0xFFFFFFFF else bad
    if check and ent.bad_block >= 0:
        st = int(cols.status[bad].cpu())
        if st == _lib.BLOCK_CHECKSUM_MISMATCH:    # (the stored CRC is in the block, not the columns)
            text = f"checksum: actual {int(cols.crc[bad].cpu().numpy().view(np.uint32))}"
        else:
            text = _lib.format_block_error(st) or "entries an iterator cannot read"
        e = BlockError(f"block {bad}: {text}")
        e.block, e.status = bad, st
        raise e
    return ent


def merge_runs(ctx: Context, ent: DeviceEntries, run_first,
               stream: torch.cuda.Stream | None = None):
    """tpz_merge_runs over `ent`'s runs (run r = entries run_first[r] .. run_first[r + 1] - 1, in
    priority order). Returns (merged DeviceEntries, src_entry int32 tensor, info numpy uint64 x 4);
    one read-back of info trims the position tensors to n_out. Raises EntryError for an empty key
    (SsTableIterator is invalid there, BlockBuilder::add asserts)."""
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    rf = np.ascontiguousarray(np.asarray(run_first, np.int64).astype(np.uint32))
    n_runs = len(rf) - 1
    if n_runs < 0:
        raise ValueError("run_first needs n_runs + 1 entries")
    n = ent.n if n_runs else 0
    out_keys = torch.empty(max(ent.keys.numel(), 16), dtype=torch.uint8, device=dev)
    out_vals = torch.empty(max(ent.vals.numel(), 16), dtype=torch.uint8, device=dev)
    out_kpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_vpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
    src = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    ctx.merge_runs_ptrs(ent.struct(), rf.ctypes.data, n_runs, out_keys.data_ptr(),
                        out_kpos.data_ptr(), out_vals.data_ptr(), out_vpos.data_ptr(),
                        src.data_ptr(), info.data_ptr(), s.cuda_stream)
    s.synchronize()
    h = info.cpu().numpy().view(np.uint64)
    if int(h[3]) != 2**64 - 1:
        raise EntryError(int(h[3]), "key must not be empty")
    n_out = int(h[0])
    merged = DeviceEntries(out_keys, out_kpos[:n_out + 1], out_vals, out_vpos[:n_out + 1],
                           ctx.device)
    return merged, src[:n_out], h


Compacted = namedtuple("Compacted", "region ext first n_blocks entries")
Compacted.__doc__ = """compact()'s output: `region` (uint8 device tensor: the output data region),
`ext` (int64 device tensor, n_blocks + 1 block extents: BlockMeta::offset), `first` (int32 device
tensor, n_blocks + 1: each block's first entry, whose key is BlockMeta::first_key), and `entries`
(the merged DeviceEntries those indices refer to)."""


def compact(ctx: Context, regions, block_size: int = 4096, codec: int = 1,
            stream: torch.cuda.Stream | None = None) -> Compacted:
    """One output table of a compaction. `regions`: the input tables' (data-region bytes, block
    extents), in priority order (sub_compact's this_tables + next_tables: an earlier table wins a
    key). codec: the output's CompressOptions tag (1 Uncompress, 2 Snappy, 3 Lz4)."""
    if codec not in (1, 2, 3):
        raise ValueError(f"codec {codec}")
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    srcs, exts, tblock, off = [], [np.zeros(1, np.uint64)], [0], 0
    for src, ext in regions:
        a = np.frombuffer(src, np.uint8) if not isinstance(src, np.ndarray) else src
        e = np.asarray(ext, np.uint64)
        srcs.append(a[:int(e[-1])])
        exts.append(e[1:] + np.uint64(off))
        off += int(e[-1])
        tblock.append(tblock[-1] + len(e) - 1)
    host = np.concatenate(srcs) if srcs else np.zeros(0, np.uint8)
    ext = np.concatenate(exts)
    batch = DeviceBatch(host, ext, ctx.device)
    ends = ext[1:][ext[1:] > ext[:-1]].astype(np.int64) - 1
    if len(ends) and np.isin(host[ends], (2, 3)).any():       # compress::decode's codec step
        batch, cst = decompress_batch(ctx, batch, stream)
        bad = np.nonzero(cst[:batch.n_blocks].cpu().numpy() != _lib.BLOCK_OK)[0]
        if len(bad):
            raise BlockError(f"block {int(bad[0])}: "
                             f"{_lib.format_block_error(_lib.BLOCK_CODEC_ERROR)}")
    cols = decode_flat(ctx, batch, stream=stream).complete()
    ent = entries_from_flat(ctx, cols, stream=stream)
    run_first = cols.first[0].cpu().numpy()[np.asarray(tblock)]
    merged, _, _ = merge_runs(ctx, ent, run_first, stream)
    first, oext, info = plan_blocks_async(ctx, merged, block_size, s)
    out = encode_blocks_async(ctx, merged, first, oext, info, stream=s)
    _, bad, nb = (int(x) for x in info[:3].cpu().numpy().view(np.uint32))   # (waits for the stream)
    if bad != 0xFFFFFFFF:
        raise EntryError(bad, f"entry exceeds block_size {block_size} - 2")
    total = int(oext[nb].cpu()) if nb else 0
    if codec != 1 and nb:
        out, oext = compress_blocks(ctx, out, oext, nb, total, codec, stream=s)
        total = int(oext[nb].cpu())
    return Compacted(out[:total], oext[:nb + 1], first[:nb + 1], nb, merged)

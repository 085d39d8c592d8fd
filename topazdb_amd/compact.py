"""Compaction on the device: decode -> merge -> plan -> encode -> compress with the entries in HBM.

`compact` is sub_compact's loop (src/level.rs:178-222) for one output table: a MergeIterator over
one SsTableIterator per input table (src/iterators/merge_iterator.rs:41-106) feeding
SsTableBuilder::add (src/table/builder.rs:49-64). The read side (tpz_decode_blocks_flat) leaves
the inputs' entries as flat columns, `entries_from_flat` (tpz_flat_entry_pos) turns those into
the write side's tpz_entries, `merge_runs` (tpz_merge_runs) merges the tables' runs with the
iterator's tie rule, and the write side (tpz_plan_blocks_async, tpz_encode_blocks_async,
tpz_compress_blocks) writes the output blocks. Tombstones (empty values) are kept: only
LsmIterator drops them, and compaction does not use it. Input tables that are already resident as
DeviceTables skip the read side: `entries_from_tables` (tpz_table_runs_layout,
tpz_table_runs_entries) gathers their decoded columns into the runs the merge takes.

`compact_task` is do_compact (src/level.rs:133-222) around that: the sub-compactions' key ranges
over the merged entries (tpz_entries_bound), SsTableBuilder's table cuts (tpz_table_cut) and every
output table as a whole SST file image in one device arena (tpz_sst_finish); `sub_ranges` restates
RwsSlice::create + split (src/level/range.rs) on the host.

`flush_runs` is the write side of the memtables (start_flush and sync(), src/lsm_storage.rs:83-143,
:298-332): sorted memtable runs in HBM merged (tpz_merge_runs) into one L0 file image with the
same plan, encode, bloom and tpz_sst_finish steps; `flush_like_start_flush` and `flush_like_sync`
state the two orders the reference merges them in.
"""
from __future__ import annotations

import bisect
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import Context
from .batch import DeviceBatch, FlatColumns, decode_flat, decompress_batch
from .encode import (DeviceEntries, EntryError, compress_blocks, compress_bound, encode_blocks_async,
                     encode_bound, plan_blocks_async)
from .table import BlockError, DeviceTable, RawTable, ReferencePanic, open_images


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


def entries_from_tables(ctx: Context, tables, check: bool = True,
                        stream: torch.cuda.Stream | None = None):
    """tpz_table_runs_layout + tpz_table_runs_entries: resident DeviceTables, in priority order,
    as (DeviceEntries, run_first): a run per table holding its entries in SsTableIterator order,
    gathered out of the slotted columns that serve the gets (no upload, no second decode).
    run_first (numpy, len(tables) + 1) is merge_runs' run table. One read-back (the totals, the
    first block whose status is neither OK nor OK_SPILLED, and run_first), then the gather.
    `.bad_block` = (run, block) of that block, or None; with `check` it raises BlockError (with
    `.table`, `.block`, `.status`), as sub_compact's `?` fails the compaction there."""
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    tables = list(tables)
    if any(isinstance(t, RawTable) for t in tables):
        raise ValueError("in-place tables answer gets; compaction inputs need DeviceTables")
    n_runs = len(tables)
    if n_runs > _lib.MERGE_MAX_RUNS:
        raise ValueError(f"{n_runs} tables: tpz_merge_runs takes at most {_lib.MERGE_MAX_RUNS} runs")
    bf = np.zeros(n_runs + 1, np.uint32)
    np.cumsum([t.n_blocks for t in tables], out=bf[1:])
    nb = int(bf[-1])
    descs = (_lib.Table * max(n_runs, 1))(*[t.table() for t in tables])
    with torch.cuda.stream(s):      # (the upload and the read-back are torch's: same stream)
        d_tabs = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(dev)
        first = torch.empty(3 * (nb + 1), dtype=torch.int64, device=dev)
        # d_info (4 u64) and d_run_first (n_runs + 1 u32) in one buffer: one read-back
        buf = torch.empty(4 + (n_runs + 2) // 2, dtype=torch.int64, device=dev)
        ctx.table_runs_layout_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                                   buf.data_ptr() + 32, buf.data_ptr(), s.cuda_stream)
        h = buf.cpu().numpy()                                           # (waits for the stream)
        n, kb, vb, bad = (int(x) for x in h[:4].view(np.uint64))
        run_first = h[4:].view(np.uint32)[:n_runs + 1].astype(np.int64)
        if n >= 2**32 - 1:
            raise ValueError(f"{n} entries: a tpz_entries holds fewer than 2^32 - 1")
        keys = torch.empty(max(kb, 16), dtype=torch.uint8, device=dev)
        vals = torch.empty(max(vb, 16), dtype=torch.uint8, device=dev)
        kpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
        vpos = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ctx.table_runs_entries_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                                    keys.data_ptr(), kb, kpos.data_ptr(), vals.data_ptr(), vb,
                                    vpos.data_ptr(), n, s.cuda_stream)
    ent = DeviceEntries(keys, kpos, vals, vpos, ctx.device)
    ent.bad_block = None if bad == 2**64 - 1 else (bad >> 32, bad & 0xFFFFFFFF)
    if check and ent.bad_block is not None:
        run, blk = ent.bad_block
        st = int(tables[run].status[blk].cpu())
        if st == _lib.BLOCK_CHECKSUM_MISMATCH:    # (the stored CRC is in the block, not the columns)
            crc = int(tables[run].cols.crc[blk].cpu().numpy().view(np.uint32))
            text = f"checksum: actual {crc}"
        else:
            text = _lib.format_block_error(st) or "entries an iterator cannot read"
        e = BlockError(f"table {run} block {blk}: {text}")
        e.table, e.block, e.status = run, blk, st
        raise e
    return ent, run_first


def _merge_inputs(ctx: Context, regions, stream: torch.cuda.Stream | None) -> DeviceEntries:
    """compact's and compact_task's inputs, by type: resident DeviceTables go through
    entries_from_tables (no host concatenation, upload or decode), (bytes, extents) tuples through
    _merge_regions; then one tpz_merge_runs over a run per table."""
    regions = list(regions)
    resident = [isinstance(r, (DeviceTable, RawTable)) for r in regions]
    if regions and all(resident):
        ent, run_first = entries_from_tables(ctx, regions, stream=stream)
        return merge_runs(ctx, ent, run_first, stream)[0]
    if any(resident):
        raise TypeError("regions mixes DeviceTables with (bytes, extents) tuples")
    return _merge_regions(ctx, regions, stream)


def _merge_regions(ctx: Context, regions, stream: torch.cuda.Stream | None) -> DeviceEntries:
    """The read side and the merge of a compaction: the input tables' blocks through the codec
    step and the flat decode, then one tpz_merge_runs over a run per table."""
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
    return merge_runs(ctx, ent, run_first, stream)[0]


Compacted = namedtuple("Compacted", "region ext first n_blocks entries")
Compacted.__doc__ = """compact()'s output: `region` (uint8 device tensor: the output data region),
`ext` (int64 device tensor, n_blocks + 1 block extents: BlockMeta::offset), `first` (int32 device
tensor, n_blocks + 1: each block's first entry, whose key is BlockMeta::first_key), and `entries`
(the merged DeviceEntries those indices refer to)."""


def compact(ctx: Context, regions, block_size: int = 4096, codec: int = 1,
            stream: torch.cuda.Stream | None = None) -> Compacted:
    """One output table of a compaction. `regions`: the input tables' (data-region bytes, block
    extents), in priority order (sub_compact's this_tables + next_tables: an earlier table wins a
    key), or the input tables as resident DeviceTables, which are gathered where they lie
    (entries_from_tables); a mixture of the two is a TypeError. codec: the output's CompressOptions
    tag (1 Uncompress, 2 Snappy, 3 Lz4)."""
    if codec not in (1, 2, 3):
        raise ValueError(f"codec {codec}")
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    merged = _merge_inputs(ctx, regions, stream)
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


# ------------------------------------------------------------------------- a whole task
OutputTable = namedtuple("OutputTable", "image size meta_off bloom_off n_blocks first_entry "
                                        "n_entries")
OutputTable.__doc__ = """One output table of compact_task: `image` (uint8 device tensor, a slice of
the task's arena: the whole SST file, CRC trailer included), `size`, `meta_off`, `bloom_off` (None
without a bloom section), `n_blocks`, and the table's entries [first_entry, first_entry +
n_entries) in the task's merged entries: the first one's key is smallest_key, the last one's
biggest_key."""


class TaskTables(list):
    """compact_task's output: the OutputTables in key order, plus `arena` (the one device tensor
    their images are slices of, image starts 256-byte aligned), `entries` (the merged
    DeviceEntries their entry ranges refer to) and `finish_args` (the device descriptors, image
    count, block bound and span tpz_sst_finish ran with; tools/tables_probe.py times it again)."""
    arena: torch.Tensor
    entries: DeviceEntries

    def open(self, ctx: Context, verify: bool = False, strict: bool = True,
             raw: bool = False) -> list:
        """The task's output tables as resident DeviceTables, in this list's order, opened where
        their images lie (table.open_images: no D2H, host parse or upload); ready for
        DeviceLevels(ctx, levels) / DeviceLsm. verify: the whole-file CRC check first (the images
        were written by this process: off by default). raw: as in-place RawTables (gets only, no
        decoded columns)."""
        if not len(self):
            return []
        base = self.arena.data_ptr()
        order = sorted(range(len(self)), key=lambda i: self[i].image.data_ptr())
        got = open_images(ctx, self.arena,
                          [(self[i].image.data_ptr() - base, self[i].size) for i in order],
                          verify, strict, raw)
        out = [None] * len(self)
        for i, t in zip(order, got):
            out[i] = t
        return out


def _bound_lower(lower) -> bytes:
    """sub_compact's lower: Included(key) as bytes or (key, True); anything else panics
    (src/level.rs:190-193)."""
    if isinstance(lower, (bytes, bytearray)):
        return bytes(lower)
    if isinstance(lower, tuple) and len(lower) == 2 and lower[1] is True:
        return bytes(lower[0])
    raise ReferencePanic("invalid lower")


def _bound_upper(upper):
    """sub_compact's upper: (key, inclusive); Unbounded (None) panics (src/level.rs:199-205)."""
    if isinstance(upper, tuple) and len(upper) == 2 and upper[0] is not None:
        return bytes(upper[0]), bool(upper[1])
    raise ReferencePanic("invalid upper")


def entries_bound(ctx: Context, ent: DeviceEntries, probes, stream=None) -> np.ndarray:
    """tpz_entries_bound: for every (key, inclusive) probe the number of `ent`'s entries with a
    key < key, or <= key when inclusive. One read-back."""
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    n = len(probes)
    pos = np.zeros(n + 1, np.int64)
    np.cumsum([len(k) for k, _ in probes], out=pos[1:])
    buf = np.frombuffer(b"".join(k for k, _ in probes) or b"\0", np.uint8).copy()
    q = torch.from_numpy(buf).to(dev)
    qp = torch.from_numpy(pos).to(dev)
    fl = torch.from_numpy(np.array([1 if i else 0 for _, i in probes] or [0], np.uint8)).to(dev)
    out = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ctx.entries_bound_ptrs(ent.struct(), q.data_ptr(), qp.data_ptr(), fl.data_ptr(), n,
                           out.data_ptr(), s.cuda_stream)
    s.synchronize()
    return out[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def _window(ent: DeviceEntries, start: int, n: int) -> _lib.Entries:
    """Entries [start, start + n) of `ent` as a tpz_entries of their own (the byte columns are
    shared, the positions stay absolute)."""
    return _lib.Entries(ent.keys.data_ptr(), ent.kpos.data_ptr() + 8 * start, ent.vals.data_ptr(),
                        ent.vpos.data_ptr() + 8 * start, n, ent.keys.numel(), ent.vals.numel())


def compact_task(ctx: Context, regions, bounds, block_size: int = 4096, codec: int = 1,
                 false_positive_rate: float = 0.1, table_capacity: int = 64 << 20,
                 stream: torch.cuda.Stream | None = None) -> TaskTables:
    """A whole compaction task (do_compact, src/level.rs:133-222) on the device: the SST files its
    sub-compactions write, as images in one device arena, each ready for one D2H copy.

    `regions`: as for compact(), the input tables in priority order, as (bytes, extents) tuples
    or as resident DeviceTables (then nothing is uploaded or decoded again); every table's keys are
    strictly increasing (with repeated keys the reference's seek lands on any of them).
    `bounds`: the sub-compactions' key ranges, a list of (lower, (upper, inclusive)) as sub_ranges
    returns them; lower is Included. The inputs are merged once and the merged entries split at the
    bounds (tpz_entries_bound); every range restarts the table and block chain, as each
    sub_compact starts a fresh SsTableBuilder. Per output table: plan a window of blocks
    (tpz_plan_blocks_async), find the table's cut in it (tpz_table_cut: reach_capacity,
    src/table/builder.rs:88-94, with TABLE_CAPACITY = table_capacity), encode the table's blocks at
    its image start (and compress them for codec 2 / 3), build its bloom filter (iff
    false_positive_rate.is_sign_positive()); tpz_sst_finish then completes every image. One
    read-back per output table with codec 1 (the cut); codecs 2 / 3 read the window's and the
    table's compressed lengths back too, compress a table's blocks a second time when the window
    held more than the table, and take one copy of the compressed region into the arena."""
    if codec not in (1, 2, 3):
        raise ValueError(f"codec {codec}")
    if table_capacity <= 0:
        raise ValueError("table_capacity 0: the reference builds a table of no entries and panics")
    segs = [(_bound_lower(lo), _bound_upper(up)) for lo, up in bounds]
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):      # (the copies and read-backs below are torch's: same stream)
        return _compact_task(ctx, regions, segs, block_size, codec, false_positive_rate,
                             table_capacity, s)


def _compact_task(ctx: Context, regions, segs, block_size: int, codec: int,
                  false_positive_rate: float, table_capacity: int, s) -> TaskTables:
    dev = _dev(ctx.device)
    stream = s
    merged = _merge_inputs(ctx, regions, stream)
    out = TaskTables()
    out.entries = merged
    out.arena = torch.empty(0, dtype=torch.uint8, device=dev)
    n = merged.n
    if not segs or n == 0:
        return out
    probes = [p for lo, up in segs for p in ((lo, False), up)]
    at = entries_bound(ctx, merged, probes, stream)
    spans = [(int(at[2 * i]), int(at[2 * i + 1])) for i in range(len(segs))]
    spans = [(lo, hi) for lo, hi in spans if hi > lo]
    if not spans:
        return out
    has_bloom = math.copysign(1.0, false_positive_rate) > 0          # is_sign_positive
    # the arena holds any outcome: every entry its own block, every block's meta, the filters of
    # all keys, and per table its offsets, CRC, filter rounding and alignment
    ment = merged.struct()
    data_bound = encode_bound(merged)
    if codec != 1:
        data_bound = compress_bound(data_bound, n)
    t_bound = len(spans) + min(n // 2, (data_bound + 2 * n) // table_capacity)
    geo_all = _lib.bloom_geometry(n, false_positive_rate) if has_bloom else None
    arena_cap = (data_bound + 6 * n + int(merged.keys.numel()) + (geo_all[0] if geo_all else 0)
                 + t_bound * (12 + 16 + 256) + 256)
    arena = torch.empty(arena_cap, dtype=torch.uint8, device=dev)
    # where each range's first window ends: one call per range, one read-back for all
    cuts = torch.empty((len(spans), 8), dtype=torch.int64, device=dev)
    for i, (lo, hi) in enumerate(spans):
        ctx.table_cut_ptrs(ment, lo, 0, hi, 0, 0, 0, 0, block_size, table_capacity,
                           cuts[i].data_ptr(), s.cuda_stream)
    s.synchronize()
    first_win = cuts[:, 7].cpu().numpy()
    cut = torch.empty(8, dtype=torch.int64, device=dev)
    descs, keep, tables, off = [], [], [], 0
    for (lo, hi), w in zip(spans, first_win):
        t, w = lo, int(w)
        while t < hi:
            win = w - t
            went = _window(merged, t, win)
            first = torch.empty(win + 1, dtype=torch.int32, device=dev)
            ext = torch.empty(win + 1, dtype=torch.int64, device=dev)
            info = torch.empty(4, dtype=torch.int32, device=dev)
            ctx.plan_blocks_async_ptrs(went, block_size, first.data_ptr(), ext.data_ptr(),
                                       info.data_ptr(), s.cuda_stream)
            img = arena[off:]
            cext, wnb = ext, 0
            if codec != 1:      # the capacity counts stored bytes: the window through the codec
                wraw = _window_bytes(merged, t, win, s)
                plain = torch.empty(wraw + 13 * win + 16, dtype=torch.uint8, device=dev)
                ctx.encode_blocks_async_ptrs(went, first.data_ptr(), ext.data_ptr(),
                                             info.data_ptr(), plain.data_ptr(), s.cuda_stream)
                _, bad, wnb = (int(x) for x in info[:3].cpu().numpy().view(np.uint32))
                if bad != 0xFFFFFFFF:
                    raise EntryError(t + bad, f"entry exceeds block_size {block_size} - 2")
                wtotal = int(ext[wnb].cpu())
                comp, cext = compress_blocks(ctx, plain, ext, wnb, wtotal, codec, stream=s)
            ctx.table_cut_ptrs(ment, t, win, hi, first.data_ptr(), ext.data_ptr(),
                               cext.data_ptr(), info.data_ptr(), block_size, table_capacity,
                               cut.data_ptr(), s.cuda_stream)
            if codec == 1:      # the table's blocks, straight to their place in the image
                ctx.encode_blocks_async_ptrs(went, first.data_ptr(), ext.data_ptr(),
                                             info.data_ptr(), img.data_ptr(), s.cuda_stream)
            h = cut.cpu().numpy().view(np.uint64)                      # (waits for the stream)
            status, nb, n_ent, data, kbytes = (int(h[j]) for j in (0, 2, 3, 4, 5))
            if status == _lib.CUT_BAD_ENTRY:
                raise EntryError(int(h[1]), f"entry exceeds block_size {block_size} - 2")
            if status == _lib.CUT_NONE and w < hi:      # (codecs 2 / 3: the window held no cut)
                w = int(h[7])
                continue
            if codec != 1:
                if status == _lib.CUT_FOUND:   # the table ends inside the window: its blocks alone
                    ctx.encode_blocks_async_ptrs(went, first.data_ptr(), ext.data_ptr(),
                                                 info.data_ptr(), plain.data_ptr(), s.cuda_stream)
                    comp, cext = compress_blocks(ctx, plain, ext, nb, data, codec, stream=s)
                data = int(cext[nb].cpu())
                img[:data].copy_(comp[:data])
            filt, flen = None, 0
            if has_bloom:
                geo = _lib.bloom_geometry(n_ent, false_positive_rate)
                if geo is None:     # fpp 0 (`% limit` divides by zero) or >= 1 (bloom.rs:49)
                    raise ReferencePanic(f"no bloom filter for {n_ent} keys at fpp "
                                         f"{false_positive_rate}")
                flen = geo[0]
                filt = torch.empty((flen + 3) // 4, dtype=torch.int32, device=dev)
                _lib.check(_lib.lib().tpz_bloom_build(
                    ctx.handle, C.c_void_p(merged.keys.data_ptr()),
                    C.c_void_p(merged.kpos.data_ptr() + 8 * t), n_ent, false_positive_rate,
                    C.c_void_p(filt.data_ptr()), C.c_void_p(s.cuda_stream)), "tpz_bloom_build")
            size = _lib.sst_image_bytes(data, nb, kbytes, flen)
            descs.append(_lib.SstImage(img.data_ptr(), data, first.data_ptr(), cext.data_ptr(), nb,
                                       t, filt.data_ptr() if filt is not None else None, flen))
            keep.append((first, cext, filt))
            tables.append((off, size, data, nb, t, n_ent, kbytes))
            off = (off + size + 255) & ~255
            t, w = t + n_ent, int(h[7])
    nt = len(descs)
    span = tables[-1][0] + tables[-1][1]
    d_desc = torch.from_numpy(np.frombuffer(bytes((_lib.SstImage * nt)(*descs)), np.uint8).copy()
                              ).to(dev)
    info = torch.empty((nt, 4), dtype=torch.int64, device=dev)
    ctx.sst_finish_ptrs(ment, d_desc.data_ptr(), nt, max(x[3] for x in tables), arena.data_ptr(),
                        span, info.data_ptr(), s.cuda_stream)
    got = info.cpu().numpy().view(np.uint64)                              # (waits for the stream)
    for (o, size, data, nb, t, n_ent, kbytes), g in zip(tables, got):
        if int(g[0]) != size:
            raise _lib.TpzError(f"tpz_sst_finish: the image at {o} has {int(g[0])} bytes, not {size}")
        boff = int(g[2])
        out.append(OutputTable(arena[o:o + size], size, int(g[1]),
                               None if boff == 2**64 - 1 else boff, nb, t, n_ent))
    out.sort(key=lambda x: x.first_entry)       # do_compact sorts by smallest_key (level.rs:167)
    out.arena = arena
    out.finish_args = (d_desc, nt, max(x[3] for x in tables), span)
    out._keep = keep        # the plans and filters the descriptors point at
    return out


def _window_bytes(ent: DeviceEntries, start: int, n: int, s) -> int:
    """Key + value bytes of entries [start, start + n): one read-back (codecs 2 / 3 size the
    window's Uncompress scratch with it)."""
    p = torch.stack((ent.kpos[start], ent.kpos[start + n], ent.vpos[start], ent.vpos[start + n]))
    k0, k1, v0, v1 = (int(x) for x in p.cpu())
    return k1 - k0 + v1 - v0


# ------------------------------------------------------------------------- memtable flush
def _run_columns(r):
    """(keys, kpos, vals, vpos) of a run: a levels.DeviceRun or a DeviceEntries."""
    return r.keys, r.kpos, r.vals, r.vpos


def flush_runs(ctx: Context, runs, block_size: int = 4096, codec: int = 1,
               false_positive_rate: float = 0.1, stream: torch.cuda.Stream | None = None):
    """Sorted memtable runs in HBM -> one L0 SST file image (an OutputTable whose `image` is a
    device tensor ready for one D2H copy), or None when the runs hold no entry (sync() builds
    nothing from an empty map, lsm_storage.rs:316-318); otherwise (table, merged): the table and
    the merged DeviceEntries its blocks hold.

    `runs`: levels.DeviceRun (or DeviceEntries) objects in priority order: tpz_merge_runs lets the
    LOWER index win a repeated key. Their columns are concatenated on the device with kpos / vpos
    rebased, merged, and built into one table with no capacity cut: SsTableBuilder in start_flush
    and sync() never tests reach_capacity. An empty key raises EntryError as tpz_plan_blocks
    reports it (BlockBuilder::add asserts, builder.rs:27). Tombstones are kept."""
    if codec not in (1, 2, 3):
        raise ValueError(f"codec {codec}")
    dev = _dev(ctx.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        return _flush_runs(ctx, list(runs), block_size, codec, false_positive_rate, s)


def _flush_runs(ctx: Context, runs, block_size: int, codec: int, false_positive_rate: float, s):
    dev = _dev(ctx.device)
    keys, kpos, vals, vpos, run_first, koff, voff = [], [], [], [], [0], 0, 0
    for r in runs:
        k, kp, v, vp = _run_columns(r)
        n = int(kp.numel()) - 1
        kb, vb = (int(x) for x in torch.stack((kp[n], vp[n])).cpu())
        keys.append(k[:kb])
        vals.append(v[:vb])
        kpos.append(kp[:n] + koff)
        vpos.append(vp[:n] + voff)
        koff, voff = koff + kb, voff + vb
        run_first.append(run_first[-1] + n)
    n = run_first[-1]
    if n == 0:
        return None
    end = torch.tensor([koff, voff], dtype=torch.int64, device=dev)
    pad = torch.zeros(16, dtype=torch.uint8, device=dev)     # (a column is never empty)
    ent = DeviceEntries(torch.cat(keys + [pad]), torch.cat(kpos + [end[:1]]),
                        torch.cat(vals + [pad]), torch.cat(vpos + [end[1:]]), ctx.device)
    merged = merge_runs(ctx, ent, run_first, s)[0]
    first, ext, info = plan_blocks_async(ctx, merged, block_size, s)
    has_bloom = math.copysign(1.0, false_positive_rate) > 0          # is_sign_positive
    n_out = merged.n
    flen = 0
    if has_bloom:
        geo = _lib.bloom_geometry(n_out, false_positive_rate)
        if geo is None:             # fpp 0 (`% limit` divides by zero) or >= 1 (bloom.rs:49)
            raise ReferencePanic(f"no bloom filter for {n_out} keys at fpp {false_positive_rate}")
        flen = geo[0]
    data_bound = encode_bound(merged)
    if codec != 1:
        data_bound = compress_bound(data_bound, n_out)
    arena = torch.empty(data_bound + 6 * n_out + int(merged.keys.numel()) + flen + 12 + 16 + 256,
                        dtype=torch.uint8, device=dev)
    plain = arena if codec == 1 else torch.empty(encode_bound(merged), dtype=torch.uint8, device=dev)
    encode_blocks_async(ctx, merged, first, ext, info, plain, s)
    _, bad, nb = (int(x) for x in info[:3].cpu().numpy().view(np.uint32))   # (waits for the stream)
    if bad != 0xFFFFFFFF:
        raise EntryError(bad, f"entry exceeds block_size {block_size} - 2")
    data = int(ext[nb].cpu())
    cext = ext
    if codec != 1:
        comp, cext = compress_blocks(ctx, plain, ext, nb, data, codec, stream=s)
        data = int(cext[nb].cpu())
        arena[:data].copy_(comp[:data])
    filt = None
    if has_bloom:
        filt = torch.empty((flen + 3) // 4, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().tpz_bloom_build(
            ctx.handle, C.c_void_p(merged.keys.data_ptr()), C.c_void_p(merged.kpos.data_ptr()),
            n_out, false_positive_rate, C.c_void_p(filt.data_ptr()), C.c_void_p(s.cuda_stream)),
            "tpz_bloom_build")
    desc = _lib.SstImage(arena.data_ptr(), data, first.data_ptr(), cext.data_ptr(), nb, 0,
                         filt.data_ptr() if filt is not None else None, flen)
    d_desc = torch.from_numpy(np.frombuffer(bytes(desc), np.uint8).copy()).to(dev)
    out = torch.empty(4, dtype=torch.int64, device=dev)
    ctx.sst_finish_ptrs(merged.struct(), d_desc.data_ptr(), 1, nb, arena.data_ptr(),
                        int(arena.numel()), out.data_ptr(), s.cuda_stream)
    g = out.cpu().numpy().view(np.uint64)                                 # (waits for the stream)
    size, boff = int(g[0]), int(g[2])
    if size == 0 or size > arena.numel():
        raise _lib.TpzError(f"tpz_sst_finish: the image has {size} bytes")
    t = OutputTable(arena[:size], size, int(g[1]), None if boff == 2**64 - 1 else boff, nb, 0,
                    n_out)
    return t, merged


def open_output(ctx: Context, table, verify: bool = False, raw: bool = False):
    """flush_runs' OutputTable as a resident DeviceTable, opened where its image lies
    (table.open_images); the L0 table a flush just wrote goes straight into DeviceLsm."""
    return open_images(ctx, table.image, [(0, table.size)], verify, raw=raw)[0]


def flush_like_start_flush(ctx: Context, view, block_size: int = 4096, codec: int = 1,
                           false_positive_rate: float = 0.1, stream=None):
    """start_flush (src/lsm_storage.rs:83-143): `view` is MemTables::view() as runs (the immutable
    memtables oldest first, the mutable one last); the immutable ones are handed to
    MergeIterator::create oldest first (:91-101), so the OLDEST memtable wins a repeated key. That
    is the reference's behaviour, kept here. Returns flush_runs' (table, merged entries) or None."""
    return flush_runs(ctx, list(view)[:-1], block_size, codec, false_positive_rate, stream)


def flush_like_sync(ctx: Context, view, block_size: int = 4096, codec: int = 1,
                    false_positive_rate: float = 0.1, stream=None):
    """sync() (src/lsm_storage.rs:298-332): use_new_table() first makes every memtable of `view`
    immutable; they are inserted into a BTreeMap oldest first (:306-314), so the NEWEST wins a
    repeated key: the runs go to the merge newest first. An empty map builds nothing (None)."""
    return flush_runs(ctx, list(view)[::-1], block_size, codec, false_positive_rate, stream)


# ------------------------------------------------------------------------- the task's ranges
class TableDesc:
    """What RwsSlice::create reads of an SsTable (src/level/range.rs:45-90): smallest and biggest
    key, the block metas' first keys and offsets, and the meta offset."""

    def __init__(self, smallest_key: bytes, biggest_key: bytes, first_keys, offsets,
                 meta_off: int):
        self.smallest_key, self.biggest_key = bytes(smallest_key), bytes(biggest_key)
        self.first_keys = [bytes(k) for k in first_keys]
        self.offsets = [int(o) for o in offsets]
        self.meta_off = int(meta_off)

    @classmethod
    def of(cls, t) -> "TableDesc":
        """From a table.SsTable (or anything with its fields), or from a resident DeviceTable:
        the block first keys and their positions are read back, the offsets and the meta offset
        are the stored extents, the biggest key is last_key()."""
        if isinstance(t, cls):
            return t
        if isinstance(t, DeviceTable):
            nb = t.n_blocks
            pos = t.first_pos[:nb + 1].cpu().numpy()
            if len(pos) != nb + 1:
                raise ValueError("the DeviceTable was built without its block first keys")
            fk =t.first_keys[:int(pos[-1])].cpu().numpy().tobytes() if nb else b""
            keys = [fk[int(pos[i]):int(pos[i + 1])] for i in range(nb)]
            if not keys:    # init_samllest_biggest_key's block_metas[0]
                raise ReferencePanic("index out of bounds: the len is 0 but the index is 0")
            ext = t.ext_host
            return cls(keys[0], t.last_key(), keys, ext[:nb], int(ext[nb]))
        return cls(t.smallest_key, t.biggest_key, [m.first_key for m in t.block_metas],
                   [m.offset for m in t.block_metas], t.block_meta_offset)

    def find_block_idx(self, key: bytes) -> int:
        """src/table.rs:178-182: partition_point(first_key <= key) - 1, saturating."""
        return max(bisect.bisect_right(self.first_keys, key) - 1, 0)

    def overlap_size(self, lower: bytes, upper: bytes) -> int:
        """SsTable::overlap_size (src/table.rs:127-141): the offset of upper's block minus the
        offset of lower's (the meta offset for a table without blocks)."""
        lo, hi = self.find_block_idx(lower), self.find_block_idx(upper)
        loff = self.offsets[lo] if lo < len(self.offsets) else self.meta_off
        roff = self.offsets[hi] if hi < len(self.offsets) else self.meta_off
        return roff - loff


def sub_ranges(this_tables, next_tables, this_level_id: int, num_sub_compact: int = 4):
    """The key ranges do_compact hands its sub-compactions (src/level.rs:148-152): RwsSlice::create
    + split (src/level/range.rs:14-90) with mean = total_size / num_sub_compact, as a list of
    (lower, (upper, inclusive)) for compact_task; lower is Included. Quirks kept: the overlap test
    is an `||` (:73, :78: true for nearly every table), a total size of 0 gives no ranges (:15-17),
    the biggest keys of this_tables count only for level 0 (:47-56), and the last upper is turned
    Included (:39-41). Tables are TableDescs or table.SsTables; no GPU involved."""
    this_t = [TableDesc.of(t) for t in this_tables]
    next_t = [TableDesc.of(t) for t in next_tables]
    keys = set()
    for t in this_t:
        keys.add(t.smallest_key)
        if this_level_id == 0:
            keys.add(t.biggest_key)
    for t in next_t:
        keys.add(t.smallest_key)
    if next_t:
        keys.add(next_t[-1].biggest_key)
    keys = sorted(keys)
    ranges, total = [], 0
    for lower, upper in zip(keys, keys[1:]):
        size = sum(t.overlap_size(lower, upper) for t in this_t + next_t
                   if t.smallest_key <= upper or t.biggest_key >= lower)
        total += size
        ranges.append((lower, upper, size))
    if total == 0:
        return []
    mean = total // num_sub_compact
    res, acc, first_key = [], 0, b""
    for lower, upper, size in ranges:
        if acc == 0:
            first_key = lower
        acc += size
        if acc >= mean:
            res.append((first_key, (upper, False)))
            acc = 0
    if acc != 0:
        res.append((first_key, (ranges[-1][1], True)))
    else:
        res[-1] = (res[-1][0], (res[-1][1][0], True))
    return res

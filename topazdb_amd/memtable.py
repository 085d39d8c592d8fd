"""Memtable runs built on the device (tpz_mem_build, tpz_wal_index, tpz_wal_entries).

`build_run` turns entries in ARRIVAL order (a write batch, or the records of a WAL) into a
levels.DeviceRun: the sort, the reference's replacement rule and MemTable::size() all happen in
HBM, and only the 64-byte info block comes back. Two rules (src/mem_table.rs):

  MEM_REPLAY  MemTable::open (:119-143): the first empty key ends the replay, the last record of
              a key wins, size adds klen + vlen of every record read.
  MEM_PUT     do_mem_put (:169-196): `versions` holds each entry's WAL append version
              (non-decreasing); the first entry of a key's highest version wins (inside one
              put_entries batch the first duplicate, not the last), and size follows :185-195.

`replay_wal` is MemTable::open over a WAL image: the record chain is walked on the host
(tpz_wal_index: it is serial and has no checksum), the image is uploaded once, split into columns
(tpz_wal_entries) and built (MEM_REPLAY). `wal_encode` restates the bytes Wal::add_entries appends
(src/wal.rs: Entry::encode per entry, src/block/builder.rs:72-81).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import torch

from . import _lib
from ._lib import MEM_PUT, MEM_REPLAY, Context, Entries
from .table import ReferencePanic, _pack

NO_ENTRY = 2**64 - 1


def wal_encode(entries) -> bytes:
    """BE u16 klen | key | BE u16 vlen | value for every entry, back to back."""
    out = []
    for k, v in entries:
        k, v = bytes(k), bytes(v)
        if len(k) > 0xFFFF or len(v) > 0xFFFF:
            raise ValueError("a WAL record holds at most 65,535 bytes of key and of value")
        out += [struct.pack(">H", len(k)), k, struct.pack(">H", len(v)), v]
    return b"".join(out)


def wal_index(image: bytes, count_only: bool = False):
    """tpz_wal_index: (record starts as a numpy uint64 array of n + 1, or None with count_only;
    info as 4 python ints: n, how the walk ended (_lib.WAL_*), the end of the last record read, the
    failing record's offset). Raises ReferencePanic where WalIterator::next panics."""
    image = bytes(image)
    buf = (C.c_uint8 * max(len(image), 1)).from_buffer_copy(image or b"\0")
    info = (C.c_uint64 * 4)()
    L = _lib.lib()
    rc = L.tpz_wal_index(buf, len(image), None, 0, info)
    if rc == _lib.ERR_SIZES:
        raise ReferencePanic(f"WAL record at byte {info[3]} of {len(image)} runs past the image "
                             "(WalIterator::next: get_u16 / slice out of range)")
    _lib.check(rc, "tpz_wal_index")
    if count_only:
        return None, [int(x) for x in info]
    rec = np.zeros(int(info[0]) + 1, np.uint64)
    _lib.check(L.tpz_wal_index(buf, len(image), C.c_void_p(rec.ctypes.data), rec.size, info),
               "tpz_wal_index")
    return rec, [int(x) for x in info]


def _columns(dev, entries) -> dict:
    if isinstance(entries, dict):
        return {k: entries[k] for k in ("keys", "kpos", "vals", "vpos")}
    entries = [(bytes(k), bytes(v)) for k, v in entries]
    cols = {}
    for name, pname, side in (("keys", "kpos", [k for k, _ in entries]),
                              ("vals", "vpos", [v for _, v in entries])):
        buf, pos = _pack(side)
        cols[name] = torch.from_numpy(buf.copy()).to(dev)
        cols[pname] = torch.from_numpy(pos).to(dev)
    return cols


def build_run(ctx: Context, entries, versions=None, mode: int | None = None, prefix: bool = True,
              key_bytes: int | None = None, val_bytes: int | None = None):
    """tpz_mem_build on the current stream. `entries`: a (key, value) list in arrival order, or a
    dict of device columns keys, kpos, vals, vpos (uint8 / int64 tensors, kpos and vpos of n + 1;
    key_bytes / val_bytes default to the last positions, read back). `versions`: one int for all
    entries, a sequence, or an int64 / uint64 device tensor; giving it selects MEM_PUT unless
    `mode` says otherwise. Returns a levels.DeviceRun over the output columns with
      .size             MemTable::size() (a python int, wrapped as usize)
      .n_consumed       entries read (REPLAY stops at the first empty key)
      .first_empty_key  the first input entry with an empty key, or None
      .src_entry        int32 device tensor: the input entry each run entry is
      .versions         int64 device tensor: the winners' versions (0 under REPLAY)."""
    from .levels import DeviceRun
    dev = torch.device("cuda", ctx.device)
    if mode is None:
        mode = MEM_REPLAY if versions is None else MEM_PUT
    cols = _columns(dev, entries)
    n = int(cols["kpos"].numel()) - 1
    if n < 0 or int(cols["vpos"].numel()) - 1 != n:
        raise ValueError("kpos and vpos hold n + 1 positions each")
    kb = int(cols["kpos"][-1].item()) if key_bytes is None else int(key_bytes)
    vb = int(cols["vpos"][-1].item()) if val_bytes is None else int(val_bytes)
    ver = None
    if versions is not None:
        if isinstance(versions, torch.Tensor):
            ver = versions.to(dev).contiguous()
            if ver.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
                ver = ver.to(torch.int64)
        elif np.isscalar(versions):
            ver = torch.from_numpy(np.full(max(n, 1), int(versions), np.uint64).view(np.int64)).to(dev)
        else:
            ver = torch.from_numpy(np.asarray(list(versions) or [0], np.uint64).view(np.int64)).to(dev)
        if n and int(ver.numel()) < n:
            raise ValueError(f"{ver.numel()} versions for {n} entries")
    if mode == MEM_PUT and ver is None:
        raise ValueError("MEM_PUT needs versions")
    out = {"keys": torch.empty(max(kb, 16), dtype=torch.uint8, device=dev),
           "vals": torch.empty(max(vb, 16), dtype=torch.uint8, device=dev),
           "kpos": torch.empty(n + 1, dtype=torch.int64, device=dev),
           "vpos": torch.empty(n + 1, dtype=torch.int64, device=dev)}
    pre = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    src = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    over = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    ent = Entries(cols["keys"].data_ptr(), cols["kpos"].data_ptr(), cols["vals"].data_ptr(),
                  cols["vpos"].data_ptr(), n, kb, vb)
    ctx.mem_build_ptrs(ent, mode, None if ver is None else ver.data_ptr(), out["keys"].data_ptr(),
                       out["kpos"].data_ptr(), out["vals"].data_ptr(), out["vpos"].data_ptr(),
                       pre.data_ptr(), src.data_ptr(), over.data_ptr(), info.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
    h = [int(x) for x in info.cpu().numpy().view(np.uint64)]     # the one read-back
    n_out = h[0]
    run = DeviceRun.__new__(DeviceRun)
    run.ctx, run.dev, run.n = ctx, dev, n_out
    run.keys, run.vals = out["keys"], out["vals"]
    run.kpos, run.vpos = out["kpos"][:n_out + 1], out["vpos"][:n_out + 1]
    run.key_bytes, run.val_bytes = h[1], h[2]
    run.prefix = pre if prefix else None
    run.size, run.n_consumed = h[4], h[5]
    run.first_empty_key = None if h[3] == NO_ENTRY else h[3]
    run.src_entry, run.versions = src[:n_out], over[:n_out]
    run.info = h
    run._inputs = (cols, ver)      # alive until the stream has run the build
    return run


def replay_wal(ctx: Context, image: bytes, prefix: bool = True):
    """MemTable::open (src/mem_table.rs:119-143) over a WAL image: a levels.DeviceRun as build_run
    returns it (.size is MemTable::size()). Raises ReferencePanic for a truncated image."""
    image = bytes(image)
    rec, winfo = wal_index(image)
    n = winfo[0]
    dev = torch.device("cuda", ctx.device)
    cap = max(len(image), 16)
    img = torch.from_numpy(np.frombuffer(image or b"\0", np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(rec.view(np.int64)).to(dev)
    cols = {"keys": torch.empty(cap, dtype=torch.uint8, device=dev),
            "vals": torch.empty(cap, dtype=torch.uint8, device=dev),
            "kpos": torch.empty(n + 1, dtype=torch.int64, device=dev),
            "vpos": torch.empty(n + 1, dtype=torch.int64, device=dev)}
    info = torch.empty(4, dtype=torch.int64, device=dev)
    ctx.wal_entries_ptrs(img.data_ptr(), len(image), d_rec.data_ptr(), n, cols["keys"].data_ptr(),
                         cols["kpos"].data_ptr(), cols["vals"].data_ptr(), cols["vpos"].data_ptr(),
                         info.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    h = [int(x) for x in info.cpu().numpy().view(np.uint64)]
    if h[3] != NO_ENTRY:          # (the index and the image disagree: not a state the host walk leaves)
        raise ReferencePanic(f"WAL record {h[3]} does not end where the next one starts")
    run = build_run(ctx, cols, mode=MEM_REPLAY, prefix=prefix, key_bytes=h[1], val_bytes=h[2])
    run.wal_info = winfo
    return run

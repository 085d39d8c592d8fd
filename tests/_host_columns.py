"""tpz_decode_blocks_host (include/tpz_gpu.h, the host pipeline) against the oracle: helpers of
tests/test_gpu_host_columns.py (not a conftest; imported by name).

decode_host() calls the entry point with every output buffer at a stated capacity, followed by a
guard region of a fixed byte pattern, and asserts after every call (TPZ_ERR_NOMEM included) that
no guard byte changed: the guards are host memory the test owns, so a write past a capacity is
caught here and not suffered. The default capacities are the exact needs, taken from the oracle
(never from the code under test): tpz_data_capacity of the decoded bytes, two u32 per entry of
every decoded block, and the spill bytes a first probing call reports. That probing call runs on
a context of its own, once per batch (Reference.spill_need): the context under test sees only the
calls whose outputs are compared with the oracle, so the state one call leaves in the context's
pooled buffers meets the next checked call and not a probe.

host_dense() reads the host columns as the header documents them (slots at
tpz_slot_base(h_dext[i], i), dense ends at h_ends[2 * h_first[i] ..], spill records at
h_spill + h_spill_off[i]) into the same dense form the oracle returns; assert_host_parity()
compares the two byte for byte.
"""
from __future__ import annotations

import numpy as np
import torch

import _oracle as O
from topazdb_amd import _lib
from topazdb_amd.batch import DenseDecode, _gather

GUARD = 4096
PATTERN = 0xA5


class Reference:
    """The oracle's answer for one batch, computed once and shared by the calls that check it:
    the dense decode, and the decoded extents (each block's Uncompress form length; a block whose
    codec step fails leaves a 1-byte stub; a batch without snappy / lz4 blocks keeps h_ext)."""

    def __init__(self, src, ext):
        self.src = np.ascontiguousarray(src, np.uint8)
        self.ext = np.ascontiguousarray(ext, np.uint64)
        e = self.ext.astype(np.int64)
        self.n = n = len(e) - 1
        self.o = O.decode_batch(self.src, self.ext)
        self.codec = any(e[i + 1] > e[i] and self.src[e[i + 1] - 1] in (2, 3) for i in range(n))
        if self.codec:
            lens = []
            for i in range(n):
                st, p = O.decompress_block(self.src[e[i]:e[i + 1]].tobytes())
                lens.append(len(p) if st == O.OK else 1)
            self.dext = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        else:
            self.dext = e.copy()
        decoded = np.isin(self.o.status, [O.OK, O.BAD_ENTRY])
        self.n_ok = np.where(decoded, self.o.count, 0).astype(np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.n_ok)]).astype(np.int64)
        self.data_need = _lib.data_capacity(int(self.dext[n]), n)
        self.ends_need = 2 * int(self.first[n])
        self._spill_need = None

    @property
    def spill_need(self) -> int:
        """The exact spill bytes of the batch (the same for every chunk size): *h_spill_used of a
        probing call without spill room, made once on a context that is used for nothing else."""
        if self._spill_need is None:
            ctx = _lib.Context(0)
            try:
                self._spill_need = probe_spill(ctx, self, 0).spill_used
            finally:
                ctx.close()
        return self._spill_need


class _Guarded:
    """`nbytes` of output followed by `guard` pattern bytes (the whole allocation starts out as
    the pattern, so an output the call never wrote shows too)."""

    def __init__(self, nbytes: int, pinned: bool, guard: int):
        self.nbytes = int(nbytes)
        total = self.nbytes + guard
        if pinned:
            self._t = torch.empty(total, dtype=torch.uint8).pin_memory()
            self.raw = self._t.numpy()
        else:
            self.raw = np.empty(total, np.uint8)
        self.raw[:] = PATTERN
        self.ptr = self.raw.ctypes.data

    def view(self, dtype):
        return self.raw[:self.nbytes].view(dtype)

    def intact(self) -> bool:
        return bool((self.raw[self.nbytes:] == PATTERN).all())


class HostOutputs:
    FIELDS = ("data", "ends", "first", "count", "status", "crc", "spill", "spill_off",
              "spill_used", "dext")

    def __init__(self, n, data_bytes, ends_cap, spill_cap, pinned, guard):
        self.n = n
        self.buf = {
            "data": _Guarded(data_bytes, pinned, guard),
            "ends": _Guarded(4 * ends_cap, pinned, guard),
            "first": _Guarded(8 * (n + 1), pinned, guard),
            "count": _Guarded(4 * n, pinned, guard),
            "status": _Guarded(n, pinned, guard),
            "crc": _Guarded(4 * n, pinned, guard),
            "spill": _Guarded(spill_cap, pinned, guard),
            "spill_off": _Guarded(8 * n, pinned, guard),
            "spill_used": _Guarded(8, pinned, guard),
            "dext": _Guarded(8 * (n + 1), pinned, guard),
        }
        self.data = self.buf["data"].view(np.uint8)
        self.ends = self.buf["ends"].view(np.uint32)
        self.first = self.buf["first"].view(np.uint64)
        self.count = self.buf["count"].view(np.uint32)
        self.status = self.buf["status"].view(np.uint8)
        self.crc = self.buf["crc"].view(np.uint32)
        self.spill = self.buf["spill"].view(np.uint8)
        self.spill_off = self.buf["spill_off"].view(np.uint64)
        self.dext = self.buf["dext"].view(np.uint64)
        self.ends_cap, self.spill_cap = int(ends_cap), int(spill_cap)
        self.rc = None

    @property
    def spill_used(self) -> int:
        return int(self.buf["spill_used"].view(np.uint64)[0])

    def assert_guards(self):
        for name in self.FIELDS:
            assert self.buf[name].intact(), f"write past the capacity of h_{name}"

    # the sizes the header says a caller reads after TPZ_ERR_NOMEM (and after a success)
    def needs(self):
        return (2 * int(self.first[self.n]), self.spill_used,
                _lib.data_capacity(int(self.dext[self.n]), self.n))


def _call(ctx, ref: Reference, chunk_blocks, data_cap, ends_cap, spill_cap, pinned, guard):
    n = ref.n
    # data_cap = 0 asks for the header's default, tpz_data_capacity(h_ext[n], n): h_data holds that
    data_bytes = data_cap if data_cap else _lib.data_capacity(int(ref.ext[n]), n)
    out = HostOutputs(n, data_bytes, ends_cap, spill_cap, pinned, guard)
    b = out.buf
    cols = _lib.HostColumns(b["data"].ptr, b["ends"].ptr, ends_cap, b["first"].ptr,
                            b["count"].ptr, b["status"].ptr, b["crc"].ptr, b["spill"].ptr,
                            spill_cap, b["spill_off"].ptr, b["spill_used"].ptr, b["dext"].ptr,
                            data_cap)
    src = ref.src
    if pinned and src.size:
        out._src = torch.from_numpy(src.copy()).pin_memory()
        src = out._src.numpy()
    src_ptr = src.ctypes.data if src.size else None
    out.rc = ctx.decode_host_ptrs(src_ptr, ref.ext.ctypes.data, n, cols, chunk_blocks)
    out.assert_guards()
    return out


def probe_spill(ctx, ref: Reference, chunk_blocks) -> HostOutputs:
    """A call with no spill room: *h_spill_used is the exact need, h_spill_off the place of every
    spill-resident block's record. (Its data buffer is sized by tpz_host_decoded_bound, as the
    header tells a caller to, so that the probe itself is short of spill room only.)"""
    bound = _lib.host_decoded_bound(ref.src.ctypes.data, ref.ext.ctypes.data, ref.n)
    data_cap = max(ref.data_need, _lib.data_capacity(bound, ref.n))
    out = _call(ctx, ref, chunk_blocks, data_cap, ref.ends_need, 0, False, GUARD)
    assert out.rc == (_lib.ERR_NOMEM if out.spill_used else _lib.SUCCESS)
    return out


def decode_host(ctx, src, ext, chunk_blocks, *, data_cap=None, ends_cap=None, spill_cap=None,
                pinned=False, guard=GUARD, ref: Reference | None = None) -> HostOutputs:
    """One tpz_decode_blocks_host call over guarded outputs; out.rc is the tpz_err. Capacities
    left None are the exact needs (see the module docstring)."""
    ref = ref or Reference(src, ext)
    if data_cap is None:
        data_cap = ref.data_need
    if ends_cap is None:
        ends_cap = ref.ends_need
    if spill_cap is None:
        spill_cap = ref.spill_need
    return _call(ctx, ref, chunk_blocks, data_cap, ends_cap, spill_cap, pinned, guard)


def host_dense(out: HostOutputs, n: int) -> DenseDecode:
    """The host columns gathered into dense arrays in block order (batch.SlottedColumns.dense
    for this layout: the ends are the dense h_ends, located by h_first)."""
    status, crc, count = out.status[:n].copy(), out.crc[:n].copy(), out.count[:n].copy()
    dext = out.dext[:n].astype(np.int64)
    first = out.first[:n + 1].astype(np.int64)
    bid = np.arange(n, dtype=np.int64)
    spilled = (status == _lib.BLOCK_OK_SPILLED) | (status == _lib.BLOCK_BAD_ENTRY)
    okm = (status == _lib.BLOCK_OK) | spilled
    n_ok = np.where(okm, count, 0).astype(np.int64)
    ebase = np.zeros(n + 1, np.int64)
    np.cumsum(n_ok, out=ebase[1:])
    total = int(ebase[-1])
    eblk = np.repeat(bid, n_ok)
    j = np.arange(total, dtype=np.int64) - ebase[eblk]
    kend_d, vend_d = out.ends[0::2], out.ends[1::2]
    pair = first[eblk] + j
    cls = np.zeros(total, np.uint8)
    ke, ve, ks, vs, base, vbase = (np.zeros(total, np.int64) for _ in range(6))
    slotm = ~spilled[eblk]
    if slotm.any():
        p = pair[slotm]
        head = j[slotm] == 0
        ke[slotm] = kend_d[p]
        ve[slotm] = vend_d[p]
        ks[slotm] = np.where(head, 0, kend_d[np.maximum(p - 1, 0)])
        vs[slotm] = np.where(head, 0, vend_d[np.maximum(p - 1, 0)])
        b_ok = okm & ~spilled & (n_ok > 0)
        ktot = np.zeros(n, np.int64)
        ktot[b_ok] = kend_d[(first[:n] + n_ok - 1)[b_ok]]
        sbase = _lib.slot_base(dext, bid)
        base[slotm] = sbase[eblk[slotm]]
        vbase[slotm] = (sbase + _lib.value_start(ktot))[eblk[slotm]]
    buf = out.data
    if spilled.any():
        sp = out.spill
        buf = np.concatenate([out.data, sp])
        for b in np.nonzero(spilled)[0]:
            m = int(count[b])
            if m == 0:
                continue
            r = int(out.spill_off[b])
            e2 = sp[r:r + 8 * m].view(np.uint32).astype(np.int64)
            kk, vv = e2[0::2], e2[1::2]
            sl = slice(int(ebase[b]), int(ebase[b + 1]))
            ke[sl], ve[sl] = kk, vv
            ks[sl] = np.concatenate([[0], kk[:-1]])
            vs[sl] = np.concatenate([[0], vv[:-1]])
            st0 = len(out.data) + r + _lib.spill_stream(m)
            base[sl] = st0
            vbase[sl] = st0 + _lib.value_start(int(kk[-1]))
            if status[b] == _lib.BLOCK_BAD_ENTRY:
                c0 = r + _lib.spill_classes(m, int(kk[-1]), int(vv[-1]))
                cls[sl] = sp[c0:c0 + m]
    klen, vlen = ke - ks, ve - vs
    keys = _gather(buf, base + ks, klen)
    vals = _gather(buf, vbase + vs, vlen)
    ref_status = np.where(status == _lib.BLOCK_OK_SPILLED, _lib.BLOCK_OK, status).astype(np.uint8)
    d = DenseDecode(ref_status, crc, n_ok.astype(np.uint32), count, klen.astype(np.uint32),
                    vlen.astype(np.uint32), keys, vals)
    d.raw_status = status
    d.cls = cls
    return d


def check_outputs(out: HostOutputs, ref: Reference) -> DenseDecode:
    """Every output of a successful call against the oracle, byte for byte."""
    n, o = ref.n, ref.o
    # (first the extents, which a call reports whole even when it returns TPZ_ERR_NOMEM: a layout
    #  that differs from the oracle's shows here and not as a buffer that was "too small")
    np.testing.assert_array_equal(np.diff(out.dext.astype(np.int64)), np.diff(ref.dext),
                                  err_msg="decoded block lengths (h_dext)")
    np.testing.assert_array_equal(out.dext.astype(np.int64), ref.dext)
    if not ref.codec:
        np.testing.assert_array_equal(out.dext, ref.ext)
    assert out.rc == _lib.SUCCESS, (out.rc, out.needs(), out.ends_cap, out.spill_cap,
                                    out.buf["data"].nbytes)
    status = np.where(out.status == _lib.BLOCK_OK_SPILLED, _lib.BLOCK_OK, out.status)
    np.testing.assert_array_equal(status, o.status)
    okm = np.isin(o.status, [O.OK, O.BAD_ENTRY])
    np.testing.assert_array_equal(np.where(okm, out.count, 0), o.count)
    assert (out.count[o.status == O.CODEC] == 0).all()
    np.testing.assert_array_equal(out.first.astype(np.int64), ref.first)
    has_crc = np.isin(o.status, [O.OK, O.CHECKSUM, O.MALFORMED, O.BAD_ENTRY])
    has_crc &= ~((o.status == O.MALFORMED) & (o.crc_actual == 0) & (o.crc_expected == 0))
    np.testing.assert_array_equal(out.crc[has_crc], o.crc_actual[has_crc])
    g = host_dense(out, n)
    np.testing.assert_array_equal(g.klen, o.klen)
    np.testing.assert_array_equal(g.vlen, o.vlen)
    assert g.keys.tobytes() == o.keys.tobytes()
    assert g.vals.tobytes() == o.vals.tobytes()
    np.testing.assert_array_equal(g.cls, o.cls)
    # a spill-resident block's pairs in h_ends are its record's (tpz_pack_ends takes them there)
    resident = (out.status == _lib.BLOCK_OK_SPILLED) | (out.status == _lib.BLOCK_BAD_ENTRY)
    for b in np.nonzero(resident)[0]:
        m, r, f = int(out.count[b]), int(out.spill_off[b]), int(ref.first[b])
        assert r + 8 * m <= out.spill_used
        np.testing.assert_array_equal(out.ends[2 * f:2 * (f + m)], out.spill[r:r + 8 * m].view(np.uint32))
    return g


def assert_host_parity(ctx, src, ext, chunk_blocks, **kw):
    """decode_host + host_dense against O.decode_batch(src, ext); returns (outputs, dense)."""
    ref = kw.pop("ref", None) or Reference(src, ext)
    out = decode_host(ctx, src, ext, chunk_blocks, ref=ref, **kw)
    return out, check_outputs(out, ref)

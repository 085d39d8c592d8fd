"""Every device entry point at byte positions past 2^31 and 2^32.

Every position of the C ABI is a u64 (tpz_batch.d_ext, tpz_entries.d_kpos / d_vpos, the d_key_pos
columns, d_span, the codec step's d_dst_ext), and include/tpz_gpu.h promises objects of many GiB;
the rest of the suite only ever hands the kernels positions of a few MiB. Here every workload (a
few MiB of real bytes) runs three ways inside tests/_bigspan.py's sparse buffers: at base 0 (the
control), at a base where one of its items straddles 2^31, and at one where it straddles 2^32. A
kernel that truncates a position to 32 bits or sign-extends it from 32 bits reads the canary or
writes where `untouched` finds it: wrong bytes and a failing assertion, no fault.

Each run is compared with the CPU oracle or model the matching test file already uses (they are
position-independent); the straddling results must also equal the control's, which only localises
a failure. Every case asserts its own straddle (an item below the line, one containing it, one
above) and `untouched()` on every span it passed.
"""
import copy
import ctypes as C
import functools
import random
import struct
import zlib

import numpy as np
import pytest
import torch

import _get_model as G
import _lsm_model as LM
import _membuild_model as MB
import _open_model as OM
import _oracle as O
import _scan_model as SM
import _tables_model as TM
import badentry_util as U
import xxhash
from _merge_model import merge_rule
from conftest import read_golden
from _bigspan import LINES, SPAN, BigSpan, assert_straddle, base_at_boundary, base_for, need_room
from test_gpu_compress import check_round_trip
from test_gpu_decode import MG, _random_blocks
from test_gpu_regular import near_regular, regular_block
from test_gpu_spill import repeated_offset_blocks
from topazdb_amd import _lib, compact, synth
from topazdb_amd.batch import (DeviceBatch, FlatColumns, SlottedColumns, crc32_ranges, decode_batch,
                               decode_flat, entry_first, open_index, open_metas, pack_ends,
                               verify_files)
from topazdb_amd.compact import entries_from_flat, merge_runs
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun, _bound
from topazdb_amd.table import DeviceTable, _pack
from topazdb_amd.encode import (DeviceEntries, bloom_build, compress_blocks, encode_blocks,
                                encode_blocks_async, plan_blocks, plan_blocks_async)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT = 0x5A5A5A5A
LINE_IDS = {LINES[0]: "2^31", LINES[1]: "2^32"}
# slot_base and entry_base of a batch rebased by a multiple of lcm(128, 96) are the base-0 ones
# shifted by constants, so the slotted layout at base B reads like the one at base 0
SLOT_ALIGN = 384


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def spans():
    """Three BigSpans (inputs and outputs), about 19 GiB in all, freed at module end."""
    need_room(3, extra=24 << 30)
    s = [BigSpan(DEV) for _ in range(3)]
    yield s
    for x in s:
        x.free()
    torch.cuda.empty_cache()


# ============================================================================ batches
def _builder_block(rng, n, klen, vlen) -> bytes:
    bb = MG.BlockBuilder(1 << 20)
    for i in range(n):
        assert bb.add(b"%06d" % i + rng.bytes(klen - 6), rng.bytes(vlen))
    return MG.encode_block(*bb.build())


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(labels, blocks): one batch of every kind of block the decode routes differently, 2-3 MiB.
    Two wave-path blocks (`edge31`, `edge32`) sit behind filler blocks sized so that their start
    is congruent to 2^31 / 2^32 modulo SLOT_ALIGN: the base that puts them exactly on the line is
    then a multiple of it."""
    rng = np.random.default_rng(2031)
    out = []

    def add(label, blk):
        out.append((label, bytes(blk)))

    def add_region(label, src, ext):
        for i in range(len(ext) - 1):
            add(label, np.asarray(src[int(ext[i]):int(ext[i + 1])], np.uint8).tobytes())

    def total():
        return sum(len(b) for _, b in out)

    def add_edge(label, line):
        need = (line - total()) % SLOT_ALIGN or SLOT_ALIGN
        add("filler", rng.bytes(need - 1) + b"\x07")       # a bad tag, whatever the bytes
        assert (line - total()) % SLOT_ALIGN == 0
        add(label, _builder_block(rng, 20, 16, 60))

    add_region("4k", *synth.make_region("4k", 120))
    for _ in range(6):                      # the line falls on a cache hit of this run ...
        add("reg_a", regular_block(rng, 34, 16, 100)[0])
    for _ in range(5):                      # ... and a geometry switch follows it
        add("reg_b", regular_block(rng, 33, 16, 100)[0])
    add_region("zipf", *synth.make_region("zipf", 150))
    add_edge("edge31", LINES[0])
    add_region("rand", *_random_blocks(rng, 120))
    for _ in range(2):                      # longer than the wave slot, n < 64
        add("big_lt64", _builder_block(rng, 20, 20, 900))
    add_region("4k", *synth.make_region("4k", 8, seed=5))
    for _ in range(2):                      # longer than the wave slot, n >= 64: the big path
        add("big_ge64", _builder_block(rng, 300, 12, 30))
    add_region("64k", *synth.make_region("64k", 3))
    for blk in repeated_offset_blocks():
        add("spill", blk)
    add_region("4k", *synth.make_region("4k", 8, seed=6))
    for _name, blk in near_regular(rng)[::4]:
        add("near", blk)
    flipped = bytearray(_builder_block(rng, 30, 16, 100))
    flipped[100] ^= 0x04
    add("crcflip", flipped)
    ents = [(U.key(i), b"value_%04d" % i) for i in range(20)]
    add("bad", U.bad_block(ents, 7, "value"))
    add("empty", b"")
    add_edge("edge32", LINES[1])
    add_region("4k", *synth.make_region("4k", 120, seed=7))
    labels = [l for l, _ in out]
    blocks = [b for _, b in out]
    assert (2 << 20) <= total() <= (3 << 20), total()
    return labels, blocks


def index_of(labels, label, k=0) -> int:
    return [i for i, l in enumerate(labels) if l == label][k]


# which block contains the line: one representative per kind the decode routes differently
BATCH_KINDS = {
    "wave": lambda lab, line: index_of(lab, "zipf", 70),
    "regular": lambda lab, line: index_of(lab, "reg_a", 2),        # the third of its run
    "bigwave": lambda lab, line: index_of(lab, "64k", 1),
    "big": lambda lab, line: index_of(lab, "big_ge64", 0),
    "spill": lambda lab, line: index_of(lab, "spill", 1),          # 300 entries at one offset
    "edge": lambda lab, line: index_of(lab, "edge31" if line == LINES[0] else "edge32"),
}
BATCH_CASES = [(line, kind) for line in LINES for kind in BATCH_KINDS]
BATCH_IDS = [f"{LINE_IDS[line]}-{kind}" for line, kind in BATCH_CASES]


def batch_base(line, kind, labels, lens, align=SLOT_ALIGN) -> int:
    j = BATCH_KINDS[kind](labels, line)
    if kind == "edge":
        b = base_at_boundary(line, lens, j)
    else:
        b = base_for(line, lens, j, align=align)
    assert b % align == 0
    return b


class Placed:
    """A batch placed at `base` of a span: the DeviceBatch over the span's view with rebased
    extents, wiped again on exit."""

    def __init__(self, span: BigSpan, blocks, base: int):
        self.span, self.base = span, base
        self.src = np.frombuffer(b"".join(blocks), np.uint8)
        self.ext0 = np.zeros(len(blocks) + 1, np.uint64)
        np.cumsum([len(b) for b in blocks], out=self.ext0[1:])
        self.total = int(self.ext0[-1])
        self.window = (base, base + self.total)

    def __enter__(self):
        self.span.place(self.src, self.base)
        self.ext = self.ext0 + np.uint64(self.base)
        self.batch = DeviceBatch(self.span.view, self.ext)
        assert self.batch.src_bytes == self.base + self.total
        return self

    def __exit__(self, *exc):
        self.span.wipe([self.window])
        return False


def span_columns(out: BigSpan, batch: DeviceBatch, first=None) -> SlottedColumns:
    """tpz_columns whose data is an output BigSpan (slot bases follow the extents), sized with
    tpz_data_capacity from the real src_bytes; the ends hold a sentinel."""
    nb = batch.n_blocks
    c = SlottedColumns.__new__(SlottedColumns)
    cap = _lib.data_capacity(batch.src_bytes, nb)
    assert cap <= SPAN
    c.device, c.n_blocks, c.entry_first, c._decoded = 0, nb, first, None
    c.data = out.view[:cap]
    n_pairs = _lib.entry_capacity(batch.src_bytes, nb) if first is None else \
        max(int(first[nb].cpu()), 1)
    c.ends = torch.full((2 * n_pairs,), SENT, dtype=torch.int32, device=DEV)
    c.count = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
    c.status = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
    c.crc = torch.zeros(nb, dtype=torch.int32, device=DEV)
    c.spill_off = torch.zeros(nb, dtype=torch.int64, device=DEV)
    c.spill_used = torch.zeros(1, dtype=torch.int64, device=DEV)
    c.set_spill_cap(16 << 20)
    return c


def dense_at(cols: SlottedColumns, base: int, ext0: np.ndarray):
    """cols.dense() of a batch rebased by `base` (a multiple of SLOT_ALIGN), reading only the
    bytes from the base on."""
    assert base % SLOT_ALIGN == 0
    cols.complete()
    assert int(cols.spill_used.cpu()) <= cols.spill_cap
    v = copy.copy(cols)
    v._decoded = None
    v.data = cols.data[base:]
    if cols.entry_first is None:
        v.ends = cols.ends[2 * 16 * (base // 96):]
    return v.dense(ext0)


def slot_windows(ext: np.ndarray) -> list:
    """The lines each block's slot owns: at most len + 129 bytes from its slot base, in whole
    128-byte lines (include/tpz_gpu.h)."""
    w = []
    for i in range(len(ext) - 1):
        s = int(_lib.slot_base(int(ext[i]), i))
        ln = int(ext[i + 1]) - int(ext[i])
        w.append((s, s + (ln + 129 + 127) // 128 * 128))
    return w


def assert_decoded(g, o):
    np.testing.assert_array_equal(g.status, o.status)
    has_crc = np.isin(o.status, [O.OK, O.CHECKSUM, O.MALFORMED, O.BAD_ENTRY])
    has_crc &= ~((o.status == O.MALFORMED) & (o.crc_actual == 0) & (o.crc_expected == 0))
    np.testing.assert_array_equal(g.crc_actual[has_crc], o.crc_actual[has_crc])
    np.testing.assert_array_equal(g.count, o.count)
    np.testing.assert_array_equal(g.klen, o.klen)
    np.testing.assert_array_equal(g.vlen, o.vlen)
    assert g.keys.tobytes() == o.keys.tobytes()
    assert g.vals.tobytes() == o.vals.tobytes()
    np.testing.assert_array_equal(g.cls, o.cls)


def assert_same_decode(g, c):
    """A straddling run against the control, raw statuses included."""
    np.testing.assert_array_equal(g.raw_status, c.raw_status)
    np.testing.assert_array_equal(g.crc_actual, c.crc_actual)
    np.testing.assert_array_equal(g.raw_count, c.raw_count)
    assert g.keys.tobytes() == c.keys.tobytes() and g.vals.tobytes() == c.vals.tobytes()


def want_packed(o):
    """tpz_pack_ends' dense {kend, vend} pairs from the oracle's entry lengths."""
    n = len(o.klen)
    w = np.zeros((n, 2), np.int64)
    for b in range(len(o.count)):
        e0, e1 = int(o.entry_base[b]), int(o.entry_base[b + 1])
        w[e0:e1, 0] = np.cumsum(o.klen[e0:e1])
        w[e0:e1, 1] = np.cumsum(o.vlen[e0:e1])
    return w.reshape(-1)


@functools.lru_cache(maxsize=None)
def batch_oracle():
    labels, blocks = mixed_batch()
    src = np.frombuffer(b"".join(blocks), np.uint8)
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    o = O.decode_batch(src, ext)
    for st in (O.OK, O.CHECKSUM, O.BAD_ENTRY, O.EMPTY, O.BAD_TAG):
        assert (o.status == st).any(), st
    return o


def run_decode(ctx, inp: BigSpan, out: BigSpan, base: int):
    """Slotted decode, exact-ends decode and tpz_pack_ends of the mixed batch at `base`; every
    result against the oracle. Returns (slotted dense, exact dense, packed ends)."""
    _, blocks = mixed_batch()
    o = batch_oracle()
    with Placed(inp, blocks, base) as p:
        wins = slot_windows(p.ext)
        owned = [(wins[0][0], wins[-1][1])]
        res = []
        try:
            for exact in (False, True):
                first = entry_first(ctx, p.batch) if exact else None
                cols = span_columns(out, p.batch, first)
                decode_batch(ctx, p.batch, cols)
                g = dense_at(cols, base, p.ext0)
                assert_decoded(g, o)
                assert out.untouched(wins), "a store outside the slots' lines"
                if not exact:
                    spilled = g.raw_status == _lib.BLOCK_OK_SPILLED
                    assert spilled.any() and (g.raw_status == _lib.BLOCK_OK).sum() > 400
                    f, d = pack_ends(ctx, p.batch, cols)
                    torch.cuda.synchronize()
                    n = int(o.count.sum())
                    np.testing.assert_array_equal(f.cpu().numpy(), o.entry_base)
                    packed = d[:2 * n].cpu().numpy().view(np.uint32).astype(np.int64)
                    np.testing.assert_array_equal(packed, want_packed(o))
                    del f, d
                res.append(g)
                out.wipe(owned)
                del cols
            assert inp.untouched([p.window]), "the input span was written"
        finally:
            out.wipe(owned)
    return res[0], res[1], packed


@pytest.fixture(scope="module")
def decode_control(ctx, spans):
    return run_decode(ctx, spans[0], spans[1], 0)


def test_decode_control(decode_control):
    """Base 0 of the same spans (run_decode compares it with the oracle)."""
    gs, ge, _ = decode_control
    assert_same_decode(ge, gs)


@pytest.mark.parametrize("line,kind", BATCH_CASES, ids=BATCH_IDS)
def test_decode_blocks(ctx, spans, decode_control, line, kind):
    """tpz_decode_blocks (slotted and exact ends, tpz_entry_first) and tpz_pack_ends."""
    labels, blocks = mixed_batch()
    base = batch_base(line, kind, labels, [len(b) for b in blocks])
    gs, ge, packed = run_decode(ctx, spans[0], spans[1], base)
    assert_same_decode(gs, decode_control[0])
    assert_same_decode(ge, decode_control[1])
    np.testing.assert_array_equal(packed, decode_control[2])


# ---------------------------------------------------------------------------- flat
def run_flat(ctx, inp: BigSpan, base: int):
    """tpz_flat_layout + tpz_decode_blocks_flat and tpz_flat_entry_pos over the result."""
    _, blocks = mixed_batch()
    o = batch_oracle()
    with Placed(inp, blocks, base) as p:
        cols = decode_flat(ctx, p.batch, FlatColumns(ctx, p.batch, spill_cap=1 << 20)).complete()
        g = cols.dense()
        assert_decoded(g, o)
        assert not (g.raw_status == _lib.BLOCK_OK_SPILLED).any()
        ent = entries_from_flat(ctx, cols, check=False)
        first = cols.first.cpu().numpy()
        kpos, vpos = ent.kpos.cpu().numpy(), ent.vpos.cpu().numpy()
        keys, vals = cols.keys.cpu().numpy(), cols.values.cpu().numpy()
        assert ent.n == int(first[0][-1]) and kpos[-1] == first[1][-1] and vpos[-1] == first[2][-1]
        assert ent.bad_block == int(np.nonzero(o.status != O.OK)[0][0])
        for b in np.nonzero(o.count)[0]:
            e0 = int(first[0][b])
            got = [(keys[kpos[e]:kpos[e + 1]].tobytes(), vals[vpos[e]:vpos[e + 1]].tobytes())
                   for e in range(e0, e0 + int(o.count[b]))]
            assert got == o.entries(int(b)), b
        assert inp.untouched([p.window]), "the input span was written"
    return g, first, kpos, vpos


@pytest.fixture(scope="module")
def flat_control(ctx, spans):
    return run_flat(ctx, spans[0], 0)


@pytest.mark.parametrize("line,kind", BATCH_CASES, ids=BATCH_IDS)
def test_decode_blocks_flat(ctx, spans, flat_control, line, kind):
    labels, blocks = mixed_batch()
    base = batch_base(line, kind, labels, [len(b) for b in blocks], align=16)
    g, first, kpos, vpos = run_flat(ctx, spans[0], base)
    assert_same_decode(g, flat_control[0])
    for a, b in zip((first, kpos, vpos), flat_control[1:]):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------- range CRC
@functools.lru_cache(maxsize=None)
def crc_files():
    """The batch's blocks as files: each followed by its big-endian CRC-32, three of them with a
    flipped byte (body, trailer) and two too short for a trailer."""
    _, blocks = mixed_batch()
    files = [bytearray(b + struct.pack(">I", zlib.crc32(b))) for b in blocks[::3]]
    files[5][7] ^= 1
    files[40][-1] ^= 0x80
    files[41][-4] ^= 2
    files[50:50] = [bytearray(b"\x01\x02"), bytearray(b"")]
    return [bytes(f) for f in files]


def run_crc(ctx, inp: BigSpan, base: int, files: bool):
    blocks = crc_files() if files else mixed_batch()[1]
    with Placed(inp, blocks, base) as p:
        if files:
            crc, st = verify_files(ctx, p.batch)
        else:
            crc, st = crc32_ranges(ctx, p.batch), None
        torch.cuda.synchronize()
        crc = crc[:len(blocks)].cpu().numpy().view(np.uint32)
        if files:
            st = st[:len(blocks)].cpu().numpy()
            for i, f in enumerate(blocks):
                if len(f) < 4:
                    assert st[i] == _lib.BLOCK_MALFORMED, i
                    continue
                want = zlib.crc32(f[:-4])
                assert crc[i] == want, i
                ok = want == struct.unpack(">I", f[-4:])[0]
                assert st[i] == (_lib.BLOCK_OK if ok else _lib.BLOCK_CHECKSUM_MISMATCH), i
            assert (st == _lib.BLOCK_CHECKSUM_MISMATCH).sum() == 3
        else:
            np.testing.assert_array_equal(crc, [zlib.crc32(b) for b in blocks])
        assert inp.untouched([p.window]), "the input span was written"
    return crc, st


CRC_CASES = [(line, j, edge) for line in LINES for j, edge in ((60, False), (300, False), (200, True))]


@pytest.mark.parametrize("files", [False, True], ids=["ranges", "files"])
@pytest.mark.parametrize("line,j,edge", CRC_CASES,
                         ids=[f"{LINE_IDS[l]}-{j}{'-edge' if e else ''}" for l, j, e in CRC_CASES])
def test_crc32_ranges_and_verify_files(ctx, spans, line, j, edge, files):
    """tpz_crc32_ranges / tpz_verify_files over the blocks taken as ranges / files, any d_src
    alignment of the ranges (the straddling bases are odd multiples of 16 or no multiple at all)."""
    blocks = crc_files() if files else mixed_batch()[1]
    j = j // 3 if files else j
    lens = [len(b) for b in blocks]
    base = base_at_boundary(line, lens, j) if edge else base_for(line, lens, j)
    assert_straddle(line, base, lens, j, boundary=edge)
    control = run_crc(ctx, spans[0], 0, files)
    got = run_crc(ctx, spans[0], base, files)
    np.testing.assert_array_equal(got[0], control[0])
    if files:
        np.testing.assert_array_equal(got[1], control[1])


# ---------------------------------------------------------------------------- codec step
@functools.lru_cache(maxsize=None)
def codec_batch():
    """The batch's well-formed blocks as snappy and lz4 blocks in turn (some left as they are),
    one truncated stream of each codec among them. Returns (blocks, oracle (status, bytes))."""
    labels, blocks = mixed_batch()
    out = []
    for i, (l, b) in enumerate(zip(labels, blocks)):
        if l in ("filler", "empty", "crcflip") or not b or b[-1] != 1:
            out.append(b)
        elif i % 5 < 2:
            out.append(O.snappy_block(b, i % 4))
        elif i % 5 < 4:
            out.append(O.lz4_block(b))
        else:
            out.append(b)
    sn = O.snappy_block(blocks[index_of(labels, "4k", 3)])
    out[10] = sn[:len(sn) // 2] + b"\x02"
    lz = O.lz4_block(blocks[index_of(labels, "4k", 4)])
    out[11] = lz[:len(lz) // 2] + b"\x03"
    want = [O.decompress_block(b) for b in out]
    assert want[10][0] == O.CODEC and want[11][0] == O.CODEC
    return out, want


def codec_item(kind: str) -> int:
    blocks, _ = codec_batch()
    labels, _ = mixed_batch()
    tags = {"snappy": 2, "lz4": 3}
    if kind == "long":              # a 64 KiB-config block: HBM to HBM, past the LDS windows
        return next(i for i, l in enumerate(labels) if l == "64k" and blocks[i][-1] in (2, 3))
    return [i for i, b in enumerate(blocks) if b and b[-1] == tags[kind] and 200 < i][0]


def run_codec(ctx, inp: BigSpan, out: BigSpan, base: int, out_base: int):
    """tpz_decompressed_sizes, tpz_decompress_blocks with d_dst_ext[0] = out_base, then the
    claimed sizes, the same decompress and tpz_decompress_check."""
    blocks, want = codec_batch()
    nb = len(blocks)
    exact = np.array([1 if st != O.OK and b[-1] == 3 else len(d) for b, (st, d) in zip(blocks, want)],
                     np.int64)
    ok = np.array([st == O.OK for st, _ in want])
    s = torch.cuda.current_stream(DEV).cuda_stream
    res = {}
    with Placed(inp, blocks, base) as p:
        b = p.batch
        for claimed in (False, True):
            size = torch.full((nb,), -1, dtype=torch.int64, device=DEV)
            ctx.decompressed_sizes_ptrs(b.src.data_ptr(), b.ext.data_ptr(), nb, b.src_bytes,
                                        size.data_ptr(), s, claimed=claimed)
            torch.cuda.synchronize()
            got = size.cpu().numpy()
            if claimed:
                np.testing.assert_array_equal(got[ok], exact[ok])
            else:
                snappy_err = np.array([st != O.OK and blk[-1] == 2 for blk, (st, _) in zip(blocks, want)])
                np.testing.assert_array_equal(got[~snappy_err], exact[~snappy_err])
            dext = np.zeros(nb + 1, np.int64)
            np.cumsum(got, out=dext[1:])
            dext += out_base
            window = (out_base, int(dext[-1]))
            assert window[1] <= SPAN
            d_dext = torch.from_numpy(dext).to(DEV)
            st = torch.full((nb,), 0xEE, dtype=torch.uint8, device=DEV)
            try:
                ctx.decompress_ptrs(b.src.data_ptr(), b.ext.data_ptr(), nb, b.src_bytes, out.ptr,
                                    d_dext.data_ptr(), st.data_ptr(), s)
                exact_sizes = ctx.decompress_check(s)
                assert exact_sizes == (not claimed), "the truncated lz4 stream's claim is not exact"
                st = st.cpu().numpy()
                data = out.read(*window)
                for i, (wst, wb) in enumerate(want):
                    assert st[i] == wst, i
                    if wst == O.OK:
                        lo = int(dext[i]) - out_base
                        assert data[lo:lo + len(wb)].tobytes() == wb, i
                assert out.untouched([window]), "a store outside the output blocks"
                res[claimed] = (got, st)
            finally:
                out.wipe([window])
        assert inp.untouched([p.window]), "the input span was written"
    return res


@pytest.fixture(scope="module")
def codec_control(ctx, spans):
    return run_codec(ctx, spans[0], spans[1], 0, 0)


@pytest.mark.parametrize("kind", ["snappy", "lz4", "long"])
@pytest.mark.parametrize("line", LINES, ids=LINE_IDS.values())
def test_codec_step(ctx, spans, codec_control, line, kind):
    """tpz_decompressed_sizes, _claimed, tpz_decompress_blocks, tpz_decompress_check: the input
    block and its output both straddle the line."""
    blocks, want = codec_batch()
    j = codec_item(kind)
    base = base_for(line, [len(b) for b in blocks], j)
    out_lens = [len(d) if st == O.OK else 1 for st, d in want]
    out_base = base_for(line, out_lens, j)
    res = run_codec(ctx, spans[0], spans[1], base, out_base)
    for claimed in (False, True):
        np.testing.assert_array_equal(res[claimed][0], codec_control[claimed][0])
        np.testing.assert_array_equal(res[claimed][1], codec_control[claimed][1])


# ---------------------------------------------------------------------------- compressor
@pytest.mark.parametrize("codec", [2, 3])
@pytest.mark.parametrize("line,kind", [(l, k) for l in LINES for k in ("wave", "bigwave", "edge")],
                         ids=[f"{LINE_IDS[l]}-{k}" for l in LINES for k in ("wave", "bigwave", "edge")])
def test_compress_blocks(ctx, spans, line, kind, codec):
    """tpz_compress_blocks with rebased input (its output starts at 0): the round trip through
    the oracle's decoders, as test_gpu_compress.check_round_trip does."""
    labels, blocks = mixed_batch()
    base = batch_base(line, kind, labels, [len(b) for b in blocks], align=16)
    outs = []
    for at in (0, base):
        with Placed(spans[0], blocks, at) as p:
            b = p.batch
            bound = int(_lib.lib().tpz_layout_compress_bound(p.total, b.n_blocks))
            out = torch.empty(bound, dtype=torch.uint8, device=DEV)
            out, oext = compress_blocks(ctx, b.src, b.ext, b.n_blocks, b.src_bytes, codec, out=out)
            torch.cuda.synchronize()
            e = oext.cpu().numpy().view(np.uint64)
            assert int(e[0]) == 0 and int(e[-1]) <= bound
            host = out[:int(e[-1])].cpu().numpy()
            check_round_trip(p.src, p.ext0, host, e, codec)
            outs.append((host.tobytes(), e.tolist()))
            assert spans[0].untouched([p.window]), "the input span was written"
    assert outs[1] == outs[0]


# ---------------------------------------------------------------------------- open
@functools.lru_cache(maxsize=None)
def open_images_case(ctx):
    """Three golden SST images and one from SsTableBuilder.build_image() whose meta section spans
    several 4 KiB tiles; each padded to a multiple of 16 (image starts are 16-byte aligned)."""
    from topazdb_amd.table import SsTableBuilder
    images = [read_golden(n + ".sst") for n in ("sst_100_b128", "sst_4k_k16_v100", "sst_zipf")]
    b = SsTableBuilder(ctx, 128, 0.1)
    for i in range(4000):
        b.add(b"key-%06d-" % i + bytes([65 + i % 26]) * (i % 23), b"v%d" % i * (i % 5))
    img = b.build_image()
    images.insert(2, img + struct.pack(">I", zlib.crc32(img)))
    m = OM.parse(images[2])
    assert m.status == OM.OK and m.info[3] > 3 * _lib.OPEN_TILE      # meta bytes: several tiles
    return images


def open_base(line: int, images, j: int) -> int:
    """The base (a multiple of 16) at which `line` lies in the middle of image j's meta section."""
    lens = [(len(i) + 15) // 16 * 16 for i in images]
    m = OM.parse(images[j])
    base = base_for(line, lens, j, frac=(m.info[2] + m.info[3] / 2) / lens[j])
    at = base + sum(lens[:j])
    margin = min(_lib.OPEN_TILE, m.info[3] // 4)
    assert at + m.info[2] + margin < line < at + m.info[2] + m.info[3] - margin
    return base


def run_open(ctx, span: BigSpan, images, base: int):
    """tpz_open_index + tpz_open_metas with rebased d_span starts, then table.open_images over the
    span's view with one get_batch and one scan per opened table against the host route."""
    from test_gpu_open import answers_equal, check_against_model
    from topazdb_amd.levels import DeviceLevels
    from topazdb_amd.table import FileObject, SsTable, open_images
    sp, at = [], base
    for img in images:
        sp.append((at, len(img)))
        span.place(img, at)
        at += (len(img) + 15) // 16 * 16
    window = (base, at)
    try:
        idx = open_index(ctx, span.view, sp)
        n = len(images)
        fb, fk = idx.file_block.cpu().numpy(), idx.file_key.cpu().numpy()
        nb, kb = int(fb[n]), int(fk[n])
        ext, pos, keys = open_metas(ctx, idx, nb, kb)
        torch.cuda.synchronize()
        r = {"info": idx.info.cpu().numpy().view(np.uint64), "fb": fb, "fk": fk,
             "ext": ext.cpu().numpy(), "pos": pos.cpu().numpy(), "keys": keys.cpu().numpy()}
        check_against_model(r, images)
        opened = open_images(ctx, span.view, sp, verify=True)
        for i, (t, img) in enumerate(zip(opened, images)):
            host = SsTable.open(i, FileObject(f"f{i}", img), ctx)
            assert (t.smallest_key, t.biggest_key) == (host.smallest_key, host.biggest_key)
            qs = [m.first_key for m in host.block_metas][::7] + [t.biggest_key, b"zz", b"\x01"]
            a, b = DeviceLevels(ctx, [[t]]), DeviceLevels(ctx, [[host]])
            answers_equal(a.get_batch(qs), b.get_batch(qs))
            rg = [(("in", qs[0]), ("ex", qs[1])), (None, None)]
            answers_equal(a.scan_batch(rg, 9), b.scan_batch(rg, 9))
        assert span.untouched([window]), "the image span was written"
    finally:
        span.wipe([window])
    return r


@pytest.mark.parametrize("line", LINES, ids=LINE_IDS.values())
@pytest.mark.parametrize("j", [1, 2])
def test_open_index_and_metas(ctx, spans, line, j):
    """The line falls inside the meta section of the 4k golden image (j = 1) or of the built
    image (j = 2): the 4 KiB tile walk crosses it, one image lies below and one above."""
    images = open_images_case(ctx)
    base = open_base(line, images, j)
    control = run_open(ctx, spans[0], images, 0)
    got = run_open(ctx, spans[0], images, base)
    for k in control:
        np.testing.assert_array_equal(got[k], control[k])


# ============================================================================ entry columns
@functools.lru_cache(maxsize=None)
def sorted_entries():
    """About 3,000 sorted entries: keys of 1-40 bytes plus five of 300 (past MERGE_LANE_COPY_MAX),
    values of 0-400 bytes plus one of 65,000, about one value in ten a tombstone."""
    rng = random.Random(77)
    keys = set()
    while len(keys) < 3000:
        keys.add(bytes(rng.randrange(97, 123) for _ in range(rng.randint(1, 40))))
    for c in b"hkmps":
        keys.add(bytes([c]) + bytes(rng.randrange(97, 123) for _ in range(299)))
    out = []
    for i, k in enumerate(sorted(keys)):
        v = b"" if rng.random() < 0.1 else rng.randbytes(rng.randint(0, 400))
        out.append((k, v))
    mid = len(out) // 2
    out[mid] = (out[mid][0], rng.randbytes(65000))
    assert sum(len(k) == 300 for k, _ in out) == 5 and _lib.MERGE_LANE_COPY_MAX < 300
    return out


def long_item(lens) -> int:
    """The longest item of the middle third."""
    n = len(lens)
    return max(range(n // 3, 2 * n // 3), key=lambda i: lens[i])


SETTINGS = ["k31", "v31", "kv32", "k32", "v32"]


def column_bases(setting: str, kvs):
    """(key base, value base) of a setting: (S31 + 5, 3), (3, S31 + 5), (S32 + 5, S32 + 11),
    (S32 + 5, 3), (3, S32 + 5); S puts the line inside a key, or inside a value, of the middle of
    the column, and the bases are no multiple of 16."""
    line = LINES[0] if setting.endswith("31") else LINES[1]
    klens, vlens = [len(k) for k, _ in kvs], [len(v) for _, v in kvs]
    kb = vb = 3
    if "k" in setting:
        j = long_item(klens)
        kb = base_for(line, klens, j, frac=0.5, odd=5)
        assert_straddle(line, kb, klens, j)
    if "v" in setting:
        j = long_item(vlens)
        vb = base_for(line, vlens, j, frac=0.5, odd=11 if setting == "kv32" else 5)
        assert_straddle(line, vb, vlens, j)
    return kb, vb


class PlacedEntries:
    """Entries whose key column lies at `kbase` of one span and whose value column at `vbase` of
    another: a DeviceEntries over the spans' views with rebased positions; key_bytes and val_bytes
    are the true readable sizes, base + column length."""

    def __init__(self, kspan: BigSpan, vspan: BigSpan, kvs, kbase: int, vbase: int):
        self.kspan, self.vspan, self.kbase, self.vbase = kspan, vspan, kbase, vbase
        self.keys, self.kpos, self.vals, self.vpos = TM.pack(kvs)
        self.n = len(kvs)
        self.klen, self.vlen = int(self.kpos[-1]), int(self.vpos[-1])
        self.kwin, self.vwin = (kbase, kbase + self.klen), (vbase, vbase + self.vlen)

    def __enter__(self):
        if self.klen:
            self.kspan.place(self.keys[:self.klen], self.kbase)
        if self.vlen:
            self.vspan.place(self.vals[:self.vlen], self.vbase)
        kp = torch.from_numpy((self.kpos + np.uint64(self.kbase)).view(np.int64)).to(DEV)
        vp = torch.from_numpy((self.vpos + np.uint64(self.vbase)).view(np.int64)).to(DEV)
        self.ent = DeviceEntries(self.kspan.view[:self.kwin[1]], kp, self.vspan.view[:self.vwin[1]], vp)
        assert self.ent.struct().key_bytes == self.kbase + self.klen
        return self

    def untouched(self) -> bool:
        return self.kspan.untouched([self.kwin]) and self.vspan.untouched([self.vwin])

    def __exit__(self, *exc):
        self.kspan.wipe([self.kwin])
        self.vspan.wipe([self.vwin])
        return False


def both_ways(run, kvs, setting):
    """run(kbase, vbase) at base 0 (the control) and at the setting's bases; both are compared
    with the model inside `run`, and with each other here."""
    control = run(0, 0)
    got = run(*column_bases(setting, kvs))
    assert len(got) == len(control)
    for a, b in zip(got, control):
        if isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, b)
        else:
            assert a == b
    return got


# ---------------------------------------------------------------------------- plan and encode
@functools.lru_cache(maxsize=None)
def encode_case(block_size: int):
    kvs = [(k, v) for k, v in sorted_entries() if 6 + len(k) + len(v) <= block_size]
    region, ext, first = O.build_blocks(*TM.pack(kvs), block_size)
    return kvs, region.tobytes(), ext.astype(np.int64), first.astype(np.int64)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("block_size", [256, 4096, 65536])
def test_plan_and_encode_blocks(ctx, spans, block_size, setting):
    """tpz_plan_blocks, tpz_plan_blocks_async, tpz_encode_blocks, tpz_encode_blocks_async against
    O.build_blocks: extents, firsts and region bytes."""
    kvs, w_region, w_ext, w_first = encode_case(block_size)
    assert len(w_ext) > 10

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], kvs, kbase, vbase) as p:
            first, ext, nb = plan_blocks(ctx, p.ent, block_size)
            out = encode_blocks(ctx, p.ent, first, ext, nb)
            first2, ext2, info = plan_blocks_async(ctx, p.ent, block_size)
            out2 = torch.full((len(w_region) + 64,), 0xC5, dtype=torch.uint8, device=DEV)
            encode_blocks_async(ctx, p.ent, first2, ext2, info, out2)
            torch.cuda.synchronize()
            _, bad, nb2 = (int(x) for x in info[:3].cpu().numpy().view(np.uint32))
            assert nb == nb2 == len(w_ext) - 1 and bad == 0xFFFFFFFF
            for f, e, o in ((first, ext, out), (first2, ext2, out2)):
                np.testing.assert_array_equal(e[:nb + 1].cpu().numpy(), w_ext)
                np.testing.assert_array_equal(f[:nb + 1].cpu().numpy().astype(np.int64), w_first)
                assert o[:len(w_region)].cpu().numpy().tobytes() == w_region
            assert bool((out2[len(w_region):] == 0xC5).all())
            assert p.untouched(), "an input span was written"
        return (nb,)

    both_ways(run, kvs, setting)


# ---------------------------------------------------------------------------- merge
@functools.lru_cache(maxsize=None)
def merge_case():
    """Three overlapping runs over the sorted entries (a key is in up to three of them, with a
    value that names its run), as one tpz_entries."""
    e = sorted_entries()
    runs = [[(k, v) for i, (k, v) in enumerate(e) if i % 2 == 0],
            [(k, b"r1" + v[:50]) for i, (k, v) in enumerate(e) if i % 3 == 0],
            [(k, v[:-1]) for i, (k, v) in enumerate(e) if i % 2 == 1 or i % 5 == 0]]
    rj = merge_rule(runs)
    return runs, [kv for r in runs for kv in r], rj, [runs[r][j] for r, j in rj]


@pytest.mark.parametrize("setting", SETTINGS)
def test_merge_runs(ctx, spans, setting):
    runs, flat, rj, want = merge_case()
    run_first = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    wk, wkpos, wv, wvpos = TM.pack(want)
    assert len(want) == len(sorted_entries()) and len(flat) > 4 * _lib.MERGE_TILE

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], flat, kbase, vbase) as p:
            merged, src, info = merge_runs(ctx, p.ent, run_first)
            assert int(info[0]) == len(want) == merged.n
            assert int(info[1]) == int(wkpos[-1]) and int(info[2]) == int(wvpos[-1])
            assert src.cpu().numpy().tolist() == [int(run_first[r]) + j for r, j in rj]
            np.testing.assert_array_equal(merged.kpos.cpu().numpy().view(np.uint64), wkpos)
            np.testing.assert_array_equal(merged.vpos.cpu().numpy().view(np.uint64), wvpos)
            assert merged.keys[:int(wkpos[-1])].cpu().numpy().tobytes() == wk[:int(wkpos[-1])].tobytes()
            assert merged.vals[:int(wvpos[-1])].cpu().numpy().tobytes() == wv[:int(wvpos[-1])].tobytes()
            assert p.untouched(), "an input span was written"
        return (merged.n,)

    both_ways(run, flat, setting)


# ---------------------------------------------------------------------------- memtable build
@functools.lru_cache(maxsize=None)
def membuild_case():
    """2,500 entries in arrival order: 2,000 of the sorted entries and 500 later puts of keys
    among them, shuffled; versions in blocks."""
    rng = random.Random(78)
    e = [kv for kv in sorted_entries()]
    rng.shuffle(e)
    ent = e[:2000] + [(e[rng.randrange(2000)][0], rng.randbytes(rng.randint(0, 60))) for _ in range(500)]
    rng.shuffle(ent)
    assert any(len(v) == 65000 for _, v in ent) and sum(len(k) == 300 for k, _ in ent) >= 3
    ver, v = [], 0
    while len(ver) < len(ent):
        v += rng.randrange(1, 4)
        ver += [v] * rng.randrange(1, 51)
    return ent, ver[:len(ent)]


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("mode", ["replay", "put"])
def test_mem_build(ctx, spans, mode, setting):
    """tpz_mem_build under both rules against _membuild_model.expect."""
    ent, ver = membuild_case()
    versions = ver if mode == "put" else None
    want = MB.expect(ent, versions)
    n = len(ent)
    s = torch.cuda.current_stream(DEV).cuda_stream

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], ent, kbase, vbase) as p:
            st = p.ent.struct()
            d_ver = None if versions is None else \
                torch.from_numpy(np.asarray(versions, np.uint64).view(np.int64)).to(DEV)
            okeys = torch.empty(st.key_bytes, dtype=torch.uint8, device=DEV)
            ovals = torch.empty(st.val_bytes, dtype=torch.uint8, device=DEV)
            okpos, ovpos, opre, over = (torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
                                        for _ in range(4))
            src = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            info = torch.full((8,), -1, dtype=torch.int64, device=DEV)
            ctx.mem_build_ptrs(st, _lib.MEM_REPLAY if versions is None else _lib.MEM_PUT,
                               None if d_ver is None else d_ver.data_ptr(), okeys.data_ptr(),
                               okpos.data_ptr(), ovals.data_ptr(), ovpos.data_ptr(), opre.data_ptr(),
                               src.data_ptr(), over.data_ptr(), info.data_ptr(), s)
            torch.cuda.synchronize()
            h = [int(x) for x in info.cpu().numpy().view(np.uint64)]
            assert h == want["info"] + [0, 0]
            n_out = h[0]
            assert src[:n_out].cpu().numpy().view(np.uint32).tolist() == want["src"]
            kp, vp = okpos[:n_out + 1].cpu().numpy().tolist(), ovpos[:n_out + 1].cpu().numpy().tolist()
            assert kp == np.cumsum([0] + [len(k) for k in want["keys"]]).tolist()
            assert vp == np.cumsum([0] + [len(v) for v in want["vals"]]).tolist()
            assert okeys[:kp[-1]].cpu().numpy().tobytes() == b"".join(want["keys"])
            assert ovals[:vp[-1]].cpu().numpy().tobytes() == b"".join(want["vals"])
            assert opre[:n_out].cpu().numpy().view(np.uint64).tolist() == want["prefix"]
            assert over[:n_out].cpu().numpy().view(np.uint64).tolist() == want["version"]
            assert p.untouched(), "an input span was written"
        return (n_out,)

    both_ways(run, ent, setting)


@pytest.mark.parametrize("setting", SETTINGS)
def test_mem_prefix_and_bloom_build(ctx, spans, setting):
    """tpz_mem_prefix against the model's prefix_of, tpz_bloom_build at fpp 0.1 and 0.01 against
    Bloom.from_keys(...).encode()."""
    from topazdb_amd.table import Bloom
    kvs = sorted_entries()
    want_prefix = [MB.prefix_of(k) for k, _ in kvs]
    hashes = [xxhash.xxh3_64_intdigest(k) for k, _ in kvs]
    want_bloom = [Bloom.from_keys(hashes, fpp).encode() for fpp in (0.1, 0.01)]

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], kvs, kbase, vbase) as p:
            pre = torch.full((p.n,), -1, dtype=torch.int64, device=DEV)
            ctx.mem_prefix_ptrs(p.ent.struct(), pre.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
            torch.cuda.synchronize()
            assert pre.cpu().numpy().view(np.uint64).tolist() == want_prefix
            got = [bloom_build(ctx, p.ent, fpp) for fpp in (0.1, 0.01)]
            assert got == want_bloom
            assert p.untouched(), "an input span was written"
        return (len(got[0]), len(got[1]))

    both_ways(run, kvs, setting)


# ---------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("setting", SETTINGS)
def test_entries_bound(ctx, spans, setting):
    """tpz_entries_bound with the entries and the probe column both rebased (the probe column in
    a third span, the line inside a probe); the Python count as in test_gpu_tables."""
    kvs = sorted_entries()
    keys = [k for k, _ in kvs]
    mid = len(keys) // 2
    probes = [keys[0], keys[-1], keys[700], keys[700][:-1], keys[700] + b"\x00", b"", b"\x00",
              b"\xff" * 20, b"user", keys[1234][:6], keys[2000] + b"\xff"]
    probes += keys[mid - 40:mid + 40] + [k for k in keys if len(k) == 300]
    probes = [(q, inc) for q in probes for inc in (False, True)]
    want = [sum(1 for k in keys if (k <= q if inc else k < q)) for q, inc in probes]
    qlens = [len(q) for q, _ in probes]
    line = LINES[0] if setting.endswith("31") else LINES[1]
    jq = long_item(qlens)
    qbase = base_for(line, qlens, jq, frac=0.5, odd=7)
    assert_straddle(line, qbase, qlens, jq)
    flags = torch.from_numpy(np.array([1 if i else 0 for _, i in probes], np.uint8)).to(DEV)

    def run(kbase, vbase):
        qb = qbase if (kbase, vbase) != (0, 0) else 0
        qwin = (qb, qb + sum(qlens))
        with PlacedEntries(spans[0], spans[1], kvs, kbase, vbase) as p:
            try:
                spans[2].place(b"".join(q for q, _ in probes), qb)
                qp = torch.from_numpy(np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64) + qb).to(DEV)
                out = torch.full((len(probes),), -1, dtype=torch.int32, device=DEV)
                ctx.entries_bound_ptrs(p.ent.struct(), spans[2].ptr, qp.data_ptr(), flags.data_ptr(),
                                       len(probes), out.data_ptr(),
                                       torch.cuda.current_stream(DEV).cuda_stream)
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint32).tolist()
                assert got == want
                assert p.untouched() and spans[2].untouched([qwin]), "an input span was written"
            finally:
                spans[2].wipe([qwin])
        return (got,)

    both_ways(run, kvs, setting)


# ---------------------------------------------------------------------------- table cuts, images
@functools.lru_cache(maxsize=None)
def task_case(ctx):
    """One range over the entries that fit 256-byte blocks, capacity 4096: the model's tables and
    every table's image from the host builder."""
    from test_gpu_tables import host_crc32
    from topazdb_amd.table import SsTableBuilder
    kvs = [(k, v) for k, v in sorted_entries() if 6 + len(k) + len(v) <= 256]
    bounds = [(kvs[0][0], (kvs[-1][0], True))]
    _, tables = TM.task_tables([kvs], bounds, 256, 4096)
    images = []
    for t0, n, _ in tables:
        b = SsTableBuilder(ctx, 256, 0.1)
        for k, v in kvs[t0:t0 + n]:
            b.add(k, v)
        img = b.build_image()
        images.append(img + struct.pack(">I", host_crc32(img)))
    return kvs, bounds, tables, images


@pytest.mark.parametrize("setting", SETTINGS)
def test_table_cut_and_task_images(ctx, spans, setting, monkeypatch):
    """compact_task's loop (tpz_entries_bound, tpz_table_cut, the planned windows, the encode in
    place, tpz_bloom_build, tpz_sst_finish) over rebased merged entries: the tables are
    _tables_model's at capacity 4096 (windows before, across and after the line: tpz_table_cut
    sums absolute kpos + vpos), every image the host builder's."""
    from test_gpu_tables import check_ranges, images_of
    kvs, bounds, tables, images = task_case(ctx)
    assert len(tables) > 20

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], kvs, kbase, vbase) as p:
            monkeypatch.setattr(compact, "_merge_regions", lambda *a: p.ent)
            out = compact.compact_task(ctx, [], bounds, block_size=256, table_capacity=4096)
            check_ranges(out, tables)
            got = images_of(out)
            assert got == images
            assert p.untouched(), "an input span was written"
        return (len(got),)

    both_ways(run, kvs, setting)


@pytest.mark.parametrize("setting", SETTINGS)
def test_sst_finish_images_in_a_span(ctx, spans, setting):
    """tpz_sst_finish with rebased entries and four images inside one output BigSpan (d_base,
    span_bytes): one below 2^31, one straddling 2^31, one straddling 2^32, one above; their data
    regions are encoded in place first. Images and d_info against SsTableBuilder.build_image() +
    tpz_host_crc32."""
    from test_gpu_tables import host_crc32
    from topazdb_amd.table import SsTableBuilder
    kvs = [(k, v) for k, v in sorted_entries() if 6 + len(k) + len(v) <= 4096]
    cut = [0, 700, 1500, 2200, len(kvs)]
    want = []
    for a, b in zip(cut, cut[1:]):
        sb = SsTableBuilder(ctx, 4096, 0.1)
        for k, v in kvs[a:b]:
            sb.add(k, v)
        img = sb.build_image()
        want.append(img + struct.pack(">I", host_crc32(img)))
    sizes = [len(w) for w in want]
    offs = [(LINES[0] - 3 * sizes[0]) // 256 * 256, (LINES[0] - sizes[1] // 2) // 256 * 256,
            (LINES[1] - sizes[2] // 2) // 256 * 256, (LINES[1] + 2 * sizes[3]) // 256 * 256]
    assert offs[0] + sizes[0] < offs[1] < LINES[0] < offs[1] + sizes[1]
    assert offs[2] < LINES[1] < offs[2] + sizes[2] < offs[3] and offs[3] + sizes[3] < SPAN
    out = spans[2]
    s = torch.cuda.current_stream(DEV).cuda_stream

    def run(kbase, vbase):
        wins = [(o, o + n) for o, n in zip(offs, sizes)]
        with PlacedEntries(spans[0], spans[1], kvs, kbase, vbase) as p:
            try:
                ment = p.ent.struct()
                descs, keep = [], []
                for i, (a, b) in enumerate(zip(cut, cut[1:])):
                    win = b - a
                    went = compact._window(p.ent, a, win)
                    first = torch.empty(win + 1, dtype=torch.int32, device=DEV)
                    ext = torch.empty(win + 1, dtype=torch.int64, device=DEV)
                    info = torch.empty(4, dtype=torch.int32, device=DEV)
                    c = torch.empty(8, dtype=torch.int64, device=DEV)
                    ctx.plan_blocks_async_ptrs(went, 4096, first.data_ptr(), ext.data_ptr(),
                                               info.data_ptr(), s)
                    ctx.table_cut_ptrs(ment, a, win, b, first.data_ptr(), ext.data_ptr(),
                                       ext.data_ptr(), info.data_ptr(), 4096, 1 << 40, c.data_ptr(), s)
                    ctx.encode_blocks_async_ptrs(went, first.data_ptr(), ext.data_ptr(),
                                                 info.data_ptr(), out.ptr + offs[i], s)
                    h = c.cpu().numpy().view(np.uint64)
                    status, nb, n_ent, data, kbytes = (int(h[j]) for j in (0, 2, 3, 4, 5))
                    assert status == _lib.CUT_NONE and n_ent == win
                    flen = _lib.bloom_geometry(win, 0.1)[0]
                    filt = torch.empty((flen + 3) // 4, dtype=torch.int32, device=DEV)
                    _lib.check(_lib.lib().tpz_bloom_build(
                        ctx.handle, C.c_void_p(p.ent.keys.data_ptr()),
                        C.c_void_p(p.ent.kpos.data_ptr() + 8 * a), win, 0.1,
                        C.c_void_p(filt.data_ptr()), C.c_void_p(s)), "tpz_bloom_build")
                    assert _lib.sst_image_bytes(data, nb, kbytes, flen) == sizes[i]
                    descs.append(_lib.SstImage(out.ptr + offs[i], data, first.data_ptr(),
                                               ext.data_ptr(), nb, a, filt.data_ptr(), flen))
                    keep.append((first, ext, filt, nb))
                d_desc = torch.from_numpy(np.frombuffer(bytes((_lib.SstImage * 4)(*descs)),
                                                        np.uint8).copy()).to(DEV)
                info = torch.empty((4, 4), dtype=torch.int64, device=DEV)
                ctx.sst_finish_ptrs(ment, d_desc.data_ptr(), 4, max(k[3] for k in keep), out.ptr,
                                    SPAN, info.data_ptr(), s)
                got_info = info.cpu().numpy().view(np.uint64)
                got = [out.read(*w).tobytes() for w in wins]
                for i, w in enumerate(want):
                    assert got[i] == w, i
                    _, meta_off, bloom_off = O.sst_parse(w)
                    assert [int(x) for x in got_info[i][:3]] == [len(w), meta_off, bloom_off], i
                assert out.untouched(wins), "a store outside the images"
                assert p.untouched(), "an input span was written"
            finally:
                out.wipe(wins)
        return (got_info,)

    both_ways(run, kvs, setting)


# ============================================================================ runs and queries
def walk_rebased(dl, keys, span: BigSpan, base: int) -> dict:
    """DeviceLevels.walk / DeviceLsm.walk with the query column (d_keys, d_key_pos) at `base` of
    a span: tpz_get_keys, or tpz_lsm_get_keys for a DeviceLsm."""
    n = len(keys)
    buf, pos = _pack(keys)
    span.place(buf[:int(pos[-1])], base)
    qp = torch.from_numpy(pos + base).to(DEV)
    out = {k: torch.empty(max(n, 1), dtype=t, device=DEV) for k, t in
           (("result", torch.uint8), ("status", torch.uint8), ("table", torch.int32),
            ("block", torch.int32), ("entry", torch.int32))}
    out["val_pos"] = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    lsm = isinstance(dl, DeviceLsm)
    pre = (dl.d_runs.data_ptr(), dl.n_runs) if lsm else ()
    (dl.ctx.lsm_get_keys_ptrs if lsm else dl.ctx.get_keys_ptrs)(
        *pre, dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
        span.ptr, qp.data_ptr(), n, out["result"].data_ptr(), out["status"].data_ptr(),
        out["table"].data_ptr(), out["block"].data_ptr(), out["entry"].data_ptr(),
        out["val_pos"].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    out["n"] = n
    out["_keys"] = (qp,)
    return out


def scan_ranges_rebased(dl, ranges, limit, lo_span, lo_base, hi_span, hi_base) -> dict:
    """scan_ranges with the lower bounds' column at `lo_base` of one span and the upper bounds'
    at `hi_base` of another: tpz_scan_ranges, or tpz_lsm_scan_ranges for a DeviceLsm."""
    n = len(ranges)
    cols, ptrs = [], []
    for side, span, base in (([_bound(r[0], True) for r in ranges], lo_span, lo_base),
                             ([_bound(r[1], False) for r in ranges], hi_span, hi_base)):
        buf, pos = _pack([k for _, k in side])
        span.place(buf[:int(pos[-1])], base)
        cols += [torch.from_numpy(pos + base).to(DEV),
                 torch.from_numpy(np.array([k for k, _ in side], np.uint8)).to(DEV)]
        ptrs += [span.ptr, cols[-2].data_ptr(), cols[-1].data_ptr()]
    out = {k: torch.empty(max(n, 1), dtype=torch.uint8, device=DEV) for k in ("result", "status")}
    out["where"] = torch.empty((max(n, 1), 3), dtype=torch.int32, device=DEV)
    for k in ("hit_table", "hit_block", "hit_entry"):
        out[k] = torch.empty(max(n * limit, 1), dtype=torch.int32, device=DEV)
    for k in ("first", "key_first", "val_first"):
        out[k] = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    out["info"] = torch.empty(3, dtype=torch.int64, device=DEV)
    lsm = isinstance(dl, DeviceLsm)
    pre = (dl.d_runs.data_ptr(), dl.n_runs) if lsm else ()
    (dl.ctx.lsm_scan_ranges_ptrs if lsm else dl.ctx.scan_ranges_ptrs)(
        *pre, dl.d_tables.data_ptr(), dl.n_tables, dl.level_first.ctypes.data, dl.n_levels, *ptrs,
        n, limit, *(out[k].data_ptr() for k in
                    ("result", "status", "where", "hit_table", "hit_block", "hit_entry", "first",
                     "key_first", "val_first", "info")),
        torch.cuda.current_stream(DEV).cuda_stream)
    out["n"], out["limit"], out["by_level"] = n, limit, False
    out["_bounds"] = cols
    return out


def column_window(keys, base):
    return (base, base + sum(len(k) for k in keys))


@functools.lru_cache(maxsize=None)
def lsm_case():
    """Two memtable runs and one table over the sorted entries: a key is in up to all three, the
    newer run holds tombstones over live values below it. Queries: held keys, their neighbours,
    absent keys; ranges over the middle of the key space."""
    rng = random.Random(79)
    e = sorted_entries()
    table = [(k, b"t=" + v[:40]) for i, (k, v) in enumerate(e) if i % 2 == 0 and len(k) <= 40]
    run0 = [(k, v) for i, (k, v) in enumerate(e) if i % 3 != 1]
    run1 = [(k, b"" if i % 4 == 0 else b"new=" + v[:30]) for i, (k, v) in enumerate(e) if i % 5 < 2]
    pieces = G.build_pieces(table, 256)
    host = [[pieces.host_table(0)]]
    keys = [k for k, _ in e]
    qs = keys[::11] + [keys[i] + b"\x00" for i in range(0, len(keys), 97)] + \
        [keys[i][:-1] for i in range(5, len(keys), 89) if len(keys[i]) > 1] + [b"zzzz", b"\x01"]
    rng.shuffle(qs)
    mid = len(keys) // 2
    ranges = [(("in", keys[mid - 30]), ("ex", keys[mid + 30])), (("ex", keys[100]), ("in", keys[140])),
              (None, ("in", keys[20])), (("in", keys[-15]), None), (("in", keys[mid]), ("in", keys[mid]))]
    ranges += [(("in", keys[i]), ("ex", keys[i + 9])) for i in range(200, 2800, 130)]
    runs = [run0, run1]
    gets = [LM.lsm_get_mem(runs, host, q) for q in qs]
    scans = [LM.lsm_scan_mem(runs, host, lo, hi, 12) for lo, hi in ranges]
    return runs, pieces, qs, gets, ranges, scans


@pytest.mark.parametrize("setting", SETTINGS)
def test_lsm_get_and_scan_over_rebased_runs(ctx, spans, setting):
    """Memtable runs as tpz_mem_run over rebased columns (tpz_mem_prefix builds their prefix
    columns there): tpz_lsm_get_keys / _values and tpz_lsm_scan_ranges / _entries with two runs and
    one table, against _lsm_model."""
    from test_gpu_get import assert_equal as assert_gets
    from test_gpu_scan import assert_equal as assert_scans
    runs, pieces, qs, gets, ranges, scans = lsm_case()
    assert sum(g.result == G.FOUND for g in gets) > 50 and sum(g.result == G.DELETED for g in gets) > 10
    assert sum(len(s.entries) for s in scans) > 100
    table = DeviceTable(ctx, pieces.region, pieces.ext, pieces.first_keys, pieces.bloom)
    flat = runs[0] + runs[1]
    rf = [0, len(runs[0]), len(flat)]

    def run(kbase, vbase):
        with PlacedEntries(spans[0], spans[1], flat, kbase, vbase) as p:
            dr = [DeviceRun(ctx, dict(keys=p.ent.keys, kpos=p.ent.kpos[a:b + 1], vals=p.ent.vals,
                                      vpos=p.ent.vpos[a:b + 1])) for a, b in zip(rf, rf[1:])]
            assert dr[1].key_bytes == kbase + p.klen and dr[0].n == len(runs[0])
            dl = DeviceLsm(ctx, dr, [[table]])
            got = dl.get_batch(qs)
            assert_gets(got, gets, qs)
            sc = dl.scan_batch(ranges, 12)
            assert_scans(sc, scans, 12, ranges)
            assert p.untouched(), "an input span was written"
        return (got["values"], sc["keys"], sc["values"])

    both_ways(run, flat, setting)


@functools.lru_cache(maxsize=None)
def query_case():
    """300 queries over the 4k golden table (held keys, neighbours, absent keys) and 300 ranges,
    with the oracle's answers through the models test_gpu_get and test_gpu_scan use."""
    rng = random.Random(80)
    f = read_golden("sst_4k_k16_v100.sst")
    pieces = G.Pieces.from_image(f)
    host = [[pieces.host_table(0)]]
    it = O.SstIter(f)
    it.seek_to_first()
    keys = []
    while it.is_valid():
        keys.append(it.key())
        it.next()
    qs = [keys[rng.randrange(len(keys))] if i % 3 else rng.randbytes(16) for i in range(290)]
    qs += [keys[0][:-1], keys[-1] + b"\x00", b"\x00", b"\xff" * 16] + [k + b"\x01" for k in keys[5:11]]
    ranges = []
    for i in range(300):
        a, b = sorted((rng.randrange(len(keys)), rng.randrange(len(keys))))
        ranges.append(((("in", "ex")[i % 2], keys[a]), (("ex", "in")[i % 3 == 0], keys[min(b, a + 6)])))
    seeks = []
    for q in qs:
        it.seek_to_key(q)
        seeks.append((it.is_valid(), it.block_idx(), it.key() if it.is_valid() else None))
    gets = [G.level_get(host, q) for q in qs]
    scans = [SM.lsm_scan(host, lo, hi, 5) for lo, hi in ranges]
    return f, pieces, qs, seeks, gets, ranges, scans


@pytest.mark.parametrize("line", LINES, ids=LINE_IDS.values())
def test_query_columns(ctx, spans, line):
    """The query columns rebased (d_keys / d_key_pos; the lo and hi bounds in two spans) for
    tpz_seek_keys, tpz_bloom_may_contain, tpz_get_keys and tpz_scan_ranges over sst_4k_k16_v100."""
    from test_gpu_get import assert_equal as assert_gets
    from test_gpu_scan import assert_equal as assert_scans
    f, pieces, qs, seeks, gets, ranges, scans = query_case()
    t = DeviceTable(ctx, pieces.region, pieces.ext, pieces.first_keys, pieces.bloom)
    host = pieces.host_table(0)
    dl = DeviceLevels(ctx, [[t]])
    qlens = [len(q) for q in qs]
    lo_keys = [_bound(r[0], True)[1] for r in ranges]
    hi_keys = [_bound(r[1], False)[1] for r in ranges]
    bases = {}
    for name, ks in (("q", qs), ("lo", lo_keys), ("hi", hi_keys)):
        lens = [len(k) for k in ks]
        j = len(ks) // 2
        bases[name] = base_for(line, lens, j, frac=0.5, odd=5)
        assert_straddle(line, bases[name], lens, j)
    s = torch.cuda.current_stream(DEV).cuda_stream
    res = []
    for at in ({"q": 0, "lo": 0, "hi": 0}, bases):
        wins = [column_window(qs, at["q"]), column_window(lo_keys, at["lo"]),
                column_window(hi_keys, at["hi"])]
        try:
            w = walk_rebased(dl, qs, spans[2], at["q"])
            qp = w["_keys"][0]
            n = len(qs)
            out = {k: torch.empty(n, dtype=d, device=DEV) for k, d in
                   (("block", torch.int32), ("entry", torch.int32), ("status", torch.uint8),
                    ("valid", torch.uint8), ("bloom", torch.uint8))}
            ctx.seek_keys_ptrs(t.table(), spans[2].ptr, qp.data_ptr(), n, out["block"].data_ptr(),
                               out["entry"].data_ptr(), out["status"].data_ptr(),
                               out["valid"].data_ptr(), s)
            ctx.bloom_ptrs(t.bloom.data_ptr(), t.bloom_len, spans[2].ptr, qp.data_ptr(), n,
                           out["bloom"].data_ptr(), s)
            torch.cuda.synchronize()
            sk = {k: v.cpu().numpy() for k, v in out.items()}
            assert (sk["status"] == _lib.BLOCK_OK).all()
            for i, (valid, blk, key) in enumerate(seeks):
                assert bool(sk["valid"][i]) == valid and int(sk["block"][i]) == blk, qs[i]
                if valid:
                    assert host.read_block(blk).key_at(int(sk["entry"][i])) == key, qs[i]
            assert sk["bloom"].astype(bool).tolist() == [host.may_contain(q) for q in qs]
            dl.walk = lambda keys: w
            got = dl.get_batch(qs)
            assert_gets(got, gets, qs)
            dl.scan_ranges = lambda rg, limit, by_level=False: scan_ranges_rebased(
                dl, rg, limit, spans[0], at["lo"], spans[1], at["hi"])
            sc = dl.scan_batch(ranges, 5)
            assert_scans(sc, scans, 5, ranges)
            for sp, win in zip((spans[2], spans[0], spans[1]), wins):
                assert sp.untouched([win]), "a query span was written"
            res.append((sk, got["values"], sc["keys"], sc["values"]))
        finally:
            for sp, win in zip((spans[2], spans[0], spans[1]), wins):
                sp.wipe([win])
    for k in res[0][0]:
        np.testing.assert_array_equal(res[1][0][k], res[0][0][k])
    assert res[1][1:] == res[0][1:]

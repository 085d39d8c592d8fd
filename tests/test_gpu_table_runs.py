"""tpz_table_runs_layout / tpz_table_runs_entries: resident tables gathered into merge runs.

The reference is the host, read from each table's own columns and statuses: per table
DeviceTable.cols.dense(), the run being the concatenated entries of its OK / OK_SPILLED blocks, the
first bad (run, block) from the statuses. Compared: the three prefix arrays, the run table, the
d_info totals, kpos, vpos and every key and value byte; the bytes past the totals (64 bytes of 0xC5)
and the position slots past n + 1 must stay as they were."""
import functools

import numpy as np
import pytest
import torch

import _oracle as O
from _bigspan import LINES, BigSpan, need_room
from test_encode_host import pack
from test_gpu_compact import long_entry_tables, mixed_batch, overlapping_tables, table_region
from test_gpu_positions import SLOT_ALIGN, Placed, dense_at, slot_windows, span_columns
from test_gpu_snappy import batch_of
from test_gpu_spill import repeated_offset_blocks
from topazdb_amd import _lib, synth
from topazdb_amd.batch import decode_batch, entry_first
from topazdb_amd.compact import entries_from_tables
from topazdb_amd.table import BlockError, DeviceTable

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FILL = 0xC5
PAD = 64
POS_SENT = -0x0123456789ABCDEF
OKS = (_lib.BLOCK_OK, _lib.BLOCK_OK_SPILLED)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def device_tables(ctx, regions, exact_ends=True):
    return [DeviceTable(ctx, np.asarray(src, np.uint8).tobytes(), ext, exact_ends=exact_ends)
            for src, ext in regions]


# ------------------------------------------------------------------------------- the reference
def table_ref(t, dense=None):
    """One table's run from its own columns: per block (n, K, V) with 0 for a block that is neither
    OK nor OK_SPILLED, the kept entries' key / value lengths and bytes, the first bad block."""
    nb = t.n_blocks
    z = np.zeros(0, np.int64)
    if nb == 0:
        return z, z, z, z, z, np.zeros(0, np.uint8), np.zeros(0, np.uint8), None
    d = dense if dense is not None else t.cols.dense(t.batch.ext_host)
    st = t.status[:nb].cpu().numpy()
    ok = np.isin(st, OKS)
    cnt = d.count.astype(np.int64)
    eb = d.entry_base
    klen, vlen = d.klen.astype(np.int64), d.vlen.astype(np.int64)
    ksum = np.concatenate([[0], np.cumsum(klen)])
    vsum = np.concatenate([[0], np.cumsum(vlen)])
    emask = np.repeat(ok, cnt)
    n = np.where(ok, cnt, 0)
    K = np.where(ok, ksum[eb[1:]] - ksum[eb[:-1]], 0)
    V = np.where(ok, vsum[eb[1:]] - vsum[eb[:-1]], 0)
    keys = d.keys[np.repeat(emask, klen)]
    vals = d.vals[np.repeat(emask, vlen)]
    bad = np.nonzero(~ok)[0]
    return n, K, V, klen[emask], vlen[emask], keys, vals, (int(bad[0]) if len(bad) else None)


def excl(x):
    out = np.zeros(len(x) + 1, np.int64)
    np.cumsum(np.asarray(x, np.int64), out=out[1:])
    return out


def host_ref(tables, denses=None):
    parts = [table_ref(t, None if denses is None else denses[i]) for i, t in enumerate(tables)]
    cat = lambda j, dt=np.int64: (np.concatenate([p[j] for p in parts]) if parts  # noqa: E731
                                  else np.zeros(0, dt))
    ref = {"first": np.concatenate([excl(cat(0)), excl(cat(1)), excl(cat(2))]),
           "run_first": excl([int(p[0].sum()) for p in parts]),
           "kpos": excl(cat(3)), "vpos": excl(cat(4)),
           "keys": cat(5, np.uint8), "vals": cat(6, np.uint8), "bad": None}
    for r, p in enumerate(parts):
        if p[7] is not None:
            ref["bad"] = (r, p[7])
            break
    return ref


# ------------------------------------------------------------------------------- the calls
def descriptors(tables):
    descs = (_lib.Table * max(len(tables), 1))(*[t.table() for t in tables])
    return torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(DEV)


def run_gather(ctx, tables, key_short=0, val_short=0, entry_short=0, aligned=None):
    """Both calls through the raw pointers, every output in a buffer with a sentinel tail.
    key_short / val_short / entry_short: the capacities handed to the gather, below the totals."""
    n_runs = len(tables)
    bf = np.zeros(n_runs + 1, np.uint32)
    np.cumsum([t.n_blocks for t in tables], out=bf[1:])
    nb = int(bf[-1])
    d_tabs = descriptors(tables)
    first = torch.full((3 * (nb + 1) + 4,), POS_SENT, dtype=torch.int64, device=DEV)
    run_first = torch.full((n_runs + 1 + 4,), -7, dtype=torch.int32, device=DEV)
    info = torch.full((4 + 2,), POS_SENT, dtype=torch.int64, device=DEV)
    ctx.table_runs_layout_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                               run_first.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    h_info = info.cpu().numpy()
    assert (h_info[4:] == POS_SENT).all() and (first[3 * (nb + 1):].cpu().numpy() == POS_SENT).all()
    assert (run_first[n_runs + 1:].cpu().numpy() == -7).all()
    n, kb, vb, bad = (int(x) for x in h_info[:4].view(np.uint64))
    key_cap, val_cap, entry_cap = max(kb - key_short, 0), max(vb - val_short, 0), max(n - entry_short, 0)
    keys = torch.full((max(kb + PAD, 16),), FILL, dtype=torch.uint8, device=DEV)
    vals = torch.full((max(vb + PAD, 16),), FILL, dtype=torch.uint8, device=DEV)
    kpos = torch.full((n + 1 + 4,), POS_SENT, dtype=torch.int64, device=DEV)
    vpos = torch.full((n + 1 + 4,), POS_SENT, dtype=torch.int64, device=DEV)
    ctx.table_runs_entries_ptrs(d_tabs.data_ptr(), n_runs, bf.ctypes.data, first.data_ptr(),
                                keys.data_ptr(), key_cap, kpos.data_ptr(), vals.data_ptr(), val_cap,
                                vpos.data_ptr(), entry_cap, aligned=aligned)
    torch.cuda.synchronize()
    return {"n": n, "kb": kb, "vb": vb,
            "bad": None if bad == 2**64 - 1 else (bad >> 32, bad & 0xFFFFFFFF),
            "first": first[:3 * (nb + 1)].cpu().numpy(),
            "run_first": run_first[:n_runs + 1].cpu().numpy().view(np.uint32).astype(np.int64),
            "keys": keys.cpu().numpy(), "vals": vals.cpu().numpy(),
            "kpos": kpos.cpu().numpy(), "vpos": vpos.cpu().numpy(),
            "caps": (key_cap, val_cap, entry_cap)}


def assert_exact(got, ref):
    n = len(ref["kpos"]) - 1
    assert (got["n"], got["kb"], got["vb"]) == (n, len(ref["keys"]), len(ref["vals"]))
    assert got["bad"] == ref["bad"]
    np.testing.assert_array_equal(got["first"], ref["first"])
    np.testing.assert_array_equal(got["run_first"], ref["run_first"])
    np.testing.assert_array_equal(got["kpos"][:n + 1], ref["kpos"])
    np.testing.assert_array_equal(got["vpos"][:n + 1], ref["vpos"])
    assert (got["kpos"][n + 1:] == POS_SENT).all() and (got["vpos"][n + 1:] == POS_SENT).all()
    assert got["keys"][:got["kb"]].tobytes() == ref["keys"].tobytes()
    assert got["vals"][:got["vb"]].tobytes() == ref["vals"].tobytes()
    assert (got["keys"][got["kb"]:] == FILL).all() and (got["vals"][got["vb"]:] == FILL).all()


def check(ctx, tables, **kw):
    ref = host_ref(tables)
    got = run_gather(ctx, tables, **kw)
    assert_exact(got, ref)
    return got, ref


# ------------------------------------------------------------------------------- entries, run table
BLOCK_SIZES = [256, 4096, 65536]


@functools.lru_cache(maxsize=None)
def case_runs(block_size: int):
    return long_entry_tables(11) if block_size == 65536 else overlapping_tables(block_size + 2)


@functools.lru_cache(maxsize=None)
def residues():
    """From the packed entries alone (no GPU): the residues mod 16 of every block's key bytes K and
    of every block's destination starts kbase / vbase, over the three cases."""
    rk, rkb, rvb = set(), set(), set()
    for bs in BLOCK_SIZES:
        K, V = [], []
        for run in case_runs(bs):
            _, _, first = O.build_blocks(*pack(run), bs)
            kl = excl([len(k) for k, _ in run])
            vl = excl([len(v) for _, v in run])
            f = first.astype(np.int64)
            K += (kl[f[1:]] - kl[f[:-1]]).tolist()
            V += (vl[f[1:]] - vl[f[:-1]]).tolist()
        rk |= {k % 16 for k in K}
        rkb |= {int(x) % 16 for x in excl(K)[:-1]}
        rvb |= {int(x) % 16 for x in excl(V)[:-1]}
    return rk, rkb, rvb


@pytest.mark.parametrize("exact_ends,codec", [(True, 1), (False, 1), (True, 2), (True, 3)])
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_entries_and_run_table(ctx, block_size, exact_ends, codec):
    """Three overlapping tables (long entries at 64 KiB: blocks of several copy windows), with
    exact and slotted ends (d_entry_first NULL), and opened from snappy and lz4 regions."""
    every = set(range(16))
    assert residues() == (every, every, every)
    runs = case_runs(block_size)
    tables = device_tables(ctx, [table_region(r, block_size, codec) for r in runs], exact_ends)
    assert all((t.cols.entry_first is not None) == exact_ends for t in tables)
    assert all((t.codec is not None) == (codec != 1) for t in tables)
    got, ref = check(ctx, tables)
    assert got["bad"] is None and got["n"] == sum(len(r) for r in runs)
    flat = [kv for r in runs for kv in r]
    assert ref["keys"].tobytes() == b"".join(k for k, _ in flat)        # the reference is the input
    assert ref["vals"].tobytes() == b"".join(v for _, v in flat)
    if block_size == 65536:
        K = np.diff(got["first"][len(got["first"]) // 3:2 * len(got["first"]) // 3])
        assert K.max() > 4 * 1024                                       # more than 4 windows of keys
    # the aligned-load form of the gather (the diagnostic export) writes the same bytes
    assert_exact(run_gather(ctx, tables, aligned=1), ref)
    # and the Python route returns the same entries
    ent, rf = entries_from_tables(ctx, tables)
    assert ent.bad_block is None and ent.n == got["n"] and rf.tolist() == ref["run_first"].tolist()
    np.testing.assert_array_equal(ent.kpos.cpu().numpy(), ref["kpos"])
    np.testing.assert_array_equal(ent.vpos.cpu().numpy(), ref["vpos"])
    assert ent.keys[:got["kb"]].cpu().numpy().tobytes() == ref["keys"].tobytes()
    assert ent.vals[:got["vb"]].cpu().numpy().tobytes() == ref["vals"].tobytes()


# ------------------------------------------------------------------------------- shapes
def k3(i: int) -> bytes:
    return bytes([1 + i // 65536, (i >> 8) & 0xFF, i & 0xFF])


def test_one_entry_blocks_and_tombstone_blocks(ctx):
    single = [(b"only-key", b"only-value")]
    fat = [(b"fat%04d" % i, bytes([i]) * 200) for i in range(40)]          # one entry per block
    dead = [(b"gone%05d" % i, b"") for i in range(300)]                    # V == 0 in every block
    tables = device_tables(ctx, [table_region(r, 256) for r in (single, fat, dead)])
    assert [t.n_blocks for t in tables][:2] == [1, 40] and tables[2].n_blocks > 10
    got, ref = check(ctx, tables)
    st = len(got["first"]) // 3
    n, V = np.diff(got["first"][:st]), np.diff(got["first"][2 * st:])
    assert (n[:41] == 1).all() and (V[41:] == 0).all() and got["n"] == 341


def test_blocks_of_more_than_255_entries(ctx):
    run = [(k3(i), b"" if i % 3 else b"v") for i in range(2500)]
    for exact in (True, False):
        tables = device_tables(ctx, [table_region(run, 4096)], exact)
        got, _ = check(ctx, tables)
        assert np.diff(got["first"][:tables[0].n_blocks + 1]).max() > 255


def test_tables_without_blocks_and_no_runs(ctx):
    a, b = overlapping_tables(5, n=120, tables=2)
    for runs in ([[], a, [], b, []], [[], []], [[]], []):
        tables = device_tables(ctx, [table_region(r, 256) for r in runs])
        got, ref = check(ctx, tables)
        assert got["n"] == sum(len(r) for r in runs) and len(got["run_first"]) == len(runs) + 1
    ent, rf = entries_from_tables(ctx, [])
    assert ent.n == 0 and rf.tolist() == [0] and ent.bad_block is None


def test_256_runs(ctx):
    runs = [[(b"r%03d-%04d" % (t, i), b"x" * ((t + i) % 23)) for i in range(1 + t % 7)]
            for t in range(_lib.MERGE_MAX_RUNS)]
    runs[17] = runs[200] = []
    tables = device_tables(ctx, [table_region(r, 256) for r in runs])
    got, ref = check(ctx, tables)
    assert len(got["run_first"]) == 257 and got["run_first"][-1] == got["n"]


def test_spilled_blocks(ctx):
    """Repeated offsets: blocks whose decoded bytes do not fit their slot are read from their
    spill records (the run holds every materialised entry)."""
    src, ext = batch_of(repeated_offset_blocks())
    plain = table_region(overlapping_tables(9, n=100, tables=1)[0], 256)
    for exact in (True, False):
        tables = device_tables(ctx, [plain, (np.ascontiguousarray(src), ext), plain], exact)
        st = tables[1].status.cpu().numpy()
        assert (st == _lib.BLOCK_OK_SPILLED).sum() >= 4 and (st == _lib.BLOCK_OK).sum() >= 3
        got, _ = check(ctx, tables)
        assert got["bad"] is None


# ------------------------------------------------------------------------------- scan edges
@functools.lru_cache(maxsize=None)
def many_blocks():
    rng = np.random.default_rng(77)
    n = 330_000                 # keys of 8..40 bytes, values of 0..60: about four entries a block
    kpos, vpos = excl(rng.integers(8, 41, n)), excl(rng.integers(0, 61, n))
    keys = rng.integers(1, 256, int(kpos[-1]), dtype=np.uint8)
    vals = rng.integers(0, 256, int(vpos[-1]), dtype=np.uint8)
    src, ext = synth.build_blocks(keys, kpos.astype(np.uint64), vals, vpos.astype(np.uint64), 256)
    assert len(ext) - 1 >= 70_001
    return src, ext


@pytest.mark.parametrize("total", [1, 2, 255, 256, 257, 1023, 1025, 70_001])
def test_scan_edges(ctx, total):
    """Block totals around the scan's thread, wave and workgroup sizes, over three tables."""
    src, ext = many_blocks()
    cuts = [0, total // 3, 2 * total // 3, total]
    regions = []
    for a, b in zip(cuts, cuts[1:]):
        lo, hi = int(ext[a]), int(ext[b])
        regions.append((src[lo:hi], ext[a:b + 1] - ext[a]))
    tables = device_tables(ctx, regions)
    assert sum(t.n_blocks for t in tables) == total
    got, _ = check(ctx, tables)
    assert got["bad"] is None and got["n"] > 0


# ------------------------------------------------------------------------------- bad blocks
def test_bad_blocks(ctx):
    """A checksum mismatch and a BAD_ENTRY block in table 1 of 3: the first in run order is named,
    neither holds entries, the others are exact, and the Python route raises there."""
    order = ["ok", "crc", "ok", "bad", "ok"]
    a, b = overlapping_tables(3, n=150, tables=2)
    regions = [table_region(a, 256), mixed_batch(order), table_region(b, 256)]
    tables = device_tables(ctx, regions)
    st = tables[1].status.cpu().numpy().tolist()
    assert st == [_lib.BLOCK_OK, _lib.BLOCK_CHECKSUM_MISMATCH, _lib.BLOCK_OK, _lib.BLOCK_BAD_ENTRY,
                  _lib.BLOCK_OK]
    got, ref = check(ctx, tables)
    assert got["bad"] == (1, 1)
    b0 = tables[0].n_blocks
    n = np.diff(got["first"][:len(got["first"]) // 3])
    assert n[b0 + 1] == 0 and n[b0 + 3] == 0 and n[b0] == 5 and n[b0 + 2] == 7 and n[b0 + 4] == 9
    ent, _ = entries_from_tables(ctx, tables, check=False)
    assert ent.bad_block == (1, 1) and ent.n == got["n"]
    with pytest.raises(BlockError) as e:
        entries_from_tables(ctx, tables)
    assert (e.value.table, e.value.block, e.value.status) == (1, 1, _lib.BLOCK_CHECKSUM_MISMATCH)
    assert "checksum" in str(e.value)
    only_bad = device_tables(ctx, [regions[0], mixed_batch(["ok", "bad"]), regions[2]])
    with pytest.raises(BlockError) as e:
        entries_from_tables(ctx, only_bad)
    assert (e.value.table, e.value.block, e.value.status) == (1, 1, _lib.BLOCK_BAD_ENTRY)


# ------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("aligned", [None, 1])
def test_capacities_short_of_the_totals(ctx, aligned):
    """key_cap and val_cap 5 bytes short, entry_cap one short: nothing at or past a capacity is
    written, everything below it is exact, and the call returns."""
    tables = device_tables(ctx, [table_region(r, 256) for r in overlapping_tables(21, n=300)])
    ref = host_ref(tables)
    got = run_gather(ctx, tables, key_short=5, val_short=5, entry_short=1, aligned=aligned)
    kc, vc, ec = got["caps"]
    n = got["n"]
    assert (kc, vc, ec) == (got["kb"] - 5, got["vb"] - 5, n - 1)
    assert got["keys"][:kc].tobytes() == ref["keys"][:kc].tobytes()
    assert got["vals"][:vc].tobytes() == ref["vals"][:vc].tobytes()
    assert (got["keys"][kc:] == FILL).all() and (got["vals"][vc:] == FILL).all()
    np.testing.assert_array_equal(got["kpos"][:ec + 1], ref["kpos"][:ec + 1])
    np.testing.assert_array_equal(got["vpos"][:ec + 1], ref["vpos"][:ec + 1])
    assert (got["kpos"][ec + 1:] == POS_SENT).all() and (got["vpos"][ec + 1:] == POS_SENT).all()


# ------------------------------------------------------------------------------- positions
@pytest.fixture(scope="module")
def spans():
    """Two BigSpans (the encoded table and its decoded data column), freed at module end."""
    try:
        need_room(2, extra=4 << 30)
    except AssertionError as e:
        pytest.skip(str(e))
    s = [BigSpan(DEV) for _ in range(2)]
    yield s
    for x in s:
        x.free()
    torch.cuda.empty_cache()


def straddle_base(line: int, ext0: np.ndarray, j: int) -> int:
    """The base (a multiple of SLOT_ALIGN) at which block j's slot starts about 1.5 KiB below
    `line`."""
    base = (line - 1536 - int(ext0[j]) - 256 * j) // SLOT_ALIGN * SLOT_ALIGN
    sb = int(_lib.slot_base(base + int(ext0[j]), j))
    assert sb < line < sb + 3000
    return base


@pytest.mark.parametrize("line", LINES, ids=["2^31", "2^32"])
def test_slots_across_a_line(ctx, spans, line):
    """A table decoded into a BigSpan so that a block's slot straddles 2^31 / 2^32 in d_data (its
    keys below the line, its values across it): the slot bases are u64. Slotted and exact ends."""
    inp, out = spans
    src, ext = synth.make_region("4k", 48)
    blocks = [src[int(ext[i]):int(ext[i + 1])].tobytes() for i in range(48)]
    with Placed(inp, blocks, straddle_base(line, ext, 20)) as p:
        wins = slot_windows(p.ext)
        owned = [(wins[0][0], wins[-1][1])]
        assert wins[20][0] < line < wins[20][1]
        try:
            for exact in (False, True):
                cols = span_columns(out, p.batch, entry_first(ctx, p.batch) if exact else None)
                decode_batch(ctx, p.batch, cols)
                d = dense_at(cols, p.base, p.ext0)
                assert (d.raw_status == _lib.BLOCK_OK).all()
                t = DeviceTable.__new__(DeviceTable)
                t.ctx, t.n_blocks, t.batch, t.cols, t.codec = ctx, 48, p.batch, cols, None
                t.status = cols.status
                t.first_keys = torch.zeros(16, dtype=torch.uint8, device=DEV)
                t.first_pos = torch.zeros(49, dtype=torch.int64, device=DEV)
                t.bloom, t.bloom_len = None, 0
                ref = host_ref([t], [d])
                for aligned in (None, 1):
                    assert_exact(run_gather(ctx, [t], aligned=aligned), ref)
                assert out.untouched(wins), "the gather wrote into the table's data"
                out.wipe(owned)
                del cols, t
            assert inp.untouched([p.window]), "the input span was written"
        finally:
            out.wipe(owned)

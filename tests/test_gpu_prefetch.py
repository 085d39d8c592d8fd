"""The wave path's one-block-ahead prefetch: the next block's bytes, its exact-ends start
(tpz_columns.d_entry_first, a scalar load issued with the prefetch) and the stores a block leaves
in flight into the next one (tpz_decode.hip, issue() and vm_pad).

What can go wrong there: a block's {kend, vend} pairs written at a stale or a neighbour's
d_entry_first (the wave's first block, the block after one the wave path hands on, a chunk
boundary, the last block), a window staged before its loads arrived or holding the previous
block's bytes, and the refill of the batch's last bytes (fix_tail) racing the prefetch. Every
check is against the CPU oracle and the block builder's own lengths."""
import numpy as np
import pytest
import torch

import _oracle as O
from test_gpu_decode import MG, _random_blocks, assert_parity, ctx  # noqa: F401 (fixture)
from test_gpu_exact import exact_entries_host
from test_gpu_flat import flat_parity
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, SlottedColumns, decode_batch, exact_columns

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A          # no {kend, vend} can equal it (ends are below 2^17)
SIZES = [1, 2, 15, 16, 17, 33, 4097]


def build_block(rng, n, kmax=20, vmin=0, vmax=40):
    """A well-formed block of n entries of random bytes; returns (bytes, [n, 2] ends)."""
    bb = MG.BlockBuilder(1 << 20)
    kl = rng.integers(1, kmax + 1, n)
    vl = rng.integers(vmin, vmax + 1, n)
    for i in range(n):
        assert bb.add(rng.bytes(int(kl[i])), rng.bytes(int(vl[i])))
    offs, data = bb.build()
    assert max(offs) < 65536
    pairs = np.stack([np.cumsum(kl), np.cumsum(vl)], axis=1).astype(np.uint32)
    return MG.encode_block(offs, data), pairs


def join(blocks, tail=0):
    """(src, ext) of the blocks back to back, `tail` bytes of filler after the last one."""
    src = np.frombuffer(b"".join(blocks) + b"\xa5" * tail, np.uint8).copy()
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    return src, ext


@pytest.fixture(scope="module")
def pool():
    """4,097 wave-path blocks of 1..63 entries (so d_entry_first is not linear in b)."""
    rng = np.random.default_rng(20)
    counts = rng.integers(1, 64, max(SIZES))
    built = [build_block(rng, int(n)) for n in counts]
    assert max(len(b) for b, _ in built) <= 4336
    return [b for b, _ in built], [p for _, p in built]


def check_layout(ctx, src, ext, pairs, exact, src_bytes=None):
    """Decodes into columns whose ends hold a sentinel; statuses, counts and CRCs are the
    oracle's, the entries' bytes too, and the ends array is exactly: every block's pairs at its
    first pair (d_entry_first[b] or tpz_entry_base), the slotted layout's zero padding to whole
    lines, and the sentinel everywhere else."""
    batch = DeviceBatch(src, ext)
    if src_bytes is not None:
        batch.src_bytes = src_bytes
    nb = batch.n_blocks
    cols = exact_columns(ctx, batch) if exact else SlottedColumns(nb, batch.src_bytes)
    cols.ends.fill_(SENT)
    decode_batch(ctx, batch, cols).complete()
    st, crc, cnt = cols.meta_host()
    o = O.decode_batch(src, ext)
    assert (o.status == O.OK).all()
    np.testing.assert_array_equal(st, o.status)            # raw: in place, none spilled
    np.testing.assert_array_equal(crc, o.crc_actual)
    np.testing.assert_array_equal(cnt, o.count)
    np.testing.assert_array_equal(cnt, [len(p) for p in pairs])
    ends = cols.ends.cpu().numpy().view(np.uint32)
    want = np.full(ends.shape, SENT, np.uint32)
    if exact:
        first = cols.entry_first.cpu().numpy()
        np.testing.assert_array_equal(
            first, np.concatenate([[0], np.cumsum(exact_entries_host(src, ext))]))
        np.testing.assert_array_equal(np.diff(first), cnt)
        assert ends.size == 2 * int(first[nb])             # the pairs tile the array
        base = first[:nb]
    else:
        base = _lib.entry_base(np.asarray(ext[:nb], np.int64), np.arange(nb, dtype=np.int64))
    for b in range(nb):
        lo, n = int(base[b]), len(pairs[b])
        want[2 * lo:2 * (lo + n)] = pairs[b].ravel()
        if not exact:
            want[2 * (lo + n):2 * (lo + ((n + 15) & ~15))] = 0
    bad = np.nonzero(ends != want)[0]
    assert bad.size == 0, ("ends differ", bad[:8], ends[bad[:8]], want[bad[:8]])
    g = cols.dense(batch.ext_host)
    assert g.keys.tobytes() == o.keys.tobytes() and g.vals.tobytes() == o.vals.tobytes()
    np.testing.assert_array_equal(g.klen, o.klen)
    np.testing.assert_array_equal(g.vlen, o.vlen)
    return cols


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "slotted"])
@pytest.mark.parametrize("nb", SIZES)
def test_ends_sit_at_their_first_pair(ctx, pool, nb, exact):
    blocks, pairs = pool
    src, ext = join(blocks[:nb])
    check_layout(ctx, src, ext, pairs[:nb], exact)
    if not exact and nb <= 33:
        assert_parity(ctx, src, ext, expect_all_ok=True)


def test_short_blocks_after_handed_on_ones(ctx, pool):
    """Blocks the wave path hands on (longer than 4,336 B: bigwave; more than 255 entries: the
    big path) between short ones, at a wave's first block, around a row boundary and last: the
    short block after one decodes with its own d_entry_first, the handed-on ones with theirs."""
    rng = np.random.default_rng(21)
    blocks, pairs = [list(x[:40]) for x in pool]
    for pos, kind in ((0, "long"), (3, "many"), (4, "many"), (15, "long"), (16, "many"),
                      (17, "long"), (30, "long"), (31, "long"), (39, "many")):
        if kind == "long":
            blk, pr = build_block(rng, int(rng.integers(5, 10)), vmin=1000, vmax=1500)
            assert len(blk) > 4336
        else:
            blk, pr = build_block(rng, int(rng.integers(256, 330)), kmax=4, vmax=4)
        blocks[pos], pairs[pos] = blk, pr
    src, ext = join(blocks)
    check_layout(ctx, src, ext, pairs, exact=True)
    check_layout(ctx, src, ext, pairs, exact=False)


@pytest.mark.parametrize("tail", [0, 1, 7, 15])
def test_last_block_near_the_end_of_the_source(ctx, pool, tail):
    """The batch's last block ends `tail` bytes before src_bytes: its last 16-byte pieces (and
    those of the blocks before it, while they end within 16 bytes of src_bytes) straddle the end
    of the source and are refilled byte by byte after the prefetch loads."""
    blocks, pairs = pool
    for nb, skip in ((1, 0), (1, 5), (2, 7), (19, 40)):
        sel = slice(skip, skip + nb)
        src, ext = join(blocks[sel], tail)
        assert len(src) == int(ext[-1]) + tail
        for exact in (True, False):
            check_layout(ctx, src, ext, pairs[sel], exact, src_bytes=len(src))


def test_three_decodes_into_garbage_agree(ctx):
    """Blocks of random bytes with valid CRCs (a window holding another block's bytes, or bytes
    from before its loads arrived, fails the CRC or the comparison), decoded three times into
    columns pre-filled with different garbage."""
    rng = np.random.default_rng(23)
    src, ext = _random_blocks(rng, 300, max_target=4300)
    batch = DeviceBatch(src, ext)
    o = O.decode_batch(src, ext)
    assert (o.status == O.OK).all()
    for exact in (True, False):
        cols = (exact_columns(ctx, batch) if exact
                else SlottedColumns(batch.n_blocks, batch.src_bytes))
        outs = []
        for fill in (0x00, 0xFF, None):
            for t in (cols.data, cols.ends, cols.count, cols.status, cols.crc):
                u = t.view(torch.uint8)
                if fill is None:
                    u.copy_(torch.randint(0, 256, u.shape, dtype=torch.uint8, device=u.device))
                else:
                    u.fill_(fill)
            decode_batch(ctx, batch, cols).complete()
            g = cols.dense(batch.ext_host)
            outs.append((g.raw_status.tobytes(), g.crc_actual.tobytes(), g.count.tobytes(),
                         g.klen.tobytes(), g.vlen.tobytes(), g.keys.tobytes(), g.vals.tobytes()))
        assert outs[0] == outs[1] == outs[2]
        assert outs[0][5] == o.keys.tobytes() and outs[0][6] == o.vals.tobytes()
        np.testing.assert_array_equal(np.frombuffer(outs[0][1], np.uint32), o.crc_actual)
        np.testing.assert_array_equal(np.frombuffer(outs[0][2], np.uint32), o.count)


@pytest.mark.parametrize("nb", [1, 2])
def test_flat_small_batches(ctx, pool, nb):
    src, ext = join(pool[0][:nb])
    flat_parity(ctx, src, ext, whole_columns=True)

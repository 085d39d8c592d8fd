"""The regular path's index cache (tpz_decode.hip, decode_block and copy_crc_piped<.., REG>): a
wave keeps the packed copy index of its last regular block's geometry (n, KL, VL) in the head of
its entry table and reuses it for every following block of that geometry; another geometry
rebuilds it, and a general parse, which writes the entry table, invalidates it. Everything is
compared with the CPU oracle.

What can go wrong there: a stale index after the geometry changed (n alone, KL alone), db (which
changes with every block's start alignment) baked into the cached words, an index used after a
general block overwrote it, the fifth copy window (not cached) next to cached ones, bytes that
depend on what the output held before."""
import numpy as np
import pytest
import torch

import _oracle as O
from test_gpu_decode import MG, assert_parity, ctx  # noqa: F401 (fixture)
from test_gpu_prefetch import check_layout, join
from test_gpu_regular import WAVE_MAX_LEN, near_regular, raw_block, regular_block, regular_fields
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, SlottedColumns, decode_batch

pytestmark = pytest.mark.gpu

RUN = 4000
RUN_SHAPES = [(34, 16, 100), (33, 16, 100), (34, 17, 100), (3, 17, 1000), (34, 16, 100)]


def some(rng, n, kl, vl, k=8):
    """k different blocks of one shape (a run cycles through them)."""
    return [regular_block(rng, n, kl, vl) for _ in range(k)]


def runs_of(rng, shapes, run):
    blocks, pairs = [], []
    for shape in shapes:
        pool = some(rng, *shape)
        for i in range(run):
            blocks.append(pool[i % len(pool)][0])
            pairs.append(pool[i % len(pool)][1])
    return blocks, pairs


@pytest.fixture(scope="module")
def runs():
    """20,000 blocks in five runs of one shape each, so that each of the 4,096 persistent waves
    decodes several blocks of a run (hits) and meets the changes between them: n alone (a
    table's short last block), KL alone, another shape altogether, and back. No block length is
    a multiple of 16, so the start alignment a0 (and db with it) takes every value 0..15 while
    the key stays put."""
    rng = np.random.default_rng(51)
    blocks, pairs = runs_of(rng, RUN_SHAPES, RUN)
    assert all(len(b) % 16 for b in blocks) and max(len(b) for b in blocks) <= WAVE_MAX_LEN
    starts = np.cumsum([0] + [len(b) for b in blocks[:-1]])
    for r in (0, 1, 2, 4):
        assert set(int(s) % 16 for s in starts[r * RUN:(r + 1) * RUN]) == set(range(16))
    return blocks, pairs


@pytest.mark.parametrize("exact", [False, True], ids=["slotted", "exact"])
def test_runs_and_switches(ctx, runs, exact):
    blocks, pairs = runs
    src, ext = join(blocks)
    check_layout(ctx, src, ext, pairs, exact)
    if not exact:
        assert_parity(ctx, src, ext, expect_all_ok=True)


def test_invalidation(ctx):
    """20,000 blocks drawn at random: 60 % one regular shape, a second regular shape, short-key
    general blocks (they write the entry table over the cached index), near-regular blocks,
    empty blocks, long blocks (handed on) and a regular block with a flipped payload bit. A
    regular block after a general one must rebuild the index; the last block is regular."""
    rng = np.random.default_rng(52)
    kinds = [[b for b, _ in some(rng, 34, 16, 100)], [b for b, _ in some(rng, 33, 16, 100, 4)]]
    zipf = []
    for _ in range(4):
        bb = MG.BlockBuilder(4000)
        while bb.add(rng.bytes(int(rng.integers(1, 12))), rng.bytes(int(rng.integers(16, 200)))):
            pass
        zipf.append(MG.encode_block(*bb.build()))
    kinds.append(zipf)
    kinds.append([blk for _, blk in near_regular(rng)[::5]])
    kinds.append([b""])
    long_ = []
    for _ in range(2):
        bb = MG.BlockBuilder(1 << 16)
        for _ in range(6):
            assert bb.add(rng.bytes(16), rng.bytes(1000))
        long_.append(MG.encode_block(*bb.build()))
    assert min(len(b) for b in long_) > WAVE_MAX_LEN
    kinds.append(long_)
    S = 4 + 16 + 100
    kinds.append([raw_block(regular_fields(rng, 34, 16, 100), flip=8 * (2 + 2 * 34 + 9 * S + 40) + 5)])
    pick = rng.choice(len(kinds), 20000, p=[0.6, 0.1, 0.12, 0.08, 0.04, 0.02, 0.04])
    blocks = [kinds[k][int(rng.integers(len(kinds[k])))] for k in pick]
    blocks[-1] = kinds[0][0]
    src, ext = join(blocks)
    g, o = assert_parity(ctx, src, ext)
    assert (o.status[pick == 0] == O.OK).all() and (o.status[pick == 1] == O.OK).all()
    flipped = np.flatnonzero(pick[:-1] == 6)
    assert len(flipped) and (o.status[flipped] == O.CHECKSUM).all() and (g.count[flipped] == 0).all()


def test_fifth_window_with_a_cached_key(ctx):
    """Runs of shapes whose stream exceeds 4096 bytes (by 1 and by 128: the fifth window takes
    the closed form, the first four the cache) between runs of the 4k shape."""
    rng = np.random.default_rng(53)
    shapes = [(34, 16, 100), (4, 16, 1040), (34, 16, 100), (1, 16, 4081), (4, 16, 1040), (34, 16, 100)]
    blocks, pairs = runs_of(rng, shapes, 2500)
    for b, p in zip(blocks[2500:2502] + blocks[7500:7502], pairs[2500:2502] + pairs[7500:7502]):
        assert len(b) <= WAVE_MAX_LEN
        assert _lib.value_start(int(p[-1, 0])) + int(p[-1, 1]) > 4096
    src, ext = join(blocks)
    check_layout(ctx, src, ext, pairs, False)
    assert_parity(ctx, src, ext, expect_all_ok=True)


def test_cached_decode_is_deterministic(ctx, runs):
    """The runs batch decoded twice into buffers pre-filled with different garbage: every byte
    the decode owns (each slot's stream up to its 128-byte line, each block's pairs up to their
    line, status, count, crc) is equal, the key/value gap included."""
    blocks, pairs = runs
    src, ext = join(blocks)
    batch = DeviceBatch(src, ext)
    nb = batch.n_blocks
    cols = SlottedColumns(nb, batch.src_bytes)
    got = []
    for seed in (1, 2):
        gen = torch.Generator(device=cols.data.device).manual_seed(seed)
        for t in (cols.data, cols.ends, cols.count, cols.status, cols.crc):
            u = t.view(torch.uint8)
            u.copy_(torch.randint(0, 256, u.shape, dtype=torch.uint8, device=u.device, generator=gen))
        decode_batch(ctx, batch, cols).complete()
        got.append([t.view(torch.uint8).cpu().numpy().reshape(-1).copy()
                    for t in (cols.data, cols.ends, cols.count, cols.status, cols.crc)])
    e = np.asarray(ext[:nb], np.int64)
    idx = np.arange(nb, dtype=np.int64)
    sb, eb = _lib.slot_base(e, idx), _lib.entry_base(e, idx)
    # the owned ranges as one mask per array (20,000 blocks: no Python loop over bytes)
    own_d = np.zeros(len(got[0][0]) + 1, np.int32)
    own_e = np.zeros(len(got[0][1]) + 1, np.int32)
    for b in range(nb):
        n, kl, vl = len(pairs[b]), int(pairs[b][0, 0]), int(pairs[b][0, 1])
        tot = _lib.value_start(n * kl) + n * vl
        own_d[int(sb[b])] += 1
        own_d[int(sb[b]) + (tot + 127) // 128 * 128] -= 1
        own_e[8 * int(eb[b])] += 1
        own_e[8 * (int(eb[b]) + (n + 15) // 16 * 16)] -= 1
    md, me = np.cumsum(own_d[:-1]) > 0, np.cumsum(own_e[:-1]) > 0
    assert md.sum() > 3000 * nb and me.sum() >= 8 * 16 * nb
    assert got[0][0][md].tobytes() == got[1][0][md].tobytes(), "data"
    assert got[0][1][me].tobytes() == got[1][1][me].tobytes(), "ends"
    assert got[0][2][:4 * nb].tobytes() == got[1][2][:4 * nb].tobytes()
    assert got[0][3][:nb].tobytes() == got[1][3][:nb].tobytes()
    assert got[0][4][:4 * nb].tobytes() == got[1][4][:4 * nb].tobytes()
    assert (got[0][3][:nb] == _lib.BLOCK_OK).all()

"""The regular path's dword index on the device (tpz_decode.hip: reg_dwords, copy_crc_piped<..,
REG, DW>): a regular block whose key and value lengths are multiples of 4 takes, per output
dword, one aligned two-dword LDS read and one byte shift, from an index of four source offsets
per chunk that the wave keeps in its whole entry table; any other regular block keeps the packed
words and the two gathers with their merge. Everything is compared with the CPU oracle: statuses,
counts, CRCs, ends and every key and value byte, in both ends layouts.

What can go wrong there: a boundary dword taken from the wrong source; the key/value gap chunk,
whose successor lies at another byte phase than the keys; db (it changes with every block's
start alignment a0) baked into the cached offsets; the words of one kind read as the other after
the geometry changed between eligible and ineligible; the second KiB of the table (windows 2 and
3) stale after a general parse wrote entries there; the fifth copy window (never cached) next to
cached ones; a "no chunk" lane reading anything but the guard's zeros; bytes that depend on what
the output held before. Batches of at most 4,096 blocks; every batch's last block ends at the
end of a source buffer whose length is no multiple of 16, so its window straddles the end."""
import numpy as np
import pytest
import torch

import _oracle as O
from test_gpu_decode import MG, assert_parity, ctx  # noqa: F401 (fixture)
from test_gpu_prefetch import check_layout, join
from test_gpu_regular import WAVE_MAX_LEN, regular_block
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, SlottedColumns, decode_batch

pytestmark = pytest.mark.gpu

GEOMS = [(16, 16), (16, 100), (20, 24), (100, 16), (16, 20), (256, 1024), (2044, 2044)]
NS = (1, 2, 3, 33, 34, 63, 64, 65, 255)
ODD = [(17, 100), (16, 101), (18, 22)]           # ineligible neighbours
SLACKS = (0, 1, 2, 3, 5, 0, 7, 0)
MAX_BLOCKS = 4096


def fits(n, kl, vl, slack=0):
    return n <= 255 and 7 + n * (6 + kl + vl) + slack <= WAVE_MAX_LEN


def pool(rng, n, kl, vl, k=len(SLACKS)):
    """k different blocks of one shape, with 0..7 bytes of slack after the last entry."""
    return [regular_block(rng, n, kl, vl, slack=s if fits(n, kl, vl, s) else 0)
            for s in SLACKS[:k]]


def runs_of(rng, shapes, run):
    blocks, pairs = [], []
    for shape in shapes:
        p = pool(rng, *shape)
        for i in range(run):
            blocks.append(p[i % len(p)][0])
            pairs.append(p[i % len(p)][1])
    return blocks, pairs


def weave(*pools, count):
    """Block i from pool i mod len(pools), cycling through each pool's blocks."""
    blocks, pairs = [], []
    for i in range(count):
        p = pools[i % len(pools)]
        b, pr = p[(i // len(pools)) % len(p)]
        blocks.append(b)
        pairs.append(pr)
    return blocks, pairs


def to_odd_end(blocks, pairs, spare):
    """The batch with blocks of `spare` (a pool) appended until its length is no multiple of 16:
    the last block then ends inside the last 16-byte line of the source buffer."""
    i = 0
    while sum(len(b) for b in blocks) % 16 == 0:
        blocks, pairs = blocks + [spare[i % len(spare)][0]], pairs + [spare[i % len(spare)][1]]
        i += 1
        assert i < 64
    assert len(blocks) <= MAX_BLOCKS
    return blocks, pairs


def starts_mod16(blocks):
    return np.cumsum([0] + [len(b) for b in blocks[:-1]]) % 16


def both_layouts(ctx, blocks, pairs):
    src, ext = join(blocks)
    assert len(src) == int(ext[-1]) and len(src) % 16 != 0
    for exact in (False, True):
        check_layout(ctx, src, ext, pairs, exact)
    assert_parity(ctx, src, ext, expect_all_ok=True)
    return src, ext


@pytest.mark.parametrize("kl,vl", GEOMS, ids=[f"{k}x{v}" for k, v in GEOMS])
def test_geometry(ctx, kl, vl):
    """Runs of every n of the issue that fits, so that a wave meets the same geometry again (a
    hit) and a change of n alone (a miss); slack after some blocks; all 16 start alignments."""
    rng = np.random.default_rng(71 + kl + vl)
    ns = [n for n in NS if fits(n, kl, vl)]
    assert ns and ns[0] == 1
    blocks, pairs = runs_of(rng, [(n, kl, vl) for n in ns], min(192, MAX_BLOCKS // len(ns) - 8))
    blocks, pairs = to_odd_end(blocks, pairs, pool(rng, 1, kl, vl))
    assert set(int(s) for s in starts_mod16(blocks)) == set(range(16))
    both_layouts(ctx, blocks, pairs)


def test_fifth_window(ctx):
    """Streams over 4096 bytes (by 128, and by 4 with n = 1): windows 0-3 from the dword index,
    the fifth by the closed form with its merge, between runs of the 4k shape."""
    rng = np.random.default_rng(72)
    shapes = [(34, 16, 100), (4, 16, 1040), (34, 16, 100), (1, 16, 4084), (4, 16, 1040), (3, 20, 1360)]
    blocks, pairs = runs_of(rng, shapes, 400)
    for i in (400, 1200, 2000):
        assert len(blocks[i]) <= WAVE_MAX_LEN
        assert _lib.value_start(int(pairs[i][-1, 0])) + int(pairs[i][-1, 1]) > 4096
    blocks, pairs = to_odd_end(blocks, pairs, pool(rng, 34, 16, 100))
    both_layouts(ctx, blocks, pairs)


@pytest.mark.parametrize("kl,vl", ODD, ids=[f"{k}x{v}" for k, v in ODD])
def test_ineligible_neighbours(ctx, kl, vl):
    """A length that is no multiple of 4 keeps the packed words: runs of it, then block by block
    in turn with an eligible geometry (each kind of index over the other in a wave's table)."""
    rng = np.random.default_rng(73 + kl + vl)
    n = min(34, (WAVE_MAX_LEN - 16) // (6 + kl + vl))
    odd, even = pool(rng, n, kl, vl), pool(rng, n, (kl + 3) & ~3, (vl + 3) & ~3)
    blocks, pairs = runs_of(rng, [(n, kl, vl), (2, kl, vl)], 600)
    b2, p2 = weave(odd, even, count=1600)
    b3, p3 = weave(odd, odd, even, even, even, count=1000)
    blocks, pairs = to_odd_end(blocks + b2 + b3, pairs + p2 + p3, odd)
    assert set(int(s) for s in starts_mod16(blocks)) == set(range(16))
    both_layouts(ctx, blocks, pairs)


def test_two_eligible_geometries_in_turn(ctx):
    rng = np.random.default_rng(74)
    a, b, c = pool(rng, 34, 16, 100), pool(rng, 33, 16, 100), pool(rng, 63, 20, 24)
    b1, p1 = weave(a, b, count=1300)
    b2, p2 = weave(a, a, c, count=1300)
    b3, p3 = weave(c, c, c, b, count=1300)
    blocks, pairs = to_odd_end(b1 + b2 + b3, p1 + p2 + p3, a)
    both_layouts(ctx, blocks, pairs)


def zipf_blocks(rng, k=6):
    out = []
    for _ in range(k):
        bb = MG.BlockBuilder(4000)
        while bb.add(rng.bytes(int(rng.integers(1, 12))), rng.bytes(int(rng.integers(16, 200)))):
            pass
        out.append(MG.encode_block(*bb.build()))
    return out


def test_general_block_between(ctx):
    """A general (zipf-shaped) block between blocks of one geometry: its parse writes the entry
    table over both halves of the index, so the next block of the geometry refills it. Fixed
    turns and a random order; the last block is regular."""
    rng = np.random.default_rng(75)
    z = zipf_blocks(rng)
    a = [b for b, _ in pool(rng, 34, 16, 100)]
    c = [b for b, _ in pool(rng, 3, 256, 1024)]
    blocks = []
    for i in range(1200):
        blocks += [a[i % len(a)], z[i % len(z)]] if i % 3 == 0 else [a[i % len(a)]]
    for i in range(600):
        blocks += [c[i % len(c)], c[(i + 1) % len(c)], z[i % len(z)]]
    kinds = [a, c, z]
    pick = rng.choice(3, MAX_BLOCKS - 8 - len(blocks), p=[0.5, 0.2, 0.3])
    blocks += [kinds[k][int(rng.integers(len(kinds[k])))] for k in pick]
    blocks.append(a[0])
    while sum(len(b) for b in blocks) % 16 == 0:
        blocks.append(a[1])
    assert len(blocks) <= MAX_BLOCKS
    src, ext = join(blocks)
    assert len(src) % 16 != 0
    g, o = assert_parity(ctx, src, ext)
    assert (o.status == O.OK).all()


def test_decode_twice_is_identical(ctx):
    """One batch of eligible, ineligible and fifth-window blocks decoded twice into buffers
    pre-filled with different garbage: every byte the decode owns (each slot's stream up to its
    128-byte line, each block's pairs up to their line, status, count, crc) is equal, the
    key/value gap and the padding included."""
    rng = np.random.default_rng(76)
    shapes = [(34, 16, 100), (33, 20, 24), (3, 100, 16), (34, 17, 100), (1, 20, 24), (4, 16, 1040),
              (34, 16, 100), (5, 100, 16), (1, 2044, 2044)]
    blocks, pairs = runs_of(rng, shapes, 440)
    blocks, pairs = to_odd_end(blocks, pairs, pool(rng, 34, 16, 100))
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
    own_d = np.zeros(len(got[0][0]) + 1, np.int32)
    own_e = np.zeros(len(got[0][1]) + 1, np.int32)
    total = 0
    for b in range(nb):
        n, kl, vl = len(pairs[b]), int(pairs[b][0, 0]), int(pairs[b][0, 1])
        tot = _lib.value_start(n * kl) + n * vl
        total += tot
        own_d[int(sb[b])] += 1
        own_d[int(sb[b]) + (tot + 127) // 128 * 128] -= 1
        own_e[8 * int(eb[b])] += 1
        own_e[8 * (int(eb[b]) + (n + 15) // 16 * 16)] -= 1
    md, me = np.cumsum(own_d[:-1]) > 0, np.cumsum(own_e[:-1]) > 0
    assert md.sum() >= total and me.sum() >= 8 * 16 * nb
    assert (got[0][3][:nb] == _lib.BLOCK_OK).all()
    assert got[0][0][md].tobytes() == got[1][0][md].tobytes(), "data"
    assert got[0][1][me].tobytes() == got[1][1][me].tobytes(), "ends"
    assert got[0][2][:4 * nb].tobytes() == got[1][2][:4 * nb].tobytes()
    assert got[0][3][:nb].tobytes() == got[1][3][:nb].tobytes()
    assert got[0][4][:4 * nb].tobytes() == got[1][4][:4 * nb].tobytes()

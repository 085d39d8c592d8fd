"""The wave path's regular-block decode (tpz_decode.hip, decode_block's regularity test and
copy_crc_piped<.., REG>): a block whose entries all have one key length and one value length,
both >= 16, at offsets i * (4 + KL + VL), is decoded from closed forms of (n, KL, VL) instead of
the entry table and the chunk map. Everything is compared with the CPU oracle: statuses, counts,
CRCs, every key and value byte, every end offset.

What can go wrong there: the reciprocal division at some (divisor, dividend), a chunk that
crosses an entry boundary or the key/value gap, the fifth copy window, a block that is almost
regular taken for regular, the hand-over of the pending CRC combine between the regular copy and
the other copies, bytes that depend on what the output held before."""
import struct

import numpy as np
import pytest
import torch

import _oracle as O
from test_gpu_decode import MG, assert_parity, ctx  # noqa: F401 (fixture)
from test_gpu_prefetch import check_layout, join
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, SlottedColumns, decode_batch

pytestmark = pytest.mark.gpu

WAVE_MAX_LEN, WAVE_MAX_N = 4336, 255     # tpz_decode.hip: kWaveMaxLen, kWaveMaxN
KLS, VLS = (16, 17, 31, 32, 48), (16, 17, 100, 1000, 4000)


def raw_block(fields, offsets=None, slack=0, tag=1, flip=None):
    """A block from (kl field, key bytes, vl field, value bytes) per entry, laid out back to
    back; `offsets` replaces the offset section, `slack` bytes follow the last entry, `flip` is a
    payload bit flipped after the CRC was taken."""
    data, offs = bytearray(), []
    for kl, k, vl, v in fields:
        offs.append(len(data))
        data += struct.pack(">H", kl) + k + struct.pack(">H", vl) + v
    data += b"\xc3" * slack
    p = bytearray(MG.block_payload(list(offs if offsets is None else offsets), bytes(data)))
    crc = MG.crc32(bytes(p))
    if flip is not None:
        p[flip // 8] ^= 1 << (flip % 8)
    return bytes(p) + struct.pack(">I", crc) + bytes([tag])


def regular_fields(rng, n, kl, vl):
    return [(kl, rng.bytes(kl), vl, rng.bytes(vl)) for _ in range(n)]


def regular_block(rng, n, kl, vl, slack=0):
    blk = raw_block(regular_fields(rng, n, kl, vl), slack=slack)
    pairs = np.stack([np.arange(1, n + 1) * kl, np.arange(1, n + 1) * vl], axis=1).astype(np.uint32)
    return blk, pairs


def largest_n(kl, vl):
    """The most entries of a regular block that the wave slot takes."""
    return min(WAVE_MAX_N, (WAVE_MAX_LEN - 7) // (6 + kl + vl))


@pytest.fixture(scope="module")
def grid():
    """Every KL x VL x n of the issue that fits a wave slot, in an order that mixes the shapes;
    slack after some blocks so that every start alignment 0..15 occurs."""
    rng = np.random.default_rng(41)
    shapes = []
    for kl in KLS:
        for vl in VLS:
            top = largest_n(kl, vl)
            assert top >= 1, (kl, vl)
            shapes += [(n, kl, vl) for n in sorted({1, 2, 3, 63, 64, 65, top}) if n <= top]
    rng.shuffle(shapes)
    built = [regular_block(rng, n, kl, vl, slack=min(int(rng.integers(0, 3)) * (i % 3 == 0),
                                                     WAVE_MAX_LEN - 7 - n * (6 + kl + vl)))
             for i, (n, kl, vl) in enumerate(shapes)]
    blocks, pairs = [b for b, _ in built], [p for _, p in built]
    assert max(len(b) for b in blocks) <= WAVE_MAX_LEN
    starts = np.cumsum([0] + [len(b) for b in blocks[:-1]])
    assert set(int(s) % 16 for s in starts) == set(range(16))
    assert any(_lib.value_start(int(p[-1, 0])) + int(p[-1, 1]) > 4096 for p in pairs)   # a fifth window
    return blocks, pairs


@pytest.mark.parametrize("exact", [False, True], ids=["slotted", "exact"])
def test_regular_blocks(ctx, grid, exact):
    """Both ends layouts; the batch's last block ends at the end of the source buffer."""
    blocks, pairs = grid
    src, ext = join(blocks)
    assert len(src) == int(ext[-1])
    check_layout(ctx, src, ext, pairs, exact)
    if not exact:
        assert_parity(ctx, src, ext, expect_all_ok=True)


def near_regular(rng):
    """(name, block): a regular block with one thing changed. Most are not regular any more and
    take the general or the spill path; `slack` stays regular."""
    out = []

    def base(n=34, kl=16, vl=100):
        return regular_fields(rng, n, kl, vl)

    def put(name, fields, **kw):
        out.append((name, raw_block(fields, **kw)))

    for n, kl, vl, where in ((34, 16, 100, (0, 17, 33)), (70, 16, 32, (64,))):
        for i in where:
            for d in (-1, 1):
                f = base(n, kl, vl)
                f[i] = (kl + d, f[i][1], vl, f[i][3])          # the field only: the entry's bytes
                put(f"kl[{i}]{d:+d} n={n}", f)                 # stay, so the next offset is off
                f = base(n, kl, vl)
                f[i] = (kl, f[i][1], vl + d, f[i][3])
                put(f"vl[{i}]{d:+d} n={n}", f)
                f = base(n, kl, vl)                            # the bytes change with the field
                f[i] = (kl + d, rng.bytes(kl + d), vl, f[i][3])
                put(f"key[{i}]{d:+d} n={n}", f)
                f = base(n, kl, vl)
                f[i] = (kl, f[i][1], vl + d, rng.bytes(vl + d))
                put(f"value[{i}]{d:+d} n={n}", f)
    S = 4 + 16 + 100
    offs = [i * S for i in range(34)]
    sw = list(offs)
    sw[5], sw[20] = sw[20], sw[5]
    put("two offsets swapped", base(), offsets=sw)
    put("all offsets equal", base(), offsets=[offs[7]] * 34)
    f = base()
    f[12] = (16, f[12][1], 100, f[12][3] + b"\x00")            # a byte no entry covers
    hole = [i * S + (i > 12) for i in range(34)]
    put("a 1-byte hole", f, offsets=hole)
    put("KL = 15", base(kl=15))
    put("VL = 15", base(vl=15))
    put("VL = 0", base(vl=0))
    put("KL = 0", [(0, b"", 100, rng.bytes(100)) for _ in range(34)])
    f = base()
    f[33] = (16, f[33][1], 101, f[33][3])                      # runs past the data: BAD_ENTRY
    put("last vl past the data", f)
    put("slack", base(), slack=9)
    put("flipped payload bit", base(), flip=8 * (2 + 2 * 34 + 20 * S + 30) + 3)
    put("bad tag", base(), tag=7)
    return out


def test_near_regular_blocks(ctx):
    rng = np.random.default_rng(42)
    cases = near_regular(rng)
    blocks = []
    for _, blk in cases:                       # a regular block on either side of each
        blocks += [regular_block(rng, 34, 16, 100)[0], blk]
    blocks.append(regular_block(rng, 5, 48, 17)[0])
    src, ext = join(blocks)
    g, o = assert_parity(ctx, src, ext)
    at = {name: 2 * i + 1 for i, (name, _) in enumerate(cases)}
    st = {name: int(o.status[b]) for name, b in at.items()}
    assert st["last vl past the data"] == O.BAD_ENTRY
    assert st["flipped payload bit"] == O.CHECKSUM and int(g.count[at["flipped payload bit"]]) == 0
    assert st["slack"] == O.OK and st["a 1-byte hole"] == O.OK and st["all offsets equal"] == O.OK
    assert st["bad tag"] not in (O.OK, O.CHECKSUM)
    assert (o.status[0::2] == O.OK).all()


def test_mixed_batch(ctx):
    """20,000 blocks drawn at random from: regular 4k blocks, blocks of short keys (the early
    combine), near-regular blocks, long blocks (handed on) and empty blocks, so that the waves
    cross between the copies with a pending combine in every order; a regular block last."""
    rng = np.random.default_rng(43)
    kinds = []
    kinds.append([regular_block(rng, 34, 16, 100)[0] for _ in range(4)] +
                 [regular_block(rng, 3, 17, 1000)[0], regular_block(rng, 65, 31, 17, slack=3)[0]])
    zipf = []
    for _ in range(4):
        bb = MG.BlockBuilder(4000)
        while bb.add(rng.bytes(int(rng.integers(1, 12))), rng.bytes(int(rng.integers(16, 200)))):
            pass
        zipf.append(MG.encode_block(*bb.build()))
    kinds.append(zipf)
    kinds.append([blk for _, blk in near_regular(rng)[::5]])
    long_ = []
    for _ in range(2):
        bb = MG.BlockBuilder(1 << 16)
        for _ in range(6):
            assert bb.add(rng.bytes(16), rng.bytes(1000))
        long_.append(MG.encode_block(*bb.build()))
    assert min(len(b) for b in long_) > WAVE_MAX_LEN
    kinds.append(long_)
    kinds.append([b""])
    pick = rng.choice(len(kinds), 20000, p=[0.4, 0.25, 0.2, 0.05, 0.1])
    blocks = [kinds[k][int(rng.integers(len(kinds[k])))] for k in pick]
    blocks[-1] = kinds[0][0]
    src, ext = join(blocks)
    assert_parity(ctx, src, ext)


def test_regular_decode_is_deterministic(ctx, grid):
    """The same regular batch decoded twice into buffers pre-filled with different garbage: every
    byte the decode writes (each slot's stream up to its 128-byte line, each block's pairs up to
    their line, status, count, crc) is equal, the key/value gap included."""
    blocks, pairs = grid
    src, ext = join(blocks)
    batch = DeviceBatch(src, ext)
    nb = batch.n_blocks
    cols = SlottedColumns(nb, batch.src_bytes)
    runs = []
    for seed in (1, 2):
        gen = torch.Generator(device=cols.data.device).manual_seed(seed)
        for t in (cols.data, cols.ends, cols.count, cols.status, cols.crc):
            u = t.view(torch.uint8)
            u.copy_(torch.randint(0, 256, u.shape, dtype=torch.uint8, device=u.device, generator=gen))
        decode_batch(ctx, batch, cols).complete()
        runs.append([t.view(torch.uint8).cpu().numpy().reshape(-1).copy()
                     for t in (cols.data, cols.ends, cols.count, cols.status, cols.crc)])
    e = np.asarray(ext[:nb], np.int64)
    idx = np.arange(nb, dtype=np.int64)
    sb, eb = _lib.slot_base(e, idx), _lib.entry_base(e, idx)
    for b in range(nb):
        n, kl, vl = len(pairs[b]), int(pairs[b][0, 0]), int(pairs[b][0, 1])
        tot = _lib.value_start(n * kl) + n * vl
        lo, hi = int(sb[b]), int(sb[b]) + (tot + 127) // 128 * 128
        assert runs[0][0][lo:hi].tobytes() == runs[1][0][lo:hi].tobytes(), ("data", b, n, kl, vl)
        lo, hi = 8 * int(eb[b]), 8 * (int(eb[b]) + (n + 15) // 16 * 16)
        assert runs[0][1][lo:hi].tobytes() == runs[1][1][lo:hi].tobytes(), ("ends", b)
    assert runs[0][2][:4 * nb].tobytes() == runs[1][2][:4 * nb].tobytes()
    assert runs[0][3][:nb].tobytes() == runs[1][3][:nb].tobytes()
    assert runs[0][4][:4 * nb].tobytes() == runs[1][4][:4 * nb].tobytes()
    assert (runs[0][3][:nb] == _lib.BLOCK_OK).all()

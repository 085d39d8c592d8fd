"""One object longer than 2^32 bytes: include/tpz_gpu.h promises CRC ranges and files "up to 2^35
bytes" each, and tpz_verify_files_flat_layout has a branch for data regions of 4 GiB or more
(tpz_flat.hip, op_zshift).

The data is a 64 MiB random shard (a 2^14-block 4k shard for the flat layout) replicated on the
device past 2^32 + 200 MiB. The reference is zlib.crc32 of the shard and of the partial copies,
combined with tests/_crc_combine.py (pinned to zlib by tests/test_crc_combine.py): no host ever
holds the 4 GiB. Bar: bit-exact CRC and status for every range and file, and every row of the
flat layout's d_first equal to the shard's per-block oracle numbers, copy after copy.
"""
import struct
import zlib

import numpy as np
import pytest
import torch

import _oracle as O
from _crc_combine import crc32_of_segments, periodic_segments
from bench import replicate_on_device, replicate_plan
from topazdb_amd import _lib, synth
from topazdb_amd.batch import DeviceBatch, crc32_ranges, flat_layout, open_flat_layout, verify_files

pytestmark = pytest.mark.gpu

S = 64 << 20                          # the shard
T = (1 << 32) + (200 << 20)           # the long object
TOTAL = T + (1 << 32) + 100           # a second range of exactly 2^32 bytes and a short one after


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big():
    """(shard bytes, device buffer): the shard repeated from offset 0 over TOTAL + 16 bytes."""
    free, _ = torch.cuda.mem_get_info()
    assert free > TOTAL + (2 << 30), f"{free >> 20} MiB free on the device"
    dev = torch.device("cuda", 0)
    shard = np.frombuffer(np.random.default_rng(2032).bytes(S), np.uint8)
    d_shard = torch.from_numpy(shard.copy()).to(dev)
    buf = torch.empty(TOTAL + 16, dtype=torch.uint8, device=dev)
    full = buf.numel() // S
    buf[:full * S].view(full, S).copy_(d_shard.expand(full, S))
    buf[full * S:].copy_(d_shard[:buf.numel() - full * S])
    yield shard.tobytes(), buf
    del buf
    torch.cuda.empty_cache()


def want_crc(shard: bytes, start: int, length: int) -> int:
    return crc32_of_segments(periodic_segments(shard, start, length))


def test_crc32_ranges_past_4_gib(ctx, big):
    """Three ranges: 2^32 + 200 MiB - 7 bytes from offset 7, then exactly 2^32 bytes, then 100."""
    shard, buf = big
    ext = [7, T, T + (1 << 32), T + (1 << 32) + 100]
    assert ext[1] - ext[0] == (1 << 32) + (200 << 20) - 7 and ext[-1] == TOTAL
    crc = crc32_ranges(ctx, DeviceBatch(buf, np.asarray(ext, np.uint64)))
    torch.cuda.synchronize()
    got = crc[:3].cpu().numpy().view(np.uint32).tolist()
    want = [want_crc(shard, ext[i], ext[i + 1] - ext[i]) for i in range(3)]
    assert got == want, ([hex(x) for x in got], [hex(x) for x in want])
    # the reference's own check: the short range through zlib directly
    ph = ext[2] % S
    assert want[2] == zlib.crc32((shard + shard)[ph:ph + 100])


def test_verify_file_past_4_gib(ctx, big):
    """One file of T bytes with its big-endian trailer: OK and the combined CRC; the same file
    with one byte flipped at offset 2^32 + 12345: CHECKSUM_MISMATCH and the CRC of the modified
    bytes."""
    shard, buf = big
    body = T - 4
    saved = buf[body:T].clone()
    flip = (1 << 32) + 12345
    try:
        crc_body = want_crc(shard, 0, body)
        trailer = bytearray(struct.pack(">I", crc_body))
        buf[body:T] = torch.frombuffer(trailer, dtype=torch.uint8).to(buf.device)
        batch = DeviceBatch(buf, np.asarray([0, T], np.uint64))
        crc, st = verify_files(ctx, batch)
        torch.cuda.synchronize()
        assert int(crc.cpu().numpy().view(np.uint32)[0]) == crc_body
        assert int(st.cpu()[0]) == _lib.BLOCK_OK
        buf[flip] ^= 0x10
        crc, st = verify_files(ctx, batch)
        torch.cuda.synchronize()
        byte = bytes([shard[flip % S] ^ 0x10])
        segs = periodic_segments(shard, 0, flip) + [(byte, 1)] + \
            periodic_segments(shard, flip + 1, body - flip - 1)
        want = crc32_of_segments(segs)
        assert want != crc_body
        assert int(crc.cpu().numpy().view(np.uint32)[0]) == want
        assert int(st.cpu()[0]) == _lib.BLOCK_CHECKSUM_MISMATCH
    finally:
        buf[flip] = int(shard[flip % S])
        buf[body:T] = saved


def test_open_flat_layout_data_region_past_4_gib(ctx):
    """tpz_verify_files_flat_layout over a file whose data region is a 2^14-block 4k shard
    replicated past 2^32 + 100 MiB (the shift of a block's CRC to the end of a data region of
    4 GiB or more) plus a 4 KiB tail with the right trailer, and a small second file after it."""
    dev = torch.device("cuda", 0)
    nb = 1 << 14
    src, ext = synth.make_region("4k", nb)
    src = np.ascontiguousarray(src[:int(ext[nb])])
    ext = np.ascontiguousarray(ext[:nb + 1], np.uint64)
    shard_bytes = int(ext[-1])
    full, part = replicate_plan(shard_bytes, nb, (1 << 32) + (100 << 20) + shard_bytes)
    assert part >= 128
    blocks, ext_all = replicate_on_device(src, ext, full, part, dev)
    n_all = blocks.n_blocks
    small = 40                                   # blocks of the second file
    cut = n_all - small
    data0 = int(ext_all[cut])
    assert data0 >= (1 << 32) + (100 << 20)
    rng = np.random.default_rng(8)
    shard = src.tobytes()
    tail0 = rng.bytes(4092)
    crc0 = crc32_of_segments(periodic_segments(shard, 0, data0) + [(tail0, 1)])
    lo1 = data0 % shard_bytes
    body1 = shard[lo1:lo1 + int(ext_all[-1]) - data0]
    assert len(body1) == int(ext_all[-1]) - data0        # the second file does not wrap the shard
    tail1 = rng.bytes(33)
    crc1 = zlib.crc32(tail1, zlib.crc32(body1))
    tails = b"\x33" * 7 + tail0 + struct.pack(">I", crc0) + tail1 + struct.pack(">I", crc1 ^ 1)
    text = [7, 7 + 4096, 7 + 4096 + 37]
    tb = DeviceBatch(np.frombuffer(tails, np.uint8), np.asarray(text, np.uint64))
    d_fb = torch.tensor(np.asarray([0, cut, n_all], np.int32), device=dev)
    crc, st, first = open_flat_layout(ctx, blocks, d_fb, tb)
    torch.cuda.synchronize()
    assert crc[:2].cpu().numpy().view(np.uint32).tolist() == [crc0, crc1]
    assert st[:2].cpu().tolist() == [_lib.BLOCK_OK, _lib.BLOCK_CHECKSUM_MISMATCH]
    # every row of d_first: copies x the shard's per-block oracle numbers
    o = O.decode_batch(src, ext)
    assert (o.status == O.OK).all()
    eb = o.entry_base
    per = np.stack([o.count.astype(np.int64),
                    np.add.reduceat(o.klen.astype(np.int64), eb[:-1]),
                    np.add.reduceat(o.vlen.astype(np.int64), eb[:-1])])
    reps = np.concatenate([np.tile(per, full), per[:, :part]], axis=1)
    want = np.zeros((3, n_all + 1), np.int64)
    np.cumsum(reps, axis=1, out=want[:, 1:])
    got = first.cpu().numpy()
    cross = int(np.searchsorted(ext_all, np.uint64(1 << 32), side="right")) - 1
    assert 0 < cross < cut and int(ext_all[cross]) < (1 << 32) < int(ext_all[cross + 1])
    np.testing.assert_array_equal(got[:, cross - 2:cross + 34], want[:, cross - 2:cross + 34])
    np.testing.assert_array_equal(got, want)
    assert got[:, -1].tolist() == (per.sum(axis=1) * full + per[:, :part].sum(axis=1)).tolist()
    # and tpz_flat_layout alone over the same batch
    ref = flat_layout(ctx, blocks)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ref.cpu().numpy(), want)
    del blocks, first, ref
    torch.cuda.empty_cache()

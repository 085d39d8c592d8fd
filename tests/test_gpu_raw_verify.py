"""tpz_raw_verify (Block::decode's checks ahead of the entries: the tag dispatch, the CRC over the
payload, n and the n offsets readable) against tpz_decode_blocks over one batch that holds every
status the decode knows. d_status equals the decode's with OK_SPILLED and BAD_ENTRY read as OK;
d_crc equals the decode's for every block."""
import struct

import numpy as np
import pytest
import torch

import _oracle as O
import _raw_model as R
import badentry_util as U
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, decode_batch

pytestmark = pytest.mark.gpu


def ents(n, tag=b"k", vlen=6):
    return [(b"%s%04d" % (tag, i), bytes([65 + i % 26]) * vlen) for i in range(n)]


def crc_block(payload: bytes, tag: int = 1) -> bytes:
    return payload + struct.pack(">I", U.MG.crc32(payload)) + bytes([tag])


def batch_blocks():
    """(name, block bytes, the status tpz_raw_verify owes it) for every case of the docstring."""
    ok = U.raw_block(*U.entries_block(ents(9)))
    offs, data = U.entries_block(ents(12, b"s"))
    spilled = U.raw_block([o for o in offs for _ in range(5)], bytes(data))     # 6n > len
    flipped = bytearray(ok)
    flipped[11] ^= 0x04
    L = _lib
    return [
        ("ok", ok, L.BLOCK_OK),
        ("empty", b"", L.BLOCK_EMPTY),
        ("tag0", ok[:-1] + b"\x00", L.BLOCK_BAD_TAG),
        ("tag7", ok[:-1] + b"\x07", L.BLOCK_BAD_TAG),
        ("tag2", ok[:-1] + b"\x02", L.BLOCK_UNSUPPORTED_CODEC),
        ("tag3", ok[:-1] + b"\x03", L.BLOCK_UNSUPPORTED_CODEC),
        ("crc", bytes(flipped), L.BLOCK_CHECKSUM_MISMATCH),
        ("len1", b"\x01", L.BLOCK_MALFORMED),                 # block.rs:49: no room for the CRC
        ("len4", b"\x00\x00\x00\x01", L.BLOCK_MALFORMED),
        ("len5_crc_ok", crc_block(b""), L.BLOCK_MALFORMED),   # :54: get_u16 on an empty payload
        ("len5_crc_bad", b"\x00\x00\x00\x09\x01", L.BLOCK_CHECKSUM_MISMATCH),
        ("len6", crc_block(b"\x00"), L.BLOCK_MALFORMED),      # :54: one payload byte
        ("len7_n0", crc_block(b"\x00\x00"), L.BLOCK_OK),      # n = 0, no data
        ("len7_n1", crc_block(b"\x00\x01"), L.BLOCK_MALFORMED),   # :56-59: the offset is missing
        ("len8_n0", crc_block(b"\x00\x00\x5a"), L.BLOCK_OK),
        ("len8_n1", crc_block(b"\x00\x01\x00"), L.BLOCK_MALFORMED),   # half an offset
        ("n_too_big", crc_block(struct.pack(">H", 400) + ok[2:-5]), L.BLOCK_MALFORMED),
        ("n0", U.raw_block([], b""), L.BLOCK_OK),
        ("offsets_fill_payload", U.raw_block([0, 0, 0], b""), L.BLOCK_OK),   # all entries BAD_KEY
        ("bad_entry_key", U.bad_block(ents(7, b"b"), 3, "key_off"), L.BLOCK_OK),
        ("bad_entry_value", U.bad_block(ents(7, b"v"), 6, "value"), L.BLOCK_OK),
        ("spilled", spilled, L.BLOCK_OK),
        ("ok_last", U.raw_block(*U.entries_block(ents(30, b"z", 40))), L.BLOCK_OK),
    ]


def test_every_status(ctx):
    cases = batch_blocks()
    names = [c[0] for c in cases]
    blocks = [c[1] for c in cases]
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    region = b"".join(blocks)
    # from the inputs: the rule's model gives every named status, the oracle sees the bad
    # entries, the spilled block cannot fit its slot, and blocks start at odd offsets
    for name, blk, want in cases:
        assert R.verify(blk)[0] == want, name
    o = O.decode_batch(np.frombuffer(region, np.uint8), ext)
    for name in ("offsets_fill_payload", "bad_entry_key", "bad_entry_value"):
        assert int(o.status[names.index(name)]) == O.BAD_ENTRY, name
    sp = blocks[names.index("spilled")]
    assert 6 * R.be16(sp, 0) > len(sp)
    assert {len(b) for b in blocks} >= {0, 1, 4, 5, 6, 7, 8}
    assert sum(int(e) % 2 for e in ext[:-1]) >= 5

    dev = torch.device("cuda", ctx.device)
    batch = DeviceBatch(np.frombuffer(region, np.uint8), ext, ctx.device)
    cols = decode_batch(ctx, batch).complete()
    torch.cuda.synchronize()
    nb = len(blocks)
    dec_st = cols.status[:nb].cpu().numpy()
    dec_crc = cols.crc[:nb].cpu().numpy().view(np.uint32)
    assert int(dec_st[names.index("spilled")]) == _lib.BLOCK_OK_SPILLED
    assert int(dec_st[names.index("bad_entry_key")]) == _lib.BLOCK_BAD_ENTRY
    assert {int(s) for s in dec_st} == {
        _lib.BLOCK_OK, _lib.BLOCK_EMPTY, _lib.BLOCK_BAD_TAG, _lib.BLOCK_UNSUPPORTED_CODEC,
        _lib.BLOCK_CHECKSUM_MISMATCH, _lib.BLOCK_MALFORMED, _lib.BLOCK_OK_SPILLED,
        _lib.BLOCK_BAD_ENTRY}

    st = torch.full((nb + 1,), 0x5A, dtype=torch.uint8, device=dev)
    crc = torch.full((nb + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ctx.raw_verify_ptrs(batch.src.data_ptr(), batch.ext.data_ptr(), nb, batch.src_bytes,
                        st.data_ptr(), crc.data_ptr(),
                        torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got_st = st.cpu().numpy()
    got_crc = crc.cpu().numpy().view(np.uint32)
    want_st = np.where(np.isin(dec_st, (_lib.BLOCK_OK_SPILLED, _lib.BLOCK_BAD_ENTRY)),
                       _lib.BLOCK_OK, dec_st)
    for i, name in enumerate(names):
        assert int(got_st[i]) == int(want_st[i]) == cases[i][2], (name, got_st[i], want_st[i])
        assert int(got_crc[i]) == int(dec_crc[i]), (name, got_crc[i], dec_crc[i])
        assert int(got_crc[i]) == R.verify(blocks[i])[1], name
    assert int(got_st[nb]) == 0x5A and int(got_crc[nb]) == 0x5A5A5A5A     # nothing past the batch


def test_unaligned_source_and_no_blocks(ctx):
    """d_src at any byte address (the blocks of an image inside an arena), and an empty batch."""
    dev = torch.device("cuda", ctx.device)
    blocks = [c[1] for c in batch_blocks()]
    ext = np.zeros(len(blocks) + 1, np.int64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    region = np.frombuffer(b"".join(blocks), np.uint8)
    nb = len(blocks)
    arena = torch.zeros(region.size + 64, dtype=torch.uint8, device=dev)
    d_ext = torch.from_numpy(ext).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    want = [R.verify(b) for b in blocks]
    for shift in (1, 7, 13):
        arena[shift:shift + region.size].copy_(torch.from_numpy(region.copy()))
        st = torch.zeros(nb, dtype=torch.uint8, device=dev)
        crc = torch.zeros(nb, dtype=torch.int32, device=dev)
        ctx.raw_verify_ptrs(arena.data_ptr() + shift, d_ext.data_ptr(), nb, int(ext[-1]),
                            st.data_ptr(), crc.data_ptr(), stream)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [w[0] for w in want], shift
        assert crc.cpu().numpy().view(np.uint32).tolist() == [w[1] for w in want], shift
    st = torch.full((2,), 0x5A, dtype=torch.uint8, device=dev)
    ctx.raw_verify_ptrs(0, 0, 0, 0, st.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0x5A, 0x5A]

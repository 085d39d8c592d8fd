"""tests/_raw_model.py (the in-place view the device computes from a block's bytes, and
tpz_raw_verify's rule) pinned against the oracle's decode: every block of the golden SSTs, the
bad-entry fixtures, and random blocks with permuted, repeated, overlapping and out-of-range
offsets. Keys, values and entry classes entry by entry; the verify rule against the oracle's block
status with BAD_ENTRY read as OK. No GPU needed."""
import glob
import os
import random
import struct

import numpy as np
import pytest

import _get_model as M
import _oracle as O
import _raw_model as R
import badentry_util as U
from test_bad_entry import TABLES
from topazdb_amd import _lib

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.sst")))


def check_blocks(region: bytes, ext) -> dict:
    """Every block of the batch against the oracle; returns the statuses and classes seen."""
    ext = np.asarray(ext, np.uint64)
    d = O.decode_batch(np.frombuffer(region, np.uint8) if region else np.zeros(0, np.uint8), ext)
    seen = {"status": set(), "cls": set()}
    for b in range(len(ext) - 1):
        blk = region[int(ext[b]):int(ext[b + 1])]
        st, crc = R.verify(bytes(blk))
        want = int(d.status[b])
        if blk and blk[-1] in (2, 3):      # the oracle runs the codec; tpz_raw_verify, like
            want = _lib.BLOCK_UNSUPPORTED_CODEC   # tpz_decode_blocks, is given its output instead
        seen["status"].add(want)
        assert st == (_lib.BLOCK_OK if want == O.BAD_ENTRY else want), (b, st, want)
        if st in (_lib.BLOCK_OK, _lib.BLOCK_CHECKSUM_MISMATCH) or (st == _lib.BLOCK_MALFORMED and crc):
            assert crc == int(d.crc_actual[b]), b
        if st != _lib.BLOCK_OK:
            continue
        v = R.RawView(bytes(blk))
        ents = d.entries(b)
        assert v.n == len(ents) == int(d.count[b]), b
        e0 = int(d.entry_base[b])
        for j, (k, val) in enumerate(ents):
            cls = int(d.cls[e0 + j])
            seen["cls"].add(cls)
            assert v.entry_class(j) == cls, (b, j)
            assert v.key_panics(j) == (cls == R.BAD_KEY) and v.seek_panics(j) == (cls != R.OK)
            assert v.entry_key(j) == k and v.entry_value(j) == val, (b, j)
    return seen


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_ssts(path):
    p = M.Pieces.from_image(open(path, "rb").read())
    # snappy and lz4 blocks: the view reads the codec step's output (the Uncompress form)
    out, ext = bytearray(), [0]
    for b in range(len(p.ext) - 1):
        st, blk = O.decompress_block(p.region[int(p.ext[b]):int(p.ext[b + 1])])
        assert st == O.OK
        out += blk
        ext.append(len(out))
    seen = check_blocks(bytes(out), ext)
    assert seen["status"] == {O.OK} and seen["cls"] == {R.OK}


@pytest.mark.parametrize("name,spec", TABLES, ids=[t[0] for t in TABLES])
def test_bad_entry_fixtures(name, spec):
    f, _ = U.table(spec)
    p = M.Pieces.from_image(f)
    seen = check_blocks(p.region, p.ext)
    assert O.BAD_ENTRY in seen["status"]
    assert seen["cls"] & {R.BAD_KEY, R.BAD_VALUE}


def random_block(rng: random.Random) -> bytes:
    """A CRC-valid block over BlockBuilder's data whose offsets are then permuted, repeated, made
    to overlap (pointing inside entries) or moved out of range; sometimes the header lies."""
    m = rng.randint(0, 12)
    ents = [(bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 6))),
             bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 9)))) for _ in range(m)]
    offs, data = U.entries_block(ents)
    data = bytes(data)
    mode = rng.randrange(6)
    if mode == 1:
        rng.shuffle(offs)
    elif mode == 2 and offs:
        offs = [rng.choice(offs) for _ in range(rng.randint(1, 20))]
    elif mode == 3:
        offs = [rng.randint(0, max(len(data) - 1, 0)) for _ in range(rng.randint(1, 16))]
    elif mode == 4:
        offs = [rng.choice([len(data), len(data) - 1, len(data) + 1, len(data) - 2, 0xFFFF,
                            rng.randint(0, len(data) + 4)]) & 0xFFFF
                for _ in range(rng.randint(1, 16))]
    elif mode == 5:
        data = data[:rng.randint(0, len(data))]                    # entries cut short
    blk = U.raw_block(offs, data)
    flip = rng.randrange(12)
    if flip == 0:                                                  # n larger than the payload holds
        p = struct.pack(">H", len(offs) + rng.randint(1, 300)) + blk[2:-5]
        blk = p + struct.pack(">I", U.MG.crc32(p)) + b"\x01"
    elif flip == 1:
        blk = blk[:-1] + bytes([rng.choice([0, 2, 3, 4, 255])])
    elif flip == 2 and len(blk) > 6:
        i = rng.randrange(len(blk) - 1)
        blk = blk[:i] + bytes([blk[i] ^ 0x10]) + blk[i + 1:]
    elif flip == 3:
        blk = blk[len(blk) - rng.randint(0, 6):]                   # 0 .. 6 bytes, tag kept
    return blk


def test_random_blocks():
    rng = random.Random(20250)
    blocks = [random_block(rng) for _ in range(400)]
    ext = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum([len(b) for b in blocks], out=ext[1:])
    seen = check_blocks(b"".join(blocks), ext)
    assert {O.OK, O.BAD_ENTRY, _lib.BLOCK_MALFORMED, _lib.BLOCK_CHECKSUM_MISMATCH,
            _lib.BLOCK_BAD_TAG, _lib.BLOCK_UNSUPPORTED_CODEC} <= seen["status"]
    assert seen["cls"] == {R.OK, R.BAD_VALUE, R.BAD_KEY}

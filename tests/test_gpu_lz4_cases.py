"""The device LZ4 decoders on sequence programs no compressor here emits: the programs of
tests/_lz4_cases.py (matches of many ring steps at every offset class, literal and match lengths
on the continuation-byte edges and far past them, every ordered pair of length classes, prefixes
larger than the decoded length) through each LZ4 parser of tpz_codec.hip.

Reference: compress::decode -> lz4::block::decompress(data, None) (src/block/compress.rs:108-111),
stated by the generator itself (no decoder builds the expected bytes; test_lz4_cases.py pins
liblz4 and both CPU restatements against it). Bar: bit for bit. A valid block gives BLOCK_OK and
the generator's bytes + tag 1, an invalid one BLOCK_CODEC_ERROR, nothing is written past
dst_ext[n], and both neighbours of every invalid block are valid blocks that stay intact.

Routes (tpz_codec.hip): ring_body<3> takes the tag-3 blocks of a batch whose source and output are
below 0x7FFFFFF0 and at least 16 bytes, and hands a block to codec_lane_kernel (lz4_walk over
lane_lit / lane_match) when a header field outruns its 16-byte window or a rule fails; with a
source span of 0x7FFFFFF0 bytes or more (passed honestly: one big allocation, the batch at its
start) the ring is not live and every tag-3 block is the lane kernel's. The wave-side decoders
(Lz4WaveOut in the LDS windows, Lz4GlobalOut past them) see a stream only in a batch of fewer
than 16 bytes, or after it failed under a claimed size."""
import random

import numpy as np
import pytest
import torch

import _lz4_cases as Z4
import _oracle as O
import _snappy_cases as S
from test_gpu_decode import ctx  # noqa: F401 (fixture)
from test_gpu_snappy import batch_of, device_codec
from test_gpu_snappy_cases import BIG_SRC, CANARY, big_src, run_codec  # noqa: F401 (fixture)
from topazdb_amd import _lib

pytestmark = pytest.mark.gpu

LIMITS = (0,) + Z4.RAISES


def valid_items(raises=LIMITS):
    """[(name, block, expected bytes)] of every valid case under each of the prefixes."""
    return [(f"{c.name}+{r}", Z4.block_of(c, r), c.out + b"\x01")
            for c in Z4.valid_cases() for r in raises]


def mixed_batch():
    """Every valid program under its own prefix and the raised ones, shuffled, with the named
    invalid blocks spread among them (each between two valid blocks):
    [(name, block, expected bytes or None)]."""
    valid = valid_items()
    random.Random(11).shuffle(valid)
    bad = [(b.name, b.block, None) for b in Z4.invalid_cases()]
    step = len(valid) // (len(bad) + 1)
    assert step >= 2
    items = []
    for i, v in enumerate(valid):
        items.append(v)
        if i % step == step - 1 and i // step < len(bad):
            items.append(bad[i // step])
    assert len(items) == len(valid) + len(bad)
    return items


def check_items(items, outs, st, oext=None):
    for i, ((name, _b, want), o, s) in enumerate(zip(items, outs, st)):
        if want is None:
            assert s == _lib.BLOCK_CODEC_ERROR, (i, name, s)
        else:
            assert s == _lib.BLOCK_OK, (i, name, s)
            assert o == want, (i, name)
    for i, it in enumerate(items):             # an invalid block's neighbours are valid blocks
        if it[2] is None:
            assert items[i - 1][2] is not None and items[i + 1][2] is not None
    if oext is not None:
        # exact sizes: the program's length + 1 (not the prefix's), 1 for an invalid tag-3 block
        sizes = np.diff(oext)
        for i, (name, _b, want) in enumerate(items):
            assert sizes[i] == (1 if want is None else len(want)), (i, name, sizes[i])


def place(big, blocks):
    """The batch at the start of the big allocation, CANARY in the MiB after it."""
    data, ext = batch_of(blocks)
    n_bytes = int(ext[-1])
    big[:n_bytes].copy_(torch.from_numpy(np.ascontiguousarray(data).copy()))
    big[n_bytes:n_bytes + (1 << 20)].fill_(CANARY)


@pytest.fixture(scope="module")
def ring_result(ctx):
    """The mixed batch through a batch-sized source."""
    items = mixed_batch()
    outs, st, _ext, oext = run_codec(ctx, [b for _n, b, _w in items])
    return items, outs, st, oext


def test_ring_route(ctx, ring_result):
    """One batch of all valid programs (each under four prefixes) and the named invalid blocks
    among them, batch-sized source: statuses, every output byte, the exact sizes (the program's
    length + 1 under a raised prefix too, 1 for an invalid block), every valid neighbour of an
    invalid block intact, nothing written past dst_ext[n] (run_codec's canary). Then the valid
    set under claimed sizes, each case at its own prefix (a raised prefix is no exact claim):
    the check passes and the bytes are the same. Last, a block one byte short of its claim
    between two exact ones: CODEC_ERROR with a 0 tag for it under the claim, the check fails."""
    items, outs, st, oext = ring_result
    assert sum(w is None for _n, _b, w in items) == len(Z4.invalid_cases())
    check_items(items, outs, st, oext)
    own = valid_items((0,))
    random.Random(12).shuffle(own)
    outs, st, _ext, oext = run_codec(ctx, [b for _n, b, _w in own], claimed=True)
    check_items(own, outs, st, oext)
    a, b, c = Z4.valid_cases()[5], Z4.valid_cases()[40], Z4.valid_cases()[90]
    blocks = [Z4.block_of(a), Z4.block_of(b, 1), Z4.block_of(c)]
    outs, st, _ext, _oext = run_codec(ctx, blocks, claimed=True, check=False)
    assert list(st) == [_lib.BLOCK_OK, _lib.BLOCK_CODEC_ERROR, _lib.BLOCK_OK]
    assert outs[0] == a.out + b"\x01" and outs[2] == c.out + b"\x01"
    assert len(outs[1]) == len(b.out) + 2 and outs[1][-1] == 0


def test_lane_route(ctx, big_src, ring_result):
    """The same batch with the ring not live (a source span of 0x7FFFFFF0 bytes and more): every
    tag-3 block is codec_lane_kernel's, lz4_walk over lane_lit / lane_match clipped by `room`.
    Against the generator, and equal to the ring route's result."""
    items, ring_outs, ring_st, ring_oext = ring_result
    blocks = [b for _n, b, _w in items]
    place(big_src, blocks)
    outs, st, _ext, oext = run_codec(ctx, blocks, src=big_src, src_bytes=BIG_SRC)
    check_items(items, outs, st, oext)
    np.testing.assert_array_equal(st, ring_st)
    np.testing.assert_array_equal(oext, ring_oext)
    for (name, _b, want), o, ro in zip(items, outs, ring_outs):
        if want is not None:
            assert o == ro, name


def probe_programs():
    rng = random.Random(0x4C10)
    probes = [
        ("literal_first", [(7, 3, 4), (3, 9, 6), (1, 2, 5)], 12),
        ("match_heavy", [(4, 1, 4), (0, 2, 7), (0, 5, 11), (0, 19, 64), (0, 7, 64), (0, 16, 33),
                         (0, 63, 8), (0, 64, 64), (0, 1, 4)], 8),
        ("off3_300", [(5, 3, 300), (0, 3, 70)], 6),
        ("off7_300", [(9, 7, 300), (2, 7, 129)], 5),
        ("off33_300", [(40, 33, 300), (1, 33, 65)], 13),
        ("off121", [(130, 121, 200), (3, 121, 70)], 5),
        ("off150", [(160, 150, 200), (0, 150, 151)], 6),
        ("off192", [(200, 192, 150), (15, 192, 193)], 5),
        ("literal_270_between", [(6, 4, 20), (270, 100, 30), (0, 8, 19)], 5),
    ]
    cases = [Z4.case(name, prog, final, rng) for name, prog, final in probes]
    for i in range(2):
        prog = []
        for _ in range(24):
            prog.append(Z4.rand_sequence(rng, Z4.produced(prog)))
        cases.append(Z4.case(f"random_{i}", prog, Z4.final_for(rng, prog), rng))
    return cases


def test_alignment(ctx):
    """Eleven probe programs (literal-first, match-heavy, 300-byte matches at offsets 3, 7 and 33,
    matches at offsets 121, 150 and 192 around the ring's lower edge, a 270-byte literal between
    two matches, random ones), each at all 64 values of its output start mod 64 times all 16
    values of its source start mod 16: the ring's lines, slots and funnels, the period carried
    from step to step, the header window and the sizes pass's 128-byte window at every alignment.
    A small LZ4 block whose output is n bytes (mod 16) longer than its source sets the skew
    between the two positions, a tag-1 pad block of 1..64 bytes (copied unchanged) the output
    start. The sizes pass is checked at every placement (run_codec sizes the output with it)."""
    rng = random.Random(0x4C11)
    probes = probe_programs()
    assert len(probes) >= 8
    # (1 literal, a match of m bytes at offset 1, 5 literals): the output is m - 8 bytes longer
    # than the source while m - 4 fits the token, m - 9 with one continuation byte
    shifters = {}
    for m in list(range(8, 19)) + list(range(20, 25)):
        c = Z4.case(f"shift_{m}", [(1, 1, m)], 5, rng)
        blk = Z4.block_of(c)
        shifters[(len(c.out) + 1 - len(blk)) % 16] = (c, blk)
    assert sorted(shifters) == list(range(16))
    items, where = [], []
    s_pos = d_pos = 0
    for pi, pr in enumerate(probes):
        for ro in range(64):
            for rs in range(16):
                sh, blk = shifters[(ro - rs - d_pos + s_pos) % 16]
                pad = (ro - d_pos - (len(sh.out) + 1) - 1) % 64 + 1
                padb = rng.randbytes(pad - 1) + b"\x01"
                items += [(sh.name, blk, sh.out + b"\x01"), ("pad", padb, padb)]
                s_pos += len(blk) + pad
                d_pos += len(sh.out) + 1 + pad
                assert d_pos % 64 == ro and s_pos % 16 == rs
                where.append((pi, len(items)))
                items.append((pr.name, Z4.block_of(pr), pr.out + b"\x01"))
                s_pos += len(pr.stream) + 5
                d_pos += len(pr.out) + 1
    outs, st, ext, oext = run_codec(ctx, [b for _n, b, _w in items])
    sizes = np.diff(oext)
    for i, ((name, _b, want), o, s) in enumerate(zip(items, outs, st)):
        assert sizes[i] == len(want), (i, name, int(ext[i]) % 16)
        assert s == _lib.BLOCK_OK and o == want, (i, name, int(oext[i]) % 64, int(ext[i]) % 16)
    achieved = {(pi, int(oext[i]) % 64, int(ext[i]) % 16) for pi, i in where}
    assert achieved == {(pi, ro, rs) for pi in range(len(probes)) for ro in range(64)
                        for rs in range(16)}


def test_end_of_source(ctx):
    """Batches whose src_bytes is exactly ext[n]: the last block's final literal run is 5..100
    bytes after zero, one or several sequences (the ring's clamped header and literal loads near
    the end of the source), alone and behind two leading blocks, under exact and claimed sizes."""
    rng = random.Random(0x4C12)
    heads = ([], [(30, 30, 12)], [(16, 16, 20), (0, 3, 300), (75, 1, 9)], [(2, 1, 270), (14, 9, 18)])
    lead = [Z4.case(f"lead_{i}", [Z4.rand_sequence(rng, 0), (20, 9, 7)], 6, rng) for i in range(2)]
    n_runs = 0
    for f in (5, 6, 15, 16, 17, 64, 80, 81, 100):
        for head in heads:
            last = Z4.case(f"tail_{f}", head, f, rng)
            for cases in ([last], lead + [last]):
                blocks = [Z4.block_of(c) for c in cases]
                if sum(map(len, blocks)) < 16:
                    continue                            # (tiny batches: test_tiny_batches)
                for claimed in (False, True):
                    outs, st, _ext, _oext = run_codec(ctx, blocks, claimed=claimed)
                    n_runs += 1
                    for c, o, s in zip(cases, outs, st):
                        assert s == _lib.BLOCK_OK and o == c.out + b"\x01", (f, head, claimed, c.name)
    assert n_runs >= 100


def test_tiny_batches(ctx):
    """A batch of one valid block whose source is shorter than 16 bytes, and one whose output is:
    neither the ring nor the lane kernel is live, so these are the only valid LZ4 streams that
    reach codec_wave_kernel (Lz4LdsSrc / Lz4WaveOut), and with a source below 16 bytes the sizes
    pass's lz4_block_length_bytes. Through the pointer calls and through device_codec.

    What a valid stream cannot reach through the ABI today (read from lz4_block and
    codec_lane_block): a source below 16 bytes holds a stream of at most 10 bytes, which decodes
    to at most 24 bytes, and an output below 16 bytes comes from a stream of at most 15 bytes, so
    such a block always fits the 16-wave windows and no match has 64 bytes behind it. The
    `!fits` route of lz4_block (Lz4GlobalOut, match_copy_g) and match_copy_wave's `off >= 64`
    branch therefore run only on a stream that already failed under a claimed size
    (test_failed_streams_under_claims), whose bytes are unspecified."""
    rng = random.Random(0x4C13)
    short_src = Z4.case("short_src", [(1, 1, 18)], 5, rng)
    short_out = Z4.case("short_out", [(2, 2, 7)], 5, rng)
    literal_only = Z4.case("literal_only", [], 14, rng)
    both = Z4.case("short_both", [(1, 1, 7)], 5, rng)
    tiny = Z4.case("five_literals", [], 5, rng)
    n_src = n_out = 0
    for c in (short_src, short_out, literal_only, both, tiny):
        for r in (0, 1, 64):
            blk = Z4.block_of(c, r)
            assert len(blk) < 16 or len(c.out) + 1 < 16
            n_src += len(blk) < 16
            n_out += len(c.out) + 1 < 16
            outs, st, _ext, _oext = run_codec(ctx, [blk])
            assert st[0] == _lib.BLOCK_OK and outs[0] == c.out + b"\x01", (c.name, r)
            outs, st = device_codec(ctx, [blk])
            assert st[0] == _lib.BLOCK_OK and outs[0] == c.out + b"\x01", (c.name, r)
    assert len(Z4.block_of(short_src)) < 16 <= len(short_src.out) + 1
    assert len(short_out.out) + 1 < 16 <= len(Z4.block_of(short_out))
    assert n_src >= 6 and n_out >= 6


def claims_batch():
    """The last-match faults of each size, each between two valid blocks (at their own prefix)."""
    rng = random.Random(14)
    by = Z4.last_match_faults()
    valid = [c for c in Z4.valid_cases() if 100 <= len(c.out) <= 3000]
    items = []
    for size in ("small", "big", "global"):
        assert len(by[size]) >= 3
        for b in by[size]:
            c = rng.choice(valid)
            items += [(c.name, Z4.block_of(c), c.out + b"\x01"), (b.name, b.block, None)]
    c = rng.choice(valid)
    items.append((c.name, Z4.block_of(c), c.out + b"\x01"))
    return items


def check_failed_under_claims(items, outs, st):
    for i, ((name, blk, want), o, s) in enumerate(zip(items, outs, st)):
        if want is None:
            assert s == _lib.BLOCK_CODEC_ERROR, (i, name, s)
            # the whole claimed range is the block's, its last byte decodes as BAD_TAG; the
            # other bytes of a failed range are unspecified
            assert len(o) == int.from_bytes(blk[:4], "little") + 1 and o[-1] == 0, (i, name)
            assert items[i - 1][2] is not None and items[i + 1][2] is not None
        else:
            assert s == _lib.BLOCK_OK and o == want, (i, name)


def test_failed_streams_under_claims(ctx, big_src):
    """Streams that fail at their last match under tpz_decompressed_sizes_claimed, which gives
    each its prefix + 1 bytes: inside the 16-wave windows, inside the one-wave windows only and
    past them (by the compressed length, and by the output alone). The ring and the lane kernel
    leave them to codec_wave_kernel / codec_big_kernel, which decode them again into the LDS
    windows or straight into dst, bounded only by the prefix. Batch-sized and inside the big
    span: CODEC_ERROR, a 0 in the last byte of the range, tpz_decompress_check false, both
    neighbours exact, the canary intact; device_codec's exact redo gives the oracle's status
    for every block."""
    items = claims_batch()
    blocks = [b for _n, b, _w in items]
    outs, st, _ext, _oext = run_codec(ctx, blocks, claimed=True, check=False)
    check_failed_under_claims(items, outs, st)
    place(big_src, blocks)
    outs, st, _ext, _oext = run_codec(ctx, blocks, src=big_src, src_bytes=BIG_SRC, claimed=True,
                                      check=False)
    check_failed_under_claims(items, outs, st)
    outs, st = device_codec(ctx, blocks)
    for (name, blk, _w), o, s in zip(items, outs, st):
        ost, ob = O.decompress_block(blk)
        assert s == ost, (name, s, ost)
        if ost == O.OK:
            assert o == ob, name


def test_offset_zero(ctx, big_src):
    """Offset-0 matches (zeros for liblz4 as the oracle restates it; the ring leaves them to the
    lane kernel's lane_match): the oracle's status and bytes, on both routes."""
    rng = random.Random(15)
    valid = [c for c in Z4.valid_cases() if 100 <= len(c.out) <= 3000]
    blocks, want = [], []
    for _name, blk in list(Z4.offset_zero_cases()) + [(None, None)]:
        c = rng.choice(valid)                       # the neighbours: the generator's bytes
        blocks.append(Z4.block_of(c))
        want.append((O.OK, c.out + b"\x01"))
        if blk is not None:
            blocks.append(blk)
            want.append(O.decompress_block(blk))
    place(big_src, blocks)
    for kw in ({}, {"src": big_src, "src_bytes": BIG_SRC}):
        outs, st, _ext, _oext = run_codec(ctx, blocks, **kw)
        for i, ((ost, ob), o, s) in enumerate(zip(want, outs, st)):
            assert s == ost, (i, s, ost)
            assert o == (ob if ost == O.OK else b"\x00"), i


def test_mixed_codecs(ctx):
    """The valid LZ4 cases interleaved with the snappy element programs and raw tag-1 blocks in
    one batch: the LZ4 ring runs over the marks the snappy ring left, and both share lines."""
    rng = random.Random(16)
    lz = valid_items((0, 11))
    sn = [(c.name, c.stream + b"\x02", c.out + b"\x01") for c in S.valid_cases()]
    raw = []
    for i in range(400):
        b = rng.randbytes(rng.randint(0, 200)) + b"\x01"
        raw.append((f"raw_{i}", b, b))
    items = lz + sn + raw
    rng.shuffle(items)
    kinds = [b[-1] for _n, b, _w in items]
    assert sum(kinds[i] != kinds[i + 1] for i in range(len(kinds) - 1)) > len(items) // 3
    outs, st, _ext, _oext = run_codec(ctx, [b for _n, b, _w in items])
    for i, ((name, _b, want), o, s) in enumerate(zip(items, outs, st)):
        assert s == _lib.BLOCK_OK and o == want, (i, name)

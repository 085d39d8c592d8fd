"""tpz_compress_blocks at the edges of its formats, of its 4,352-byte staging window and of its
per-wave hash table (the families of _compress_cases.py), both codecs throughout.

The encoders' bytes cannot be pinned against snap or liblz4 (test_gpu_compress.py), so every
family is held to the same gates instead: the raw call writes nothing outside an exactly sized
d_dst / d_dst_ext (canaries on both sides); every block decodes through the oracle
(test_gpu_compress.check_round_trip) and through the auditors of _codec_audit.py to its payload;
the streams keep the rules tpz_compress.hip states about itself and, for LZ4, the end rules
tpz_gpu.h promises (no decoder enforces the 12-byte one); and the device's own codec step reads
back exactly the source. On top of that each family pins what it was built for: which side of
kCMaxStaged compresses, the literal header widths, the element classes the emit branches produce,
the encoded size of periodic data (a finder that stopped finding would pass every round trip)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _codec_audit as A
import _compress_cases as CC
import _oracle as O
from test_gpu_compress import check_round_trip
from test_gpu_decode import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib, synth
from topazdb_amd.batch import DeviceBatch, decode_batch, decompress_batch
from topazdb_amd.encode import compress_bound

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FRONT = 64            # canary bytes before each output (a 16-byte aligned offset)
BACK = 4096           # canary bytes behind it


def raw_compress(ctx, src, ext, codec):
    """tpz_compress_blocks into a d_dst of exactly tpz_layout_compress_bound bytes and a d_dst_ext
    of exactly n + 1 u64, both cut out of canary-filled tensors. Returns (out bytes, out ext)."""
    ext = np.asarray(ext, np.uint64)
    b = DeviceBatch(np.ascontiguousarray(src, np.uint8), ext)
    n = b.n_blocks
    bound = compress_bound(b.src_bytes, n)
    dev = b.src.device
    raw = torch.full((FRONT + bound + BACK,), CANARY, dtype=torch.uint8, device=dev)
    raw_e = torch.full((FRONT + 8 * (n + 1) + BACK,), CANARY, dtype=torch.uint8, device=dev)
    dst, dext = raw[FRONT:FRONT + bound], raw_e[FRONT:FRONT + 8 * (n + 1)]
    assert dst.data_ptr() % 16 == 0 and dext.data_ptr() % 16 == 0 and b.src.data_ptr() % 16 == 0
    bt = _lib.Batch(b.src.data_ptr(), b.ext.data_ptr(), n, b.src_bytes)
    s = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().tpz_compress_blocks(ctx.handle, C.byref(bt), codec,
                                              C.c_void_p(dst.data_ptr()),
                                              C.c_void_p(dext.data_ptr()),
                                              C.c_void_p(s.cuda_stream)), "tpz_compress_blocks")
    torch.cuda.synchronize(dev)
    h, he = raw.cpu().numpy(), raw_e.cpu().numpy()
    for name, a, used in (("d_dst", h, bound), ("d_dst_ext", he, 8 * (n + 1))):
        assert (a[:FRONT] == CANARY).all(), "%s: a store before the buffer" % name
        bad = np.nonzero(a[FRONT + used:] != CANARY)[0]
        assert len(bad) == 0, "%s: a store %d bytes past the buffer's end" % (name, bad[0])
    e = he[FRONT:FRONT + 8 * (n + 1)].view(np.uint64).copy()
    assert int(e[0]) == 0, e[0]
    assert (np.diff(e.astype(np.int64)) >= 0).all(), "d_dst_ext decreases"
    assert int(e[-1]) <= bound, (int(e[-1]), bound)
    return h[FRONT:FRONT + int(e[-1])].copy(), e


def audit_block(enc: bytes, codec: int):
    """(decoded, items) of an encoded block, its tag checked and taken off; LZ4 with the end rules."""
    assert enc[-1] == codec, enc[-1]
    return A.snappy_audit(enc[:-1]) if codec == 2 else A.lz4_audit(enc[:-1], end_rules=True)


def encoded_len(items, n: int, codec: int) -> int:
    """An encoded block's length from its audited elements alone (header, elements, tag)."""
    if codec == 2:
        head = 1
        while n >> (7 * head):
            head += 1
        return head + 1 + sum(1 + e[2] + e[1] if e[0] == "lit" else {"copy1": 2, "copy2": 3}[e[0]]
                              for e in items)
    return 4 + 1 + sum(1 + le + ll + (2 + me if ml else 0) for ll, _off, ml, le, me in items)


def gates(ctx, src, ext, codec):
    """The gates every family passes. Returns ([encoded block], [audited items or None])."""
    out, oext = raw_compress(ctx, src, ext, codec)
    check_round_trip(src, ext, out, oext, codec)
    encs, items, want = [], [], []
    for i in range(len(ext) - 1):
        blk = bytes(src[int(ext[i]):int(ext[i + 1])])
        enc = bytes(out[int(oext[i]):int(oext[i + 1])])
        encs.append(enc)
        if blk and blk[-1] == 1:
            try:
                dec, it = audit_block(enc, codec)
                A.device_rules(it, codec)
            except A.AuditError as err:
                raise AssertionError("block %d (%d bytes): %s" % (i, len(blk), err)) from err
            oracle = O.snappy_decompress(enc[:-1]) if codec == 2 else O.lz4_block_decompress(enc[:-1])
            assert dec == oracle == blk[:-1], i
            assert len(enc) == encoded_len(it, len(blk) - 1, codec), i
            items.append(it)
            want.append(blk)
        else:
            assert enc == blk, i
            items.append(None)
            want.append(O.decompress_block(blk)[1])     # a tag-2 block passed on: its plain form
    # the device reads what it wrote
    b2, st = decompress_batch(ctx, DeviceBatch(out, oext))
    torch.cuda.synchronize()
    assert (st[:len(ext) - 1].cpu().numpy() == _lib.BLOCK_OK).all()
    wext = np.zeros(len(want) + 1, np.uint64)
    np.cumsum([len(w) for w in want], out=wext[1:])
    np.testing.assert_array_equal(b2.ext_host, wext)
    got = b2.src[:int(wext[-1])].cpu().numpy()
    assert got.tobytes() == b"".join(want)
    return encs, items


_RUNS = {}


def run_blocks(ctx, name, blocks, codec):
    """gates() of a family's batch, once per (family, codec) in this module."""
    if (name, codec) not in _RUNS:
        src, ext = CC.batch(blocks)
        _RUNS[name, codec] = gates(ctx, src, ext, codec)
    return _RUNS[name, codec]


def has_match(items, codec) -> bool:
    return any(e[0] != "lit" for e in items) if codec == 2 else len(items) > 1


def one_literal(items, m, codec) -> bool:
    if codec == 2:
        return len(items) == 1 and items[0][:2] == ("lit", m)
    return len(items) == 1 and items[0][:3] == (m, 0, 0)


@pytest.mark.parametrize("codec", [2, 3])
def test_tiny(ctx, codec):
    """m = 0..20: below 4 bytes snappy's finder is off, below 13 LZ4 may hold no match (the
    auditor's rule); m = 0 is the preamble (and an empty sequence) alone."""
    blocks = CC.tiny()
    encs, items = run_blocks(ctx, "tiny", blocks, codec)
    empty = b"\x00\x02" if codec == 2 else b"\x00\x00\x00\x00\x00\x03"
    for blk, enc, it in zip(blocks, encs, items):
        m = len(blk) - 1
        if m == 0:
            assert enc == empty
            dec = O.snappy_decompress(enc[:-1]) if codec == 2 else O.lz4_block_decompress(enc[:-1])
            assert dec == b""
        if m < (4 if codec == 2 else 13):
            assert not has_match(it, codec), (m, it)


@pytest.mark.parametrize("codec", [2, 3])
def test_ends(ctx, codec):
    """The last start of a match from both sides: a word that comes back k bytes before the end
    is matched from k = 4 on by snappy (to the last byte) and from k = 12 on by LZ4 (to 5 bytes
    before the end), and at no smaller k. tpz_gpu.h promises LZ4's 12, and no decoder checks it."""
    blocks, ks = CC.ends()
    _encs, items = run_blocks(ctx, "ends", blocks, codec)
    for k, it in zip(ks, items):
        n = 108 + k
        if codec == 2:
            want = [("lit", n, 1)] if k < 4 else \
                [("lit", 108, 1), ("copy1", 108, min(8, k))] + ([("lit", k - 8, 0)] if k > 8 else [])
        else:
            ml = min(8, k - 5)
            want = [(n, 0, 0, 1, 0)] if k < 12 else [(108, 108, ml, 1, 0), (k - ml, 0, 0, 0, 0)]
        assert it == want, (k, it)


@pytest.mark.parametrize("codec", [2, 3])
def test_window(ctx, codec):
    """kCMaxStaged from both sides at every start residue: a payload of up to 4,336 bytes is
    staged and compressed (a match, and the periodic bound below), a longer one is one literal."""
    blocks, index = CC.window()
    encs, items = run_blocks(ctx, "window", blocks, codec)
    ext = CC.batch(blocks)[1]
    for bi, m, r in index:
        assert int(ext[bi]) % 16 == r
        if m <= CC.WINDOW_MAX:
            assert has_match(items[bi], codec), (m, r)
            assert len(encs[bi]) <= m // 20 + 140, (m, r, len(encs[bi]))
        else:
            assert one_literal(items[bi], m, codec), (m, r, items[bi][:4])
    assert {r for _b, _m, r in index} == set(range(16))


@pytest.mark.parametrize("codec", [2, 3])
def test_offsets(ctx, codec):
    """A word repeated once at distance D and runs of period 1, 2, 3 and 5 (a copy that overlaps
    itself); the copy-1 / copy-2 classes they reach are asserted with the lengths family."""
    blocks, cases = CC.offsets()
    encs, items = run_blocks(ctx, "offsets", blocks, codec)
    for (kind, P, m), it, enc in zip(cases, items, encs):
        if kind == "run":       # the periodic bound (see test_periodic), 24 more literal bytes
            assert has_match(it, codec) and len(enc) <= m // 20 + 140 + 24, (P, len(enc))


@pytest.mark.parametrize("codec", [2, 3])
def test_periodic(ctx, codec):
    """Period P <= 64 over m bytes encodes to at most m // 20 + 140 bytes. Derived, not measured:
    the first 64-position window can match nothing (a candidate lies before the window); in the
    second at least one lane hits, since every word of the period was inserted; that match runs to
    the end. So the stream is at most 127 literal bytes and their header, then 3 bytes per 60
    copied (snappy) or 2 + m / 255 (LZ4), then the preamble, the final literals and the tag."""
    blocks, cases = CC.periodic()
    encs, items = run_blocks(ctx, "periodic", blocks, codec)
    for (P, m), enc in zip(cases, encs):
        assert len(enc) <= m // 20 + 140, (P, m, len(enc))


@pytest.mark.parametrize("codec", [2, 3])
def test_long(ctx, codec):
    """Payloads past the window, up to 16 MiB + 1: exactly one literal element or sequence, the
    snappy literal header 2, 3 and 4 length bytes wide on the right sides of 65,536 and 2^24."""
    blocks, cases = CC.long_blocks()
    encs, items = run_blocks(ctx, "long", blocks, codec)
    width = {}
    for (m, kind), it in zip(cases, items):
        assert one_literal(it, m, codec), (m, kind, it[:4])
        if codec == 2:
            width[m] = it[0][2]
        else:
            assert it[0][3] == (m - 15) // 255 + 1, (m, it[0])
    if codec == 2:
        assert [width[m] for m in (4337, 65535, 65536, 65537, 70000, 1 << 24, (1 << 24) + 1)] \
            == [2, 2, 2, 3, 3, 3, 4], width


def _coverage(codec, all_items):
    """The element classes of the lengths sweep (and the offsets family) that the device's
    streams did not show, as names."""
    missing = []

    def need(name, ok):
        if not ok:
            missing.append(name)

    if codec == 2:
        els = [e for it in all_items for e in it]
        matches = [p for it in all_items for _off, p in A.snappy_matches(it)]
        need("literal 60 inline", ("lit", 60, 0) in els)
        need("literal 61, 1 length byte", ("lit", 61, 1) in els)
        need("literal 256, 1 length byte", ("lit", 256, 1) in els)
        need("literal 257, 2 length bytes", ("lit", 257, 2) in els)
        need("copy1", any(e[0] == "copy1" for e in els))
        need("copy2 of <= 11 bytes at offset >= 2048",
             any(e[0] == "copy2" and e[2] <= 11 and e[1] >= 2048 for e in els))
        need("match of 65..67 cut 60 + rest", any(p in ([60, 5], [60, 6], [60, 7]) for p in matches))
        need("match of 68 cut 64 + 4", [64, 4] in matches)
    else:
        seqs = [s for it in all_items for s in it[:-1]]
        need("literal_len 14", any(s[0] == 14 and s[3] == 0 for s in seqs))
        need("literal_len 15 (extension byte 0)", any(s[0] == 15 and s[3] == 1 for s in seqs))
        need("literal_len 16", any(s[0] == 16 and s[3] == 1 for s in seqs))
        need("literal_len >= 270 (two extension bytes)",
             any(s[0] >= 270 and s[3] == 2 for s in seqs))
        need("match_len 18", any(s[2] == 18 and s[4] == 0 for s in seqs))
        need("match_len 19 (extension byte 0)", any(s[2] == 19 and s[4] == 1 for s in seqs))
        need("match_len 20", any(s[2] == 20 and s[4] == 1 for s in seqs))
        need("match_len >= 274 (two extension bytes)",
             any(s[2] >= 274 and s[4] == 2 for s in seqs))
    return missing


@pytest.mark.parametrize("codec", [2, 3])
def test_lengths(ctx, codec):
    """A literal of a bytes then a match of M bytes over the sweep of _compress_cases.lengths: the
    gates, and every class of element the emit branches can write is among what the device
    emitted. The 10-bit hash collides, so a case need not give exactly (a, M): the classes are
    asserted over the whole sweep, never per case."""
    blocks, _cases = CC.lengths()
    _e, items = run_blocks(ctx, "lengths", blocks, codec)
    _e, far = run_blocks(ctx, "offsets", CC.offsets()[0], codec)
    missing = _coverage(codec, items + far)
    assert not missing, "classes the device never emitted: " + "; ".join(missing)


@pytest.mark.parametrize("codec", [2, 3])
def test_reuse(ctx, codec):
    """More than two blocks per wave: a wave's second and third block meet the hash table the
    block before left behind, with positions past the new block's end. Only the gates: a stale
    bucket that verifies is a legitimate match, so the bytes may differ from a fresh wave's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = CC.reuse(cus)
    assert len(blocks) > 2 * 16 * cus
    run_blocks(ctx, "reuse", blocks, codec)


@pytest.mark.parametrize("codec", [2, 3])
@pytest.mark.parametrize("n", CC.COUNTS_N)
def test_counts(ctx, n, codec):
    """Block counts around the workgroup's 16 waves and the scan's 1,024: the extents are the
    blocks' own encoded lengths (re-measured from the audited elements in gates()); empty blocks
    and other tags come back byte for byte."""
    blocks = CC.counts(n)
    encs, items = run_blocks(ctx, "counts%d" % n, blocks, codec)
    assert len(encs) == n
    for blk, enc, it in zip(blocks, encs, items):
        if not blk or blk[-1] != 1:
            assert it is None and enc == blk


@pytest.mark.parametrize("codec", [2, 3])
def test_decode_parity(ctx, codec):
    """synth blocks -> compress -> the codec step -> decode == the oracle's entries of the source."""
    src, ext = synth.make_region("4kc", 64)
    src = np.asarray(src, np.uint8)[:int(ext[-1])]
    out, oext = raw_compress(ctx, src, ext, codec)
    b2, st = decompress_batch(ctx, DeviceBatch(out, oext))
    assert (st[:len(ext) - 1].cpu().numpy() == _lib.BLOCK_OK).all()
    g = decode_batch(ctx, b2).dense(b2.ext_host)
    o = O.decode_batch(src, ext)
    np.testing.assert_array_equal(g.status, o.status)
    assert g.keys.tobytes() == o.keys.tobytes() and g.vals.tobytes() == o.vals.tobytes()

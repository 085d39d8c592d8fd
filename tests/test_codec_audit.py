"""The stream auditors of _codec_audit.py cannot be vacuous: they decode the known-answer streams
to their recorded output, agree with the oracle's decoders on everything the host encoders
(tpz_snappy_encode_blocks / tpz_lz4_encode_blocks, tpz_host_builder.cpp) make of the compressor
edge cases, and every rule they state has a hand-made stream, a byte or two away from a valid
one, that trips it. The host encoders' streams are held to the rules they share with the device
compressor on the way (device_rules, LZ4's end rules)."""
import json
import os
import re

import numpy as np
import pytest

import _codec_audit as A
import _compress_cases as CC
import _oracle as O
import lz4_streams as LS
from conftest import GOLDEN
from topazdb_amd import synth


def _kat(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def test_snappy_kat():
    n_ok = 0
    for k in _kat("snappy_kat.json"):
        s = bytes.fromhex(k["stream"])
        if k["out"] is None:
            with pytest.raises(A.AuditError):
                A.snappy_audit(s)
        else:
            dec, els = A.snappy_audit(s)
            assert dec == bytes.fromhex(k["out"]) == O.snappy_decompress(s), k["name"]
            assert sum(e[2] if e[0] != "lit" else e[1] for e in els) == len(dec)
            n_ok += 1
    assert n_ok >= 9
    # the element lists themselves, by hand
    assert A.snappy_audit(bytes.fromhex("0a1068656c6c6f120500"))[1] == [("lit", 5, 0), ("copy2", 5, 5)]
    assert A.snappy_audit(bytes.fromhex("09086162630903"))[1] == [("lit", 3, 0), ("copy1", 3, 6)]
    assert A.snappy_audit(bytes.fromhex("080c7778797a0f04000000"))[1] == [("lit", 4, 0), ("copy4", 4, 4)]


# liblz4 decodes these two, and so does the oracle; an exact-format auditor must not: offset 0 is
# outside the format (liblz4 1.9.3 reads zeros there), and short_decode produces fewer bytes than
# its size prefix (lz4::block::decompress truncates)
_LZ4_KAT_TOLERATED = {"offset_zero": "offset 0", "short_decode": "size prefix says"}


def test_lz4_kat():
    n_ok = 0
    for k in _kat("lz4_kat.json"):
        s = bytes.fromhex(k["stream"])
        if k["name"] in _LZ4_KAT_TOLERATED:
            assert k["out"] is not None
            with pytest.raises(A.AuditError, match=_LZ4_KAT_TOLERATED[k["name"]]):
                A.lz4_audit(s, end_rules=False)
        elif k["out"] is None:
            with pytest.raises(A.AuditError):
                A.lz4_audit(s, end_rules=True)
        else:
            dec, seqs = A.lz4_audit(s, end_rules=False)
            assert dec == bytes.fromhex(k["out"]) == O.lz4_block_decompress(s), k["name"]
            assert sum(q[0] + q[2] for q in seqs) == len(dec) and seqs[-1][1:3] == (0, 0)
            n_ok += 1
    assert n_ok >= 5
    assert A.lz4_audit(bytes.fromhex("1e0000001f7a010005503132333435"))[1] == \
        [(1, 1, 24, 0, 1), (5, 0, 0, 0, 0)]


def test_lz4_streams_valid():
    """The streams of lz4_streams.py that liblz4 accepts (its crafted list, and the random format
    streams the oracle accepts) audit to what the oracle decodes; the end rules are the
    encoder's, stricter than the decoder's, so they stay off here."""
    n = 0
    for name, s, size, ok in LS.crafted():
        if ok:
            dec, _ = A.lz4_audit(size.to_bytes(4, "little") + s, end_rules=False)
            assert dec == O.lz4_decompress_safe(s, size) and len(dec) == size, name
            n += 1
    assert n >= 3
    n = 0
    for s, size in LS.format_streams(np.random.default_rng(5), 400):
        want = O.lz4_decompress_safe(s, size)
        if want is not None and len(want) == size:
            dec, _ = A.lz4_audit(size.to_bytes(4, "little") + s, end_rules=False)
            assert dec == want
            n += 1
    assert n >= 50, n


@pytest.fixture(scope="module")
def batches():
    return CC.all_batches()


@pytest.mark.parametrize("codec", [2, 3])
def test_host_encoders_over_the_cases(batches, codec):
    """Over every family: auditor == oracle == payload on the host encoders' output, which also
    keeps device_rules and LZ4's end rules (tpz_host_builder.cpp states the same ones)."""
    n_match = 0
    for name, blocks in batches.items():
        src, ext = CC.batch(blocks)
        out, oext = (synth.snappy_blocks if codec == 2 else synth.lz4_blocks)(src, ext)
        assert len(oext) == len(ext)
        for i, blk in enumerate(blocks):
            enc = bytes(out[int(oext[i]):int(oext[i + 1])])
            if not blk or blk[-1] != 1:
                assert enc == blk, (name, i)
                continue
            assert enc[-1] == codec, (name, i)
            try:
                if codec == 2:
                    dec, items = A.snappy_audit(enc[:-1])
                    want = O.snappy_decompress(enc[:-1])
                    n_match += any(e[0] != "lit" for e in items)
                else:
                    dec, items = A.lz4_audit(enc[:-1], end_rules=True)
                    want = O.lz4_block_decompress(enc[:-1])
                    n_match += len(items) > 1
                A.device_rules(items, codec)
            except A.AuditError as err:
                raise AssertionError("%s block %d: %s" % (name, i, err)) from err
            assert dec == want == blk[:-1], (name, i)
            if len(blk) == 1:       # m = 0: the preamble (and one empty sequence) alone
                assert enc == (b"\x00\x02" if codec == 2 else b"\x00\x00\x00\x00\x00\x03")
    assert n_match > 1000, n_match


def test_case_families_are_what_they_claim():
    blocks, index = CC.window()
    _src, ext = CC.batch(blocks)
    assert [(m, r) for _b, m, r in index[:-1]] == [(m, r) for m in CC.WINDOW_M for r in range(16)]
    for bi, m, r in index:
        assert int(ext[bi]) % 16 == r and len(blocks[bi]) == m + 1
        p = blocks[bi][:-1]
        assert p[-64:] == p[:64] and p[:m - 64] == (p[:7] * m)[:m - 64]
    assert index[-1][0] == len(blocks) - 1 and index[-1][1] <= CC.WINDOW_MAX
    assert len(CC.reuse(4)) == 2 * 16 * 4 + 37
    for n in CC.COUNTS_N:
        b = CC.counts(n)
        assert len(b) == n and max(len(x) for x in b) <= 41
    a, b = CC.lengths()[0], CC.lengths()[0]
    assert a == b                                   # fixed seeds


# ---- every rule has a stream that trips it ----------------------------------------------------
# "abcdefgh", then a copy-2 of 8 bytes from 8 back
_S = bytes.fromhex("101c") + b"abcdefgh" + bytes.fromhex("1e0800")

_SNAPPY_BAD = [
    ("non-minimal varint", b"\x90\x00" + _S[1:], "non-minimal"),
    ("varint of 6 bytes", b"\x90\x80\x80\x80\x80\x00" + _S[1:], "overlong"),
    ("varint past 32 bits", b"\xff\xff\xff\xff\x7f" + _S[1:], "overlong"),
    ("varint cut short", b"\x90", "varint preamble runs past"),
    ("preamble one too large", b"\x11" + _S[1:], "preamble says 17"),
    ("literal past the stream", _S[:6], "literal of 8 bytes runs past the stream"),
    ("literal length bytes past the stream", b"\x10\xf4\x07", "length bytes run past"),
    ("literal past the preamble", b"\x04" + _S[1:], "literal of 8 bytes runs past the preamble"),
    ("copy past the preamble", b"\x0f" + _S[1:], "copy of 8 bytes runs past the preamble"),
    ("copy header past the stream", _S[:-1], "copy's header runs past"),
    ("offset 0", _S[:-2] + b"\x00\x00", "offset 0"),
    ("offset one past the bytes produced", _S[:-2] + b"\x09\x00", "offset 9 reaches before the 8"),
    ("a trailing byte", _S + b"\x00", "1 bytes left over"),
]


@pytest.mark.parametrize("name,stream,msg", _SNAPPY_BAD, ids=[b[0] for b in _SNAPPY_BAD])
def test_snappy_violations(name, stream, msg):
    assert A.snappy_audit(_S) == (b"abcdefgh" * 2, [("lit", 8, 0), ("copy2", 8, 8)])
    with pytest.raises(A.AuditError, match=re.escape(msg)):
        A.snappy_audit(stream)


def _lz4(prefix, *seqs):
    return prefix.to_bytes(4, "little") + b"".join(seqs)


_L8, _T5 = b"abcdefgh", b"vwxyz"
# 8 literals, a match of 8 from 8 back, 5 literals: n = 21, the match starts at 8 <= n - 12 = 9
# and ends at 16 = n - 5, both rules met with nothing to spare on the end
_B = _lz4(21, LS.sequence(_L8, 8, 8), LS.sequence(_T5, None, 0))

_LZ4_BAD = [
    ("size prefix one too large", _lz4(22, LS.sequence(_L8, 8, 8), LS.sequence(_T5, None, 0)),
     True, "size prefix says 22"),
    ("size prefix too small", _lz4(15, LS.sequence(_L8, 8, 8), LS.sequence(_T5, None, 0)),
     False, "match of 8 bytes runs past the size prefix"),
    ("literals past the size prefix", _lz4(7, LS.sequence(_L8, 8, 8), LS.sequence(_T5, None, 0)),
     False, "literals run past the size prefix"),
    ("offset 0", _lz4(21, LS.sequence(_L8, 0, 8), LS.sequence(_T5, None, 0)), True, "offset 0"),
    ("offset one past the bytes produced",
     _lz4(21, LS.sequence(_L8, 9, 8), LS.sequence(_T5, None, 0)), True,
     "offset 9 reaches before the 8"),
    ("the last sequence carries a match", _lz4(16, LS.sequence(_L8, 8, 8)), False,
     "last sequence carries a match"),
    ("the last token carries a match length", _B[:-6] + b"\x51" + _T5, True,
     "last sequence carries a match length"),
    # the match one longer, the tail one shorter: it ends at 17 = n - 4
    ("match ends at n - 4", _lz4(21, LS.sequence(_L8, 8, 9), LS.sequence(_T5[:4], None, 0)),
     True, "ends at 17, past n - 5 = 16"),
    # two more literals, the match two shorter: it starts at 10 = n - 11
    ("match starts at n - 11", _lz4(21, LS.sequence(_L8 + b"ij", 8, 6), LS.sequence(_T5, None, 0)),
     True, "starts at 10, past n - 12 = 9"),
    ("a match in a block under 13 bytes",
     _lz4(12, LS.sequence(b"abcd", 4, 4), LS.sequence(b"wxyz", None, 0)), True,
     "block of 12 < 13"),
    ("a trailing byte", _B + b"\x00", True, "1 bytes left over"),
    ("literals past the block", _B[:-1], True, "5 literals run past the block"),
    ("offset past the block", _B[:14], True, "offset runs past the block"),
    ("length continuation past the block", _lz4(300, b"\xf0\xff"), True,
     "continuation runs past"),
    ("no sequence", _lz4(0), True, "no sequence"),
    ("no size prefix", b"\x15\x00\x00", True, "no size prefix"),
]


@pytest.mark.parametrize("name,block,end_rules,msg", _LZ4_BAD, ids=[b[0] for b in _LZ4_BAD])
def test_lz4_violations(name, block, end_rules, msg):
    dec, seqs = A.lz4_audit(_B, end_rules=True)
    assert dec == _L8 * 2 + _T5 and seqs == [(8, 8, 8, 0, 0), (5, 0, 0, 0, 0)]
    with pytest.raises(A.AuditError, match=re.escape(msg)):
        A.lz4_audit(block, end_rules=end_rules)


def test_end_rules_are_the_encoders_only():
    """Without end_rules the two end-rule streams are plain LZ4 and decode."""
    for name, block, _e, msg in _LZ4_BAD:
        if "past n -" in msg:
            dec, _ = A.lz4_audit(block, end_rules=False)
            assert len(dec) == 21, name


_RULES_BAD = [
    (2, [("lit", 4, 0), ("copy4", 4, 4)], "copy-4"),
    (2, [("lit", 4, 0), ("copy1", 2048, 4)], "copy-1"),
    (2, [("lit", 4, 0), ("copy1", 4, 12)], "copy-1"),
    (2, [("lit", 4, 0), ("copy2", 4, 65)], "copy-2 of 65"),
    (2, [("lit", 4, 0), ("copy2", 4, 64), ("copy2", 4, 3)], "a piece under 4"),
    (2, [("lit", 4, 0), ("copy2", 4, 3)], "a piece under 4"),
    (3, [(4, 4, 3, 0, 0), (5, 0, 0, 0, 0)], "match of 3 < 4"),
]


@pytest.mark.parametrize("codec,items,msg", _RULES_BAD)
def test_device_rules_violations(codec, items, msg):
    with pytest.raises(A.AuditError, match=re.escape(msg)):
        A.device_rules(items, codec)


def test_device_rules_pass():
    A.device_rules([("lit", 70, 1), ("copy2", 9, 64), ("copy2", 9, 4), ("lit", 1, 0),
                    ("copy2", 9, 60), ("copy2", 9, 5), ("copy1", 2047, 11), ("copy2", 2048, 11)], 2)
    A.device_rules([(0, 1, 4, 0, 0), (300, 9, 300, 2, 2), (0, 0, 0, 0, 0)], 3)
    assert A.snappy_matches([("copy2", 9, 64), ("copy2", 9, 4), ("lit", 1, 0), ("copy2", 9, 8),
                             ("copy1", 7, 8)]) == [(9, [64, 4]), (9, [8]), (7, [8])]

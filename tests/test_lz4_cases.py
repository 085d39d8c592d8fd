"""The sequence-program generator of tests/_lz4_cases.py against liblz4 and both LZ4 restatements,
the classes its programs reach, and how far the ring kernel's acceptance reaches into them.

The generator writes a stream and the bytes it stands for without any decoder, so here it is the
reference: LZ4_decompress_safe of liblz4 1.9.3 (the library the reference's `lz4` crate binds,
src/block/compress.rs:108-111), the C oracle (oracle/tpz_lz4.c) and the Python restatement
(make_golden.lz4_decompress_safe) must return its bytes for every valid program, at its own
prefix and at the raised ones, and reject every named invalid stream. The class counters are
asserted from the programs themselves, so that a later edit of the generator cannot silently drop
a shape tests/test_gpu_lz4_cases.py relies on."""
import _lz4_cases as Z4
import _oracle as O
from test_lz4_oracle import G, check, lib_decompress, needs_lib, ring_rules

LIMITS = (0,) + Z4.RAISES


def parts(block):
    """(stream, prefix as the i32 the reference reads) of a tag-3 block of 5 bytes or more."""
    return block[4:-1], int.from_bytes(block[:4], "little", signed=True)


def test_generator_is_deterministic():
    a = Z4.window_programs() + Z4.offset_programs()[:8] + Z4.random_programs(20)
    b = Z4.window_programs() + Z4.offset_programs()[:8] + Z4.random_programs(20)
    assert a == b
    f = [(20, 7, 30), (3, 20, 40)]
    assert Z4._faults("x", f, 8, Z4.random.Random(1)) == Z4._faults("x", f, 8, Z4.random.Random(1))


@needs_lib
def test_liblz4_decodes_valid_programs_to_the_generators_bytes():
    for c in Z4.valid_cases():
        for r in LIMITS:
            assert lib_decompress(c.stream, len(c.out) + r) == c.out, (c.name, r)


def test_oracle_decodes_valid_programs_to_the_generators_bytes():
    for c in Z4.valid_cases():
        for r in LIMITS:
            assert O.lz4_decompress_safe(c.stream, len(c.out) + r) == c.out, (c.name, r)
            assert O.decompress_block(Z4.block_of(c, r)) == (O.OK, c.out + b"\x01"), (c.name, r)


def test_python_restatement_decodes_valid_programs_to_the_generators_bytes():
    for c in Z4.valid_cases():
        for r in LIMITS:
            assert G.lz4_decompress_safe(c.stream, len(c.out) + r) == c.out, (c.name, r)


def test_invalid_streams_are_rejected():
    """Every named invalid block is an Err for the reference: a stream fault by
    LZ4_decompress_safe under the block's prefix (all three decoders), a prefix or source-length
    fault by lz4::block::decompress's own checks (both restatements of it; liblz4 never runs)."""
    bad = Z4.invalid_cases()
    names = {b.name.split("@")[0] for b in bad}
    assert names >= {"offset_past_output_first", "offset_past_output_last", "offset_65535_short",
                     "literal_past_input", "cut_literal_length", "cut_match_length",
                     "output_one_longer", "ends_in_match", "match_in_last_5",
                     "literal_into_last_12", "prefix_above_limit", "prefix_negative"}
    n_stream = 0
    for b in bad:
        assert O.decompress_block(b.block) == (O.CODEC, b""), (b.name, b.rule)
        assert O.lz4_block_decompress(b.block[:-1]) is None, (b.name, b.rule)
        assert G.lz4_block_decompress(b.block[:-1]) is None, (b.name, b.rule)
        if b.name.startswith(("prefix_", "source_")):
            continue
        n_stream += 1
        s, prefix = parts(b.block)
        assert O.lz4_decompress_safe(s, prefix) is None, (b.name, b.rule)
        assert G.lz4_decompress_safe(s, prefix) is None, (b.name, b.rule)
    assert n_stream >= 2 * 10 + 3 * 3          # two full sets, three more sizes of the last-match faults


@needs_lib
def test_liblz4_rejects_invalid_streams():
    for b in Z4.invalid_cases():
        if not b.name.startswith(("prefix_", "source_")):
            assert lib_decompress(*parts(b.block)) is None, (b.name, b.rule)


def test_last_match_faults_come_in_three_sizes():
    by = Z4.last_match_faults()
    for size in ("small", "big", "global"):
        kinds = {b.name.split("@")[0] for b in by[size]}
        assert kinds == {"offset_past_output_last", "ends_in_match", "match_in_last_5"}, size
    # past the one-wave windows by the compressed length, and by the output alone
    assert any(len(b.block) - 1 > 65504 for b in by["global"])
    assert any(len(b.block) - 1 <= 65504 and parts(b.block)[1] > 94192 for b in by["global"])
    # a claimed-size pass takes the prefix of each (tpz_codec.hip, codec_sizes_kernel)
    for bs in by.values():
        for b in bs:
            assert 0 <= parts(b.block)[1] <= 256 * (len(b.block) - 5) + 64, b.name


@needs_lib
def test_offset_zero_streams():
    """liblz4 and both restatements agree on the offset-0 streams (into a zeroed output)."""
    cases = Z4.offset_zero_cases()
    assert len(cases) >= 9
    for _name, blk in cases:
        check(*parts(blk))


def test_classes_of_the_valid_programs():
    cases = Z4.valid_cases()
    r = Z4.Reach(cases)
    for n in Z4.LITERAL_LENGTHS:
        assert r.lit_lengths[n] > 0, n
    for n in Z4.MATCH_LENGTHS:
        assert r.match_lengths[n] > 0, n
    for off in Z4.OFFSETS:
        assert r.offsets[off] > 0, off
        # (a match is at least 4 bytes: none is shorter than an offset below 5, or equal to one
        # below 4)
        if off >= 5:
            assert r.relation[off, "lt"] > 0, off
        if off >= 4:
            assert r.relation[off, "eq"] > 0, off
        assert r.relation[off, "gt"] > 0, off
        if off < 64:
            assert r.steps3[off] > 0, off
    for lc in Z4.LIT_RANGES:
        for mc in Z4.MATCH_RANGES:
            assert r.lit_match[lc, mc] >= 3, (lc, mc)
            assert r.match_lit[mc, lc] >= 3, (mc, lc)
    for f in Z4.FINALS:
        assert r.finals[f] > 0, f
        for nseq in (0, 1, 2):
            assert r.after[f, nseq] > 0, (f, nseq)


def ring_accepts(c, raise_by):
    """The ring model on a valid case under a prefix: liblz4's rules as the ring applies them
    (ring_rules) and the reach of its header window."""
    got = ring_rules(c.stream, len(c.out) + raise_by, len(c.out))
    assert got is None or got == c.out, c.name
    return got is not None, Z4.header_window_ok(c.stream)


def test_reach_of_the_ring():
    """The ring model accepts every valid case whose literal and match lengths are all at most
    1,000, at every prefix, and none of them outruns the 16-byte header window (refilled below 8
    bytes): what test_gpu_lz4_cases.py::test_ring_route checks is the ring's work, what it hands
    to the lane kernel are the longer fields alone. Per offset class and per match-length class at
    least one case is accepted by the rules; with the header window, every class but a match of
    70,000 bytes (274 continuation bytes) is."""
    cases = Z4.valid_cases()
    by_rules_off, by_rules_ml, ring_off, ring_ml = set(), set(), set(), set()
    n_short = handed = 0
    for c in cases:
        short = Z4.max_length(c) <= Z4.RING_MAX
        n_short += short
        for r in LIMITS:
            rules, window = ring_accepts(c, r)
            if short:
                assert rules and window, (c.name, r, rules, window)
            if r == 0:
                handed += not (rules and window)
                for _ll, off, ml in c.program:
                    if rules:
                        by_rules_off.add(off)
                        by_rules_ml.add(ml)
                    if rules and window:
                        ring_off.add(off)
                        ring_ml.add(ml)
    assert n_short > len(cases) * 3 // 4
    assert set(Z4.OFFSETS) <= by_rules_off and set(Z4.MATCH_LENGTHS) <= by_rules_ml
    assert set(Z4.OFFSETS) <= ring_off
    assert set(Z4.MATCH_LENGTHS) - ring_ml == {70000}
    # the lane kernel's share on a batch-sized source: cases with a longer field only (a long
    # field that meets a full window still fits it)
    assert 20 <= handed <= len(cases) - n_short

"""The element-program generator of tests/_snappy_cases.py against both snappy restatements, and
the element shapes its programs reach.

The generator writes a stream and the bytes it stands for without any decoder, so here it is the
reference: the C oracle (oracle/tpz_snappy.c) and the Python restatement
(make_golden.snappy_decompress) must return its bytes for every valid program and reject every
named invalid stream. The reach conditions are asserted from the programs themselves, so that a
later edit of the generator cannot silently drop a shape tests/test_gpu_snappy_cases.py relies on:
literal -> literal, wide literal headers, copies shorter than 4 bytes, every ordered pair of
element kinds, offsets of 65,536 and more."""
import _oracle as O
import _snappy_cases as S
from test_snappy_oracle import MG

PY_LIMIT = 20000          # the Python restatement is checked on outputs up to this many bytes


def test_generator_is_deterministic():
    a = S.window_programs() + S.far_programs()[:1] + S.random_programs(20, 2, 2)
    b = S.window_programs() + S.far_programs()[:1] + S.random_programs(20, 2, 2)
    assert a == b
    assert S._invalid_after("x", [S.lit(20)], S.random.Random(1)) == \
        S._invalid_after("x", [S.lit(20)], S.random.Random(1))


def test_valid_programs_decode_to_the_generators_bytes():
    n_py = 0
    for c in S.valid_cases():
        assert O.snappy_decompress(c.stream) == c.out, c.name
        if len(c.out) <= PY_LIMIT:
            n_py += 1
            assert MG.snappy_decompress(c.stream) == c.out, c.name
    assert n_py > 1500


def test_invalid_streams_are_rejected():
    bad = S.invalid_cases()
    assert len(bad) >= 3 * 40
    for b in bad:
        assert O.snappy_decompress(b.stream) is None, (b.name, b.rule)
        assert MG.snappy_decompress(b.stream) is None, (b.name, b.rule)


def test_invalid_streams_are_one_step_from_valid():
    """The streams that break an offset or a length rule decode once that one value is mended:
    each is rejected for the rule it names, not for a malformed prefix."""
    rng = S.random.Random(3)
    for tag, prefix in (("lit20", [S.lit(20)]), ("lit70", [S.lit(70), (S.C2, 9, 33), S.lit(9)])):
        pb, pout = S.emit_body(prefix, rng)
        d = len(pout)
        for kind in (S.C1, S.C2, S.C4):
            ok = S.varint(d + 5) + pb + S.enc_copy(kind, 5, d)
            assert O.snappy_decompress(ok) == pout + pout[:5]
            assert MG.snappy_decompress(ok) == pout + pout[:5]
        tail = S.enc_lit_header(6, 1) + b"1234567"
        assert O.snappy_decompress(S.varint(d + 7) + pb + tail) == pout + b"1234567"


def check_reach(r, pair_floor, forms=True):
    for a in S.KINDS:
        for b in S.KINDS:
            assert r.pairs[a, b] >= pair_floor, (a, b, r.pairs[a, b])
    for hw in (1, 2, 3, 4, 5):
        assert r.lit_headers[hw, True] + r.lit_headers[hw, False] > 0, hw
    if not forms:
        return
    # every header width in its shortest and in a wide form (1 byte has no wide form; the
    # shortest 5-byte header needs a literal above 16 MiB)
    for hw in (1, 2, 3, 4):
        assert r.lit_headers[hw, True] > 0, hw
    for hw in (2, 3, 4, 5):
        assert r.lit_headers[hw, False] > 0, hw


def test_reach_of_the_valid_programs():
    cases = S.valid_cases()
    r = S.Reach(cases)
    check_reach(r, 50)
    for n in S.LITERAL_LENGTHS:
        assert r.lit_lengths[n] > 0, n
    assert any(n > 65536 for n in r.lit_lengths)
    for n in range(1, 101):
        for hl in (1, 2, 3, 5):
            assert (n, hl) in r.lit_then, (n, hl)
    for n in range(1, 65):
        assert r.copy_lengths[S.C2, n] > 0 and r.copy_lengths[S.C4, n] > 0, n
    for n in range(4, 12):
        assert r.copy_lengths[S.C1, n] > 0, n
    # offsets: every value 1..136 (the period registers, the ring with its half-slot edge, the
    # first stored-line offsets), each below 64 also with a longer copy; a few hundred; a few
    # thousand; the oldest byte at small and large outputs; 65,536 and more
    for off in range(1, 137):
        assert r.offsets[off] > 0, off
    for off in range(1, 64):
        assert r.overlaps[S.C2, off] > 0 and r.overlaps[S.C4, off] > 0, off
    for off in range(1, 11):
        assert r.overlaps[S.C1, off] > 0, off
    assert sum(v for o, v in r.offsets.items() if 137 <= o < 1000) >= 100
    assert sum(v for o, v in r.offsets.items() if 1000 <= o < 10000) >= 100
    assert min(r.oldest) < 16 and sum(128 < d < 1000 for d in r.oldest) > 5
    assert sum(d >= 1000 for d in r.oldest) > 5 and sum(d >= 65536 for d in r.oldest) >= 6
    assert len(r.far) >= 50 and {65536, 65537} <= {o for o, _ in r.far}
    assert all(70000 <= out <= 200000 for _, out in r.far)


def test_reach_of_each_wave_side_route():
    """When the ring is not live a block goes to the 16-wave kernel's windows, the one-wave
    kernel's or snappy_decode_global by its sizes: each of the three gets every ordered pair and
    every header width, and the offsets of 65,536 and more go to the global decoder."""
    cases = S.valid_cases()
    by = {k: [c for c in cases if S.route_of(c) == k] for k in ("small", "big", "global")}
    assert len(by["small"]) > 1000 and len(by["big"]) >= 40 and len(by["global"]) >= 30
    for k, cs in by.items():
        check_reach(S.Reach(cs), 1, forms=False)
    assert all(S.route_of(c) == "global" for c in cases if c.name.startswith("far_"))
    g = by["global"]
    assert any(len(c.stream) + 1 > 65505 and len(c.out) + 17 <= S.BIG_OUT for c in g)
    assert any(len(c.out) + 17 > S.BIG_OUT for c in g)

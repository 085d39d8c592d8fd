"""Snappy streams built from element programs: the reference for the device snappy decoders on
streams no compressor here emits (tests/test_snappy_cases.py, tests/test_gpu_snappy_cases.py).

A *program* is a list of elements of the snappy raw format (the format `snap::raw::Decoder::
decompress_vec` reads, src/block/compress.rs:104-107):

    ("lit", n, hw)        a literal of n bytes whose header is hw bytes long (1: n - 1 in the tag,
                          n <= 60; 2..5: tag 60..63 and n - 1 in hw - 1 little-endian bytes, which
                          need not be the shortest form: the format and snap accept a wide header)
    ("copy1", n, off)     4 <= n <= 11, off < 2048              2 header bytes
    ("copy2", n, off)     1 <= n <= 64, off < 65536             3 header bytes
    ("copy4", n, off)     1 <= n <= 64, off < 2^32              5 header bytes

`emit` writes the stream (varint preamble + elements) and, as it goes, the bytes the stream stands
for: a literal's bytes are appended, a copy is applied to the generator's own output (byte by byte
where it overlaps itself). No decoder takes part, so these bytes are the reference: the C oracle
and make_golden.snappy_decompress are checked against them (test_snappy_cases.py), not trusted.

Everything is seeded (random.Random, whose randbytes / randrange sequences are fixed by the
language): two calls give identical bytes. Pure Python, no numpy.

The varint preamble is always the shortest form: its edge forms stay with the known answers of
tests/golden/snappy_kat.json. A shortest 5-byte literal header needs a literal above 16 MiB and is
left out; the 5-byte header occurs in its wide form only.
"""
import functools
import random
from collections import Counter, namedtuple

LIT, C1, C2, C4 = "lit", "copy1", "copy2", "copy4"
KINDS = (LIT, C1, C2, C4)
COPY_HL = {C1: 2, C2: 3, C4: 5}

# literal lengths every suite run must reach (plus one above 65,536, see literal_programs)
LITERAL_LENGTHS = (1, 2, 15, 16, 17, 59, 60, 61, 63, 64, 65, 79, 80, 81, 127, 128, 129, 300)
LONG_LITERAL = 70000

# the device's window sizes (tpz_codec.hip: kSmallIn / kSmallOut, kBigIn / kBigOut, kInSlack 32,
# 16 bytes of output slack): which decoder takes a block when the one-block-per-lane ring does not
SMALL_IN, SMALL_OUT, BIG_IN, BIG_OUT = 4608, 5120, 65536, 94208

Case = namedtuple("Case", "name program stream out")       # a valid stream and its bytes
Bad = namedtuple("Bad", "name rule stream")                # a stream snap's decoder rejects


def lit(n, hw=None):
    return (LIT, n, hw if hw is not None else min_hw(n))


def min_hw(n):
    """The shortest literal header for n bytes."""
    return 1 if n <= 60 else 2 if n <= 1 << 8 else 3 if n <= 1 << 16 else 4 if n <= 1 << 24 else 5


def header_len(e):
    return e[2] if e[0] == LIT else COPY_HL[e[0]]


def varint(v):
    b = bytearray()
    while v >= 0x80:
        b.append(v & 0x7F | 0x80)
        v >>= 7
    b.append(v)
    return bytes(b)


def enc_lit_header(field, hw):
    """A literal header of hw bytes whose length field (length - 1) is `field`; unchecked."""
    if hw == 1:
        return bytes([field << 2])
    return bytes([(58 + hw) << 2]) + field.to_bytes(hw - 1, "little")


def enc_copy(kind, n, off):
    """A copy element; unchecked (the invalid streams put offsets no output has)."""
    if kind == C1:
        return bytes([1 | (n - 4) << 2 | (off >> 8) << 5, off & 0xFF])
    if kind == C2:
        return bytes([2 | (n - 1) << 2]) + off.to_bytes(2, "little")
    return bytes([3 | (n - 1) << 2]) + off.to_bytes(4, "little")


def emit_body(program, rng):
    """(element bytes, output bytes) of a program; literal bytes come from rng."""
    body, out = bytearray(), bytearray()
    for e in program:
        if e[0] == LIT:
            _, n, hw = e
            assert n >= 1 and (n <= 60 if hw == 1 else 2 <= hw <= 5 and n - 1 < 1 << 8 * (hw - 1)), e
            data = rng.randbytes(n)
            body += enc_lit_header(n - 1, hw)
            body += data
            out += data
        else:
            kind, n, off = e
            d = len(out)
            assert 1 <= off <= d, (e, d)
            assert (4 <= n <= 11 and off < 2048) if kind == C1 else \
                (1 <= n <= 64 and off < (1 << 16 if kind == C2 else 1 << 32)), e
            body += enc_copy(kind, n, off)
            if off >= n:
                out += out[d - off:d - off + n]
            else:
                for _ in range(n):                         # overlaps itself: repeats with period off
                    out.append(out[-off])
    return bytes(body), bytes(out)


def emit(program, rng):
    """(stream, output bytes) of a program."""
    body, out = emit_body(program, rng)
    return varint(len(out)) + body, out


def case(name, program, rng):
    stream, out = emit(program, rng)
    return Case(name, tuple(program), stream, out)


def produced(program):
    return sum(e[1] for e in program)


# ------------------------------------------------------------------ random elements
def rand_literal(rng, small=True):
    r = rng.random()
    n = rng.randint(1, 20) if r < 0.6 else rng.randint(21, 150) if r < 0.93 or small else \
        rng.randint(151, 700)
    lo = min_hw(n)
    hw = lo if rng.random() < 0.5 else rng.randint(lo, 5)
    return lit(n, hw)


def rand_copy(rng, d, kind=None):
    """A copy valid after d >= 1 output bytes, of every offset class."""
    kind = kind or rng.choice((C1, C2, C4))
    cap = min(d, 2047 if kind == C1 else 65535 if kind == C2 else d)
    r = rng.random()
    off = rng.randint(1, min(15, cap)) if r < 0.3 else rng.randint(1, min(136, cap)) if r < 0.7 \
        else rng.randint(1, cap) if r < 0.9 else cap
    n = rng.randint(4, 11) if kind == C1 else rng.randint(1, 64)
    return (kind, n, off)


def rand_element(rng, d, kind=None):
    kind = kind or rng.choice(KINDS)
    return rand_literal(rng) if kind == LIT or d == 0 else rand_copy(rng, d, kind)


# ------------------------------------------------------------------ the valid programs
def window_programs():
    """Each literal length 1..100 followed by an element whose header is 1, 2, 3, 4 and 5 bytes
    long, a literal and (2, 3, 5) a copy: the next header lies in the literal's last loaded piece.
    Half of them start with another literal (literal -> literal)."""
    rng = random.Random(0x5A01)
    cases = []
    for L in range(1, 101):
        followers = [("l1", lambda d: lit(rng.randint(1, 9), 1)), ("l2", lambda d: lit(rng.randint(1, 80), 2)),
                     ("l3", lambda d: lit(rng.randint(1, 9), 3)), ("l4", lambda d: lit(rng.randint(1, 9), 4)),
                     ("l5", lambda d: lit(rng.randint(1, 9), 5)), ("c1", lambda d: rand_copy(rng, d, C1)),
                     ("c2", lambda d: rand_copy(rng, d, C2)), ("c4", lambda d: rand_copy(rng, d, C4))]
        for fname, follower in followers:
            prog = []
            if rng.random() < 0.5:
                prog.append(rand_literal(rng))
            lo = min_hw(L)
            prog.append(lit(L, lo if rng.random() < 0.7 else rng.randint(lo, 5)))
            prog.append(follower(produced(prog)))
            prog.append(rand_copy(rng, produced(prog)))
            prog.append(lit(rng.randint(1, 8)))
            cases.append(case(f"window_L{L}_{fname}", prog, rng))
    return cases


def literal_programs():
    """Every listed literal length with every header width that can hold it, after a short random
    prefix and before a copy; LONG_LITERAL with its 4-byte (shortest) and 5-byte header."""
    rng = random.Random(0x5A02)
    cases = []
    for n in LITERAL_LENGTHS + (LONG_LITERAL,):
        for hw in range(min_hw(n), 6):
            for rep in range(2):
                prog = []
                for _ in range(rng.randint(0, 2)):
                    prog.append(rand_element(rng, produced(prog)))
                prog.append(lit(n, hw))
                prog.append(rand_copy(rng, produced(prog)))
                prog.append(lit(rng.randint(1, 30)))
                cases.append(case(f"literal_{n}_hw{hw}_{rep}", prog, rng))
    return cases


def _copies_at(rng, prog, off, lengths):
    """Appends copies of the given lengths at offset `off` (kinds at random among those that can
    hold it), a few short literals between them."""
    for n in lengths:
        kinds = ((C1,) if 4 <= n <= 11 and off < 2048 else ()) + \
            ((C2,) if off < 65536 else ()) + (C4,)
        prog.append((rng.choice(kinds), n, off))
        if rng.random() < 0.15:
            prog.append(lit(rng.randint(1, 5)))


def copy_programs():
    """Every offset 1..136 (the period registers below 16, the ring's 128 bytes with its half-slot
    edge at 120..128, the stored lines beyond) with every copy length 1..64, twice; then offsets of
    a few hundred and a few thousand. Each program starts with a literal and a copy whose offset is
    exactly the bytes produced so far (the oldest byte)."""
    rng = random.Random(0x5A03)
    cases = []
    for off in range(1, 137):
        for rep in range(2):
            first = off + rng.randint(0, 40)
            prog = [lit(first), (rng.choice((C2, C4)), rng.randint(1, 64), first)]
            lengths = list(range(1, 65))
            rng.shuffle(lengths)
            _copies_at(rng, prog, off, lengths)
            cases.append(case(f"copy_off{off}_{rep}", prog, rng))
    for off in (137, 192, 200, 255, 256, 257, 300, 511, 512, 1000, 2047, 2048, 3000, 5000, 8191,
                20000, 65535):
        first = off + (rng.randint(0, 40) if off < 65535 else 0)     # (65,536 and more: far_programs)
        prog = [lit(first), (C2 if rng.random() < 0.5 else C4, rng.randint(1, 64), first)]
        _copies_at(rng, prog, off, [rng.randint(1, 64) for _ in range(24)])
        cases.append(case(f"copy_off{off}", prog, rng))
    return cases


def far_programs():
    """copy-4 offsets of 65,536 and more, in outputs of 70,000-200,000 bytes: the first copy
    reaches the oldest byte, the rest mix the far offset with near ones and literals."""
    rng = random.Random(0x5A04)
    cases = []
    for off in (65536, 65537, 70000, 100000, 131072, 150000):
        first = max(off, 70000) + rng.randint(100, 5000)
        prog = [lit(first, rng.choice((4, 5))), (C4, rng.randint(1, 64), first)]
        for _ in range(30):
            r = rng.random()
            d = produced(prog)
            if r < 0.5:
                prog.append((C4, rng.randint(1, 64), rng.randint(off, d) if rng.random() < 0.5 else off))
            elif r < 0.8:
                prog.append(rand_copy(rng, d))
            else:
                prog.append(rand_literal(rng))
        cases.append(case(f"far_off{off}", prog, rng))
    return cases


def random_programs(n_small=600, n_big=48, n_global=32):
    """Random programs of 1-40 elements in three sizes, named after the decoder that takes them
    when the ring does not (route_of): short ones, ones a long literal pushes past the small
    windows, and ones past the big windows (by their output, or by their compressed length alone)."""
    rng = random.Random(0x5A05)
    cases = []
    for size, count in (("small", n_small), ("big", n_big), ("global", n_global)):
        for i in range(count):
            prog = []
            for _ in range(rng.randint(1, 40)):
                prog.append(rand_element(rng, produced(prog)))
            if size != "small":
                n = rng.randint(5200, 30000) if size == "big" else \
                    rng.randint(70000, 76000) if i % 2 else rng.randint(94300, 120000)
                at = rng.randint(0, len(prog))
                # (elements after the insertion keep their offsets: a copy reaches further back)
                prog.insert(at, lit(n, rng.randint(min_hw(n), 5)))
            cases.append(case(f"random_{size}_{i}", prog, rng))
    return cases


@functools.lru_cache(maxsize=None)
def valid_cases():
    """Every valid case, in a fixed order."""
    cases = window_programs() + literal_programs() + copy_programs() + far_programs() + \
        random_programs()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


# ------------------------------------------------------------------ the named invalid streams
def _invalid_after(tag, prefix, rng):
    """The named invalid streams behind one valid prefix program (which ends in a literal)."""
    pb, pout = emit_body(prefix, rng)
    d = len(pout)
    bad = []

    def add(name, rule, want, body):
        bad.append(Bad(f"{name}@{tag}", rule, varint(want) + bytes(body)))

    for kind in (C1, C2, C4):
        add(f"offset_0_{kind}", "a copy's offset is at least 1", d + 5, pb + enc_copy(kind, 5, 0))
        add(f"offset_past_output_{kind}", "a copy's offset is at most the bytes produced", d + 5,
            pb + enc_copy(kind, 5, d + 1))
    tail_lit = enc_lit_header(6, 1) + rng.randbytes(7)
    tail_copy = enc_copy(C2, 7, 3)
    add("last_literal_overruns", "no element writes past the declared length", d + 6, pb + tail_lit)
    add("last_copy_overruns", "no element writes past the declared length", d + 6, pb + tail_copy)
    add("declared_one_more_literal", "the elements produce the declared length", d + 8, pb + tail_lit)
    add("declared_one_more_copy", "the elements produce the declared length", d + 8, pb + tail_copy)
    add("trailing_literal", "no element follows a full output", d + 7,
        pb + tail_lit + enc_lit_header(0, 1) + b"x")
    add("trailing_copy", "no element follows a full output", d + 7, pb + tail_copy + enc_copy(C1, 4, 1))
    add("literal_past_input", "a literal's bytes lie inside the input", d + 7, pb + tail_lit[:-1])
    for hw in (2, 3, 4, 5):
        full = enc_lit_header(3, hw) + rng.randbytes(4)
        for k in range(1, hw):
            add(f"cut_literal_hw{hw}_after{k}", "an element's header lies inside the input", d + 4,
                pb + full[:k])
    for kind in (C1, C2, C4):
        full = enc_copy(kind, 6, 2)
        for k in range(1, COPY_HL[kind]):
            add(f"cut_{kind}_after{k}", "an element's header lies inside the input", d + 6,
                pb + full[:k])
    # 4-byte literal lengths around the ring's `big` bound (length field >= 0x7FFFFFF0) and the
    # wave decoder's clamp (0x7FFFFFFF): as the length and as the length field
    values = (0x7FFFFFEF, 0x7FFFFFF0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
    for field in sorted({v - 1 for v in values} | set(values)):
        add(f"literal_field_{field:#010x}", "a literal's bytes lie inside the input", d + 10,
            pb + enc_lit_header(field, 5) + rng.randbytes(10))
    for off in (0x80000000, 0xFFFFFFFF):
        add(f"copy4_offset_{off:#010x}", "a copy's offset is at most the bytes produced", d + 5,
            pb + enc_copy(C4, 5, off))
    return bad


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """Every named invalid stream, each one byte or one value away from a valid program: behind a
    20-byte literal, and behind a 70-byte literal, a copy and a 9-byte literal (the broken
    element's header then comes out of a literal's last piece)."""
    rng = random.Random(0x5A06)
    bad = _invalid_after("lit20", [lit(20)], rng)
    bad += _invalid_after("lit70", [lit(70), (C2, 9, 33), lit(9)], rng)
    bad += _invalid_after("lit300", [lit(300, 5), (C4, 64, 300), lit(75, 3)], rng)
    assert len({b.name for b in bad}) == len(bad)
    return tuple(bad)


# ------------------------------------------------------------------ what the programs reach
def route_of(c):
    """The decoder a case's block (stream + tag byte) goes to when the ring is not live: the
    16-wave kernel's windows, the one-wave kernel's, or snappy_decode_global (tpz_codec.hip,
    codec_block: `fits`)."""
    n, dn = len(c.stream), len(c.out) + 1
    if n + 32 <= SMALL_IN and dn + 16 <= SMALL_OUT:
        return "small"
    if n + 32 <= BIG_IN and dn + 16 <= BIG_OUT:
        return "big"
    return "global"


class Reach:
    """Counts of the element shapes a set of cases holds."""

    def __init__(self, cases):
        self.pairs = Counter()            # (kind, next kind)
        self.lit_headers = Counter()      # (header bytes, is the shortest form)
        self.lit_lengths = Counter()
        self.lit_then = set()             # (literal length, next element's header bytes)
        self.copy_lengths = Counter()     # (kind, length)
        self.offsets = Counter()          # offset
        self.overlaps = Counter()         # (kind, offset) with length > offset
        self.oldest = []                  # bytes produced at a copy whose offset is exactly that
        self.far = []                     # (offset, output bytes) of copies with offset >= 65,536
        for c in cases:
            d = 0
            for i, e in enumerate(c.program):
                nxt = c.program[i + 1] if i + 1 < len(c.program) else None
                if nxt is not None:
                    self.pairs[e[0], nxt[0]] += 1
                if e[0] == LIT:
                    self.lit_headers[e[2], e[2] == min_hw(e[1])] += 1
                    self.lit_lengths[e[1]] += 1
                    if nxt is not None:
                        self.lit_then.add((e[1], header_len(nxt)))
                else:
                    kind, n, off = e
                    self.copy_lengths[kind, n] += 1
                    self.offsets[off] += 1
                    if n > off:
                        self.overlaps[kind, off] += 1
                    if off == d:
                        self.oldest.append(d)
                    if off >= 65536:
                        self.far.append((off, len(c.out)))
                d += e[1]

"""LZ4 block streams built from sequence programs: the reference for the device LZ4 decoders on
streams no compressor here emits (tests/test_lz4_cases.py, tests/test_gpu_lz4_cases.py).

A *program* is a list of sequences `(lit_len, offset, match_len)` and a final literal run. `emit`
writes the LZ4 block stream (token, length continuation bytes 15 + 255 k + r, literals, u16 LE
offset, match length - 4 with its continuation bytes: lz4_streams.sequence) and, as it goes, the
bytes the stream stands for: a literal's bytes (from random.Random) are appended, a match is copied
byte by byte from the generator's own output. No decoder takes part, so these bytes are the
reference: liblz4, the C oracle and make_golden.lz4_decompress_safe are checked against them
(test_lz4_cases.py), not trusted.

A *block* is the i32 LE size prefix, the stream and tag 3 (compress::encode with
CompressOptions::Lz4, src/block/compress.rs:73-77). lz4::block::decompress(data, None)
(compress.rs:108-111) runs LZ4_decompress_safe with the prefix as the output limit and keeps the
bytes it returns, so a valid program is also valid under a larger prefix: the expected bytes and
the expected decoded length stay the program's.

Valid programs follow liblz4 1.9.3's end-of-buffer rules (oracle/tpz_lz4.c:53-173, lz4_walk in
tpz_codec.hip): the last sequence is literals only, at least 5 of them; the last match starts at
least 12 bytes before the end of the output; 1 <= offset <= bytes produced.

Everything is seeded: two calls give identical bytes. Pure Python, no numpy."""
import functools
import random
from collections import Counter, namedtuple

from lz4_streams import sequence

LITERAL_LENGTHS = (0, 1, 14, 15, 16, 64, 65, 80, 81, 127, 128, 129, 269, 270, 271, 300, 1000,
                   2000, 4000, 70000)
MATCH_LENGTHS = (4, 5, 18, 19, 20, 63, 64, 65, 67, 68, 127, 128, 129, 273, 274, 300, 1000, 70000)
OFFSETS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 112, 119, 120, 121,
           127, 128, 129, 136, 150, 191, 192, 193, 255, 256, 257, 4095, 4096, 65534, 65535)
FINALS = (5, 6, 12, 13, 64, 100)
RAISES = (1, 11, 64)                    # each valid program also with its prefix raised by these
RING_MAX = 1000                         # lengths up to here fit the ring's 16-byte header window

# the device's window sizes (tpz_codec.hip: kSmallIn / kSmallOut, kBigIn / kBigOut, kInSlack 32,
# 16 bytes of output slack): which wave-side decoder takes a block the lane kernels left
SMALL_IN, SMALL_OUT, BIG_IN, BIG_OUT = 4608, 5120, 65536, 94208

Case = namedtuple("Case", "name program final stream out")   # a valid stream and its bytes
Bad = namedtuple("Bad", "name rule block")                   # a block the reference rejects
Emitted = namedtuple("Emitted", "pieces lits out at")


def emit_parts(program, final, rng):
    """The stream of a program sequence by sequence: (the encoded sequences, the final one last;
    their literal bytes; the output bytes; the bytes produced before each match)."""
    pieces, lits, at = [], [], []
    out = bytearray()
    for ll, off, ml in program:
        data = rng.randbytes(ll)
        out += data
        d = len(out)
        assert ml >= 4 and 1 <= off <= d and off < 1 << 16, ((ll, off, ml), d)
        pieces.append(sequence(data, off, ml))
        lits.append(data)
        at.append(d)
        for _ in range(ml):                                  # byte by byte: overlaps repeat
            out.append(out[-off])
    data = rng.randbytes(final)
    out += data
    pieces.append(sequence(data, None, 0))
    lits.append(data)
    # liblz4's rules for a stream it accepts at its exact length
    assert final >= 5, final
    assert not program or final + program[-1][2] >= 12, (program[-1], final)
    return Emitted(pieces, lits, bytes(out), at)


def emit(program, final, rng):
    """(stream, output bytes) of a program."""
    e = emit_parts(program, final, rng)
    return b"".join(e.pieces), e.out


def case(name, program, final, rng):
    stream, out = emit(program, final, rng)
    return Case(name, tuple(program), final, stream, out)


def block_of(c, raise_by=0):
    """The tag-3 block of a valid case, its prefix raised by `raise_by`."""
    return (len(c.out) + raise_by).to_bytes(4, "little") + c.stream + b"\x03"


def produced(program):
    return sum(ll + ml for ll, _off, ml in program)


def max_length(c):
    """The longest literal or match of a case."""
    return max([c.final] + [max(ll, ml) for ll, _off, ml in c.program])


# ------------------------------------------------------------------ classes
def lit_class(n):
    """short: in the token; 15-class: one continuation byte; long: two or more."""
    return "short" if n < 15 else "15" if n < 270 else "long"


def match_class(n):
    return "short" if n - 4 < 15 else "15" if n - 4 < 270 else "long"


LIT_RANGES = {"short": (1, 14), "15": (15, 269), "long": (270, 600)}
MATCH_RANGES = {"short": (4, 18), "15": (19, 273), "long": (274, 600)}


# ------------------------------------------------------------------ random parts
def rand_offset(rng, d):
    """An offset valid after d >= 1 output bytes, of every class."""
    d = min(d, 65535)
    r = rng.random()
    return rng.randint(1, min(15, d)) if r < 0.3 else rng.randint(1, min(200, d)) if r < 0.7 \
        else rng.randint(1, d) if r < 0.9 else d


def rand_lit(rng):
    r = rng.random()
    return 0 if r < 0.25 else rng.randint(1, 14) if r < 0.65 else rng.randint(15, 90) if r < 0.95 \
        else rng.randint(91, 400)


def rand_match(rng):
    r = rng.random()
    return rng.randint(4, 18) if r < 0.55 else rng.randint(19, 140) if r < 0.93 \
        else rng.randint(141, 700)


def rand_sequence(rng, d):
    ll = rand_lit(rng)
    if d + ll == 0:
        ll = rng.randint(1, 14)
    return (ll, rand_offset(rng, d + ll), rand_match(rng))


def final_for(rng, program):
    """A final literal run the last match allows."""
    need = max(5, 12 - program[-1][2]) if program else 5
    return rng.choice([f for f in FINALS if f >= need])


def bulk(rng, target):
    """Sequences that produce exactly `target` bytes, every length at most RING_MAX (the ring
    decodes them: no header outruns its window)."""
    assert target >= 5
    prog, d = [], 0
    while d < target:
        left = target - d
        if left > 4 * RING_MAX:
            ll, ml = rng.randint(1, RING_MAX), rng.randint(4, RING_MAX)
        elif left > 2 * RING_MAX:                            # (leaves more than RING_MAX)
            ll, ml = rng.randint(1, RING_MAX // 2), rng.randint(4, RING_MAX // 2)
        else:                                                # the last one: exactly what is left
            ml = rng.randint(max(4, left - RING_MAX), min(RING_MAX, left - 1))
            ll = left - ml
        prog.append((ll, rand_offset(rng, d + ll), ml))
        d += ll + ml
    assert produced(prog) == target and all(1 <= ll <= RING_MAX and 4 <= ml <= RING_MAX
                                            for ll, _o, ml in prog)
    return prog


# ------------------------------------------------------------------ the valid programs
def window_programs():
    """Literal lengths 0..20 between matches of each length class, twice in a row: the ring's
    16-byte header window (refilled below 8 bytes) at every residue a literal leaves in it."""
    rng = random.Random(0x4C01)
    cases = []
    for L in range(0, 21):
        for mc in MATCH_RANGES:
            prog = [(5, 3, 8)]
            for _ in range(2):
                prog.append((L, rand_offset(rng, produced(prog) + L), rng.randint(*MATCH_RANGES[mc])))
            cases.append(case(f"window_L{L}_{mc}", prog, final_for(rng, prog), rng))
    return cases


def literal_programs():
    """Every listed literal length as a stream's first literal, as a literal after a match (0: a
    match directly after a match) and as the final run."""
    rng = random.Random(0x4C02)
    cases = []
    for L in LITERAL_LENGTHS:
        if L:
            prog = [(L, rand_offset(rng, L), rand_match(rng))]
            cases.append(case(f"literal_{L}_first", prog, final_for(rng, prog), rng))
        for rep in range(2):
            prog = [rand_sequence(rng, 0)]
            prog.append((L, rand_offset(rng, produced(prog) + L), rand_match(rng)))
            prog.append(rand_sequence(rng, produced(prog)))
            cases.append(case(f"literal_{L}_mid{rep}", prog, final_for(rng, prog), rng))
        if L >= 5:
            cases.append(case(f"literal_{L}_final", [(3, 2, 9)], L, rng))
    return cases


def match_programs():
    """Every listed match length at offsets of each path of the ring: the period registers (below
    16), the shortened steps (16..63), the ring and the stored lines."""
    rng = random.Random(0x4C03)
    cases = []
    for M in MATCH_LENGTHS:
        for off in ((3, 33, 200) if M > RING_MAX else (1, 7, 16, 33, 64, 150, 200, 300)):
            prog = [(off + rng.randint(0, 9), off, M)]
            prog.append(rand_sequence(rng, produced(prog)))
            cases.append(case(f"match_{M}_off{off}", prog, final_for(rng, prog), rng))
    return cases


def offset_programs():
    """Every listed offset with a match shorter than it (the format has none below offset 5: a
    match is at least 4 bytes), equal to it (from offset 4) and longer than it; below 64 also with
    a match of more than 128 bytes (three ring steps or more). The first match starts at most 40
    bytes after the oldest byte it can reach. Offsets above RING_MAX: behind one long literal, and
    (the shorter match) behind sequences the ring decodes."""
    rng = random.Random(0x4C04)
    cases = []
    for off in OFFSETS:
        variants = []
        if off >= 5:
            variants.append(("lt", rng.randint(4, min(off - 1, 300))))
        if off >= 4:
            variants.append(("eq", off))
        variants.append(("gt", max(4, off + rng.randint(1, 70))))
        if off < 64:
            variants.append(("steps", rng.randint(129, 400)))
        for vname, ml in variants:
            first = off if off >= 65534 else off + rng.randint(0, 40)
            prog = [(first, off, ml)]
            ll = rand_lit(rng)
            prog.append((ll, off, rand_match(rng)))
            cases.append(case(f"offset_{off}_{vname}", prog, final_for(rng, prog), rng))
            if off > RING_MAX and vname == "lt":
                ll = rng.randint(1, 14)
                prog = bulk(rng, off - ll + (0 if off >= 65534 else rng.randint(0, 40)))
                prog.append((ll, off, ml))
                prog.append((rand_lit(rng), off, rand_match(rng)))
                cases.append(case(f"offset_{off}_lt_ring", prog, final_for(rng, prog), rng))
    return cases


def pair_programs():
    """Every ordered pair of {short, 15-class, long literal} x {short, 15-class, long match} as
    neighbours: the literal before the match (one sequence) and the match before the literal (the
    next sequence's)."""
    rng = random.Random(0x4C05)
    cases = []
    for lc in LIT_RANGES:
        for mc in MATCH_RANGES:
            for lc2 in LIT_RANGES:
                ll = rng.randint(*LIT_RANGES[lc])
                prog = [(ll, rand_offset(rng, ll), rng.randint(*MATCH_RANGES[mc]))]
                ll2 = rng.randint(*LIT_RANGES[lc2])
                prog.append((ll2, rand_offset(rng, produced(prog) + ll2), rand_match(rng)))
                cases.append(case(f"pair_{lc}_{mc}_{lc2}", prog, final_for(rng, prog), rng))
    return cases


def final_programs():
    """Every listed final literal run after zero, one and several sequences."""
    rng = random.Random(0x4C06)
    cases = []
    for f in FINALS:
        for nseq in (0, 1, 4):
            prog = []
            for _ in range(nseq):
                prog.append(rand_sequence(rng, produced(prog)))
            if prog and f + prog[-1][2] < 12:
                ll, off, ml = prog[-1]
                prog[-1] = (ll, off, 12 - f)
            cases.append(case(f"final_{f}_after{nseq}", prog, f, rng))
    return cases


def random_programs(n=160):
    """Random programs of 1-24 sequences."""
    rng = random.Random(0x4C07)
    cases = []
    for i in range(n):
        prog = []
        for _ in range(rng.randint(1, 24)):
            prog.append(rand_sequence(rng, produced(prog)))
        cases.append(case(f"random_{i}", prog, final_for(rng, prog), rng))
    return cases


@functools.lru_cache(maxsize=None)
def valid_cases():
    """Every valid case, in a fixed order."""
    cases = window_programs() + literal_programs() + match_programs() + offset_programs() + \
        pair_programs() + final_programs() + random_programs()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


# ------------------------------------------------------------------ the named invalid streams
def blk(prefix, stream):
    return (prefix & 0xFFFFFFFF).to_bytes(4, "little") + bytes(stream) + b"\x03"


def _last_match_faults(tag, program, final, rng):
    """The faults at the last match of a valid program: built at three sizes (size_class)."""
    e = emit_parts(program, final, rng)
    k = len(program) - 1
    ll, _off, ml = program[k]
    n = len(e.out)
    head = b"".join(e.pieces[:k])
    bad = [
        Bad(f"offset_past_output_last@{tag}", "a match's offset is at most the bytes produced",
            blk(n, head + sequence(e.lits[k], e.at[k] + 1, ml) + e.pieces[-1])),
        Bad(f"ends_in_match@{tag}", "the last sequence is literals only",
            blk(n - final, b"".join(e.pieces[:-1]))),
        Bad(f"match_in_last_5@{tag}", "a match ends at least 5 bytes before the end of the output",
            blk(n - final + 4, b"".join(e.pieces[:-1]) + sequence(e.lits[-1][:4], None, 0))),
    ]
    return bad


def _faults(tag, program, final, rng):
    """Every named invalid stream one byte or one value away from a valid program whose last
    match is 19 bytes or more (liblz4 checks such a match against the end of the output on
    every path)."""
    assert program[-1][2] >= 19
    e = emit_parts(program, final, rng)
    k = len(program) - 1
    n = len(e.out)
    stream = b"".join(e.pieces)
    body = b"".join(e.pieces[:-1])
    bad = []

    def add(name, rule, prefix, s):
        bad.append(Bad(f"{name}@{tag}", rule, blk(prefix, s)))

    ll, _off, ml = program[0]
    add("offset_past_output_first", "a match's offset is at most the bytes produced", n,
        sequence(e.lits[0], e.at[0] + 1, ml) + b"".join(e.pieces[1:]))
    ll, _off, ml = program[k]
    assert e.at[k] < 65535
    add("offset_65535_short", "a match's offset is at most the bytes produced", n,
        b"".join(e.pieces[:k]) + sequence(e.lits[k], 65535, ml) + e.pieces[-1])
    add("literal_past_input", "a literal's bytes lie inside the input", n, stream[:-1])
    add("cut_literal_length", "a length's continuation bytes lie inside the input",
        n - final + 300, body + b"\xF0\xFF")
    cut = sequence(e.lits[k], 7, 300)
    assert cut[-2:] == b"\xFF\x1A"
    add("cut_match_length", "a length's continuation bytes lie inside the input", e.at[k] + 300,
        b"".join(e.pieces[:k]) + cut[:-1])
    add("output_one_longer", "no sequence writes past the prefix", n - 1, stream)
    add("literal_into_last_12", "a literal run into the last 12 output bytes is the last sequence",
        n - final + 12, body + sequence(rng.randbytes(3), 4, 4) + sequence(rng.randbytes(5), None, 0))
    add("prefix_above_limit", "the prefix is at most 0x7E000000", 0x7E000001, stream)
    add("prefix_negative", "the prefix is not negative", 0x80000000 + n, stream)
    add("prefix_minus_one", "the prefix is not negative", 0xFFFFFFFF, stream)
    return bad + _last_match_faults(tag, program, final, rng)


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """Every named invalid block: all of them behind two short programs, the last-match faults
    also past the 16-wave windows and past the one-wave windows (by the compressed length, and by
    the output alone); sources shorter than 4 bytes."""
    rng = random.Random(0x4C08)
    bad = _faults("small", [(20, 7, 30), (3, 20, 40)], 8, rng)
    bad += _faults("small15", [(15, 15, 19), (0, 1, 270), (14, 300, 289)], 5, rng)
    bad += _last_match_faults("big", [(6000, 100, 40), (10, 3000, 300)], 8, rng)
    # (an offset has 16 bits: the last match stands below 65,535 output bytes in each)
    bad += _last_match_faults("global_in", [(65000, 9, 4), (500, 100, 300)], 9, rng)
    bad += _last_match_faults("global_out", [(10, 3, 30), (4, 20, 95000)], 7, rng)
    for k in range(4):
        bad.append(Bad(f"source_{k}_bytes", "the source holds the 4-byte prefix",
                       bytes([9, 0, 0][:k]) + b"\x03"))
    assert len({b.name for b in bad}) == len(bad)
    return tuple(bad)


def last_match_faults():
    """The last-match faults of invalid_cases by size: {"small" | "big" | "global": [Bad]}."""
    by = {"small": [], "big": [], "global": []}
    for b in invalid_cases():
        if b.name.split("@")[0] in ("offset_past_output_last", "ends_in_match", "match_in_last_5"):
            by[size_class(b.block)].append(b)
    return by


@functools.lru_cache(maxsize=None)
def offset_zero_cases():
    """Valid programs with one match's offset set to 0: not an error for liblz4 as the oracle
    restates it (the match reads zeros). [(name, block)]: the expected status and bytes are the
    oracle's, nothing is assumed here."""
    rng = random.Random(0x4C09)
    out = []
    progs = [("short", [(9, 4, 7), (2, 5, 30), (0, 1, 5)], 12),
             ("steps", [(40, 40, 300), (17, 33, 150), (1, 200, 70)], 12),
             ("long", [(300, 150, 1000), (0, 7, 20), (70, 1, 64)], 64)]
    for pname, prog, final in progs:
        e = emit_parts(prog, final, rng)
        for k, (ll, _off, ml) in enumerate(prog):
            s = b"".join(e.pieces[:k]) + sequence(e.lits[k], 0, ml) + b"".join(e.pieces[k + 1:])
            out.append((f"offset_0_{pname}_{k}", blk(len(e.out), s)))
    return tuple(out)


# ------------------------------------------------------------------ what the programs reach
def size_class(block):
    """The wave-side windows a block fits with its prefix as the claimed size (tpz_codec.hip,
    lz4_block: `fits`): the 16-wave kernel's, the one-wave kernel's, or neither (HBM to HBM)."""
    n = len(block) - 1
    dn = int.from_bytes(block[:4], "little") + 1
    if n + 32 <= SMALL_IN and dn + 16 <= SMALL_OUT:
        return "small"
    if n + 32 <= BIG_IN and dn + 16 <= BIG_OUT:
        return "big"
    return "global"


def header_window_ok(stream):
    """Whether the ring's header parse (tpz_codec.hip, ring_body<3>) finds every field of a
    well-formed stream inside its window: 16 bytes, refilled when fewer than 8 are left after a
    header (and its literal). False: the parse sets `bad` and the lane kernel takes the block."""
    n, ip, hvv = len(stream), 0, 16
    need_off = False
    while ip < n:
        o, lit, is_lit = 0, 0, False
        if not need_off:
            t = stream[ip]
            lit, mln, o = t >> 4, t & 15, 1
            if lit == 15:
                while True:
                    if o >= hvv:
                        return False
                    x = stream[ip + o]
                    lit += x
                    o += 1
                    if x != 255:
                        break
            is_lit = lit > 0
        if not is_lit:
            if o + 2 > hvv:
                return False
            o += 2
            if mln == 15:
                while True:
                    if o >= hvv:
                        return False
                    x = stream[ip + o]
                    o += 1
                    if x != 255:
                        break
        used = o + lit if is_lit else o
        ip += used
        need_off = is_lit
        hvv = hvv - used if used < hvv else 0
        if hvv < 8 and ip < n:
            hvv = 16
    return True


class Reach:
    """Counts of the shapes a set of cases holds."""

    def __init__(self, cases):
        self.lit_lengths = Counter()      # literal length (0: a match directly after a match)
        self.match_lengths = Counter()
        self.offsets = Counter()
        self.relation = Counter()         # (offset, "lt" | "eq" | "gt"): the match against it
        self.steps3 = Counter()           # offsets below 64 with a match of more than 128 bytes
        self.lit_match = Counter()        # (literal class, match class) of one sequence
        self.match_lit = Counter()        # (match class, the next sequence's literal class)
        self.finals = Counter()
        self.after = Counter()            # (final run, sequences before it: 0, 1, "more")
        for c in cases:
            for i, (ll, off, ml) in enumerate(c.program):
                if ll or i:
                    self.lit_lengths[ll] += 1
                self.match_lengths[ml] += 1
                self.offsets[off] += 1
                self.relation[off, "lt" if ml < off else "eq" if ml == off else "gt"] += 1
                if off < 64 and ml > 128:
                    self.steps3[off] += 1
                if ll:
                    self.lit_match[lit_class(ll), match_class(ml)] += 1
                nxt = c.program[i + 1][0] if i + 1 < len(c.program) else 0
                if nxt:
                    self.match_lit[match_class(ml), lit_class(nxt)] += 1
            self.lit_lengths[c.final] += 1
            self.finals[c.final] += 1
            self.after[c.final, min(len(c.program), 2)] += 1

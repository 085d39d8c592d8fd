"""The regular-block copy's index arithmetic (tpz_decode.hip: reg_recip, reg_div, reg_entry),
restated in Python and checked against plain integer division and a byte-by-byte model of the
block's output stream. No GPU.

A regular block has n entries at db + i S, S = 4 + KL + VL, every key KL and every value VL bytes
(both >= 16). Its stream is the n keys back to back, then from vs = value_start(n KL) the n
values. Output chunk c covers stream bytes [16 c, 16 c + 16)."""
import numpy as np
import pytest

SHIFT = 26                       # kRegShift
MAX_DIVIDEND = 4352              # a wave-path stream is shorter (kWinBytes)
DIVISORS = range(16, 4337)       # 16 .. kWaveMaxLen


def reg_div(y, m):
    """reg_div: (y * m) >> 26, the factors cut to 13 and 23 bits, the quotient to 10."""
    return (((y & 0x1FFF) * (m & 0x7FFFFF)) >> SHIFT) & 0x3FF


def test_reciprocal_division_is_exact():
    """Every divisor, every dividend, every multiplier the kernel can come to use:
    floor(2^26 / d) + 1 .. + 3."""
    y = np.arange(MAX_DIVIDEND, dtype=np.int64)
    for d in DIVISORS:
        want = y // d
        f = (1 << SHIFT) // d
        for m in (f + 1, f + 2, f + 3):
            assert m < (1 << 23) and 0 <= m * d - (1 << SHIFT) < (1 << SHIFT) // MAX_DIVIDEND
            np.testing.assert_array_equal(reg_div(y, m), want, err_msg=f"d={d} m={m}")


def test_kernel_multiplier_lies_in_the_exact_range():
    """reg_recip: trunc(rcp(d) * 2^26) + 2 in float32, for a reciprocal within 1 ulp of 1 / d
    (v_rcp_f32's bound): the correctly rounded one and both neighbours."""
    d = np.array(list(DIVISORS), np.int64)
    r = (np.float32(1.0) / d.astype(np.float32)).astype(np.float32)
    f = (1 << SHIFT) // d
    for rcp in (np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(1))):
        m = (rcp * np.float32(1 << SHIFT)).astype(np.float32).astype(np.int64) + 2
        assert ((m >= f + 1) & (m <= f + 3)).all(), d[(m < f + 1) | (m > f + 3)][:8]


def reg_entry(x0, n, KL, VL, db, isk):
    """reg_entry: (e0, d0, d1) of the chunk at x0; isk: the chunk starts in the keys."""
    kc = n * KL
    vs = (kc + 15) & ~15
    S = 4 + KL + VL
    mk, mv = (1 << SHIFT) // KL + 2, (1 << SHIFT) // VL + 2
    gap = (2 + KL) - vs - (n - 1) * (4 + VL)
    L, base = (KL, 0) if isk else (VL, vs)
    T = S - L
    j = reg_div(x0 - base, mk if isk else mv)
    assert j == (x0 - base) // L
    last = j + 1 == n
    e0 = 0xFFFF if (not isk and last) else base + (j + 1) * L
    d0 = (db + 2 if isk else db + 4 + KL - vs) + j * T
    d1 = d0 + (gap if (isk and last) else T)
    return e0, d0, d1


def chunk_sources(c, n, KL, VL, db):
    """The source offset of each of chunk c's 16 bytes, as the copy assembles it: bytes before
    e0 from x + d0, the others (a crossing) from x + d1."""
    kc = n * KL
    vs = (kc + 15) & ~15
    x0 = 16 * c
    w = c // 64
    # (the kernel picks the scalar form for a window wholly in one region: the same values)
    if 1024 * (w + 1) <= kc:
        isk = True
    elif 1024 * w >= vs:
        isk = False
    else:
        isk = x0 < kc
    assert isk == (x0 < kc)
    e0, d0, d1 = reg_entry(x0, n, KL, VL, db, isk)
    cross = e0 < x0 + 16
    split = e0 - x0 if cross else 16
    assert not cross or 0 < split < 16
    return [x0 + i + (d0 if i < split else d1) for i in range(16)], cross


def stream_model(n, KL, VL, db):
    """Source offset of every stream byte, entry by entry, byte by byte (-1: the key/value gap)."""
    S = 4 + KL + VL
    kc = n * KL
    vs = (kc + 15) & ~15
    src = [-1] * (vs + n * VL)
    for i in range(n):
        for t in range(KL):
            src[i * KL + t] = db + i * S + 2 + t
        for t in range(VL):
            src[vs + i * VL + t] = db + i * S + 4 + KL + t
    return src


SHAPES = [(n, kl, vl) for kl in (16, 17, 31, 32, 48) for vl in (16, 17, 100, 1000, 4000)
          for n in (1, 2, 3, 34, 63, 64, 65, min(255, 4329 // (6 + kl + vl)))
          if 1 <= n <= min(255, 4329 // (6 + kl + vl))]
SHAPES += [(1, 16, 4309), (1, 4309, 16), (2, 2000, 160), (120, 16, 16), (7, 300, 301)]


@pytest.mark.parametrize("db", [2 + 2 * 34, 15 + 2 + 2 * 255])
def test_chunks_against_the_stream_model(db):
    for n, KL, VL in SHAPES:
        S = 4 + KL + VL
        want = stream_model(n, KL, VL, db)
        kc, tot = n * KL, len(want)
        vs = (kc + 15) & ~15
        for c in range((tot + 15) // 16):
            got, cross = chunk_sources(c, n, KL, VL, db)
            for i, g in enumerate(got):
                x = 16 * c + i
                # every read stays in the block's entries or the 16 bytes after them
                assert db <= g < db + n * S + 16, (n, KL, VL, c, i, g)
                if x < tot and want[x] >= 0:
                    assert g == want[x], (n, KL, VL, c, i)
                elif kc <= x < vs:
                    # the gap: what the general path reads there, the bytes before value 0
                    assert g == db + 4 + KL - (vs - x), (n, KL, VL, c, i)
            # a chunk crosses where an entry ends inside it, and only there
            x0 = 16 * c
            ends = [e for e in list(range(KL, kc + 1, KL)) + list(range(vs + VL, tot, VL))
                    if x0 < e < x0 + 16]
            assert cross == bool(ends), (n, KL, VL, c)

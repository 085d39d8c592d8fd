"""The regular path's dword index (tpz_decode.hip: reg_eligible, reg_dwords, dw_unpack and the
DW gathers of copy_crc_piped<.., REG, DW>), restated in Python beside the packed word it is made
from (reg_pack, restated as pack in test_regular_cache_pack.py). No GPU.

When a regular block's key and value lengths are both multiples of 4, every entry boundary of its
output stream falls on a dword of its chunk, so output dword k of chunk c = 64 w + lane is four
whole bytes of one source. A wave keeps, per lane and copy window 0-3, two words:
  lo = f_0 | f_1 << 16,  hi = f_2 | f_3 << 16,  f_k = (4 k < m ? A : B) + 4 k
with A, B, m the fields of the packed word (the chunk's source, its successor's, the bytes before
the boundary; all relative to db, which changes with every block and is added on use); no chunk c:
both words 0, and the reads go to the zeroed guard. The copy reads, per dword, the aligned LDS
dword under db + f_k and its neighbour (ds_read2_b32) and shifts the four bytes out
(v_alignbyte_b32 by the address's low two bits).

For every n in 1..255 and every KL, VL in 16..4336 that are multiples of 4 and fit a wave block,
the bytes those four reads take must be the bytes of merge_at(gather(d0), gather(d1), m), for every
lane and window, and every field must fit its width. That is checked on the source offsets for
every geometry (the sources are relative to db, so db's alignment does not enter), and on real
bytes, through a model of the aligned reads and the byte shift, at all 16 start alignments of db
for a grid of geometries. A geometry with a length that is no multiple of 4 is never eligible."""
import numpy as np
import pytest

from test_regular_cache_pack import BIAS, NO_CHUNK, WAVE_MAX_LEN, closed_form, fits, pack

GUARD = 96                                          # kGuard
LENGTHS = (16, 20, 24, 28, 32, 48, 100, 256, 1000, 1024, 2044, 4000)


def reg_eligible(KL, VL):
    return ((KL | VL) & 3) == 0


def reg_dwords(word):
    """reg_dwords: (lo, hi) of packed words (any shape), in the kernel's 32-bit arithmetic."""
    M = 0xFFFFFFFF
    word = word.astype(np.int64)
    A, B, m = word & 0x1FFF, (((word >> 13) & 0x1FFF) - BIAS) & M, (word >> 26) & 31
    f = [(np.where(4 * k < m, A, B) + 4 * k) & M for k in range(4)]
    none = (word >> 31) != 0
    lo = np.where(none, 0, (f[0] | (f[1] << 16)) & M)
    hi = np.where(none, 0, (f[2] | (f[3] << 16)) & M)
    return lo, hi


def dw_fields(lo, hi):
    """dw_unpack without the base: the four offsets, and whether the lane has a chunk."""
    return [lo & 0xFFFF, lo >> 16, hi & 0xFFFF, hi >> 16], lo != 0


def pack_many(n, KL, VLs):
    """reg_pack for windows 0-3 of (n, KL, VL) for every VL of VLs at once: arrays [VL, chunk] of
    the packed word and of the closed form's act, cross, A = x0 + d0, B = x0 + d1, m = e0 - x0."""
    VL = np.asarray(VLs, np.int64)[:, None]
    x0 = 16 * np.arange(256, dtype=np.int64)[None, :]
    kc = n * KL
    vs = (kc + 15) & ~15
    isk = x0 < kc
    L = np.where(isk, KL, VL)
    base = np.where(isk, 0, vs)
    T = 4 + KL + VL - L
    j = (x0 - base) // L
    last = j + 1 == n
    e0 = np.where(~isk & last, 0xFFFF, base + (j + 1) * L)
    d0 = np.where(isk, 2, 4 + KL - vs) + j * T
    d1 = d0 + np.where(isk & last, (2 + KL) - vs - (n - 1) * (4 + VL), T)
    act = x0 // 16 < (vs + n * VL + 15) >> 4
    cross = e0 < x0 + 16
    A, B, m = x0 + d0, x0 + d1, e0 - x0
    M = 0xFFFFFFFF
    word = np.where(cross, (A & 0x1FFF) | (((B + BIAS) & 0x1FFF) << 13) | ((m << 26) & M),
                    (A & 0x1FFF) | (16 << 26))
    return np.where(act, word, NO_CHUNK), act, act & cross, A, B, m


def check_offsets(n, KL, VLs):
    """Every chunk of windows 0-3 of every (n, KL, VL): byte i of the chunk comes from A + i
    before the boundary (i < m) and from B + i after it; dword k's four bytes, f_k .. f_k + 3,
    must be those (its first and its last byte decide: a side, once left, is not come back to)."""
    word, act, cross, A, B, m = pack_many(n, KL, VLs)
    t = (n, KL)
    lo, hi = reg_dwords(word)
    f, has = dw_fields(lo, hi)
    assert (has == act).all(), t
    assert (lo[~act] == 0).all() and (hi[~act] == 0).all(), t
    assert (m[cross] % 4 == 0).all() and (m[cross] >= 4).all() and (m[cross] <= 12).all(), t
    split = np.where(cross, m, 16)
    for k in range(4):
        assert (f[k][act] < (1 << 13)).all(), t                     # the field's width
        for i in (4 * k, 4 * k + 3):
            want = np.where(i < split, A, B) + i
            assert (f[k][act] + (i - 4 * k) == want[act]).all(), (t, k, i)
    # every source lies in the entries region: at or after db, and ends within 16 bytes of its end
    top = n * (4 + KL + np.asarray(VLs, np.int64))[:, None] + 16
    assert (f[0][act] >= 2).all() and ((f[3] + 4 <= top) | ~act).all(), t
    return int(act.size)


def test_pack_many_is_pack():
    """The batched restatement above against test_regular_cache_pack.pack, triple by triple."""
    for n, KL, VLs in [(34, 16, (100, 16, 20)), (1, 16, (4080, 4084, 300)), (113, 16, (16,)),
                       (3, 20, (24, 1000)), (2, 2000, (152,)), (33, 17, (100, 101))]:
        word, act, cross, A, B, m = pack_many(n, KL, VLs)
        for r, VL in enumerate(VLs):
            assert fits(n, KL, VL)
            np.testing.assert_array_equal(word[r].astype(np.uint32), pack(n, KL, VL))
            a1, c1, e0, d0, d1 = closed_form(n, KL, VL)
            np.testing.assert_array_equal(act[r], a1)
            np.testing.assert_array_equal(cross[r], c1)


def test_every_eligible_geometry():
    """Every n in 1..255 and every KL, VL in 16..4336, multiples of 4, that fit a wave block."""
    seen = 0
    for n in range(1, 256):
        room = (WAVE_MAX_LEN - 7) // n - 6              # KL + VL at most
        for KL in range(16, room - 16 + 1, 4):
            VLs = np.arange(16, room - KL + 1, 4)
            assert len(VLs) and fits(n, KL, int(VLs[-1])) and not fits(n, KL, int(VLs[-1]) + 4)
            assert reg_eligible(KL, VLs).all()
            seen += check_offsets(n, KL, VLs) // 256
    assert seen > 900000


def test_other_lengths_are_never_eligible():
    L = np.arange(16, WAVE_MAX_LEN + 1, dtype=np.int64)
    KL, VL = L[:, None], L[None, :]
    odd = (KL % 4 != 0) | (VL % 4 != 0)
    assert odd.sum() > 0 and not reg_eligible(KL, VL)[odd].any()
    assert reg_eligible(KL, VL)[~odd].all()
    for shape in [(17, 100), (16, 101), (18, 22), (19, 19), (4335, 16), (16, 4333)]:
        assert not reg_eligible(*shape)


# ---------------------------------------------------------------- on real bytes
def gather(lds, x):
    """gath_issue + gath_finish: five aligned dwords from x & ~3, shifted by x & 3: 16 bytes."""
    p = x & ~3
    return bytes(lds[p + (x & 3):p + (x & 3) + 16])


def merge_at(a, w, m):
    return a[:m] + w[m:]


def read2_alignbyte(lds, a):
    """One output dword of the DW copy: the aligned dword under a and its neighbour, then
    v_alignbyte_b32(hi, lo, a & 3) = bits [8 s, 8 s + 32) of hi:lo."""
    p = a & ~3
    d0 = int.from_bytes(lds[p:p + 4], "little")
    d1 = int.from_bytes(lds[p + 4:p + 8], "little")
    return ((((d1 << 32) | d0) >> (8 * (a & 3))) & 0xFFFFFFFF).to_bytes(4, "little")


def check_bytes(rng, n, KL, VL, starts=range(16)):
    """A window of random bytes with the guard's zeros before it, the block's entries region at
    each of db = 2 + 2 n + a0: every chunk's four reads against merge_at of the two gathers."""
    assert fits(n, KL, VL) and reg_eligible(KL, VL)
    word = pack(n, KL, VL)
    lo, hi = reg_dwords(word)
    f, has = dw_fields(lo, hi)
    A = word.astype(np.int64) & 0x1FFF
    B = ((word.astype(np.int64) >> 13) & 0x1FFF) - BIAS
    m = (word.astype(np.int64) >> 26) & 31
    for a0 in starts:
        db = a0 + 2 + 2 * n
        lds = bytes(GUARD) + rng.bytes(db + n * (4 + KL + VL) + 48)   # lds[GUARD + x] = win[x]
        for c in range(256):
            if has[c]:
                d0, d1 = GUARD + db + int(A[c]), (GUARD + db + int(B[c]) if m[c] < 16 else 0)
                want = merge_at(gather(lds, d0), gather(lds, d1), int(m[c]))
                base = GUARD + db
            else:
                want, base = bytes(16), 0                         # the guard's zeros
            got = b"".join(read2_alignbyte(lds, base + int(f[k][c])) for k in range(4))
            assert got == want, (n, KL, VL, a0, c)


def test_reads_on_bytes_at_every_alignment():
    rng = np.random.default_rng(61)
    shapes = [(34, 16, 100), (33, 16, 100), (1, 16, 16), (2, 20, 24), (3, 100, 16), (34, 16, 20),
              (3, 256, 1024), (1, 2044, 2044), (1, 16, 4080), (113, 16, 16)]
    for n, KL, VL in shapes:
        check_bytes(rng, n, KL, VL)
    # the last key's chunk crosses into the key/value gap at another byte phase than the keys
    for n, KL, VL in [(1, 20, 24), (3, 20, 16), (5, 100, 16)]:
        assert (n * KL) % 16
        check_bytes(rng, n, KL, VL)


@pytest.mark.parametrize("KL", LENGTHS)
def test_length_grid_on_bytes(KL):
    """The smallest, a middle and the largest n of every pair of the grid, at the four byte phases
    of db (the 16 start alignments: test_reads_on_bytes_at_every_alignment)."""
    rng = np.random.default_rng(62 + KL)
    for VL in LENGTHS:
        top = (WAVE_MAX_LEN - 7) // (6 + KL + VL)
        for n in sorted({1, 2, top // 2, top} - {0}):
            if fits(n, KL, VL) and n <= 255:
                check_bytes(rng, n, KL, VL, range(4))

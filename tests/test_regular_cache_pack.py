"""The regular path's index cache (tpz_decode.hip: reg_pack, reg_unpack in copy_crc_piped<.., REG>,
reg_key), restated in Python next to the closed form it replaces (RegForm::entry, restated as
reg_entry in test_regular_index.py). No GPU.

A wave keeps, per lane and copy window 0-3, one word of what the gathers and the merge of chunk
c = 64 w + lane take, relative to db (which changes with every block and is added on use):
  bits  0-12  A = x0 + d0 - db, the chunk's source
  bits 13-25  B + 16, B = x0 + d1 - db, its successor's source (a crossing chunk's only, else 0)
  bits 26-30  m = e0 - x0, the bytes before the boundary (1..15), or 16: no crossing
  bit  31     no chunk c: both gathers read the guard
For every chunk of windows 0-3 the unpacked (A, B, m, cross, act) must be the closed form's, and
every field must fit its width. The cache's key is (n, KL, VL) in one word."""
import numpy as np
import pytest

from test_regular_index import reg_entry

BIAS, NO_CHUNK = 16, 0x80000000 | (16 << 26)       # kRegBias, kRegNoChunk
WAVE_MAX_LEN = 4336                                 # kWaveMaxLen
LENGTHS = (16, 17, 31, 32, 48, 100, 1000, 4000)


def fits(n, kl, vl):
    return 1 <= n <= 255 and kl >= 16 and vl >= 16 and 7 + n * (6 + kl + vl) <= WAVE_MAX_LEN


def closed_form(n, KL, VL):
    """RegForm::entry at db = 0 for chunks 0..255, with numpy: (act, cross, e0, d0, d1)."""
    c = np.arange(256, dtype=np.int64)
    x0 = 16 * c
    kc = n * KL
    vs = (kc + 15) & ~15
    S = 4 + KL + VL
    gap = (2 + KL) - vs - (n - 1) * (4 + VL)
    isk = x0 < kc
    L = np.where(isk, KL, VL)
    base = np.where(isk, 0, vs)
    T = S - L
    j = (x0 - base) // L                  # (reg_div: exact, test_regular_index.py)
    last = j + 1 == n
    e0 = np.where(~isk & last, 0xFFFF, base + (j + 1) * L)
    d0 = np.where(isk, 2, 4 + KL - vs) + j * T
    d1 = d0 + np.where(isk & last, gap, T)
    nch = (vs + n * VL + 15) >> 4
    act = c < nch
    return act, act & (e0 < x0 + 16), e0, d0, d1


def pack(n, KL, VL):
    """reg_pack for windows 0-3: 256 words, in 32-bit arithmetic as the kernel's."""
    act, _, e0, d0, d1 = closed_form(n, KL, VL)
    x0 = 16 * np.arange(256, dtype=np.int64)
    M = 0xFFFFFFFF
    cross = e0 < x0 + 16                  # (before the chunk test, as reg_pack)
    a = ((x0 + d0) & M) & 0x1FFF
    b = (((x0 + d1 + BIAS) & M) & 0x1FFF) << 13
    w = np.where(cross, a | b | (((e0 - x0) & M) << 26) & M, a | (16 << 26))
    return np.where(act, w, NO_CHUNK).astype(np.uint32)


def unpack(w):
    """reg_unpack, without db: (A, B, m, cross, act)."""
    w = w.astype(np.int64)
    m = (w >> 26) & 31
    return w & 0x1FFF, ((w >> 13) & 0x1FFF) - BIAS, m, m < 16, (w >> 31) == 0


def check(n, KL, VL):
    assert fits(n, KL, VL)
    act, cross, e0, d0, d1 = closed_form(n, KL, VL)
    x0 = 16 * np.arange(256, dtype=np.int64)
    A, B, m, ucross, uact = unpack(pack(n, KL, VL))
    t = (n, KL, VL)
    np.testing.assert_array_equal(uact, act, err_msg=str(t))
    np.testing.assert_array_equal(ucross, cross, err_msg=str(t))
    # the fields before packing fit their widths (so the masks in reg_pack cut nothing off)
    S = 4 + KL + VL
    assert ((x0 + d0)[act] >= 0).all() and ((x0 + d0)[act] + 16 <= n * S + 16).all(), t
    assert n * S + 16 < (1 << 13)
    assert ((x0 + d1 + BIAS)[cross] >= BIAS).all() and ((x0 + d1 + BIAS)[cross] < (1 << 13)).all(), t
    assert ((e0 - x0)[cross] >= 1).all() and ((e0 - x0)[cross] <= 15).all(), t
    # the unpacked values are the closed form's
    np.testing.assert_array_equal(A[act], (x0 + d0)[act], err_msg=str(t))
    np.testing.assert_array_equal(B[cross], (x0 + d1)[cross], err_msg=str(t))
    np.testing.assert_array_equal(m[cross], (e0 - x0)[cross], err_msg=str(t))
    assert (m[~cross] == 16).all() and (A[~act] == 0).all(), t
    return act, cross, A, B, m


def test_numpy_closed_form_is_reg_entry():
    """The vectorised restatement above against test_regular_index.reg_entry, chunk by chunk."""
    for n, KL, VL in [(34, 16, 100), (33, 16, 100), (3, 17, 1000), (1, 16, 4080), (113, 16, 16),
                      (65, 31, 17), (2, 2000, 160), (1, 4000, 300)]:
        act, cross, e0, d0, d1 = closed_form(n, KL, VL)
        for c in np.flatnonzero(act):
            want = reg_entry(16 * int(c), n, KL, VL, 0, 16 * int(c) < n * KL)
            assert (int(e0[c]), int(d0[c]), int(d1[c])) == want, (n, KL, VL, c)


def test_every_n_of_the_length_grid():
    """Every n that fits a wave slot for KL, VL in the grid, and the largest lengths with n = 1."""
    seen = 0
    for KL in LENGTHS:
        for VL in LENGTHS:
            for n in range(1, 256):
                if not fits(n, KL, VL):
                    break
                check(n, KL, VL)
                seen += 1
    assert seen > 1000
    top = WAVE_MAX_LEN - 7 - 6 - 16
    assert fits(1, 16, top) and not fits(1, 16, top + 1)
    check(1, 16, top)
    check(1, top, 16)
    check(1, top // 2, top + 16 - top // 2)


def test_random_triples():
    rng = np.random.default_rng(47)
    done = 0
    while done < 20000:
        n = int(rng.integers(1, 114))
        room = (WAVE_MAX_LEN - 7) // n - 6
        if room < 32:
            continue
        KL = int(rng.integers(16, room - 16 + 1))
        VL = int(rng.integers(16, room - KL + 1))
        check(n, KL, VL)
        done += 1


def test_boundaries():
    # the last key's chunk crosses into the key/value gap: its successor is what the general path
    # reads there, the bytes before value 0 (at 4 + KL from db), and stays at or after db
    for n, KL, VL in [(34, 17, 100), (1, 17, 16), (3, 31, 16), (110, 17, 16), (1, 4001, 16)]:
        act, cross, A, B, m = check(n, KL, VL)
        kc = n * KL
        vs = (kc + 15) & ~15
        c = (kc - 1) // 16
        assert kc % 16 and cross[c] and m[c] == kc - 16 * c
        assert B[c] == 4 + KL - (vs - 16 * c) and B[c] >= 0
        assert A[c] + m[c] == (n - 1) * (4 + KL + VL) + 2 + KL      # the last key's end
    # keys that end on a chunk boundary: no gap chunk, no crossing there
    act, cross, *_ = check(34, 16, 100)
    assert not cross[34 * 16 // 16 - 1]
    # the last value has no successor
    for n, KL, VL in [(34, 16, 100), (1, 16, 17), (2, 16, 31)]:
        act, cross, *_ = check(n, KL, VL)
        assert not cross[np.flatnonzero(act)[-1]]
    # n = 1
    act, cross, A, B, m = check(1, 16, 16)
    assert act.sum() == 2 and not cross.any() and list(A[:2]) == [2, 4 + 16]
    # a stream of exactly 4096 bytes fills the four windows; one byte more starts a fifth, which
    # is not in the cache (the kernel takes the closed form there)
    act, *_ = check(1, 16, 4080)
    assert act.all()
    act, *_ = check(1, 16, 4081)
    assert act.all() and (16 + 4081 + 15) // 16 == 257


def reg_key(n, KL, VL):
    return (0x80000000 | VL << 13 | KL) if n == 1 else (n << 24 | VL << 12 | KL)


def test_key_is_injective():
    """One word for (n, KL, VL): n >= 2 leaves both lengths under 4096 and n under 128, n = 1
    leaves them under 8192, and bit 31 tells the two forms apart; 0 (no index) is no block's."""
    for n in range(2, 256):
        room = (WAVE_MAX_LEN - 7) // n - 6
        if room >= 32:
            assert room - 16 < 4096 and n < 128
    assert WAVE_MAX_LEN - 7 - 6 - 16 < 8192
    rng = np.random.default_rng(48)
    for _ in range(20000):
        n = int(rng.integers(1, 114))
        room = (WAVE_MAX_LEN - 7) // n - 6
        if room < 32:
            continue
        KL = int(rng.integers(16, room - 16 + 1))
        VL = int(rng.integers(16, room - KL + 1))
        k = reg_key(n, KL, VL)
        assert 0 < k < (1 << 32)
        if k >> 31:
            back = (1, k & 0x1FFF, (k >> 13) & 0x1FFF)
        else:
            back = (k >> 24, k & 0xFFF, (k >> 12) & 0xFFF)
        assert back == (n, KL, VL)

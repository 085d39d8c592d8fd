"""tpz_merge_runs where the small cases of tests/test_gpu_merge.py do not reach: levels whose
partition kernel needs a second workgroup, 256 runs of which nearly all are empty, every key /
value length around the copy's 16-byte pieces and the lane / wave switch at every destination
offset mod 16, and key compares that are decided at every byte offset 0..40 and around 64. All
against tests/_merge_model.merge_rule through test_gpu_merge.assert_merge: n_out, every key and
value byte, every position and d_src_entry, exactly. Each test asserts from its inputs, before the
device runs, that they reach the path it is named for.
"""
import random

import numpy as np
import pytest
import torch

from _merge_model import merge_rule
from test_encode_host import pack
from test_gpu_merge import assert_merge
from topazdb_amd import _lib

pytestmark = pytest.mark.gpu

T = _lib.MERGE_TILE
PART_THREADS = 256      # merge_partition_kernel: one thread per slot


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def level_shapes(run_lens):
    """Per tree level of tpz_merge_runs: (partition slots, pairs, entry index the odd last list is
    copied through from, or None), as launch_merge computes them."""
    R = len(run_lens)
    rf = np.concatenate([[0], np.cumsum(run_lens)]).tolist()
    out, lvl = [], 0
    while (1 << lvl) < R:
        wd = 1 << lvl
        nlists = (R + wd - 1) // wd
        npairs = nlists // 2
        tiles = sum((rf[min(2 * q * wd + 2 * wd, R)] - rf[2 * q * wd] + T - 1) // T
                    for q in range(npairs))
        out.append((tiles + npairs, npairs, rf[(nlists - 1) * wd] if nlists & 1 else None))
        lvl += 1
    return out


def bulk_runs(seed: int, n_runs: int, per: int):
    """n_runs sorted runs of `per` entries: keys of 6..14 bytes drawn from a pool of about 1.5
    times the entry count (so equal keys abound, inside runs and across them, and their groups
    straddle tile boundaries), values of 0..12 bytes that name their entry."""
    rng = np.random.default_rng(seed)
    total = n_runs * per
    pool_n = total * 3 // 2
    raw = rng.bytes(14 * pool_n)
    lens = rng.integers(6, 15, pool_n).tolist()
    pool = [raw[14 * i:14 * i + l] for i, l in enumerate(lens)]
    runs = []
    for r in range(n_runs):
        keys = sorted(pool[i] for i in rng.integers(0, pool_n, per).tolist())
        vl = rng.integers(0, 13, per).tolist()
        runs.append([(k, (b"%03d.%06d...." % (r, j))[:l]) for j, (k, l) in enumerate(zip(keys, vl))])
    return runs


@pytest.mark.parametrize("n_runs,per", [(2, 150_000), (8, 40_000), (5, 60_000)])
def test_partition_takes_a_second_workgroup(ctx, n_runs, per):
    """More than 256 partition slots at a level: merge_partition_kernel's blockIdx.x > 0, and
    find_pair over several pairs of many tiles each. Five runs leave an odd list at levels 0 and
    1, copied through from entry 240,000."""
    shapes = level_shapes([per] * n_runs)
    assert max(s for s, _, _ in shapes) > PART_THREADS
    if n_runs == 2:
        assert (per + per + T - 1) // T + 1 > 256 and shapes == [((2 * per + T - 1) // T + 1, 1, None)]
    if n_runs == 8:
        assert [p for _, p, _ in shapes] == [4, 2, 1] and all(s > PART_THREADS for s, _, _ in shapes)
    if n_runs == 5:
        assert [x0 for _, _, x0 in shapes] == [4 * per, 4 * per, None] and shapes[2][0] > PART_THREADS
    runs = bulk_runs(n_runs * 1000 + 1, n_runs, per)
    merged, want = assert_merge(ctx, runs)
    assert len(want) < n_runs * per          # some entries lost to a lower run


@pytest.mark.parametrize("filled", [(3, 130, 250), (0, 255)])
def test_sparse_256_runs(ctx, filled):
    """TPZ_MERGE_MAX_RUNS runs, nearly all empty: pairs of no tiles at every level, lists that are
    copied through or merged with nothing, and the winner's run found among empty ones."""
    rng = random.Random(len(filled))
    space = [b"sparse%05d" % i + b"x" * (i % 5) for i in range(5000)]
    runs = [[] for _ in range(_lib.MERGE_MAX_RUNS)]
    for r in filled:
        runs[r] = [(k, b"%d|%d" % (r, j)) for j, k in enumerate(sorted(rng.sample(space, 3000)))]
    assert len(runs) == 256 and sum(1 for r in runs if r) == len(filled)
    assert len(set(k for r in filled for k, _ in runs[r])) < 3000 * len(filled)   # keys overlap
    shapes = level_shapes([len(r) for r in runs])
    assert len(shapes) == 8 and shapes[0][1] == 128
    merged, want = assert_merge(ctx, runs)
    assert 3000 < len(want) < 3000 * len(filled)


# ---- the copy sweep ----------------------------------------------------------------------------

COPY_LENS = sorted(set(range(1, 34)) | {47, 48, 49, 255, 256, 257, 258, 271, 272, 273, 1023, 1024,
                                        1025, 1039, 1040, 1041, 4101})


class _KeyMaker:
    """Strictly increasing keys of any lengths >= 1: a 3-byte big-endian counter (b0, b1, b2)
    leads every key of 3 or more bytes; a 2-byte key opens a new (b0, b1), a 1-byte key a new b0
    (a proper prefix sorts before its extensions)."""

    def __init__(self, rng):
        self.b, self.rng = [0, 0, 0], rng

    def key(self, n: int) -> bytes:
        b = self.b
        if n == 1:
            b[0], b[1], b[2] = b[0] + 1, 0, 0
        elif n == 2 or b[2] == 255:
            b[1], b[2] = b[1] + 1, 0
            if b[1] == 256:
                b[0], b[1] = b[0] + 1, 0
        else:
            b[2] += 1
        assert b[0] < 256
        return bytes(b[:min(n, 3)]) + self.rng.randbytes(max(0, n - 3))


def sweep_lengths(lens, min_fill: int):
    """A list of (length, is_filler) in which every length of `lens` starts at every offset
    mod 16 (offsets are running sums); fillers of min_fill .. min_fill + 15 bytes set the
    residues."""
    out, off = [], 0
    for n in lens:
        for a in range(16):
            f = (a - off) % 16
            if f:
                f += 16 if f < min_fill else 0
                out.append((f, True))
                off += f
            assert off % 16 == a
            out.append((n, False))
            off += n
    return out


def sweep_entries(seed: int):
    """Sorted, distinct-keyed entries whose keys and values cover the sweep; [(key, value,
    key_is_filler)]. The value list is independent of the key list (values carry no order)."""
    rng = random.Random(seed)
    kl = sweep_lengths(COPY_LENS, 3)
    vl = sweep_lengths([0] + COPY_LENS, 0)
    n = max(len(kl), len(vl))
    kl += [(3, True)] * (n - len(kl))
    vl += [(0, True)] * (n - len(vl))
    km = _KeyMaker(rng)
    return [(km.key(k), rng.randbytes(v), kf) for (k, kf), (v, _) in zip(kl, vl)]


def coverage(lens, pos):
    """{(length, offset mod 16)} of the entries at positions `pos` (n + 1 running sums)."""
    p = np.asarray(pos, np.int64)
    return set(zip(np.diff(p).tolist(), (p[:-1] % 16).tolist())) & {(n, a) for n in lens for a in range(16)}


def assert_sweep_is_full(want):
    wk, wkpos, wv, wvpos = pack(want)
    assert len(coverage(COPY_LENS, wkpos)) == 16 * len(COPY_LENS)
    assert len(coverage([0] + COPY_LENS, wvpos)) == 16 * (len(COPY_LENS) + 1)
    lane = _lib.MERGE_LANE_COPY_MAX          # both sides of the lane / whole-wave switch
    assert {lane - 1, lane, lane + 1, lane + 2} <= set(COPY_LENS)
    assert max(COPY_LENS) > 64 * 16 * 4      # whole-wave copy: lanes take more than four pieces


def test_copy_sweep_single_run(ctx):
    """R = 1: the output is the input; every (length, destination offset mod 16) of a key and of a
    value, source and destination offsets equal."""
    ents = [(k, v) for k, v, _ in sweep_entries(1)]
    assert all(a[0] < b[0] for a, b in zip(ents, ents[1:]))
    assert_sweep_is_full(ents)
    merged, want = assert_merge(ctx, [ents])
    assert want == ents


def test_copy_sweep_two_runs(ctx):
    """The same sweep as run 1 of two: run 0 holds copies of some filler keys, which run 1 holds
    twice (both go), with values of other lengths. The kept entries still cover every (length,
    offset), and their source and destination offsets differ by every residue mod 16."""
    rng = random.Random(2)
    ents = sweep_entries(2)
    fillers = [i for i, e in enumerate(ents) if e[2]]
    lose = set(fillers[::5])
    run0 = [(ents[i][0], ents[i][1]) for i in sorted(lose)]
    run1 = []
    for i, (k, v, _) in enumerate(ents):
        if i in lose:     # two copies of run 0's key, their value bytes no multiple of 16
            run1 += [(k, rng.randbytes(rng.choice([1, 2, 3, 5, 7, 11, 13, 17]))) for _ in range(2)]
        else:
            run1.append((k, v))
    runs = [run0, run1]
    want = [runs[r][j] for r, j in merge_rule(runs)]
    assert want == [(k, v) for k, v, _ in ents]
    assert_sweep_is_full(want)
    # source offsets (in the concatenated input columns) against destination offsets
    flat = run0 + run1
    fk, fkpos, fv, fvpos = pack(flat)
    wk, wkpos, wv, wvpos = pack(want)
    src = np.array([(len(run0) if r else 0) + j for r, j in merge_rule(runs)])
    from_run1 = src >= len(run0)
    assert from_run1.sum() == len(ents) - len(lose) and len(lose) > 100
    assert any(len(k) % 16 for k, _ in run0)
    kres = (fkpos[src].astype(np.int64) - wkpos[:-1].astype(np.int64)) % 16
    vres = (fvpos[src].astype(np.int64) - wvpos[:-1].astype(np.int64)) % 16
    assert set(kres[from_run1].tolist()) == set(range(16))
    assert set(vres[from_run1].tolist()) == set(range(16))
    assert_merge(ctx, runs)


# ---- the compare sweep -------------------------------------------------------------------------

COMPARE_AT = list(range(41)) + [63, 64, 65]


def compare_family(t: int, heads):
    """Keys of runs 0 and 1 that share their first t bytes (three sub-families with one leading
    byte each; t = 0 has no shared bytes): pairs that differ at byte t by 0x00 / 0x01 and
    0x7f / 0x80 with the smaller key in either run, a key of t bytes against its extensions in
    either run, and an equal key of t bytes in both runs."""
    def prefix(head):
        return (bytes([head]) + bytes((7 * j + 3 * t + 1) & 0xFF for j in range(1, t)))[:t]
    p, q, r = (prefix(h) for h in heads)
    run0 = [p + b"\x01", p + b"\x7fzz", p + b"\x00\xaa", p + b"\x80\xbb\xbb"]
    run1 = [p + b"\x00", p + b"\x80zz", p + b"\x01\xaa", p + b"\x7f\xbb\xbb"]
    if t:
        run0 += [p, q, r + b"\x00", r + b"\x00\x00"]              # p in both runs: run 0's wins
        run1 += [p, q + b"\x00", q + b"\xff" * 9, r]
    return run0, run1


def common_prefix(a: bytes, b: bytes) -> int:
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def test_compare_sweep(ctx):
    """Keys compared at every offset: inside the 8-byte prefix, in tail_cmp's 8-byte loop, in its
    byte tail, and by length alone."""
    heads = [h for h in range(0x02, 0x100) if h not in (0x7f, 0x80)]
    run0, run1 = [], []
    for i, t in enumerate(COMPARE_AT):
        a, b = compare_family(t, heads[3 * i:3 * i + 3])
        run0 += a
        run1 += b
    assert len(set(run0)) == len(run0) and len(set(run1)) == len(run1)
    # what the families hold, read back from the keys themselves
    differ, extend, equal = set(), set(), set()
    for k0 in run0:
        for k1 in run1:
            c = common_prefix(k0, k1)
            if c < min(len(k0), len(k1)):
                differ.add((c, k0[c], k1[c]))
            elif len(k0) != len(k1):
                extend.add((c, len(k0) < len(k1)))
            else:
                equal.add(c)
    for t in COMPARE_AT:
        assert {(t, 0x01, 0x00), (t, 0x00, 0x01), (t, 0x7f, 0x80), (t, 0x80, 0x7f)} <= differ
        if t:
            assert {(t, True), (t, False)} <= extend and t in equal
    runs = [[(k, b"%d|%d" % (r, j)) for j, k in enumerate(sorted(keys))]
            for r, keys in enumerate((run0, run1))]
    merged, want = assert_merge(ctx, runs)
    assert len(want) == len(run0) + len(run1) - (len(COMPARE_AT) - 1)    # run 1's equal keys go
    assert all(v.startswith(b"0|") for k, v in want if k in set(run1) and k in set(run0))

"""tests/_crc_combine.py (the reference of the tests over objects longer than 2^32 bytes) against
zlib.crc32 of the concatenation."""
import zlib

import numpy as np

from _crc_combine import crc32_combine, crc32_of_segments, periodic_segments


def test_random_pairs():
    rng = np.random.default_rng(1)
    for _ in range(200):
        la, lb = (int(x) for x in rng.integers(0, 70001, 2))
        a, b = rng.bytes(la), rng.bytes(lb)
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def test_special_lengths():
    rng = np.random.default_rng(2)
    a = rng.bytes(12345)
    for lb in (0, 1, 1 << 16, (1 << 24) + 1):
        b = rng.bytes(lb)
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(b, zlib.crc32(a)), lb
        assert crc32_combine(0, zlib.crc32(b), lb) == zlib.crc32(b), lb      # empty a


def test_chain_of_70():
    rng = np.random.default_rng(3)
    parts = [rng.bytes(int(rng.integers(0, 5000))) for _ in range(70)]
    crc = 0
    for p in parts:
        crc = crc32_combine(crc, zlib.crc32(p), len(p))
    assert crc == zlib.crc32(b"".join(parts))


def test_segments_and_periodic():
    """The two helpers the GPU tests build their references with: repeated segments, and a
    window of an endlessly repeated shard from any phase."""
    rng = np.random.default_rng(4)
    shard = rng.bytes(1000)
    assert crc32_of_segments([(shard, 70), (b"", 3), (shard[:7], 1), (b"x", 0)]) == \
        zlib.crc32(shard * 70 + shard[:7])
    rep = shard * 9
    for start, length in ((0, 0), (0, 1000), (7, 993), (7, 994), (999, 2), (1000, 3001),
                          (123, 5000), (2500, 10), (0, 9000)):
        want = zlib.crc32(rep[start:start + length])
        assert crc32_of_segments(periodic_segments(shard, start, length)) == want, (start, length)

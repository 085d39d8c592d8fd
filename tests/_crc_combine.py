"""crc32_combine in pure Python: CRC-32 (ISO-HDLC, zlib's) of a + b from crc(a), crc(b), len(b).

Appending n zero bytes to a message is a linear map of its CRC register over GF(2): a 32 x 32 bit
matrix, the n-th power of the one-zero-bit operator. crc(a + b) = Z^(8 len_b) crc(a) ^ crc(b)
(the pre- and post-inversions cancel). The power is taken by repeated squaring, as zlib's
crc32_combine does. The tests of objects longer than 2^32 bytes build their reference from the
CRC of one shard this way; tests/test_crc_combine.py pins it to zlib.crc32(a + b).
"""
import zlib

POLY = 0xEDB88320     # reflected CRC-32 polynomial


def _times(mat, vec: int) -> int:
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1
        i += 1
    return s


def _square(mat):
    return [_times(mat, mat[i]) for i in range(32)]


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    if len_b <= 0:
        return crc_a
    odd = [POLY] + [1 << i for i in range(31)]       # the operator for one zero bit
    even = _square(odd)                               # two bits
    odd = _square(even)                               # four bits
    while True:                                       # first squaring below: one zero byte
        even = _square(odd)
        if len_b & 1:
            crc_a = _times(even, crc_a)
        len_b >>= 1
        if not len_b:
            break
        odd = _square(even)
        if len_b & 1:
            crc_a = _times(odd, crc_a)
        len_b >>= 1
        if not len_b:
            break
    return crc_a ^ crc_b


def crc32_of_segments(segments) -> int:
    """CRC-32 of the concatenation of `segments`, each (bytes-like, repeat count)."""
    crc = 0
    for data, times in segments:
        n = len(data)
        if n == 0 or times <= 0:
            continue
        # crc of `times` copies by doubling: (crc, length) of 1, 2, 4, ... copies
        acc, acc_len, pw, pw_len = 0, 0, zlib.crc32(data), n
        t = times
        while t:
            if t & 1:
                acc = crc32_combine(acc, pw, pw_len)
                acc_len += pw_len
            t >>= 1
            if t:
                pw = crc32_combine(pw, pw, pw_len)
                pw_len *= 2
        crc = crc32_combine(crc, acc, acc_len)
    return crc


def periodic_segments(shard, start: int, length: int):
    """The segments of `length` bytes from offset `start` of the endless repetition of `shard`."""
    mv = memoryview(shard)
    s = len(mv)
    ph = start % s
    head = min(length, (s - ph) % s)
    full, tail = divmod(length - head, s)
    return [(mv[ph:ph + head], 1), (mv, full), (mv[:tail], 1)]

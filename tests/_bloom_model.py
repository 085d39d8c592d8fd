"""Bloom::from_keys (src/bloom.rs:48-70) restated in numpy (test infrastructure, CPU only).

table.Bloom.from_keys walks every probe in Python: 6 M loop turns for 400,000 keys at k = 15.
`from_hashes` does the same arithmetic a probe round at a time; tests/test_bloom_model.py pins it
to Bloom.from_keys byte for byte. The geometry is table.Bloom's, not the device library's.
"""
from __future__ import annotations

import numpy as np

from topazdb_amd.table import Bloom


def from_hashes(hashes: np.ndarray, fpp: float) -> bytes:
    """Bloom::encode's bytes for the filter of `hashes` (uint64): probe j of hash h sets bit
    (h + j * rotr(h, 34)) mod limit, in wrapping u64 arithmetic; k goes in the last byte."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64).copy()
    nbytes, k = Bloom.geometry(len(h), fpp)
    filt = np.zeros(nbytes, np.uint8)
    filt[-1] = k
    limit = np.uint64((nbytes - 1) * 8)
    if len(h) == 0:
        return filt.tobytes()
    delta = (h >> np.uint64(34)) | (h << np.uint64(30))        # Bloom::delta
    one = np.uint8(1)
    for _ in range(k):
        pos = h % limit
        np.bitwise_or.at(filt, (pos >> np.uint64(3)).astype(np.int64),
                         one << (pos & np.uint64(7)).astype(np.uint8))
        h += delta                                             # wraps mod 2^64
    return filt.tobytes()

"""tests/_bloom_model.from_hashes (the numpy Bloom::from_keys the large GPU bloom cases compare
against) equals table.Bloom.from_keys byte for byte, and the kernel constants that the GPU tests
read from topazdb_amd._lib are the ones in the sources (no GPU, no library)."""
import os
import random
import re

import numpy as np
import pytest

from _bloom_model import from_hashes
from topazdb_amd import _lib
from topazdb_amd.table import Bloom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = _lib.BLOOM_SLICE_BITS


@pytest.mark.parametrize("n,fpp", [(1, 0.1), (3, 0.01), (100, 0.1), (1000, 0.3), (5000, 0.001),
                                   (3000, 1e-300)])
def test_from_hashes_matches_from_keys(n, fpp):
    rng = random.Random(n * 7 + 1)
    hs = [rng.getrandbits(64) for _ in range(n)]
    assert from_hashes(np.array(hs, np.uint64), fpp) == Bloom.from_keys(hs, fpp).encode()


def test_no_hashes():
    assert from_hashes(np.zeros(0, np.uint64), 0.1) == Bloom.from_keys([], 0.1).encode() == b"\x01"


def test_probes_at_the_ends_and_at_a_slice_boundary():
    """Hashes whose first probe is bit 0, bit limit - 1 and both sides of bit 2^19 (h < limit:
    the probe is h itself), hashes that wrap (h + delta past 2^64) and h = 0 (delta 0: every
    probe on bit 0)."""
    n, fpp = 3000, 1e-300
    nbytes, k = Bloom.geometry(n, fpp)
    limit = (nbytes - 1) * 8
    assert k == 15 and limit > 2 * SLICE
    rng = random.Random(99)
    special = [0, limit - 1, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, limit, 2 * limit - 1,
               2**64 - 1, 2**64 - limit, 2**63, (2**64 - 1) // limit * limit]
    hs = special + [rng.getrandbits(64) for _ in range(n - len(special))]
    got = from_hashes(np.array(hs, np.uint64), fpp)
    assert got == Bloom.from_keys(hs, fpp).encode()
    only = from_hashes(np.array(special[:6] + [0] * (n - 6), np.uint64), fpp)
    for bit in (0, limit - 1, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE):
        assert only[bit // 8] >> (bit % 8) & 1, bit
    assert only[-1] == 15 and only == Bloom.from_keys(special[:6] + [0] * (n - 6), fpp).encode()


def test_duplicates_and_a_limit_that_is_no_multiple_of_32():
    n, fpp = 777, 0.003
    nbytes, k = Bloom.geometry(n, fpp)
    assert (nbytes - 1) * 8 % 32 != 0
    rng = random.Random(5)
    hs = [rng.getrandbits(64) for _ in range(n - 100)]
    hs += hs[:100]
    assert from_hashes(np.array(hs, np.uint64), fpp) == Bloom.from_keys(hs, fpp).encode()


@pytest.mark.parametrize("n,fpp", [(0, 0.1), (1, 0.1), (1000, 0.3), (2000, 1e-300), (373408, 1e-300),
                                   (373409, 1e-300), (5, 0.999999)])
def test_geometry_is_from_keys_sizing(n, fpp):
    """Bloom.geometry is the sizing half of from_keys (the filter's length and last byte)."""
    nbytes, k = Bloom.geometry(n, fpp)
    if n <= 1000:
        f = Bloom.from_keys([0] * n, fpp).encode()
        assert (len(f), f[-1]) == (nbytes, k)
    if (n, fpp) == (373408, 1e-300):
        assert (nbytes, k) == (67108829, 15)
    if (n, fpp) == (373409, 1e-300):
        assert (nbytes, k) == (67109009, 15)


@pytest.mark.parametrize("name,source,pattern", [
    ("MERGE_TILE", "tpz_internal.h", r"kMergeTile\s*=\s*(\d+)"),
    ("MERGE_LANE_COPY_MAX", "tpz_merge.hip", r"kLaneCopyMax\s*=\s*(\d+)"),
    ("BLOOM_MAX_SLICES", "tpz_seek.hip", r"kBloomMaxSlices\s*=\s*(\d+)"),
    ("BLOOM_WG_PROBES", "tpz_seek.hip", r"kBloomWgProbes\s*=\s*(\d+)"),
    ("BLOOM_SLICE_BITS", "tpz_seek.hip", r"kBloomSliceLog\s*=\s*(\d+)")])
def test_mirrored_constants_match_the_kernels(name, source, pattern):
    """The path-reach assertions of the GPU tests compute with _lib's copies of these constants;
    a kernel constant that moves without its copy fails here."""
    text = open(os.path.join(ROOT, "topazdb_amd", "csrc", source)).read()
    found = re.findall(pattern, text)
    assert len(found) == 1, (name, found)
    value = int(found[0])
    assert getattr(_lib, name) == (1 << value if name == "BLOOM_SLICE_BITS" else value)

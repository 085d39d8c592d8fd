"""tpz_bloom_build's launch shapes: filters of many slices, more than 256 workgroups, the
1024-slice limit with the atomic kernel behind it, and last slices that are mostly past the
filter. Every case asserts its own reach from tpz_bloom_geometry and the kernel constants
mirrored in topazdb_amd._lib before it touches the device, then compares the filter byte for byte
with tests/_bloom_model.from_hashes over the host xxh3_64 of the same keys, and probes 2,000 of
the keys on the device (tpz_bloom_may_contain).

The filter is sized by fpp and k is clamped to 15, so a tiny fpp buys many slices with few keys:
fpp = 1e-300 gives about 1,438 bits a key.
"""
import numpy as np
import pytest
import torch
import xxhash

from _bloom_model import from_hashes
from topazdb_amd import _lib
from topazdb_amd.encode import DeviceEntries, bloom_build
from topazdb_amd.table import Bloom

pytestmark = pytest.mark.gpu

SLICE = _lib.BLOOM_SLICE_BITS
MAX_SLICES = _lib.BLOOM_MAX_SLICES
TINY = 1e-300
SCAN = 256     # threads of the scan workgroups: their carry loops turn again past 256 items


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


def reach(n: int, fpp: float):
    """(slices, workgroups of the partitioned build, limit in bits) for n keys at fpp."""
    geo = _lib.bloom_geometry(n, fpp)
    assert geo == Bloom.geometry(n, fpp)
    limit = (geo[0] - 1) * 8
    per_wg = _lib.BLOOM_WG_PROBES // geo[1]
    return (limit + SLICE - 1) // SLICE, max(1, (n + per_wg - 1) // per_wg), limit


def keys_for(n: int, dups: int = 300):
    """n random keys of 1..24 bytes as (key bytes, positions); the last min(dups, n // 4) repeat
    the first ones."""
    dups = min(dups, n // 4)
    rng = np.random.default_rng(n)
    kl = rng.integers(1, 25, n - dups)
    kl = np.concatenate([kl, kl[:dups]])
    kpos = np.concatenate([[0], np.cumsum(kl)]).astype(np.uint64)
    fresh = rng.integers(0, 256, int(kpos[n - dups]), dtype=np.uint8)
    return np.concatenate([fresh, fresh[:int(kpos[dups])]]), kpos


def reference(n: int, fpp: float):
    """(key bytes, positions, the filter Bloom::from_keys builds over the keys' xxh3_64)."""
    keys, kpos = keys_for(n)
    buf, p = keys.tobytes(), kpos.tolist()
    hs = np.fromiter((xxhash.xxh3_64_intdigest(buf[p[i]:p[i + 1]]) for i in range(n)), np.uint64, n)
    return keys, kpos, from_hashes(hs, fpp)


def build_and_compare(ctx, n: int, fpp: float) -> int:
    """The device's filter for case (n, fpp) equals the model's; 2,000 of its keys are found.
    Returns the filter's length."""
    keys, kpos, want = reference(n, fpp)
    vpos = np.zeros(n + 1, np.uint64)
    ent = DeviceEntries(keys, kpos, np.zeros(0, np.uint8), vpos)
    got = bloom_build(ctx, ent, fpp)
    assert len(got) == len(want) == _lib.bloom_geometry(n, fpp)[0]
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        diff = np.nonzero(g != w)[0]
        bad = int(diff[0])
        raise AssertionError(f"{len(diff)} filter bytes differ, the first at byte {bad} of "
                             f"{len(got)} (slice {bad * 8 // SLICE}): {g[bad]:#04x}, not {w[bad]:#04x}")
    # probe 2,000 keys spread over the case (the first and the last included)
    pick = np.unique(np.linspace(0, n - 1, min(n, 2000)).astype(np.int64))
    p = kpos.astype(np.int64)
    ql = p[pick + 1] - p[pick]
    qpos = np.concatenate([[0], np.cumsum(ql)]).astype(np.int64)
    q = np.concatenate([keys[p[i]:p[i + 1]] for i in pick.tolist()])
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(np.frombuffer(got, np.uint8).copy()).to(dev)
    d_q, d_qp = torch.from_numpy(q).to(dev), torch.from_numpy(qpos).to(dev)
    out = torch.zeros(len(pick), dtype=torch.uint8, device=dev)
    ctx.bloom_ptrs(d_f.data_ptr(), len(got), d_q.data_ptr(), d_qp.data_ptr(), len(pick),
                   out.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1).all()
    return len(got)


def slice_limit_pair():
    """(n, n + 1): the most keys whose filter still has MAX_SLICES slices, and the fewest past."""
    lo, hi = 250_000, 400_000              # reach(lo) <= MAX_SLICES < reach(hi)
    assert reach(lo, TINY)[0] <= MAX_SLICES < reach(hi, TINY)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reach(mid, TINY)[0] <= MAX_SLICES:
            lo = mid
        else:
            hi = mid
    return lo, hi


def test_six_slices_three_workgroups(ctx):
    """Slice indices above 1 and a last slice that ends inside the filter's last words."""
    S, nwg, limit = reach(2000, TINY)
    assert (S, nwg) == (6, 3) and limit % SLICE != 0
    build_and_compare(ctx, 2000, TINY)


def test_more_than_256_slices(ctx):
    """bloom_scatter_kernel's scan of a workgroup's counts over the slices carries into a second
    turn; bloom_hist_scan_kernel's rows still fit one."""
    S, nwg, limit = reach(100_000, TINY)
    assert (S, nwg) == (275, 123) and S > SCAN >= nwg
    build_and_compare(ctx, 100_000, TINY)


def test_more_than_256_workgroups(ctx):
    """bloom_hist_scan_kernel's carry over the workgroups (and the scatter's over the slices)."""
    S, nwg, limit = reach(250_000, TINY)
    assert SCAN < S <= MAX_SLICES and nwg > SCAN
    build_and_compare(ctx, 250_000, TINY)


@pytest.mark.parametrize("side", [0, 1])
def test_either_side_of_the_slice_limit(ctx, side):
    """MAX_SLICES slices: the partitioned build at its largest (the scatter's LDS at its limit);
    one key more: the atomic kernel, the production fallback."""
    n = slice_limit_pair()[side]
    S, nwg, limit = reach(n, TINY)
    assert S == MAX_SLICES + side and reach(n - 1, TINY)[0] <= S <= reach(n + 1, TINY)[0]
    build_and_compare(ctx, n, TINY)


def test_past_the_slice_limit(ctx):
    """bloom_build_kernel (device-scope atomics into a 72 MB filter): the production fallback."""
    S, nwg, limit = reach(400_000, TINY)
    assert S > MAX_SLICES
    build_and_compare(ctx, 400_000, TINY)


def test_last_slice_of_under_32_bits(ctx):
    """A last slice that holds less than one word: the fill kernel stores one word of it, and that
    word also holds the k byte."""
    fpp = 1e-100
    n = next(n for n in range(1, 50_000)
             if reach(n, fpp)[2] > SLICE and 1 <= reach(n, fpp)[2] % SLICE <= 31)
    S, nwg, limit = reach(n, fpp)
    assert n < 5000 and S == 2 and 1 <= limit - SLICE <= 31
    build_and_compare(ctx, n, fpp)


def test_limit_that_is_no_multiple_of_32(ctx):
    """The filter's last word is part bits, part k byte, in a slice that is not the first."""
    n = next(n for n in range(3000, 4000) if reach(n, TINY)[2] % 32 not in (0, 24))
    S, nwg, limit = reach(n, TINY)
    assert S > 1 and limit % 32 in (8, 16)       # the k byte is not the word's last byte either
    build_and_compare(ctx, n, TINY)

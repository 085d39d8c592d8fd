"""bench.py --dump-outputs: the arrays it writes are the decoded columns of the sampled blocks."""
import os

import numpy as np
import pytest
import torch

import bench
from topazdb_amd import _lib
from topazdb_amd.batch import DeviceBatch, decode_batch

pytestmark = pytest.mark.gpu


def test_dump_outputs_match_generator(tmp_path):
    """300 4k blocks, one with a flipped bit: 64 sampled blocks (the budget) and a 128-block
    metadata sample (a batch larger than meta_max). Keys, values and ends of the sampled OK
    blocks equal the generator's; the bad block keeps its status and contributes no bytes; a
    second dump writes the same arrays."""
    nb, bad = 300, 43       # (block 43 is in both seeded samples, checked below)
    src, ext, gen, n_ent, _, _ = bench.make_shard("4k", nb, 0)
    src = src.copy()
    src[int(ext[bad]) + 100] ^= 0x40
    keys, kpos, vals, vpos = gen
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    cols = decode_batch(ctx, DeviceBatch(src, ext))
    budget = 64 * 4155 + 100
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    names = bench.dump_outputs(d1, cols, ext, dev, data_budget=budget, meta_max=128)
    assert bench.dump_outputs(d2, cols, ext, dev, data_budget=budget, meta_max=128) == names
    ctx.close()
    got = {n: np.load(os.path.join(d1, n + ".npy")) for n in names}
    assert sorted(got) == ["count", "crc", "ends", "keys", "meta_blocks", "sample_blocks",
                           "status", "values"]
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, np.load(os.path.join(d2, n + ".npy"))), n
    assert sum(a.nbytes for a in got.values()) <= 24 * 128 + 4 * budget

    meta = got["meta_blocks"].astype(np.int64)
    assert len(meta) == 128 and (np.diff(meta) > 0).all() and meta[-1] < nb
    exp_status = np.where(meta == bad, _lib.BLOCK_CHECKSUM_MISMATCH, _lib.BLOCK_OK)
    assert np.array_equal(got["status"], exp_status)
    ok = meta != bad
    assert np.array_equal(got["count"][ok], n_ent[meta[ok]])
    stored = np.array([int.from_bytes(src[int(ext[b + 1]) - 5:int(ext[b + 1]) - 1].tobytes(), "big")
                       for b in meta[ok]], np.float64)
    assert np.array_equal(got["crc"][ok], stored)          # an OK block's CRC is its stored one

    pick = got["sample_blocks"].astype(np.int64)
    assert len(pick) == 64 and (np.diff(pick) > 0).all()
    assert bad in pick and bad in meta
    e0 = np.zeros(nb + 1, np.int64)
    np.cumsum(n_ent, out=e0[1:])
    ek, ev, ee = [], [], []
    for b in pick[pick != bad]:
        lo, hi = int(e0[b]), int(e0[b + 1])
        ek.append(keys[int(kpos[lo]):int(kpos[hi])])
        ev.append(vals[int(vpos[lo]):int(vpos[hi])])
        ee.append(np.stack([kpos[lo + 1:hi + 1] - kpos[lo], vpos[lo + 1:hi + 1] - vpos[lo]], 1))
    assert np.array_equal(got["keys"], np.concatenate(ek))
    assert np.array_equal(got["values"], np.concatenate(ev))
    assert np.array_equal(got["ends"], np.concatenate(ee))

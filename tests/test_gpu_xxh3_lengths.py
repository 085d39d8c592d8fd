"""The device build of tpz_xxh3.h on keys of every length class, through every kernel that hashes:
bloom_kernel (tpz_bloom_may_contain), the three routes of tpz_bloom_build, the walks of
tpz_get_keys and tpz_lsm_get_keys, and the filters of SST images written on the device.

The hash reference is the xxhash package's xxh3_64, the filter reference tests/_bloom_model.py
from_hashes; everything is compared bit for bit. The inputs (tests/_xxh3_cases.py) hold one key
per length from 0 to 2200 and at the 1 KiB block counts up to the 65,535-byte key, and 13,266
single-bit mutants none of which the model filter accepts (tests/test_xxh3_cases.py), so a device
hash that is wrong for one length shows as a key its own filter rejects.
"""
import struct
import zlib

import numpy as np
import pytest
import torch

import _get_model as G
import _lsm_model as L
import _open_model as OM
import _xxh3_cases as X
from _bloom_model import from_hashes
from topazdb_amd import _lib
from topazdb_amd.encode import DeviceEntries, bloom_build
from topazdb_amd.levels import DeviceLsm, DeviceRun
from topazdb_amd.table import Bloom, DeviceTable, FileObject, SsTable, SsTableBuilder

pytestmark = pytest.mark.gpu

BLOCK_SIZE = 16384


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------- 1. probe
def probe(ctx, d_filter, filter_len: int, items, lead: int) -> np.ndarray:
    """tpz_bloom_may_contain of every item, packed after `lead` bytes, in one launch."""
    dev = torch.device("cuda", ctx.device)
    col, pos = X.pack(items, lead)
    d_q = torch.from_numpy(col.copy()).to(dev)
    d_qp = torch.from_numpy(pos.view(np.int64).copy()).to(dev)
    out = torch.full((len(items),), 0xEE, dtype=torch.uint8, device=dev)
    ctx.bloom_ptrs(d_filter.data_ptr(), filter_len, d_q.data_ptr(), d_qp.data_ptr(), len(items),
                   out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_probe_every_length_every_alignment(ctx):
    filt = X.model_filter(X.PROBE_FPP)
    assert len(filt) == 39702 and filt[-1] == 15
    keys, muts = X.keys(), X.mutants()
    mutant_bytes = [m for _, _, m in muts]
    want = X.may_contain(filt, X.mutant_hashes()).astype(np.uint8)
    d_f = torch.from_numpy(np.frombuffer(filt, np.uint8).copy()).to(torch.device("cuda", ctx.device))
    for lead in X.LEADS:
        got = probe(ctx, d_f, len(filt), keys, lead)
        bad = np.nonzero(got != 1)[0]
        assert bad.size == 0, (f"lead {lead}: the filter built from the keys rejects {bad.size} of "
                               f"them, the first of {X.LENGTHS[bad[0]]} bytes (answer {got[bad[0]]}); "
                               f"lengths {[X.LENGTHS[i] for i in bad[:20]]}")
        got = probe(ctx, d_f, len(filt), mutant_bytes, lead)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"lead {lead}: {bad.size} mutants answered unlike the model, the "
                               f"first of {X.LENGTHS[muts[bad[0]][0]]} bytes flipped at "
                               f"{muts[bad[0]][1]}: {got[bad[0]]}, not {want[bad[0]]}")


# ------------------------------------------------------------------------------- 2. build
def build_and_compare(ctx, items, hs: np.ndarray, fpp: float) -> None:
    """tpz_bloom_build over the items equals from_hashes over their xxhash hashes `hs`; on a
    mismatch the lengths whose one-key model filter the device's filter does not cover are named."""
    col, pos = X.pack(items)
    n = len(items)
    ent = DeviceEntries(col, pos, np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64), ctx.device)
    got, want = bloom_build(ctx, ent, fpp), from_hashes(hs, fpp)
    assert len(got) == len(want) == _lib.bloom_geometry(n, fpp)[0]
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        lost = [len(items[i]) for i in np.nonzero(~X.may_contain(got[:-1] + want[-1:], hs))[0]]
        raise AssertionError(f"{int((g != w).sum())} of {len(w)} filter bytes differ at fpp {fpp}; "
                             f"{len(lost)} keys lack bits of their own, of lengths {lost[:20]}")


def long_key_bloom_case(ctx) -> None:
    """The 2,209 keys at fpp 1e-300: 7 slices, 3 workgroups of 819 keys (the partitioned route by
    default; tests/test_gpu_env_paths.py runs it under the two build variables as well)."""
    assert X.reach(len(X.LENGTHS), X.TINY) == (7, 3, 819, 15) and 7 <= _lib.BLOOM_MAX_SLICES
    build_and_compare(ctx, X.keys(), X.key_hashes(), X.TINY)


def test_build_seven_slices_three_workgroups(ctx):
    """bloom_count_kernel and bloom_scatter_kernel each hash every key."""
    long_key_bloom_case(ctx)


def test_build_one_slice_few_probes(ctx):
    """fpp 0.1: k = 3, so a workgroup takes 4,096 keys and its 256 threads each walk several keys
    of more than 1 KiB; one slice."""
    S, nwg, per_wg, k = X.reach(len(X.LENGTHS), 0.1)
    assert (S, nwg, per_wg, k) == (1, 1, 4096, 3)
    assert sum(n > 1024 for n in X.LENGTHS[::256]) >= 4          # a thread's keys, 256 apart
    build_and_compare(ctx, X.keys(), X.key_hashes(), 0.1)


@pytest.mark.parametrize("n", X.SINGLE)
def test_build_single_key(ctx, n):
    """One key, 15 probes into 1,440 bits: the filter pins all but a sliver of the key's 64-bit
    hash (the chance that a wrong hash sets the same 15 bits is below 1e-40)."""
    assert X.reach(1, X.TINY) == (1, 1, 819, 15) and Bloom.geometry(1, X.TINY)[0] == 181
    i = X.LENGTHS.index(n)
    build_and_compare(ctx, [X.keys()[i]], X.key_hashes()[i:i + 1], X.TINY)


# (3. the env-selected build routes: tests/test_gpu_env_paths.py calls long_key_bloom_case)
# ------------------------------------------------------------------------------- 4. gets
_gets = {}


def get_case():
    """(pieces, queries, held keys, host tables), built once: two L0 tables and one L1 table over
    keys of TABLE_LENGTHS, their filters from the xxhash hashes; the queries are every held key,
    its neighbours and its mutants."""
    if not _gets:
        from test_gpu_get import neighbours
        ents, held = X.table_sets()
        pieces = [[G.build_pieces(e, BLOCK_SIZE, X.TABLE_FPP) for e in lv] for lv in ents]
        for lv, tabs in zip(ents, pieces):
            for e, p in zip(lv, tabs):      # the filters stand on xxhash, not on the host build
                assert p.bloom == from_hashes(X.hashes([k for k, _ in e]), X.TABLE_FPP)
        qs = list(held)
        for k in held:
            qs += neighbours(k) + X.mutants_of(k)
        qs = list(dict.fromkeys(qs))        # (the five one-byte keys share the empty neighbour)
        host = [[p.host_table(j) for j, p in enumerate(lv)] for lv in pieces]
        _gets.update(pieces=pieces, qs=qs, held=held, host=host)
    return _gets["pieces"], _gets["qs"], _gets["held"], _gets["host"]


def test_get_keys_through_the_filters(ctx):
    from test_gpu_get import check
    pieces, qs, held, host = get_case()
    model = [G.level_get(host, q) for q in qs]
    # the model's may_contain hashes on the host: xxhash's value for every query
    assert [_lib.xxh3_64(q) for q in qs] == X.hashes(qs).tolist()
    assert all(g.result in (G.FOUND, G.DELETED) for g in model[:len(held)])
    assert {g.table for g in model[:len(held)]} == {0, 1, 2}
    assert sum(g.result == G.DELETED for g in model) >= 20
    others = model[len(held):]
    assert sum(g.result == G.ABSENT for g in others) * 2 >= len(others) >= 800
    check(ctx, pieces, qs, model)


def test_lsm_get_keys_through_the_filters(ctx):
    from test_gpu_get import assert_equal
    pieces, qs, held, host = get_case()
    run = [(b"run-%02d" % i, b"" if i == 3 else b"m0=%d" % i) for i in range(10)]
    qs = qs + [k for k, _ in run]
    model = [L.lsm_get_mem([run], host, q) for q in qs]
    assert sum(g.table != G.NONE and bool(g.table & L.HIT_MEM) for g in model) == len(run)
    assert all(g.result in (G.FOUND, G.DELETED) and g.table in (0, 1, 2) for g in model[:len(held)])
    assert sum(g.result == G.ERROR for g in model) == 1 and b"" in qs     # the one empty key
    tables = [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom) for p in lv] for lv in pieces]
    dl = DeviceLsm(ctx, [DeviceRun(ctx, run)], tables)
    assert_equal(dl.get_batch(qs), model, qs)


# ------------------------------------------------------------------------------- 5. SST images
def check_image(ctx, img: bytes, keys, name: str) -> None:
    """The image's filter section is Bloom::from_keys over the keys' xxhash hashes, and the opened
    table's device filter holds every key."""
    p = OM.parse(img)
    assert p.status == OM.OK and p.info[4] != OM.NONE
    section = img[p.info[4]:p.info[4] + p.info[5]]
    assert section == Bloom.from_keys(X.hashes(keys).tolist(), X.TABLE_FPP).encode(), name
    t = SsTable.open(0, FileObject.open_many([(name, img)], ctx)[0], ctx)
    assert t.may_contain_gpu(keys).all(), name


def test_sst_written_on_the_device(ctx):
    ents = X.sst_entries()
    keys = [k for k, _ in ents]
    b = SsTableBuilder(ctx, BLOCK_SIZE, X.TABLE_FPP)
    for k, v in ents:
        b.add(k, v)
    img = b.build_image()
    check_image(ctx, img + struct.pack(">I", zlib.crc32(img)), keys, "builder")


def test_sst_written_by_compact_task(ctx):
    """The same entries as two input tables of a task (every second entry each), cut into several
    output tables: every output image's filter is the model's over that table's keys."""
    from test_gpu_compact import table_region
    from test_gpu_tables import images_of
    from topazdb_amd.compact import compact_task
    import _tables_model as TM
    ents = X.sst_entries()
    runs, bounds = [ents[0::2], ents[1::2]], [(b"", (b"\xff", True))]
    merged, want = TM.task_tables(runs, bounds, BLOCK_SIZE, 1)
    assert merged == ents and [(t0, n) for t0, n, _ in want] == [(0, 28), (28, 23), (51, 9)]
    out = compact_task(ctx, [table_region(r, BLOCK_SIZE) for r in runs], bounds,
                       block_size=BLOCK_SIZE, false_positive_rate=X.TABLE_FPP, table_capacity=1)
    assert [(t.first_entry, t.n_entries) for t in out] == [(t0, n) for t0, n, _ in want]
    for j, (t, img) in enumerate(zip(out, images_of(out))):
        keys = [k for k, _ in ents[t.first_entry:t.first_entry + t.n_entries]]
        assert _lib.bloom_geometry(len(keys), X.TABLE_FPP) == Bloom.geometry(len(keys), X.TABLE_FPP)
        check_image(ctx, img, keys, "task-%d" % j)

"""compact.flush_runs and its two wrappers (start_flush and sync(), src/lsm_storage.rs:83-143,
:298-332): sorted memtable runs in HBM -> one L0 SST file image, against
table.SsTableBuilder.build_image() over the merged entries a dict overlay gives, byte for byte,
and through SsTable.open and DeviceLsm.get."""
import random
import struct
import zlib

import pytest
import torch

import _get_model as G
import _lsm_model as M
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import compact
from topazdb_amd.encode import EntryError
from topazdb_amd.levels import DeviceLsm, DeviceRun
from topazdb_amd.table import FileObject, SsTable, SsTableBuilder

pytestmark = pytest.mark.gpu


def view_of(n_runs: int, seed: int = 7) -> list:
    """MemTables::view() as runs: n_runs immutable memtables oldest first, then an empty mutable
    one. 84 possible keys, so keys repeat across runs; a value names its run."""
    rng = random.Random(seed + n_runs)
    return [M.random_run(rng, r, 60) for r in range(n_runs)] + [[]]


def overlay(runs) -> list:
    """The lower index wins a repeated key (tpz_merge_runs)."""
    merged = {}
    for run in runs:
        for k, v in run:
            merged.setdefault(k, v)
    return sorted(merged.items())


def reference_image(ctx, ents, block_size) -> bytes:
    b = SsTableBuilder(ctx, block_size, 0.1)
    for k, v in ents:
        b.add(k, v)
    data = b.build_image()
    return data + struct.pack(">I", zlib.crc32(data))          # FileObject::create


def image_of(t) -> bytes:
    return t.image.cpu().numpy().tobytes()


@pytest.mark.parametrize("block_size", [256, 4096])
@pytest.mark.parametrize("n_runs", [1, 2, 5])
def test_flush_image_equals_the_builder(ctx, tmp_path, n_runs, block_size):
    view = view_of(n_runs)
    dview = [DeviceRun(ctx, r) for r in view]
    oldest_wins, newest_wins = overlay(view[:-1]), overlay(view[::-1])
    repeated = {k for k, _ in oldest_wins if sum(k in dict(r) for r in view) > 1}
    assert (len(repeated) >= 5) == (n_runs > 1)
    a, a_ents = compact.flush_like_start_flush(ctx, dview, block_size)
    b, b_ents = compact.flush_like_sync(ctx, dview, block_size)
    assert image_of(a) == reference_image(ctx, oldest_wins, block_size)
    assert image_of(b) == reference_image(ctx, newest_wins, block_size)
    assert a.n_entries == len(oldest_wins) == a_ents.n and a.size == len(image_of(a))
    if block_size == 256 and n_runs > 1:
        assert a.n_blocks > 1
    # the two orders differ exactly on the repeated keys (a value names its run, so only a key
    # whose oldest and newest copies are both tombstones reads the same)
    differ = {k for (k, v), (k2, v2) in zip(oldest_wins, newest_wins) if v != v2}
    assert [k for k, _ in oldest_wins] == [k for k, _ in newest_wins] and differ <= repeated
    assert all(dict(oldest_wins)[k] == dict(newest_wins)[k] == b"" for k in repeated - differ)
    assert (len(differ) >= 5) == (n_runs > 1)
    # the images open, and with the remaining (empty) memtable they answer get as before the flush
    tables = []
    for j, t in enumerate((a, b)):
        path = tmp_path / f"flush_{j}.sst"
        path.write_bytes(image_of(t))
        tables.append(SsTable.open(j, FileObject.open(str(path), ctx), ctx))
        assert tables[-1].num_of_blocks() == t.n_blocks and tables[-1].bloom is not None
    qs = [k for k, _ in oldest_wins] + [k + b"\0" for k, _ in oldest_wins[::4]]
    before = DeviceLsm(ctx, dview, []).get_batch(qs)
    want = [M.lsm_get_mem(view, [], q) for q in qs]
    assert [int(r) for r in before["result"]] == [g.result for g in want]
    after_sync = DeviceLsm(ctx, dview[-1:], [[tables[1]]]).get_batch(qs)
    after_flush = DeviceLsm(ctx, dview[-1:], [[tables[0]]]).get_batch(qs)

    def answers(r):
        return [(int(r["result"][i]), r["values"][int(r["val_pos"][i]):int(r["val_pos"][i + 1])])
                for i in range(len(qs))]

    assert answers(after_sync) == answers(before)
    agree = [i for i, q in enumerate(qs) if q not in differ]
    assert len(agree) >= 10
    assert [answers(after_flush)[i] for i in agree] == [answers(before)[i] for i in agree]


def test_flush_of_nothing_and_of_an_empty_key(ctx):
    """sync() builds nothing from an empty map; an empty key is the builder's assert."""
    assert compact.flush_like_sync(ctx, [DeviceRun(ctx, []), DeviceRun(ctx, [])]) is None
    assert compact.flush_like_start_flush(ctx, [DeviceRun(ctx, [(b"a", b"1")])]) is None
    assert compact.flush_runs(ctx, []) is None
    with pytest.raises(EntryError, match="key must not be empty"):
        compact.flush_runs(ctx, [DeviceRun(ctx, [(b"a", b"1")]), DeviceRun(ctx, [(b"", b"x"), (b"b", b"2")])])
    torch.cuda.synchronize()


def test_flush_keeps_tombstones_and_feeds_the_levels(ctx, tmp_path):
    """The reference's get-after-sync sequence (src/tests/storage.rs:167-182) with the sync on the
    device: the flushed table under a newer memtable."""
    view = [DeviceRun(ctx, [(b"1", b"233"), (b"2", b"2333")]), DeviceRun(ctx, [])]
    t, _ = compact.flush_like_sync(ctx, view, 4096)
    path = tmp_path / "l0.sst"
    path.write_bytes(image_of(t))
    table = SsTable.open(0, FileObject.open(str(path), ctx), ctx)
    dl = DeviceLsm(ctx, [DeviceRun(ctx, [(b"3", b"23333")])], [[table]])
    assert [dl.get(k) for k in (b"1", b"2", b"3")] == [b"233", b"2333", b"23333"]
    dl = DeviceLsm(ctx, [DeviceRun(ctx, [(b"2", b""), (b"3", b"23333")])], [[table]])
    assert dl.get(b"2") is None and dl.get(b"1") == b"233"
    t2, ents = compact.flush_like_sync(ctx, dl.runs + [DeviceRun(ctx, [])], 4096)
    assert ents.n == 2 and t2.n_entries == 2                    # the tombstone is an entry
    assert G.Pieces.from_image(image_of(t2)).first_keys == [b"2"]

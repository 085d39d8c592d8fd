"""tpz_lsm_scan_ranges / tpz_lsm_scan_entries (LsmStorage::scan whole for batches of ranges over
memtable runs plus resident tables, src/lsm_storage.rs:335-374) against the line-by-line model of
tests/_lsm_model.py, which tests/test_lsm_model.py ties to the closed form and to the reference's
own scan tests.

Every case compares d_result, d_status, d_where, the hit columns up to each scan's count, the
three prefix arrays, d_kpos, d_vpos and the key and value bytes with the model, exactly, and first
asserts from the model alone that its inputs reach what the case names.
"""
import numpy as np
import pytest
import torch

import _get_model as G
import _lsm_cases as C
import _lsm_model as M
import _scan_cases as K
import _scan_model as S
from test_gpu_scan import GUARD, RANGE_OUT, assert_equal, drain, raw_inputs, raw_outputs
from test_gpu_table import ctx  # noqa: F401 (fixture)
from test_lsm_model import coverage, eager_case
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import BlockError, DeviceTable, FileObject, SsTable

pytestmark = pytest.mark.gpu

BIG = 1 << 10


# ------------------------------------------------------------------------------- harness
def device_tables(ctx, pieces):
    return [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom) for p in lv] for lv in pieces]


def device_lsm(ctx, case: C.LsmCase, prefix=True) -> DeviceLsm:
    return DeviceLsm(ctx, [DeviceRun(ctx, r, prefix) for r in case.runs],
                     device_tables(ctx, case.pieces))


def check(ctx, case: C.LsmCase, limit, idx=None, dl=None) -> DeviceLsm:
    idx = list(range(len(case.ranges))) if idx is None else idx
    dl = dl or device_lsm(ctx, case)
    ranges = [case.ranges[r] for r in idx]
    assert_equal(dl.scan_batch(ranges, limit), case.models(limit, idx), limit, ranges)
    return dl


# ------------------------------------------------------------------------------- 1. reference cases
def test_reference_scan_cases(ctx, tmp_path):
    """src/tests/storage.rs:110-246 through SsTable.open, DeviceRun and DeviceLsm: the memtables
    as runs, the synced tables as L0; scan_batch and the scan() iterator."""
    for name, (runs, l0, scans) in M.reference_cases().items():
        pieces = K.pieces_of([l0], 64)
        tables = []
        for j, p in enumerate(pieces[0]):
            path = tmp_path / f"{name}_{j}.sst"
            path.write_bytes(p.image())
            tables.append(SsTable.open(j, FileObject.open(str(path), ctx), ctx))
        ranges = [(lo, hi) for lo, hi, _ in scans]
        host = K.host_levels(pieces)
        models = [M.lsm_scan_mem(runs, host, lo, hi, 16) for lo, hi in ranges]
        assert [m.entries for m in models] == [w for _, _, w in scans], name
        dl = DeviceLsm(ctx, [DeviceRun(ctx, r) for r in runs], [tables] + [[] for _ in range(5)])
        assert_equal(dl.scan_batch(ranges, 16), models, 16, ranges)
        for lo, hi, want in scans:
            assert drain(dl.scan(lo, hi)) == want, (name, lo, hi)
            assert drain(dl.scan(lo, hi, page=1)) == want, (name, lo, hi)


# ------------------------------------------------------------------------------- 2. random sets
@pytest.mark.parametrize("limit", K.LIMITS)
@pytest.mark.parametrize("i", range(len(C.RANDOM_IDS)), ids=C.RANDOM_IDS)
def test_random_sets(ctx, i, limit):
    """Every bound-kind pair over bounds drawn from the keys of tables and runs, their neighbours
    and absent keys."""
    seen = coverage()
    assert min(v for k, v in seen.items() if k != "quirk") >= 20 and seen["quirk"] >= 1, seen
    case = C.random_case(i)
    assert {(lo and lo[0], hi and hi[0]) for lo, hi in case.ranges} == set(K.KIND_PAIRS)
    assert len(case.runs) == C.RANDOM[i][1] and all(1 <= len(r) <= 60 for r in case.runs)
    check(ctx, case, limit)


def test_prefix_column_or_not(ctx):
    """d_prefix == NULL bisects on the keys: identical outputs, long keys (every 8-byte prefix
    ties) included."""
    for i in (0, len(C.RANDOM) - 1):
        case = C.random_case(i)
        assert case.runs
        for prefix in (True, False):
            dl = device_lsm(ctx, case, prefix)
            assert all((r.prefix is not None) == prefix for r in dl.runs)
            assert_equal(dl.scan_batch(case.ranges, 3), case.models(3), 3, case.ranges)


# ------------------------------------------------------------------------------- 3. quirks
A, B, Cc, D, E = (b"a", b"1"), (b"b", b"2"), (b"c", b"3"), (b"d", b"4"), (b"e", b"5")


def test_empty_key_run_and_degenerate_bounds(ctx):
    """A run whose first key is empty contributes nothing unless the lower bound steps past that
    key; inverted and equal-Excluded bounds leave the run cursors empty; e0 past the end comes
    from an SST lane only."""
    run = [(b"", b"empty"), (b"b", b"run"), (b"f", b"run")]
    lowers = [None, ("in", b""), ("ex", b""), ("after", b""), ("in", b"a")]
    case = C.small_case([[B], run], [[[A, D]]], [(lo, None) for lo in lowers])
    m = case.models(8)
    assert [x.stats["mem_cursors"] for x in m] == [1, 1, 2, 2, 2]
    assert m[0].entries == [A, B, D] and m[2].entries == [A, (b"b", b"run"), D, (b"f", b"run")]
    check(ctx, case, 8)
    run = [B, Cc, D]
    bounds = [(("in", b"d"), ("in", b"b")), (("ex", b"c"), ("in", b"c")), (("in", b"c"), ("ex", b"c")),
              (("ex", b"c"), ("ex", b"c")), (("after", b"c"), ("in", b"c")), (("in", b"c"), ("in", b"c"))]
    case = C.small_case([run], [[[A, Cc, E]]], bounds)
    m = case.models(8)
    assert [x.stats["mem_cursors"] for x in m] == [0, 0, 0, 0, 0, 1]
    assert any(x.stats["quirk"] for x in m[:5]) and C.in_run(m[5].hits[0][0])
    check(ctx, case, 8)
    case = C.small_case([[(b"a0", b"r"), E]], [[[A, D]]],
                        [(("in", b"b"), ("in", b"c")), (("after", b"b"), ("in", b"c"))])
    assert [x.entries for x in case.models(8)] == [[D], []] and case.model(0, 8).stats["quirk"]
    check(ctx, case, 8)


# ------------------------------------------------------------------------------- 4. the maximum
def max_case() -> C.LsmCase:
    runs = [[(b"m%02d" % ((3 * r + j) % 50), b"" if (r + j) % 5 == 2 else b"r%d:%d" % (r, j))
             for j in range(1 + r % 5)] for r in range(_lib.MEM_MAX_RUNS)]
    runs = [sorted(dict(r).items()) for r in runs]
    l0 = [[(b"m%02d" % ((t + j) % 50), b"" if (t + j) % 7 == 0 else b"%d:%d" % (t, j))
           for j in range(1 + t % 4)] for t in range(44)]
    l0 = [sorted(set(e)) for e in l0]
    low = [[(b"z%d%d" % (t, j), b"low") for j in range(3)] for t in range(4)]
    return C.small_case(runs, [l0, low], [(None, None), (("in", b"m10"), ("ex", b"z2"))])


def test_sixteen_runs_and_forty_eight_tables(ctx):
    """Every lane of the merge wave holds a live cursor in the unbounded scan."""
    case = max_case()
    assert len(case.runs) == 16 and sum(len(lv) for lv in case.pieces) == 48
    m, full = case.model(0, 16), case.model(0, BIG)
    assert m.stats["cursors"] == 48 and m.stats["mem_cursors"] == 16
    assert full.stats["skips"] > 0 and full.stats["mem"]["ties"] > 0 and full.stats["tombstones"] > 0
    assert (m.result, full.result) == (S.MORE, S.DONE) and len(full.hits) > 16
    runs_hit = {t & ~M.HIT_MEM for t, _, _ in full.hits if C.in_run(t)}
    tables_hit = {t for t, _, _ in full.hits if not C.in_run(t)}
    assert {0, 15} <= runs_hit and min(tables_hit) < 44 and 47 in tables_hit   # L0 and the level below
    dl = check(ctx, case, 16)
    check(ctx, case, BIG, dl=dl)
    assert drain(dl.scan(page=7)) == full.entries
    with pytest.raises(ValueError):              # 65 cursors: refused, nothing falls back
        DeviceLsm(ctx, dl.runs, [dl.tables + dl.tables[:1]])
    lf = np.array([0, 49], np.uint32)
    with pytest.raises(_lib.TpzError):
        dl.ctx.lsm_scan_ranges_ptrs(dl.d_runs.data_ptr(), 16, dl.d_tables.data_ptr(), 49,
                                    lf.ctypes.data, 1,
                                    *([dl.d_tables.data_ptr()] * 6), 1, 1,
                                    *([dl.d_tables.data_ptr()] * 10))


# ------------------------------------------------------------------------------- 5. errors
def test_the_eager_skip_ends_the_scan_one_element_early(ctx):
    """A corrupt block under a key a run also holds: TwoMergeIterator moves the SST side past the
    key before it is yielded, so the count is one lower than a flat merge's, and 0 when it is the
    first key (tests/test_lsm_model.py asserts both from the model)."""
    case, bad, last_before = eager_case()
    cs = _lib.BLOCK_CHECKSUM_MISMATCH
    m = case.models(BIG)
    for r in (0, 1, 2):
        flat = M.flat_scan_mem(case.runs, case.host, *case.ranges[r], BIG)
        assert (m[r].result, m[r].status, m[r].where) == (S.ERROR, cs, (1, bad, 0))
        assert len(flat.hits) == len(m[r].hits) + 1
    assert m[1].hits == [] and len(m[0].hits) >= 5
    n = len(m[0].hits)
    assert case.model(0, n).result == S.ERROR and case.model(0, n - 1).result == S.MORE
    dl = check(ctx, case, BIG)
    check(ctx, case, n, dl=dl)
    check(ctx, case, n - 1, dl=dl)
    it = dl.scan(*case.ranges[0], page=4)
    got = []
    with pytest.raises(BlockError, match=r"checksum: expected \d+, actual \d+"):
        while it.is_valid():
            got.append((it.key(), it.value()))
            it.next()
    assert got == m[0].entries
    with pytest.raises(BlockError, match=r"checksum: expected"):
        dl.scan(*case.ranges[1])


# ------------------------------------------------------------------------------- 6. paging
@pytest.mark.parametrize("i", [0, 2], ids=[C.RANDOM_IDS[0], C.RANDOM_IDS[2]])
def test_pages_of_three(ctx, i):
    """The scan() iterator with page=3: the model's unpaged sequence."""
    case = C.random_case(i)
    dl = device_lsm(ctx, case)
    held = sorted({k for lv in case.ents for e in lv for k, _ in e} | {k for r in case.runs for k, _ in r})
    for lo, hi in ((None, None), (("in", held[3]), ("ex", held[-3])), (("ex", held[0]), None)):
        want = M.lsm_scan_mem(case.runs, case.host, lo, hi, 1 << 20)
        assert want.result == S.DONE and len(want.entries) >= 12 and want.stats["skips"] > 0
        assert M.paged_scan_mem(case.runs, case.host, lo, hi, 3)[0] == want.entries
        assert drain(dl.scan(lo, hi, page=3)) == want.entries


# ------------------------------------------------------------------------------- 7. capacity
LENGTHS = [1, 15, 16, 17, 33, 255, 256, 257, 1000]


def length_case() -> C.LsmCase:
    import random
    rng = random.Random(61)
    ents = sorted((b"k%04d" % n + b"x" * (n if n > 250 else n % 19),
                   bytes(rng.getrandbits(8) for _ in range(n))) for n in LENGTHS)
    run, tab = ents[::2], ents[1::2]
    other = sorted((b"k%04d" % n + b"y" * (n % 5), b"v" * (1 + n % 40)) for n in range(0, 1100, 37))
    keys = [k for k, _ in ents]
    ranges = [(None, None)] + [(("in", k), None) for k in keys] + [(("ex", keys[2]), ("in", keys[-2]))]
    return C.LsmCase([other[::2], run], [[tab], [other]], K.pieces_of([[tab], [other]], 4096), ranges)


def run_ranges(dl, cols, out, n, limit, stream=0):
    dl.ctx.lsm_scan_ranges_ptrs(dl.d_runs.data_ptr(), dl.n_runs, dl.d_tables.data_ptr(),
                                dl.n_tables, dl.level_first.ctypes.data, dl.n_levels,
                                *(c.data_ptr() for c in cols), n, limit,
                                *(out[k].data_ptr() for k, _, _ in RANGE_OUT), stream)


def test_capacities_are_respected(ctx):
    case = length_case()
    limit = 8
    models = case.models(limit)
    want = K.expected(models, limit)
    kinds = [C.in_run(t) for m in models for t, _, _ in m.hits]
    assert any(kinds) and not all(kinds)
    long_src = {C.in_run(t) for m in models for (t, _, _), (k, v) in zip(m.hits, m.entries)
                if len(v) > 256 or len(k) > 256}
    assert long_src == {True, False}               # wave-copied entries from a run and a table
    dl = check(ctx, case, limit)
    n = len(case.ranges)
    out, sizes = raw_outputs(dl, n, limit)
    cols = raw_inputs(dl, case.ranges)
    run_ranges(dl, cols, out, n, limit)
    torch.cuda.synchronize()
    for k, _, _ in RANGE_OUT:                      # nothing is written past a column's end
        tail = out[k][sizes[k]:].view(torch.uint8).cpu().numpy()
        assert (tail == 0xA5).all(), k
    hits = out["hit_table"][:n * limit].cpu().numpy().view(np.uint32).reshape(n, limit)
    for i, m in enumerate(models):                 # ... nor past a scan's count in its hit row
        assert (hits[i, len(m.hits):] == 0xA5A5A5A5).all(), i
    n_ent, kbytes, vbytes = (int(x) for x in out["info"][:3].cpu().numpy())
    assert (n_ent, kbytes, vbytes) == (len(want["kpos"]) - 1, len(want["keys"]), len(want["values"]))

    def gather(key_cap, val_cap):
        kp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
        vp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
        kb = torch.full((kbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        vb = torch.full((vbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        dl.ctx.lsm_scan_entries_ptrs(dl.d_runs.data_ptr(), dl.n_runs, dl.d_tables.data_ptr(),
                                     dl.n_tables, n, limit, out["hit_table"].data_ptr(),
                                     out["hit_block"].data_ptr(), out["hit_entry"].data_ptr(),
                                     out["first"].data_ptr(), kb.data_ptr(), key_cap, kp.data_ptr(),
                                     vb.data_ptr(), val_cap, vp.data_ptr())
        torch.cuda.synchronize()
        assert (kp[n_ent + 1:] == -1).all() and (vp[n_ent + 1:] == -1).all()
        assert np.array_equal(kp[:n_ent + 1].cpu().numpy().astype(np.uint64), want["kpos"])
        assert np.array_equal(vp[:n_ent + 1].cpu().numpy().astype(np.uint64), want["vpos"])
        return kb.cpu().numpy().tobytes(), vb.cpu().numpy().tobytes()

    # exact, one byte short, inside a wave-copied value / key, and 0
    e1000 = next(j for j in range(n_ent) if want["vpos"][j + 1] - want["vpos"][j] == 1000)
    e300 = next(j for j in range(n_ent) if want["kpos"][j + 1] - want["kpos"][j] > 256)
    for kc, vc in ((kbytes, vbytes), (kbytes - 1, vbytes - 1),
                   (int(want["kpos"][e300]) + 100, int(want["vpos"][e1000]) + 499), (0, 0)):
        k, v = gather(kc, vc)
        assert k[:kc] == want["keys"][:kc] and k[kc:] == b"\xa5" * (kbytes + 256 - kc), kc
        assert v[:vc] == want["values"][:vc] and v[vc:] == b"\xa5" * (vbytes + 256 - vc), vc


# ------------------------------------------------------------------------------- 8. graph capture
def test_lsm_scan_ranges_in_a_graph(ctx):
    """tpz_lsm_scan_ranges captured and replayed once (tests/test_gpu_scan.py's pattern): an
    uncaptured first call grows the stream's workspace, so the captured one allocates nothing."""
    case = C.random_case(1)
    limit, n = 3, len(case.ranges)
    want = K.expected(case.models(limit), limit)
    dl = device_lsm(ctx, case)
    cols = raw_inputs(dl, case.ranges)
    out, sizes = raw_outputs(dl, n, limit)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run_ranges(dl, cols, out, n, limit, s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            run_ranges(dl, cols, out, n, limit, s.cuda_stream)
    for k, _, _ in RANGE_OUT:
        out[k].view(torch.uint8).fill_(0xA5)
    g.replay()
    torch.cuda.synchronize()
    for k in ("result", "status"):
        assert np.array_equal(out[k][:n].cpu().numpy(), want[k]), k
    assert np.array_equal(out["where"][:3 * n].cpu().numpy().view(np.uint32).reshape(n, 3),
                          want["where"])
    for k in ("first", "key_first", "val_first"):
        assert np.array_equal(out[k][:n + 1].cpu().numpy().astype(np.uint64), want[k]), k
    hits = [out[k][:n * limit].cpu().numpy().view(np.uint32).reshape(n, limit)
            for k in ("hit_table", "hit_block", "hit_entry")]
    for i, h in enumerate(want["hits"]):
        for c in range(3):
            assert np.array_equal(hits[c][i, :len(h)], h[:, c]), (i, c)
    assert out["info"][:3].tolist() == [int(want[k][n]) for k in ("first", "key_first", "val_first")]


# ------------------------------------------------------------------------------- 9. no runs
def test_no_runs_equals_scan_ranges(ctx):
    """n_runs == 0: tpz_scan_ranges' / tpz_scan_entries' outputs byte for byte."""
    case = C.random_case(3)
    assert case.runs == []
    tables = device_tables(ctx, case.pieces)
    for limit in (3, 64):
        a = DeviceLsm(ctx, [], tables).scan_batch(case.ranges, limit)
        b = DeviceLevels(ctx, tables).scan_batch(case.ranges, limit)
        want = K.expected(case.models(limit), limit)
        for k in a:
            if k.startswith("hit_"):             # (a row is defined up to the scan's count)
                for i, h in enumerate(want["hits"]):
                    assert np.array_equal(a[k][i, :len(h)], b[k][i, :len(h)]), (k, i)
            elif isinstance(a[k], bytes):
                assert a[k] == b[k] and len(a[k]) > 0, k
            else:
                assert a[k].tobytes() == b[k].tobytes(), k
    none = DeviceLsm(ctx, [], [])
    ranges = [(None, None), (("in", b"a"), ("ex", b"b"))]
    assert_equal(none.scan_batch(ranges, 4), [M.lsm_scan_mem([], [], lo, hi, 4) for lo, hi in ranges],
                 4, ranges)
    assert_equal(none.scan_batch([], 4), [], 4, [])
    assert drain(none.scan()) == []

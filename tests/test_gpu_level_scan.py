"""tpz_level_scan_ranges / tpz_level_scan_entries (LsmStorage::scan with one merge cursor per level
below L0, so a level may hold any number of tables) against the per-table models that follow the
reference line by line (tests/_scan_model.py lsm_scan, tests/_lsm_model.py lsm_scan_mem), which
tests/test_level_scan_model.py ties to the level cursor's semantics.

Every comparison is exact, as tests/test_gpu_scan.py's assert_equal does it: d_result, d_status,
d_where, the hit columns up to each scan's count, the three prefix arrays, d_kpos, d_vpos and the
key and value bytes. Every case first asserts from the models alone that its inputs reach what it
names.
"""
import numpy as np
import pytest
import torch

import _get_model as G
import _level_scan_cases as L
import _level_scan_model as LM
import _lsm_cases as C
import _scan_cases as K
import _scan_model as S
from test_gpu_scan import GUARD, RANGE_OUT, assert_equal, drain, raw_inputs, raw_outputs
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import BlockError, DeviceTable

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- harness
def device(ctx, case):
    tables = [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom) for p in lv]
              for lv in case.pieces]
    if getattr(case, "runs", None):
        return DeviceLsm(ctx, [DeviceRun(ctx, r) for r in case.runs], tables)
    return DeviceLevels(ctx, tables)


def check(ctx, case, limit, idx=None, dl=None):
    """The level path (forced) over the case's ranges against the per-table model."""
    idx = list(range(len(case.ranges))) if idx is None else idx
    dl = dl or device(ctx, case)
    ranges = [case.ranges[r] for r in idx]
    got = dl.scan_batch(ranges, limit, by_level=True)
    assert_equal(got, case.models(limit, idx), limit, ranges)
    return dl, got


def level_of(case, t: int) -> int:
    first = np.cumsum([0] + [len(lv) for lv in case.pieces])
    return int(np.searchsorted(first, t, side="right")) - 1


# ------------------------------------------------------------------------------- 1. wide levels
def wide_coverage() -> dict:
    """What the wide set's scans reach, from the models alone."""
    case = L.wide_case()
    seen = dict.fromkeys(("crossing", "dropped_below", "dropped_above", "lower_in_gap",
                          "upper_in_gap", "inverted", "starts_in_next", "quirk_from_level", "more",
                          "done"), 0)
    assert all(S.open_failure(t) is None for lv in case.host for t in lv)     # (sets the keys)
    gaps = [(a.biggest_key, b.smallest_key) for lv in case.host[1:] for a, b in zip(lv, lv[1:])]
    bigs = {t.biggest_key: L.table_index(case, lv, j) for lv in (1, 2)
            for j, t in enumerate(case.host[lv])}
    for r, (lo, hi) in enumerate(case.ranges):
        m = case.model(r, L.BIG)
        per_level = [[t for t, _, _ in m.hits if level_of(case, t) == lv] for lv in (1, 2)]
        seen["crossing"] += any(len(set(h)) > 1 for h in per_level)
        for lv in (1, 2):
            tables = case.host[lv]
            seen["dropped_below"] += lo is not None and tables[-1].biggest_key < lo[1]
            seen["dropped_above"] += hi is not None and tables[0].smallest_key > hi[1]
        seen["lower_in_gap"] += lo is not None and any(a < lo[1] < b for a, b in gaps)
        seen["upper_in_gap"] += hi is not None and any(a < hi[1] < b for a, b in gaps)
        seen["inverted"] += lo is not None and hi is not None and lo[1] > hi[1]
        if lo is not None and lo[0] == "ex" and lo[1] in bigs:     # Excluded at a biggest key
            g = bigs[lo[1]]
            mine = [t for t, _, _ in m.hits if level_of(case, t) == level_of(case, g)]
            seen["starts_in_next"] += bool(mine) and min(mine) == g + 1
        seen["quirk_from_level"] += bool(m.stats["quirk"] and level_of(case, m.hits[0][0]) >= 1)
        seen["done"] += m.result == S.DONE
        seen["more"] += case.model(r, 3).result == S.MORE
    return seen


@pytest.mark.parametrize("limit", L.LIMITS)
def test_wide_levels(ctx, limit):
    """3 L0 tables, 70 tables in L1, 100 in L2: 173 tables under 5 cursors, every bound-kind
    pair."""
    case = L.wide_case()
    assert [len(lv) for lv in case.pieces] == [3, 70, 100]
    assert {(lo and lo[0], hi and hi[0]) for lo, hi in case.ranges} == set(K.KIND_PAIRS)
    if limit == L.LIMITS[0]:
        seen = wide_coverage()
        assert min(seen.values()) >= 1 and seen["crossing"] >= 20, seen
        assert max(len(m.hits) for m in case.models(L.BIG)) < L.BIG
    dl, _ = check(ctx, case, limit)
    assert dl.n_cursors == 5 and dl.n_tables == 173
    # the dispatch: more than 64 tables take the level path without being asked
    ranges = case.ranges[:20]
    assert_equal(dl.scan_batch(ranges, limit), case.models(limit, range(20)), limit, ranges)


def test_the_quirk_from_a_level_cursor(ctx):
    """L1 = {a, d}, {f, g}: scan(In(b), In(c)) yields d (e0 is never end-checked), and
    scan(Ex(d), In(e)) yields nothing: the cursor does not enter the table the filter dropped."""
    case = L.quirk_case()
    m = case.models(8)
    assert m[0].entries == [(b"d", b"4")] and m[0].stats["quirk"] == 1
    assert m[1].entries == [] and m[2].entries == [(b"f", b"6"), (b"g", b"7")]
    check(ctx, case, 8)
    check(ctx, case, 1)


# ------------------------------------------------------------------------------- 2. both paths
def both_paths(ctx, case, limit):
    L.assert_honest(case.ents)
    dl = device(ctx, case)
    assert dl.n_tables + len(getattr(case, "runs", [])) <= _lib.SCAN_MAX_TABLES
    lvl = dl.scan_batch(case.ranges, limit, by_level=True)
    tab = dl.scan_batch(case.ranges, limit)
    models = case.models(limit)
    assert_equal(lvl, models, limit, case.ranges)
    assert_equal(tab, models, limit, case.ranges)
    for k in ("result", "status", "where", "first", "key_first", "val_first", "kpos", "vpos"):
        assert np.array_equal(lvl[k], tab[k]), k
    assert lvl["keys"] == tab["keys"] and lvl["values"] == tab["values"]
    for i, m in enumerate(models):
        for k in ("hit_table", "hit_block", "hit_entry"):
            assert np.array_equal(lvl[k][i, :len(m.hits)], tab[k][i, :len(m.hits)]), (k, i)


@pytest.mark.parametrize("limit", K.LIMITS)
@pytest.mark.parametrize("i", range(len(K.RANDOM_IDS)), ids=K.RANDOM_IDS)
def test_same_answers_as_the_per_table_path(ctx, i, limit):
    """tests/_scan_cases.py's random sets (the long-key prefix-tie set included) through both
    paths."""
    both_paths(ctx, K.random_case(i), limit)


@pytest.mark.parametrize("limit", K.LIMITS)
@pytest.mark.parametrize("i", range(len(C.RANDOM_IDS)), ids=C.RANDOM_IDS)
def test_same_answers_as_the_per_table_path_with_runs(ctx, i, limit):
    both_paths(ctx, C.random_case(i), limit)


# ------------------------------------------------------------------------------- 3. runs on top
def test_runs_on_top(ctx):
    """16 runs, 4 L0 tables, three levels of 30 tables through DeviceLsm."""
    case = L.runs_case()
    assert len(case.runs) == 16 and [len(lv) for lv in case.pieces] == [4, 30, 30, 30]
    full = case.model(0, L.BIG)
    assert full.result == S.DONE and full.stats["skips"] > 0
    # run 15 holds the last key of an L1 table: the eager skip moves the level cursor past it,
    # into the next table, before the key is yielded from the run
    at = case.model(1, L.BIG)
    assert at.entries[0] == (case.last, b"newest") and at.hits[0][0] == (M_HIT | 15)
    lm = LM.level_scan(case.runs, case.host, *case.ranges[1], 1)
    assert lm.stats["skips"] >= 1 and lm.stats["tables_entered"] >= 1
    # a run's tombstone hides a key only L3 holds
    assert case.model(2, L.BIG).entries == [] and case.model(2, L.BIG).stats["tombstones"] == 1
    assert case.hidden in {k for e in case.ents[3] for k, v in e if v}
    dl, _ = check(ctx, case, L.BIG)
    assert isinstance(dl, DeviceLsm) and dl.n_runs + dl.n_cursors == 23
    for limit in K.LIMITS:
        check(ctx, case, limit, dl=dl)


M_HIT = _lib.HIT_MEM


# ------------------------------------------------------------------------------- 4. the maximum
def test_sixty_four_cursors(ctx):
    """16 runs, 42 L0 tables and 6 levels of 12 tables: 114 tables, every lane of the merge wave
    live at the start of the unbounded scan. 65 cursors are refused."""
    case = L.max_case()
    assert len(case.runs) == 16 and [len(lv) for lv in case.pieces] == [42] + [12] * 6
    m = case.model(0, 16)
    assert m.stats["mem_cursors"] == 16 and m.stats["cursors"] == 42 + 72 and m.result == S.MORE
    lm = LM.level_scan(case.runs, case.host, None, None, 16)
    assert lm.stats["mem_cursors"] + lm.stats["cursors"] == _lib.LEVEL_SCAN_MAX_CURSORS
    dl, _ = check(ctx, case, 16)
    check(ctx, case, L.BIG, dl=dl)
    assert drain(dl.scan(page=7)) == case.model(0, L.BIG).entries
    tables = [list(lv) for lv in dl.levels]
    with pytest.raises(ValueError):              # 16 + 43 + 6
        DeviceLsm(ctx, dl.runs, [tables[0] + tables[0][:1]] + tables[1:])
    with pytest.raises(ValueError):              # 16 runs + 49 L0 tables
        DeviceLsm(ctx, dl.runs, [(tables[0] * 2)[:49]])
    wide = DeviceLevels(ctx, [(tables[0] * 2)[:65]])          # 65 L0 tables, no runs
    for by_level in (False, True):
        with pytest.raises(_lib.TpzError):
            wide.scan_batch([(None, None)], 4, by_level=by_level)


# ------------------------------------------------------------------------------- 5. errors
def error_check(ctx, name):
    case, lv, t = L.error_cases()[name]
    g = L.table_index(case, lv, t)
    dl = None
    for limit in L.ERROR_LIMITS:
        dl, _ = check(ctx, case, limit, dl=dl)
    return case, g, dl


def test_a_corrupt_block0_far_away_fails_the_scan_at_creation(ctx):
    """A failing head in (a, z]: ERROR with nothing yielded although `limit` 1 would never reach
    the table; the same table outside [a, z] does nothing."""
    case, lv, t = L.error_cases()["block0"]
    g = L.table_index(case, lv, t)
    honest = L.wide_case()
    far = near = outside = 0
    for r in range(len(case.ranges)):
        m, h = case.model(r, 1), honest.model(2 * r, 1)
        if m.result == S.ERROR:
            assert (m.status, m.where, m.hits) == (_lib.BLOCK_CHECKSUM_MISMATCH, (g, 0, 0), [])
            far += h.result == S.MORE and h.hits[0][0] != g and abs(h.hits[0][0] - g) > 20
            near += bool(h.hits) and h.hits[0][0] == g
        else:
            assert LM.same(m, h)
            outside += 1
    assert far >= 5 and outside >= 20, (far, near, outside)
    error_check(ctx, "block0")


def test_a_corrupt_middle_block_is_met_during_the_merge(ctx):
    case, lv, t = L.error_cases()["middle"]
    g = L.table_index(case, lv, t)
    errs = [m for m in case.models(L.BIG) if m.result == S.ERROR]
    assert len(errs) >= 10 and all(m.where == (g, 1, 0) for m in errs)
    assert sum(1 for m in errs if len(m.hits) >= 5) >= 5       # entries come before the failure
    assert any(m.result == S.MORE for m in case.models(1))     # a page that ends before it
    error_check(ctx, "middle")


def test_a_table_that_could_not_be_opened_fails_every_scan(ctx):
    """A corrupt last block in the middle of the 100-table level."""
    case, lv, t = L.error_cases()["last"]
    g = L.table_index(case, lv, t)
    nb = L.n_blocks(case.pieces[lv][t])
    assert lv == 2 and 40 <= t < 100
    want = (S.ERROR, _lib.BLOCK_CHECKSUM_MISMATCH, (g, nb - 1, G.NONE), [])
    assert all((m.result, m.status, m.where, m.hits) == want for m in case.models(1))
    _, _, dl = error_check(ctx, "last")
    with pytest.raises(BlockError, match=r"checksum: expected"):
        dl.scan(("in", b"a"), ("in", b"b"))


def test_a_malformed_probe_entry_in_a_later_table(ctx):
    """Block 0's entry n // 2 is unreadable: create_and_seek_to_key's bisection panics there
    (a failing head for keyed lower bounds), create_and_seek_to_first does not (the scan fails
    when the merge reaches the entry)."""
    case, lv, t = L.error_cases()["probe"]
    g = L.table_index(case, lv, t)
    keyed = [m for (lo, _), m in zip(case.ranges, case.models(L.BIG)) if lo and m.result == S.ERROR]
    unb = [m for (lo, _), m in zip(case.ranges, case.models(L.BIG)) if not lo and m.result == S.ERROR]
    assert len(keyed) >= 5 and len(unb) >= 2
    assert all(m.status == _lib.BLOCK_MALFORMED and m.where[:2] == (g, 0) for m in keyed + unb)
    assert sum(1 for m in keyed if not m.hits) >= 5 and all(m.hits for m in unb)
    error_check(ctx, "probe")


def test_an_empty_block0_is_skipped(ctx):
    """A table whose block 0 holds no entry: create_and_seek_to_first leaves its cursor invalid
    (an Unbounded scan passes the table over), create_and_seek_to_key moves to block 1."""
    case, lv, t = L.error_cases()["empty0"]
    g = L.table_index(case, lv, t)
    assert all(m.result != S.ERROR for m in case.models(L.BIG))
    unb = case.model(next(r for r, (lo, hi) in enumerate(case.ranges) if lo is None and hi is None),
                     L.BIG)
    assert g not in {x for x, _, _ in unb.hits} and {g - 1, g + 1} <= {x for x, _, _ in unb.hits}
    assert any(g in {x for x, _, _ in m.hits} for m in case.models(L.BIG))
    error_check(ctx, "empty0")


def test_the_first_failure_in_priority_order_is_reported(ctx):
    """An L0 table whose seek fails and a level table whose head fails, in one scan."""
    base = L.wide_case()
    t0 = next(j for j, p in enumerate(base.pieces[0]) if L.n_blocks(p) >= 2)
    k0 = base.ents[0][t0][0][0]                                  # the L0 table's smallest key
    t2 = next(t for t in range(3, 100) if L.n_blocks(base.pieces[2][t]) >= 2)
    last2 = base.ents[2][t2][-1][0]
    assert last2 + b"\0" < k0
    ranges = [(None, None), (("in", b"a"), None), (None, ("in", last2 + b"\0")),
              (None, ("ex", base.ents[2][1][0][0]))]
    case = L.variant(base, [(0, t0, lambda p: L.corrupt(p, 0)), (2, t2, lambda p: L.corrupt(p, 0))],
                     ranges=ranges)
    g2 = L.table_index(case, 2, t2)
    m = case.models(4)
    assert [x.result for x in m[:3]] == [S.ERROR] * 3
    assert m[0].where == (t0, 0, 0) and m[1].where == (t0, 0, 0)       # L0 comes first
    assert m[2].where == (g2, 0, 0)          # the L0 table is dropped: the level's head is left
    assert m[3].result != S.ERROR and m[3].hits                        # neither is in the range
    check(ctx, case, 4)


# ------------------------------------------------------------------------------- 6. paging
def test_pages_across_table_boundaries(ctx):
    case = L.wide_case()
    dl = device(ctx, case)
    l1 = case.ents[1]
    lo, hi = ("in", l1[30][0][0]), ("in", l1[42][-1][0])
    want = S.lsm_scan(case.host, lo, hi, L.BIG)
    tables = {t for t, _, _ in want.hits if level_of(case, t) == 1}
    assert want.result == S.DONE and len(tables) >= 10 and len(want.entries) >= 40
    assert drain(dl.scan(lo, hi, page=1)) == want.entries
    assert drain(dl.scan(lo, hi, page=7)) == want.entries
    full = S.lsm_scan(case.host, None, None, L.BIG)
    assert drain(dl.scan(page=7)) == full.entries
    case = L.runs_case()
    dl = device(ctx, case)
    want = case.model(0, L.BIG)
    assert drain(dl.scan(page=7)) == want.entries
    l2 = case.ents[2]
    lo, hi = ("ex", l2[3][-1][0]), ("ex", l2[9][0][0])
    want = L.M.lsm_scan_mem(case.runs, case.host, lo, hi, L.BIG)
    assert len(want.entries) >= 15
    assert drain(dl.scan(lo, hi, page=1)) == want.entries


# ------------------------------------------------------------------------------- 7. edges
A, Bb, Cc, D, E, F = [(bytes([97 + i]), b"%d" % i) for i in range(6)]


def test_edges(ctx):
    ranges = [(None, None), (("in", b"b"), ("ex", b"e")), (("ex", b"c"), None), (None, ("in", b"c")),
              (("after", b"a"), ("in", b"f"))]
    sets = {
        "no_tables": ([], []),
        "no_tables_six_levels": ([], [[] for _ in range(6)]),
        "runs_only": ([[A, (b"c", b"")], [Bb, Cc]], [[], []]),
        "an_empty_level_between": ([], [[[Bb]], [[A], [Cc, D]], [], [[A, (b"c", b"x")], [E], [F]]]),
        "a_level_of_one_table": ([[D]], [[], [[A, Cc, E]], [[Bb]]]),
    }
    for name, (runs, ents) in sets.items():
        case = L.LevelCase(runs, ents, K.pieces_of(ents, L.BLOCK), ranges)
        dl, got = check(ctx, case, 8)
        check(ctx, case, 1, dl=dl)
        assert_equal(dl.scan_batch([], 8, by_level=True), [], 8, [])      # n_scans == 0
        if name.startswith("no_tables"):
            assert (got["first"] == 0).all() and (got["result"] == S.DONE).all()
        if name == "runs_only":
            assert case.model(0, 8).entries == [A, Bb, Cc]
        if name == "an_empty_level_between":
            assert case.model(0, 8).entries == [A, Bb, Cc, D, E, F]


# ------------------------------------------------------------------------------- 8. precondition
def broken_sets():
    rng_tabs = [[(L.key(10 * t + j), b"v%d.%d" % (t, j)) for j in range(0, 10, 3)] for t in range(12)]
    overlapping = [[(L.key(7 * t + j), b"o%d.%d" % (t, j)) for j in range(0, 20, 4)] for t in range(12)]
    return {"overlapping": [[rng_tabs[0]], overlapping],
            "reversed": [[rng_tabs[0]], list(reversed(rng_tabs))]}


@pytest.mark.parametrize("name", ["overlapping", "reversed"])
def test_a_broken_precondition_stays_in_bounds(ctx, name):
    """A level below L0 that overlaps or is stored in reverse order (descriptors truthful): the
    results are unspecified; the call returns, counts stay within `limit`, and nothing is written
    past a column's end or past key_cap / val_cap."""
    ents = broken_sets()[name]
    with pytest.raises(AssertionError):
        L.assert_honest(ents)
    case = L.LevelCase([], ents, K.pieces_of(ents, L.BLOCK), [])
    dl = device(ctx, case)
    pairs = [(L.key(a), L.key(b)) for a, b in ((0, 200), (35, 60), (60, 35), (57, 57), (3, 118))]
    ranges = K.ranges_of(pairs)
    n, limit = len(ranges), 5
    cols = raw_inputs(dl, ranges)
    out, sizes = raw_outputs(dl, n, limit)
    dl.ctx.level_scan_ranges_ptrs(0, 0, dl.d_tables.data_ptr(), dl.n_tables,
                                  dl.level_first.ctypes.data, dl.n_levels,
                                  *(c.data_ptr() for c in cols), n, limit,
                                  *(out[k].data_ptr() for k, _, _ in RANGE_OUT), 0)
    torch.cuda.synchronize()
    for k, _, _ in RANGE_OUT:
        tail = out[k][sizes[k]:].view(torch.uint8).cpu().numpy()
        assert (tail == 0xA5).all(), k
    first = out["first"][:n + 1].cpu().numpy()
    assert first[0] == 0 and (np.diff(first) >= 0).all() and (np.diff(first) <= limit).all()
    n_ent, kbytes, vbytes = (int(x) for x in out["info"][:3].cpu().numpy())
    assert n_ent == first[n] and 0 <= kbytes <= 5 * n_ent and 0 <= vbytes <= 8 * n_ent
    kp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
    vp = torch.full((n_ent + 1 + GUARD,), -1, dtype=torch.int64, device=dl.dev)
    for kc, vc in ((kbytes, vbytes), (kbytes // 2, vbytes // 3)):
        kb = torch.full((kbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        vb = torch.full((vbytes + 256,), 0xA5, dtype=torch.uint8, device=dl.dev)
        dl.ctx.level_scan_entries_ptrs(0, 0, dl.d_tables.data_ptr(), dl.n_tables, n, limit,
                                       out["hit_table"].data_ptr(), out["hit_block"].data_ptr(),
                                       out["hit_entry"].data_ptr(), out["first"].data_ptr(),
                                       kb.data_ptr(), kc, kp.data_ptr(), vb.data_ptr(), vc,
                                       vp.data_ptr(), 0)
        torch.cuda.synchronize()
        assert (kp[n_ent + 1:] == -1).all() and (vp[n_ent + 1:] == -1).all()
        assert (kb[kc:] == 0xA5).all() and (vb[vc:] == 0xA5).all()

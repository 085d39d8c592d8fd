"""The model of LsmStorage::get / LsmStorage::scan over memtable runs plus SSTs
(tests/_lsm_model.py) against the reference's own tests, a closed form on honest inputs, and the
quirks one by one (CPU only). The GPU tests compare the device against this model."""
import functools

import pytest

import _get_model as G
import _lsm_cases as C
import _lsm_model as M
import _scan_cases as K
import _scan_model as S
from topazdb_amd import _lib

BIG = 1 << 20
NONE3 = (G.NONE,) * 3


def scan(runs, level_ents, lower, upper, limit=BIG, block_size=64):
    return M.lsm_scan_mem(runs, K.host_levels(K.pieces_of(level_ents, block_size)), lower, upper,
                          limit)


# ------------------------------------------------------------------------------- the reference's tests
@pytest.mark.parametrize("name", sorted(M.reference_cases()))
def test_reference_scan_cases(name):
    """src/tests/storage.rs:110-246: the memtables as runs, the synced tables as L0."""
    runs, l0, scans = M.reference_cases()[name]
    for lo, hi, want in scans:
        m = scan(runs, [l0], lo, hi)
        assert (m.result, m.entries) == (S.DONE, want), (lo, hi)
        assert M.paged_scan_mem(runs, K.host_levels(K.pieces_of([l0], 64)), lo, hi, 1)[0] == want
        assert all(C.in_run(t) == (k in dict(runs[0])) for (t, _, _), (k, _) in zip(m.hits, m.entries))


def test_reference_get_after_sync():
    """src/tests/storage.rs:167-182."""
    host = K.host_levels(K.pieces_of([[[(b"1", b"233"), (b"2", b"2333")]]], 64))
    runs = [[(b"3", b"23333")]]
    assert [M.lsm_get_mem(runs, host, k).value for k in (b"1", b"2", b"3")] == \
        [b"233", b"2333", b"23333"]
    runs = [[(b"2", b""), (b"3", b"23333")]]
    g = M.lsm_get_mem(runs, host, b"2")
    assert (g.result, g.table, g.block, g.entry) == (G.DELETED, M.HIT_MEM | 0, 0, 0)
    assert M.lsm_get_mem(runs, host, b"").result == G.ERROR


# ------------------------------------------------------------------------------- closed form
@pytest.mark.parametrize("i", range(len(C.RANDOM_IDS)), ids=C.RANDOM_IDS)
def test_model_equals_closed_form(i):
    case = C.random_case(i)
    for r, (lo, hi) in enumerate(case.ranges):
        m = case.model(r, BIG)
        assert m.result == S.DONE
        assert m.entries == M.closed_scan_mem(case.runs, case.ents, lo, hi), (lo, hi)
        assert M.flat_scan_mem(case.runs, case.host, lo, hi, BIG).hits == m.hits
    for r in range(0, len(case.ranges), 7):
        lo, hi = case.ranges[r]
        assert M.paged_scan_mem(case.runs, case.host, lo, hi, 3)[0] == case.model(r, BIG).entries
    held = sorted({k for lv in case.ents for e in lv for k, _ in e} | {k for r in case.runs for k, _ in r})
    for k in held + [k + b"\0" for k in held[::5]]:
        g = M.lsm_get_mem(case.runs, case.host, k)
        assert (g.value if g.result == G.FOUND else None) == M.closed_get_mem(case.runs, case.ents, k)


# ------------------------------------------------------------------------------- quirks
A, B, Cc, D, E = (b"a", b"1"), (b"b", b"2"), (b"c", b"3"), (b"d", b"4"), (b"e", b"5")


@pytest.mark.parametrize("lower,contributes", [(None, False), (("in", b""), False),
                                               (("ex", b""), True), (("after", b""), True),
                                               (("in", b"a"), True)])
def test_a_run_starting_with_the_empty_key(lower, contributes):
    """batch_put does not assert on keys: a cursor that starts on the empty key is invalid
    (MemTableIterator::is_valid) and MergeIterator::create drops it; the memtable then
    contributes nothing."""
    run = [(b"", b"empty"), (b"b", b"run"), (b"f", b"run")]
    m = scan([run], [[[A, D]]], lower, None)
    assert m.result == S.DONE and m.stats["mem_cursors"] == int(contributes)
    assert m.entries == ([A, (b"b", b"run"), D, (b"f", b"run")] if contributes else [A, D])
    # ... whatever an older run holds
    m = scan([[B], run], [[[A, D]]], lower, None)
    assert m.entries == ([A, (b"b", b"run"), D, (b"f", b"run")] if contributes else [A, B, D])


def test_e0_past_the_end_comes_from_an_sst_lane_only():
    """Run cursors are bounded above, so the unchecked e0 can only be an SST entry: with a run key
    in range e0 is that key and the scan ends at the table's key past the end."""
    tables = [[[A, D]]]
    m = scan([[(b"a0", b"r"), E]], tables, ("in", b"b"), ("in", b"c"))
    assert (m.entries, m.stats["quirk"], m.stats["mem_cursors"]) == ([D], 1, 0)
    m = scan([[(b"bb", b"r"), E]], tables, ("in", b"b"), ("in", b"c"))
    assert (m.entries, m.stats["quirk"], m.stats["mem_cursors"]) == ([(b"bb", b"r")], 0, 1)
    m = scan([[(b"bb", b""), E]], tables, ("in", b"b"), ("in", b"c"))     # a tombstone as e0
    assert (m.entries, m.stats["quirk"]) == ([], 0)
    m = scan([[(b"bb", b"r"), E]], tables, ("after", b"b"), ("in", b"c"))
    assert m.entries == [(b"bb", b"r")]
    m = scan([[(b"a0", b"r"), E]], tables, ("after", b"b"), ("in", b"c"))  # After checks e0
    assert m.entries == []


@pytest.mark.parametrize("lower,upper", [(("in", b"d"), ("in", b"b")), (("ex", b"c"), ("in", b"c")),
                                         (("in", b"c"), ("ex", b"c")), (("ex", b"c"), ("ex", b"c")),
                                         (("after", b"c"), ("in", b"c"))])
def test_inverted_and_equal_excluded_bounds(lower, upper):
    """The run cursors are empty; what the tables yield is the SST half's answer, e0 included."""
    run = [B, Cc, D]
    host = K.host_levels(K.pieces_of([[[A, Cc, E]]], 64))
    m = M.lsm_scan_mem([run], host, lower, upper, BIG)
    assert m.stats["mem_cursors"] == 0
    assert m.entries == S.lsm_scan(host, lower, upper, BIG).entries
    if lower[0] != "after":                      # (the closed form has no end-checked e0)
        assert m.entries == M.closed_scan_mem([run], [[[A, Cc, E]]], lower, upper)
    assert all(not C.in_run(t) for t, _, _ in m.hits)
    one = M.lsm_scan_mem([run], host, ("in", b"c"), ("in", b"c"), BIG)   # equal and Included: one key
    assert one.entries == [Cc] and C.in_run(one.hits[0][0])


def corrupt(p, block):
    region = bytearray(p.region)
    region[int(p.ext[block]) + 7] ^= 0x80                      # the block's CRC no longer matches
    p.region = bytes(region)


@functools.lru_cache(maxsize=None)
def eager_case(bad=3):
    """tests/test_gpu_scan.py's corrupt_case under a run that holds the last key before the bad
    block (and the key two before it): the SST side reads the bad block while it leaves that key,
    which TwoMergeIterator makes it do before the key is yielded."""
    keys = [b"ek%04d" % i for i in range(300)]
    old = [(k, b"old:" + k) for k in keys]
    mid = [(k, b"mid:" + k) for k in keys[::3]]
    pieces = K.pieces_of([[old, mid]], 256)
    p = pieces[0][1]
    corrupt(p, bad)
    fk = p.first_keys
    in_before = [k for k, _ in mid if fk[bad - 1] <= k < fk[bad]]
    last_before = in_before[-1]
    run = [(in_before[-3], b"run:a"), (last_before, b"run:b"), (b"zz", b"run:z")]
    ranges = [(("in", fk[bad - 1]), None),          # 0: the run's key mid-scan
              (("in", last_before), None),          # 1: the run's key first: create() fails
              (("ex", in_before[-2]), None),        # 2: ... reached after an Excluded lower bound
              (("in", fk[bad - 1]), ("ex", last_before)),   # 3: ends before the run's key is looked at
              (("in", fk[0]), ("in", fk[1]))]       # 4: far from it
    return C.LsmCase([run], [[old, mid]], pieces, ranges), bad, last_before


def test_the_eager_skip_reports_errors_one_element_early():
    case, bad, last_before = eager_case()
    cs = _lib.BLOCK_CHECKSUM_MISMATCH
    for r in (0, 1, 2):
        two = case.model(r, BIG)
        lo, hi = case.ranges[r]
        flat = M.flat_scan_mem(case.runs, case.host, lo, hi, BIG)
        assert (two.result, two.status, two.where) == (S.ERROR, cs, (1, bad, 0)), r
        assert (flat.result, flat.status, flat.where) == (S.ERROR, cs, (1, bad, 0)), r
        assert len(two.hits) + 1 == len(flat.hits), r
        assert flat.entries[:-1] == two.entries and flat.entries[-1] == (last_before, b"run:b")
        assert two.stats["skips"] >= 1
    assert len(case.model(0, BIG).hits) >= 5 and case.model(1, BIG).hits == []
    assert {t for t, _, _ in case.model(2, BIG).hits} == {0}         # the older table's two keys between
    # a limit that ends exactly before the failing step: MORE's extra next is that step
    n = len(case.model(0, BIG).hits)
    assert case.model(0, n).result == S.ERROR and len(case.model(0, n).hits) == n
    assert case.model(0, n - 1).result == S.MORE
    assert any(C.in_run(t) for t, _, _ in case.model(0, BIG).hits)     # the run's earlier key came out
    for r in (3, 4):
        assert case.model(r, BIG).result == S.DONE and case.model(r, BIG).hits, r


# ------------------------------------------------------------------------------- coverage
@functools.lru_cache(maxsize=None)
def coverage() -> dict:
    """What the random cases' scans meet, over all cases and limits, from the model alone."""
    seen = dict.fromkeys(("done", "more", "nothing", "run_over_run", "run_over_sst",
                          "sst_between_runs", "run_tombstone_hides_sst", "more_ends_on_run",
                          "after_page_inside_run", "quirk"), 0)
    for i in range(len(C.RANDOM_IDS)):
        case = C.random_case(i)
        hidden = C.hidden_keys(case)
        for limit in K.LIMITS:
            for (lo, hi), m in zip(case.ranges, case.models(limit)):
                assert m.result != S.ERROR
                seen["done"] += m.result == S.DONE
                seen["more"] += m.result == S.MORE
                seen["nothing"] += not m.hits
                seen["run_over_run"] += m.stats["mem"]["ties"] > 0
                seen["run_over_sst"] += m.stats["skips"] > 0
                kinds = [C.in_run(t) for t, _, _ in m.hits]
                seen["sst_between_runs"] += any(kinds[j - 1] and not kinds[j] and kinds[j + 1]
                                                for j in range(1, len(kinds) - 1))
                if m.entries:
                    first, last = m.entries[0][0], m.entries[-1][0]
                    seen["run_tombstone_hides_sst"] += any(first < k < last for k in hidden)
                seen["more_ends_on_run"] += m.result == S.MORE and kinds[-1]
                seen["quirk"] += m.stats["quirk"]
        for lo, hi in case.ranges[::9]:          # the pages of a consumer, three entries each
            s = M.lsm_scan_mem(case.runs, case.host, lo, hi, 3)
            while s.result == S.MORE:
                s = M.lsm_scan_mem(case.runs, case.host, ("after", s.entries[-1][0]), hi, 3)
                seen["after_page_inside_run"] += bool(s.hits) and C.in_run(s.hits[0][0]) \
                    and s.hits[0][2] > 0
    return seen


def test_random_cases_reach_what_they_are_for():
    seen = coverage()
    assert min(seen.values()) >= 1, seen
    assert min(v for k, v in seen.items() if k != "quirk") >= 20, seen

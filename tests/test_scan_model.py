"""The closed form of a scan over an honest table set equals the restated LsmStorage::scan
(tests/_scan_model.py), and the restatement passes the reference's own scan tests
(src/tests/storage.rs:110-246). Tables are built on the host and decoded by the oracle; no GPU."""
import pytest

import _get_model as G
import _scan_cases as K
import _scan_model as S


def levels_of(l0_tables, block_size=64):
    pieces = K.pieces_of([l0_tables], block_size)
    return K.host_levels(pieces)


@pytest.mark.parametrize("i", range(len(K.RANDOM_IDS)), ids=K.RANDOM_IDS)
def test_closed_form_equals_the_restated_scan(i):
    """Every bound-kind pair, bounds from the keys, their neighbours and absent keys; an
    unlimited scan is the closed form, a limited one its head."""
    case = K.random_case(i)
    big = 1 << 20
    results = {S.DONE: 0, S.MORE: 0}
    for r, (lo, hi) in enumerate(case.ranges):
        want = S.closed_scan(case.ents, lo, hi)
        full = S.lsm_scan(case.host, lo, hi, big)
        assert (full.result, full.status, full.where) == (S.DONE, 0, (G.NONE,) * 3), (lo, hi)
        assert full.entries == want, (lo, hi)
        tables = K.flat(case.host)
        for (t, b, e), (k, v) in zip(full.hits, full.entries):  # the positions hold the entries
            blk = tables[t].read_block(b)
            assert (blk.key_at(e), blk.value_at(e)) == (k, v)
        for limit in K.LIMITS:
            m = case.model(r, limit)
            assert m.entries == want[:limit] and m.hits == full.hits[:limit], (lo, hi, limit)
            # MORE iff the iterator is still valid after `limit` entries
            assert m.result == (S.MORE if len(want) > limit else S.DONE), (lo, hi, limit)
            results[m.result] += 1
    assert min(results.values()) >= 50, results


def test_reference_scan_cases():
    """src/tests/storage.rs:110-246: scan_memtable_1, _2 and their after_sync forms."""
    for name, (l0, scans) in S.reference_cases().items():
        levels = levels_of(l0)
        for lo, hi, want in scans:
            s = S.lsm_scan(levels, lo, hi, 16)
            assert (s.result, s.entries) == (S.DONE, want), (name, lo, hi, s)
            assert S.closed_scan([l0], lo, hi) == want, (name, lo, hi)
        # the six levels of LevelController::open, the lower five empty
        s = S.lsm_scan(levels + [[] for _ in range(5)], None, None, 16)
        assert s.entries == scans[0][2]


def test_first_element_is_never_end_checked():
    """LsmIterator::new (lsm_iterator.rs:22-33): over {a, d}, scan [b, c] yields d."""
    l0 = [[(b"a", b"1"), (b"d", b"4")]]
    levels = levels_of(l0)
    s = S.lsm_scan(levels, ("in", b"b"), ("in", b"c"), 8)
    assert (s.result, s.entries, s.stats["quirk"]) == (S.DONE, [(b"d", b"4")], 1)
    assert S.closed_scan([l0], ("in", b"b"), ("in", b"c")) == [(b"d", b"4")]
    # ... but a table wholly past the range is dropped by the filter, and `after` checks e0
    assert S.lsm_scan(levels_of([[(b"d", b"4")]]), ("in", b"b"), ("in", b"c"), 8).entries == []
    assert S.lsm_scan(levels, ("after", b"b"), ("in", b"c"), 8).entries == []
    assert S.lsm_scan(levels, ("ex", b"b"), ("in", b"c"), 8, after=True).entries == []


@pytest.mark.parametrize("limit", [1, 3])
def test_pages_concatenate_to_the_unpaged_scan(limit):
    pulled = 0
    for i in range(len(K.RANDOM_IDS)):
        case = K.random_case(i)
        for lo, hi in case.ranges[::7]:
            want = S.lsm_scan(case.host, lo, hi, 1 << 20)
            got, last = S.paged_scan(case.host, lo, hi, limit)
            assert got == want.entries and last.result == S.DONE, (lo, hi)
            pulled += len(got) > limit
    assert pulled >= 50


def test_no_tables_and_bad_kinds():
    for levels in ([], [[] for _ in range(6)]):
        s = S.lsm_scan(levels, ("in", b"a"), None, 4)
        assert (s.result, s.status, s.where, s.entries) == (S.DONE, 0, (G.NONE,) * 3, [])
    levels = levels_of([[(b"a", b"1")]])
    for lo, hi in ((("bad", b"a"), None), (None, ("after", b"a"))):
        s = S.lsm_scan(levels, lo, hi, 4)
        assert (s.result, s.status, s.where) == (S.ERROR, S._lib.BLOCK_MALFORMED, (G.NONE,) * 3)

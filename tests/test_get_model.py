"""The closed form of a get over an honest table set equals the restated LevelController::get
(tests/_get_model.py), and the restatement passes the reference's own get tests
(src/level/test.rs:117-183). Tables are built on the host and decoded by the oracle; no GPU."""
import random

import _get_model as M


def host_levels(level_ents, block_size, filters):
    """Host SsTables of the entry lists; `filters(level, table)` says whether a table gets one."""
    out, tid = [], 0
    for lv, tabs in enumerate(level_ents):
        row = []
        for t, ents in enumerate(tabs):
            fpp = 0.1 if filters(lv, t) else None
            row.append(M.build_pieces(ents, block_size, fpp).host_table(tid))
            tid += 1
        out.append(row)
    return out


def test_closed_form_equals_the_restated_get():
    rng = random.Random(20240611)
    outcomes = {M.FOUND: 0, M.DELETED: 0, M.ABSENT: 0}
    for case in range(2000):
        lower = [rng.randint(0, 3) for _ in range(rng.randint(0, 3))]
        ents = M.random_set(rng, rng.randint(0, 4), lower, rng.randint(1, 6), max_len=2)
        mask = rng.getrandbits(16)
        levels = host_levels(ents, rng.choice([24, 40, 64]), lambda lv, t: (mask >> (3 * lv + t)) & 1)
        held = sorted({k for lv in ents for tab in lv for k, _ in tab})
        qs = held + [M.random_key(rng, b"ab\x00\xff", 3) for _ in range(6)] + [b"", b"\xff" * 4]
        for q in qs:
            g = M.level_get(levels, q)
            want = M.closed_get(ents, q)
            assert g.result != M.ERROR and g.status == 0, (case, q)
            assert (g.value if g.result == M.FOUND else None) == want, (case, q, g)
            assert (g.result == M.FOUND) == (want is not None), (case, q, g)
            if g.result != M.ABSENT:      # the position is the entry holding the key
                t = [t for lv in levels for t in lv][g.table]
                assert t.read_block(g.block).key_at(g.entry) == q
                assert t.read_block(g.block).value_at(g.entry) == g.value
            outcomes[g.result] += 1
    assert min(outcomes.values()) > 1000, outcomes


def test_reference_get_cases():
    """src/level/test.rs:117-183: get_simple_key, get_simple_not_exist (before and after the
    push), get_key_new_old, get_key_delete."""
    for name, (l0, asks) in M.reference_cases().items():
        levels = host_levels([l0], 64, lambda lv, t: True)
        if l0:
            assert len(levels[0][0].block_metas) > 1, name      # block size 64: several blocks
        for key, want in asks:
            g = M.level_get(levels, key)
            assert (g.value if g.result == M.FOUND else None) == want, (name, key, g)
            assert M.closed_get([l0], key) == want, (name, key)
        if name == "get_key_delete":
            assert all(M.level_get(levels, k).result == M.DELETED for k, _ in asks)
            assert all(M.level_get(levels, k).table == 1 for k, _ in asks)


def test_no_levels_at_all():
    assert M.level_get([], b"k") == M.Get(M.ABSENT, 0, M.NONE, M.NONE, M.NONE, b"")
    assert M.closed_get([], b"k") is None

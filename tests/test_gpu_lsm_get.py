"""tpz_lsm_get_keys / tpz_lsm_get_values (LsmStorage::get for batches of keys over memtable runs
plus resident tables, src/lsm_storage.rs:198-213) and tpz_mem_prefix against the line-by-line
model of tests/_lsm_model.py, which tests/test_lsm_model.py ties to the closed form.

Every case compares d_result, d_status, d_table, d_block, d_entry, d_val_pos and the value bytes
with the model, exactly, and first asserts from the model alone that its inputs reach what the
case names. Shapes are the smallest that reach each path.
"""
import random

import numpy as np
import pytest
import torch

import _get_model as G
import _lsm_model as M
from test_gpu_get import assert_equal, count, neighbours
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import DeviceTable, ReferencePanic

pytestmark = pytest.mark.gpu

ALPHABET = b"ab\x00\xff"


# ------------------------------------------------------------------------------- harness
def device_tables(ctx, pieces):
    return [[DeviceTable(ctx, p.region, p.ext, p.first_keys, p.bloom) for p in lv] for lv in pieces]


def host_levels(pieces):
    return [[p.host_table(j) for j, p in enumerate(lv)] for lv in pieces]


def device_lsm(ctx, runs, tables, prefix=True) -> DeviceLsm:
    return DeviceLsm(ctx, [DeviceRun(ctx, r, prefix) for r in runs], tables)


def in_run(g) -> bool:
    return g.table != G.NONE and bool(g.table & M.HIT_MEM)


# ------------------------------------------------------------------------------- 1. random sets
#         seed, runs, L0, lower levels, block size
RANDOM = [(21, 0, 2, [2, 0], 64), (22, 1, 2, [1], 256), (23, 3, 3, [2, 0, 1], 64),
          (24, 5, 1, [2], 256)]
_cache = {}


def random_case(seed, n_runs, l0, lower, block_size):
    """Table sets of at most 60 keys a table and runs of at most 60 keys over one 4-letter
    alphabet (84 possible keys: every key repeats across runs and tables), computed once."""
    if seed not in _cache:
        rng = random.Random(seed)
        ents = G.random_set(rng, l0, lower, 60, ALPHABET, 3, 0.25)
        pieces = [[G.build_pieces(e, block_size) for e in tabs] for tabs in ents]
        runs = [M.random_run(rng, r) for r in range(n_runs)]
        held = sorted({k for lv in ents for tab in lv for k, _ in tab} | {k for r in runs for k, _ in r})
        qs = list(held)
        for k in held:
            qs += [q for q in neighbours(k) if q]
        qs += [bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 6))) for _ in range(40)]
        qs.insert(len(qs) // 2, b"")                             # the one empty key
        host = host_levels(pieces)
        _cache[seed] = ents, pieces, runs, qs, [M.lsm_get_mem(runs, host, q) for q in qs]
    return _cache[seed]


@pytest.mark.parametrize("seed,n_runs,l0,lower,block_size", RANDOM,
                         ids=[f"runs{c[1]}_b{c[4]}" for c in RANDOM])
def test_random_sets(ctx, seed, n_runs, l0, lower, block_size):
    ents, pieces, runs, qs, model = random_case(seed, n_runs, l0, lower, block_size)
    assert min(count(model, r) for r in (G.FOUND, G.DELETED, G.ABSENT)) >= 10
    assert count(model, G.ERROR) == 1 and model[qs.index(b"")].table == G.NONE
    assert {g.table & ~M.HIT_MEM for g in model if in_run(g)} == set(range(n_runs))
    assert any(not in_run(g) and g.result == G.FOUND for g in model)      # the walk still answers
    if n_runs:
        # a tombstone in a run hides a live value below it; an older run answers past a newer one
        hidden = sum(1 for q, g in zip(qs, model) if g.result == G.DELETED and in_run(g)
                     and G.level_get(host_levels(pieces), q).result == G.FOUND)
        assert hidden >= 3
    dl = device_lsm(ctx, runs, device_tables(ctx, pieces))
    assert_equal(dl.get_batch(qs), model, qs)
    for q, g in list(zip(qs, model))[::37]:
        if g.result != G.ERROR:
            assert dl.get(q) == (g.value if g.result == G.FOUND else None)
    with pytest.raises(ReferencePanic, match="key cannot be empty"):
        dl.get(b"")


# ------------------------------------------------------------------------------- 2. batch sizes
def test_batch_sizes(ctx):
    """1, 257 and 2049 queries: the value-length scan's partial-sum boundaries."""
    ents, pieces, runs, qs, model = random_case(*RANDOM[2])
    rng = random.Random(5)
    idx = [rng.randrange(len(qs)) for _ in range(2049)]
    big_q, big_m = [qs[i] for i in idx], [model[i] for i in idx]
    dl = device_lsm(ctx, runs, device_tables(ctx, pieces))
    for n in (1, 257, 2049):
        got = dl.get_batch(big_q[:n])
        assert_equal(got, big_m[:n], big_q[:n])
        assert len(got["val_pos"]) == n + 1 and got["val_pos"][0] == 0
    assert_equal(dl.get_batch([]), [], [])


# ------------------------------------------------------------------------------- 3. sixteen runs
def test_sixteen_runs(ctx):
    rng = random.Random(31)
    runs = [M.random_run(rng, r, 20, max_len=4) for r in range(_lib.MEM_MAX_RUNS)]
    ents = G.random_set(rng, 1, [], 60, ALPHABET, 3, 0.25)
    pieces = [[G.build_pieces(e, 64) for e in tabs] for tabs in ents]
    qs = sorted({k for r in runs for k, _ in r} | {k for k, _ in ents[0][0]})
    model = [M.lsm_get_mem(runs, host_levels(pieces), q) for q in qs]
    assert {g.table & ~M.HIT_MEM for g in model if in_run(g)} >= {0, 15}
    assert any(not in_run(g) and g.result == G.FOUND for g in model)
    assert_equal(device_lsm(ctx, runs, device_tables(ctx, pieces)).get_batch(qs), model, qs)
    with pytest.raises(ValueError):
        DeviceLsm(ctx, [DeviceRun(ctx, r) for r in runs] + [DeviceRun(ctx, runs[0])], [])


# ------------------------------------------------------------------------------- 4. prefix ties
def tie_case():
    """40-byte keys sharing 32-byte prefixes (every 8-byte prefix ties: the key bytes decide), and
    keys shorter than 8 bytes that differ only by trailing zero bytes (`a` and `a\\0` share a
    prefix: the lengths decide)."""
    rng = random.Random(41)
    stems = [bytes(rng.choice(b"xy") for _ in range(32)) for _ in range(3)]
    longs = sorted({s + bytes(rng.choice(b"pq") for _ in range(8)) for s in stems for _ in range(25)})
    shorts = sorted({b + b"\0" * z for b in (b"a", b"ab", b"b", b"\0") for z in range(0, 7)
                     if len(b) + z < 8} | {b"a" + b"\0" * 7, b"a" + b"\0" * 8})
    keys = sorted(set(longs) | set(shorts))
    runs = [[(k, b"r0:" + k[-3:]) for k in keys[::2]], [(k, b"" if i % 5 == 0 else b"r1:" + k[-3:])
                                                        for i, k in enumerate(keys[::3])]]
    qs = list(keys)
    for k in keys:
        qs += [q for q in neighbours(k) if q]
    qs += [s for s in stems] + [s + b"p" * 7 for s in stems] + [b"a" + b"\0" * 9]
    return runs, qs, [M.lsm_get_mem(runs, [], q) for q in qs]


@pytest.mark.parametrize("prefix", [True, False], ids=["prefix", "keys"])
def test_prefix_ties(ctx, prefix):
    runs, qs, model = tie_case()
    assert min(count(model, r) for r in (G.FOUND, G.DELETED, G.ABSENT)) >= 5
    assert any(g.result == G.ABSENT and len(q) < 8 and q.endswith(b"\0")
               and any(k == q.rstrip(b"\0") for k, _ in runs[0] + runs[1])
               for q, g in zip(qs, model))                       # a padded twin of a held key is absent
    assert_equal(device_lsm(ctx, runs, [], prefix).get_batch(qs), model, qs)


def test_mem_prefix_matches_numpy(ctx):
    runs, _, _ = tie_case()
    run = runs[0] + [(b"\xff" * 9, b"v")]
    want = np.array([int.from_bytes(k[:8].ljust(8, b"\0"), "big") for k, _ in run], np.uint64)
    d = DeviceRun(ctx, run)
    torch.cuda.synchronize()
    assert (d.prefix.cpu().numpy().view(np.uint64) == want).all()
    assert DeviceRun(ctx, [], True).n == 0 and DeviceRun(ctx, run, False).prefix is None


# ------------------------------------------------------------------------------- 5. values
LENGTHS = [1, 16, 255, 256, 257, 1000]


def value_case():
    rng = random.Random(51)
    vals = {n: bytes(rng.getrandbits(8) for _ in range(n)) for n in LENGTHS}
    run = sorted((b"len%05d" % n, vals[n]) for n in LENGTHS[::2])
    tab = sorted((b"len%05d" % n, vals[n]) for n in LENGTHS[1::2])
    pieces = [[G.build_pieces(tab, 4096)]]
    qs = [b"len%05d" % n for n in LENGTHS] + [b"nokey", b"len01000", b"len00257"]
    return [run], pieces, qs, [M.lsm_get_mem([run], host_levels(pieces), q) for q in qs]


def test_values_from_runs_and_tables(ctx):
    """Lane-copied and wave-copied values (past 256 bytes) from a run and from a table in one
    gather; a capacity one byte short, inside a wave-copied run value, and at 0."""
    runs, pieces, qs, model = value_case()
    assert max(len(g.value) for g in model if in_run(g)) > 256
    assert max(len(g.value) for g in model if not in_run(g)) > 256
    dl = device_lsm(ctx, runs, device_tables(ctx, pieces))
    assert_equal(dl.get_batch(qs), model, qs)
    want = b"".join(g.value for g in model)
    total, guard = len(want), 256
    w = dl.walk(qs)
    torch.cuda.synchronize()
    assert int(w["val_pos"][len(qs)]) == total
    i257 = max(i for i, g in enumerate(model) if len(g.value) == 257)
    inside = sum(len(g.value) for g in model[:i257]) + 100
    for cap in (total, total - 1, inside, 0):
        buf = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=dl.dev)
        dl.ctx.lsm_get_values_ptrs(dl.d_runs.data_ptr(), dl.n_runs, dl.d_tables.data_ptr(),
                                   dl.n_tables, len(qs), w["result"].data_ptr(),
                                   w["table"].data_ptr(), w["block"].data_ptr(),
                                   w["entry"].data_ptr(), w["val_pos"].data_ptr(), buf.data_ptr(),
                                   cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tobytes()
        assert out[:cap] == want[:cap], cap
        assert out[cap:] == b"\xa5" * (total + guard - cap), cap


def test_gather_checks_run_and_entry(ctx):
    """Positions that name no run or no entry copy nothing (the gather trusts nothing it is
    handed)."""
    runs, pieces, qs, model = value_case()
    dl = device_lsm(ctx, runs, device_tables(ctx, pieces))
    w = dl.walk(qs)
    torch.cuda.synchronize()
    total = int(w["val_pos"][len(qs)])
    hit = next(i for i, g in enumerate(model) if in_run(g) and g.result == G.FOUND)
    for col, bad in (("table", (M.HIT_MEM | 1) - (1 << 32)), ("entry", len(runs[0]))):
        keep = w[col][hit].item()
        w[col][hit] = bad
        out = dl.values(w, total).cpu().numpy().tobytes()
        w[col][hit] = keep
        a, b = (int(w["val_pos"][hit + k]) for k in (0, 1))
        want = b"".join(g.value for g in model)
        assert out[:a] == want[:a] and out[b:] == want[b:]


# ------------------------------------------------------------------------------- 6. no runs
def test_no_runs_equals_get_keys(ctx):
    """n_runs == 0: tpz_get_keys' / tpz_get_values' outputs byte for byte for non-empty keys."""
    ents, pieces, runs, qs, model = random_case(*RANDOM[0])
    qs = [q for q in qs if q]
    tables = device_tables(ctx, pieces)
    a, b = DeviceLsm(ctx, [], tables).get_batch(qs), DeviceLevels(ctx, tables).get_batch(qs)
    for k in ("result", "status", "table", "block", "entry", "val_pos"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["values"] == b["values"] and len(a["values"]) > 0
    assert_equal(DeviceLsm(ctx, [], []).get_batch([b"a", b"b"]),
                 [G.Get(G.ABSENT, 0, G.NONE, G.NONE, G.NONE, b"")] * 2, [b"a", b"b"])

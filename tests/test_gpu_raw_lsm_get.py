"""tpz_raw_lsm_get_keys / tpz_raw_lsm_get_values: LsmStorage::get over memtable runs plus in-place
tables (RawTable), against the model of tests/_lsm_model.py and against DeviceLsm over
DeviceTables of the same pieces: runs answering, runs missing, tombstones in runs, no runs, the
empty-key rule. Every field and the value bytes, exactly."""
import numpy as np
import pytest
import torch

import _get_model as G
import _lsm_cases as LC
import _lsm_model as M
from test_gpu_get import assert_equal, count
from test_gpu_lsm_get import (RANDOM, device_lsm, device_tables, host_levels, in_run, random_case,
                              value_case)
from test_gpu_raw_get import assert_same, raw_table
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib
from topazdb_amd.levels import DeviceLevels, DeviceLsm, DeviceRun
from topazdb_amd.table import ReferencePanic

pytestmark = pytest.mark.gpu


def raw_tables(ctx, pieces):
    return [[raw_table(ctx, p) for p in lv] for lv in pieces]


def check(ctx, runs, pieces, qs, model) -> DeviceLsm:
    rl = device_lsm(ctx, runs, raw_tables(ctx, pieces))
    assert rl.raw or not rl.tables
    got = rl.get_batch(qs)
    assert_equal(got, model, qs)
    assert_same(got, device_lsm(ctx, runs, device_tables(ctx, pieces)).get_batch(qs))
    return rl


@pytest.mark.parametrize("seed,n_runs,l0,lower,block_size", RANDOM,
                         ids=[f"runs{c[1]}_b{c[4]}" for c in RANDOM])
def test_random_sets(ctx, seed, n_runs, l0, lower, block_size):
    ents, pieces, runs, qs, model = random_case(seed, n_runs, l0, lower, block_size)
    assert min(count(model, r) for r in (G.FOUND, G.DELETED, G.ABSENT)) >= 10
    assert count(model, G.ERROR) == 1 and model[qs.index(b"")].table == G.NONE   # the empty key
    assert {g.table & ~M.HIT_MEM for g in model if in_run(g)} == set(range(n_runs))
    assert any(not in_run(g) and g.result == G.FOUND for g in model)     # the runs miss, a table answers
    if n_runs:
        assert any(in_run(g) and g.result == G.DELETED for g in model)   # a tombstone in a run
    rl = check(ctx, runs, pieces, qs, model)
    for q, g in list(zip(qs, model))[::41]:
        if g.result != G.ERROR:
            assert rl.get(q) == (g.value if g.result == G.FOUND else None)
    with pytest.raises(ReferencePanic, match="key cannot be empty"):
        rl.get(b"")


def test_lsm_scan_cases_as_gets(ctx):
    """The table sets and runs of tests/_lsm_cases.py, asked for the keys their runs and tables
    hold and for the keys a run's tombstone hides."""
    for i in (0, 2):
        case = LC.random_case(i)
        hidden = LC.hidden_keys(case)
        qs = sorted({k for r in case.runs for k, _ in r} |
                    {k for lv in case.ents for e in lv for k, _ in e})[::2] + sorted(hidden)
        qs = [q for q in qs if q]
        model = [M.lsm_get_mem(case.runs, case.host, q) for q in qs]
        assert hidden and all(model[qs.index(k)].result == G.DELETED for k in hidden)
        assert any(in_run(g) for g in model) and any(not in_run(g) and g.result == G.FOUND
                                                     for g in model)
        check(ctx, case.runs, case.pieces, qs, model)


def test_values_from_runs_and_raw_tables(ctx):
    runs, pieces, qs, model = value_case()
    assert max(len(g.value) for g in model if in_run(g)) > 256
    assert max(len(g.value) for g in model if not in_run(g)) > 256
    rl = check(ctx, runs, pieces, qs, model)
    want = b"".join(g.value for g in model)
    total, guard = len(want), 256
    w = rl.walk(qs)
    torch.cuda.synchronize()
    assert int(w["val_pos"][len(qs)]) == total
    i257 = max(i for i, g in enumerate(model) if len(g.value) == 257)
    inside = sum(len(g.value) for g in model[:i257]) + 100
    for cap in (total, total - 1, inside, 0):
        buf = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=rl.dev)
        ctx.raw_lsm_get_values_ptrs(rl.d_runs.data_ptr(), rl.n_runs, rl.d_tables.data_ptr(),
                                    rl.n_tables, len(qs), w["result"].data_ptr(),
                                    w["table"].data_ptr(), w["block"].data_ptr(),
                                    w["entry"].data_ptr(), w["val_pos"].data_ptr(),
                                    buf.data_ptr(), cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy().tobytes()
        assert out[:cap] == want[:cap], cap
        assert out[cap:] == b"\xa5" * (total + guard - cap), cap


def test_no_runs_equals_raw_get_keys(ctx):
    """n_runs == 0: tpz_raw_get_keys' outputs byte for byte for non-empty keys; the empty key is
    the lsm flavour's assert only."""
    ents, pieces, runs, qs, model = random_case(*RANDOM[0])
    assert runs == []
    tables = raw_tables(ctx, pieces)
    nonempty = [q for q in qs if q]
    a = DeviceLsm(ctx, [], tables).get_batch(nonempty)
    b = DeviceLevels(ctx, tables).get_batch(nonempty)
    assert_same(a, b)
    assert len(a["values"]) > 0
    e = DeviceLsm(ctx, [], tables).get_batch([b""])
    assert (int(e["result"][0]), int(e["status"][0]), int(e["table"][0])) == \
        (G.ERROR, _lib.BLOCK_MALFORMED, G.NONE)
    assert int(DeviceLevels(ctx, tables).get_batch([b""])["result"][0]) != G.ERROR
    assert_equal(DeviceLsm(ctx, [DeviceRun(ctx, [(b"a", b"1")])], []).get_batch([b"a", b"b"]),
                 [G.Get(G.FOUND, 0, M.HIT_MEM, 0, 0, b"1"),
                  G.Get(G.ABSENT, 0, G.NONE, G.NONE, G.NONE, b"")], [b"a", b"b"])

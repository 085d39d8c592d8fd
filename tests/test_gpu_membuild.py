"""tpz_mem_build / tpz_wal_entries on the device against tests/_membuild_model.py: every output
column, d_src_entry, the prefix and version columns and every d_info word, under both rules
(MemTable::open's replay and do_mem_put's versions), then the runs under DeviceLsm and the flush."""
import random

import numpy as np
import pytest
import torch

import _membuild_model as M
from test_gpu_table import ctx  # noqa: F401 (fixture)
from topazdb_amd import _lib, compact
from topazdb_amd.levels import DeviceLsm, DeviceRun
from topazdb_amd.memtable import build_run, replay_wal, wal_encode
from topazdb_amd.table import ReferencePanic, _pack

pytestmark = pytest.mark.gpu

CANARY = 0xC5
GUARD = 64          # elements of canary behind every output


def guarded(n: int, dtype, dev):
    """A tensor of n + GUARD elements whose every byte is CANARY."""
    t = torch.empty(n + GUARD, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(CANARY)
    return t


def intact(t, used: int) -> bool:
    return bool((t[used:].view(torch.uint8) == CANARY).all().item())


def raw_build(ctx, entries, versions=None, kpos=None, vpos=None):
    """tpz_mem_build through the pointer call, every output behind a canary guard. Returns the
    outputs as host values, cut by what d_info says, and asserts the guards."""
    dev = torch.device("cuda", ctx.device)
    mode = _lib.MEM_REPLAY if versions is None else _lib.MEM_PUT
    n = len(entries)
    kbuf, kp = _pack([k for k, _ in entries])
    vbuf, vp = _pack([v for _, v in entries])
    kb, vb = int(kp[-1]), int(vp[-1])
    if kpos is not None:
        kp, vp = np.asarray(kpos, np.int64), np.asarray(vpos, np.int64)
    d = [torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev) for x in (kbuf, kp, vbuf, vp)]
    ver = None
    if versions is not None:
        ver = torch.from_numpy(np.asarray(list(versions) or [0], np.uint64).view(np.int64)).to(dev)
    okeys, ovals = guarded(kb, torch.uint8, dev), guarded(vb, torch.uint8, dev)
    okpos, ovpos = guarded(n + 1, torch.int64, dev), guarded(n + 1, torch.int64, dev)
    opre, over = guarded(n, torch.int64, dev), guarded(n, torch.int64, dev)
    src = guarded(n, torch.int32, dev)
    info = guarded(8, torch.int64, dev)
    ent = _lib.Entries(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, kb, vb)
    ctx.mem_build_ptrs(ent, mode, None if ver is None else ver.data_ptr(), okeys.data_ptr(),
                       okpos.data_ptr(), ovals.data_ptr(), ovpos.data_ptr(), opre.data_ptr(),
                       src.data_ptr(), over.data_ptr(), info.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    for t, used in ((okeys, kb), (ovals, vb), (okpos, n + 1), (ovpos, n + 1), (opre, n), (over, n),
                    (src, n), (info, 8)):
        assert intact(t, used), "written past a stated capacity"
    h = [int(x) for x in info[:8].cpu().numpy().view(np.uint64)]
    return dict(info=h, n=n, keys=okeys[:kb].cpu().numpy().tobytes(),
                vals=ovals[:vb].cpu().numpy().tobytes(),
                kpos=okpos[:n + 1].cpu().numpy(), vpos=ovpos[:n + 1].cpu().numpy(),
                prefix=opre[:n].cpu().numpy().view(np.uint64), version=over[:n].cpu().numpy().view(np.uint64),
                src=src[:n].cpu().numpy().view(np.uint32))


def check(ctx, entries, versions=None):
    entries = [(bytes(k), bytes(v)) for k, v in entries]
    want = M.expect(entries, versions)
    g = raw_build(ctx, entries, versions)
    assert g["info"] == want["info"] + [0, 0]
    n_out = want["info"][0]
    assert [int(x) for x in g["src"][:n_out]] == want["src"]
    kp, vp = [int(x) for x in g["kpos"][:n_out + 1]], [int(x) for x in g["vpos"][:n_out + 1]]
    assert kp == list(np.cumsum([0] + [len(k) for k in want["keys"]]))
    assert vp == list(np.cumsum([0] + [len(v) for v in want["vals"]]))
    assert g["keys"][:kp[-1]] == b"".join(want["keys"])
    assert g["vals"][:vp[-1]] == b"".join(want["vals"])
    assert [int(x) for x in g["prefix"][:n_out]] == want["prefix"]
    assert [int(x) for x in g["version"][:n_out]] == want["version"]
    assert want["keys"] == sorted(set(want["keys"]))           # strictly increasing, [u8] order
    return want


def block_versions(rng, n, lo=1, hi=50):
    out, v = [], 0
    while len(out) < n:
        v += rng.randrange(1, 4)
        out += [v] * rng.randrange(lo, hi + 1)
    return out[:n]


def random_batch(rng, n, stem=b""):
    """n entries over about n / 2 keys of 1 .. 20 bytes: about half the entries repeat a key, within
    a version block and across blocks."""
    pool = [stem + bytes(rng.randrange(256) for _ in range(rng.randrange(1, 21)))
            for _ in range(max(n // 2, 1))]
    return [(rng.choice(pool), bytes(rng.randrange(256) for _ in range(rng.randrange(0, 24))))
            for _ in range(n)]


SIZES = [0, 1, 2, 1023, 1024, 1025, 2049, 3 * 1024, 5 * 1024 + 7, 70001]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_both_modes(ctx, n):
    """Tile edges (1023 / 1024 / 1025), an odd list copied through (3 and 5 tiles + 7), several merge
    levels (70,001: 69 tiles, 7 levels)."""
    rng = random.Random(n)
    ent = random_batch(rng, n)
    w = check(ctx, ent)
    assert w["info"][5] == n
    w = check(ctx, ent, block_versions(rng, n))
    if n >= 1023:
        assert w["info"][0] < n                       # duplicates were there to resolve


def test_keys_that_tie_on_every_prefix(ctx):
    rng = random.Random(5)
    ent = random_batch(rng, 2500, stem=b"a-common-stem-of-24-bytes")[:2500]
    assert len({k[:24] for k, _ in ent}) == 1
    check(ctx, ent)
    check(ctx, ent, block_versions(rng, len(ent)))


def test_zero_padding_family_and_one_byte_keys(ctx):
    rng = random.Random(6)
    fam = [b"a", b"a\0", b"a\0\0", b"", b"a\0\0\0\0\0\0\0", b"a\0\0\0\0\0\0\0\0", b"\0", b"\0\0"]
    ent = [(rng.choice(fam), bytes([i % 251]) * (i % 5)) for i in range(300)]
    w = check(ctx, ent, block_versions(rng, len(ent), 1, 9))
    assert w["keys"] == sorted(fam)                  # the empty key is an ordinary key under PUT
    check(ctx, [(k, v) for k, v in ent if k])        # REPLAY over the family without the empty key
    one = [(bytes([rng.randrange(256)]), bytes([i & 255])) for i in range(1500)]
    check(ctx, one)
    check(ctx, one, block_versions(rng, len(one)))


def test_long_key_and_value_take_the_wave_copy(ctx):
    rng = random.Random(8)
    ent = random_batch(rng, 200)
    ent[17] = (b"K" * 300, b"\x11" * 65535)
    ent[90] = (b"K" * 300, b"\x22" * 301)
    ent[150] = (b"K" * 299 + b"L", b"")
    assert 300 > _lib.MERGE_LANE_COPY_MAX
    check(ctx, ent)
    check(ctx, ent, [3] * len(ent))


def test_empty_values_are_kept(ctx):
    ent = [(b"k%03d" % (i % 40), b"" if i % 3 else b"v%d" % i) for i in range(200)]
    w = check(ctx, ent)
    assert b"" in w["vals"]
    check(ctx, ent, [1] * 100 + [2] * 100)


@pytest.mark.parametrize("versions", ["one", "distinct"])
def test_one_key_repeated(ctx, versions):
    n = 5 * 1024 + 7
    ent = [(b"the-one-key-0016", bytes([i & 255]) * (i % 7)) for i in range(n)]
    ver = [9] * n if versions == "one" else list(range(1, n + 1))
    w = check(ctx, ent, ver)
    assert w["src"] == ([0] if versions == "one" else [n - 1])
    assert check(ctx, ent)["src"] == [n - 1]


def test_sorted_and_reverse_sorted_input(ctx):
    keys = sorted({b"key-%06d" % (i * 7919 % 100000) for i in range(3000)})
    ent = [(k, k[-3:]) for k in keys]
    for order in (ent, ent[::-1]):
        w = check(ctx, order)
        assert w["info"][0] == len(keys)
        check(ctx, order, [1] * len(order))


def test_put_versions_in_blocks(ctx):
    rng = random.Random(11)
    ent = random_batch(rng, 6000)
    ver = block_versions(rng, len(ent), 1, 50)
    w = check(ctx, ent, ver)
    m, size = M.model_put(ent, ver)                  # and against the line-by-line do_mem_put
    assert dict(zip(w["keys"], w["vals"])) == {k: v for k, (v, _) in m.items()}
    assert w["info"][4] == size


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_replay_stops_at_the_first_empty_key(ctx, where):
    rng = random.Random(12)
    ent = random_batch(rng, 2100)
    at = {"first": 0, "middle": 1111, "last": 2099}[where]
    ent[at] = (b"", b"terminator")
    if where == "middle":
        ent[1500] = (b"", b"")                      # a later one changes nothing
    w = check(ctx, ent)
    assert w["info"][3] == at and w["info"][5] == at
    assert w["info"][0] == len({k for k, _ in ent[:at]})


def test_a_second_batch_over_the_first_output(ctx):
    rng = random.Random(13)
    first, second = random_batch(rng, 1500), random_batch(rng, 1300)
    second += [(k, b"again") for k, _ in first[:200]]
    v1, v2 = block_versions(rng, len(first)), [10**6] * len(second)
    a = check(ctx, first, v1)
    carried = list(zip(a["keys"], a["vals"]))
    b = check(ctx, carried + second, a["version"] + v2)
    m, size = M.model_put(first + second, v1 + v2)
    assert dict(zip(b["keys"], b["vals"])) == {k: v for k, (v, _) in m.items()}
    assert dict(zip(b["keys"], b["version"])) == {k: ver for k, (_, ver) in m.items()}
    held = sum(len(k) + len(v) for k, v in carried)
    assert (a["info"][4] + b["info"][4] - held) % 2**64 == size


def test_replay_wal_equals_open(ctx):
    rng = random.Random(14)
    ent = random_batch(rng, 2600)
    ent[40] = (b"W" * 300, b"\x33" * 65535)
    img = wal_encode(ent)
    run = replay_wal(ctx, img)
    m, size = M.mem_open(img)
    assert run.size == size and run.n == len(m) and run.n_consumed == len(ent)
    assert run.first_empty_key is None
    kp, vp = run.kpos.cpu().numpy(), run.vpos.cpu().numpy()
    kb, vb = run.keys.cpu().numpy().tobytes(), run.vals.cpu().numpy().tobytes()
    got = {kb[kp[i]:kp[i + 1]]: vb[vp[i]:vp[i + 1]] for i in range(run.n)}
    assert got == {k: v for k, (v, _) in m.items()}
    assert [kb[kp[i]:kp[i + 1]] for i in range(run.n)] == sorted(m)
    assert [ent[i][0] for i in run.src_entry.cpu().numpy()] == sorted(m)
    # an empty key ends it, and a cut image is the reference's panic
    ent[1000] = (b"", b"x")
    run = DeviceRun.from_wal(ctx, wal_encode(ent))
    m, size = M.mem_open(wal_encode(ent))
    assert (run.size, run.n, run.n_consumed, run.first_empty_key) == (size, len(m), 1000, 1000)
    with pytest.raises(ReferencePanic):
        replay_wal(ctx, img[:-1])
    empty = replay_wal(ctx, b"")
    assert (empty.n, empty.size, empty.n_consumed) == (0, 0, 0)


def test_garbage_positions_and_decreasing_versions_stay_in_bounds(ctx):
    """Precondition violations: no value is asserted, only that nothing is written outside the
    stated capacities (raw_build checks every guard) and that the call ends."""
    rng = random.Random(15)
    ent = random_batch(rng, 3000)
    n = len(ent)
    garbage_k = [rng.randrange(0, 1 << 40) if i % 3 else rng.randrange(0, 64) for i in range(n + 1)]
    garbage_v = [rng.randrange(0, 40000) for _ in range(n + 1)]
    raw_build(ctx, ent, None, garbage_k, garbage_v)
    raw_build(ctx, ent, [rng.randrange(5) for _ in range(n)], garbage_k, garbage_v)
    raw_build(ctx, ent, list(range(n, 0, -1)))
    g = raw_build(ctx, ent, [n - i // 2 for i in range(n)])
    assert g["info"][0] <= n


def test_built_runs_under_the_lsm_and_the_flush(ctx):
    rng = random.Random(16)
    batches = [random_batch(rng, 700, stem=b"k") for _ in range(3)]
    vers = [block_versions(rng, 700) for _ in range(2)]
    runs = [DeviceRun.build(ctx, batches[0], versions=vers[0]),
            build_run(ctx, batches[1], versions=vers[1]),
            DeviceRun.from_wal(ctx, wal_encode(batches[2]))]
    maps = [M.model_put(batches[0], vers[0])[0], M.model_put(batches[1], vers[1])[0],
            M.mem_open(wal_encode(batches[2]))[0]]
    dicts = [{k: v for k, (v, _) in m.items()} for m in maps]
    for r, d in zip(runs, dicts):
        assert r.n == len(d) and r.prefix is not None
    dl = DeviceLsm(ctx, runs, [])
    qs = sorted({k for d in dicts for k in d})[::3] + [b"k-absent", b"j"]
    got = dl.get_batch(qs)
    for i, q in enumerate(qs):
        want = next((d[q] for d in dicts[::-1] if q in d), None)     # the newest run first
        res = int(got["result"][i])
        val = got["values"][int(got["val_pos"][i]):int(got["val_pos"][i + 1])]
        if want is None:
            assert res == _lib.GET_ABSENT
        elif want == b"":
            assert res == _lib.GET_DELETED
        else:
            assert res == _lib.GET_FOUND and val == want
    merged = {}
    for d in dicts:
        merged.update(d)
    it, out = dl.scan(), []
    while it.is_valid():
        out.append((it.key(), it.value()))
        it.next()
    assert out == sorted((k, v) for k, v in merged.items() if v)      # LsmIterator skips tombstones
    host = [DeviceRun(ctx, sorted(d.items())) for d in dicts]
    a, a_ents = compact.flush_like_sync(ctx, runs + [DeviceRun(ctx, [])])
    b, b_ents = compact.flush_like_sync(ctx, host + [DeviceRun(ctx, [])])
    assert a.image.cpu().numpy().tobytes() == b.image.cpu().numpy().tobytes()
    assert a_ents.n == b_ents.n == len(merged)

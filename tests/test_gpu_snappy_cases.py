"""The device snappy decoders on streams no compressor here emits: the element programs of
tests/_snappy_cases.py (literal -> literal, wide literal headers, copies of 1-3 bytes, every
ordered pair of element kinds, every offset class up to 65,536 and more) through each of the three
parsers of tpz_codec.hip.

Reference: compress::decode -> snap::raw::Decoder::decompress_vec (src/block/compress.rs:104-107),
stated by the generator itself (no decoder builds the expected bytes; test_snappy_cases.py pins
both CPU restatements against it). Bar: bit for bit. A valid stream gives BLOCK_OK and the
generator's bytes + tag 1, an invalid one BLOCK_CODEC_ERROR.

Routes (tpz_codec.hip): ring_body<2> takes every valid block of a batch whose source and output
are below 0x7FFFFFF0 and at least 16 bytes; with a source span of 0x7FFFFFF0 bytes or more (passed
honestly: one big allocation, the batch at its start) the ring is not live and the blocks go to
snappy_decode in the 16-wave kernel's windows, in the one-wave kernel's, or to
snappy_decode_global, by their sizes (_snappy_cases.route_of)."""
import random

import numpy as np
import pytest
import torch

import _snappy_cases as S
from test_gpu_decode import ctx  # noqa: F401 (fixture)
from test_gpu_snappy import batch_of, device_codec
from topazdb_amd import _lib

pytestmark = pytest.mark.gpu

CANARY = 0xC5
SLACK = 4096
BIG_SRC = 0x7FFFFFF0 + 16 + (1 << 20)        # the ring needs src_bytes below 0x7FFFFFF0


def block_of(c):
    return c.stream + b"\x02"


def run_codec(ctx, blocks, src=None, src_bytes=None, claimed=False, check=True):
    """tpz_decompressed_sizes + prefix sum + tpz_decompress_blocks into an output filled with
    CANARY that has SLACK bytes after dst_ext[n]: (block outputs, statuses, ext, dst_ext). `src`:
    a device tensor that already holds the batch at its start, passed with `src_bytes`. `claimed`:
    tpz_decompressed_sizes_claimed; `check`: what tpz_decompress_check must then return."""
    data, ext = batch_of(blocks)
    n = len(blocks)
    if src is None:
        src = torch.from_numpy(np.ascontiguousarray(data).copy()).cuda()
        src_bytes = int(ext[-1])
    assert src_bytes <= src.numel()
    d_ext = torch.from_numpy(ext.view(np.int64).copy()).cuda()
    size = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.decompressed_sizes_ptrs(src.data_ptr(), d_ext.data_ptr(), n, src_bytes, size.data_ptr(),
                                claimed=claimed)
    dext = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(size, 0, out=dext[1:])
    total = int(dext[-1])
    dst = torch.full((total + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.decompress_ptrs(src.data_ptr(), d_ext.data_ptr(), n, src_bytes, dst.data_ptr(),
                        dext.data_ptr(), st.data_ptr())
    assert ctx.decompress_check() == check
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    oext = dext.cpu().numpy()
    assert (host[total:] == CANARY).all(), "bytes written past dst_ext[n]"
    raw = host.tobytes()
    outs = [raw[oext[i]:oext[i + 1]] for i in range(n)]
    return outs, st.cpu().numpy(), ext.astype(np.int64), oext


def mixed_batch():
    """Every valid program, shuffled, with the named invalid streams spread among them (each
    between two valid blocks): [(name, block, expected bytes or None)]."""
    valid = [(c.name, block_of(c), c.out + b"\x01") for c in S.valid_cases()]
    random.Random(7).shuffle(valid)
    bad = [(b.name, b.stream + b"\x02", None) for b in S.invalid_cases()]
    step = len(valid) // (len(bad) + 1)
    assert step >= 2
    items = []
    for i, v in enumerate(valid):
        items.append(v)
        if i % step == step - 1 and i // step < len(bad):
            items.append(bad[i // step])
    assert len(items) == len(valid) + len(bad)
    return items


def check_items(items, outs, st):
    for i, ((name, _b, want), o, s) in enumerate(zip(items, outs, st)):
        if want is None:
            assert s == _lib.BLOCK_CODEC_ERROR, (i, name, s)
        else:
            assert s == _lib.BLOCK_OK, (i, name, s)
            assert o == want, (i, name)
    for i, it in enumerate(items):             # an invalid block's neighbours are valid blocks
        if it[2] is None:
            assert items[i - 1][2] is not None and items[i + 1][2] is not None


@pytest.fixture(scope="module")
def ring_result(ctx):
    """The mixed batch through a batch-sized source: every valid block is the ring's."""
    items = mixed_batch()
    outs, st, _ext, _oext = run_codec(ctx, [b for _n, b, _w in items])
    return items, outs, st


def test_ring_route(ring_result):
    """One batch of all valid programs and the named invalid streams among them: statuses and
    every output byte, every valid neighbour of an invalid block intact, nothing written past
    dst_ext[n] (run_codec's canary)."""
    items, outs, st = ring_result
    assert sum(w is None for _n, _b, w in items) == len(S.invalid_cases())
    check_items(items, outs, st)


def probe_programs():
    rng = random.Random(0x5A10)
    probes = [
        ("literal_first", [S.lit(7), (S.C1, 4, 3), S.lit(3), (S.C2, 2, 9), S.lit(1), S.lit(2, 3)]),
        ("copy_heavy", [S.lit(4), (S.C2, 1, 1), (S.C4, 3, 2), (S.C1, 11, 5), (S.C2, 64, 19),
                        (S.C4, 64, 7), (S.C2, 33, 16), (S.C1, 8, 63), (S.C2, 64, 64), (S.C4, 2, 1)]),
        ("literal_70", [S.lit(70), (S.C2, 5, 70), S.lit(12, 3), (S.C4, 1, 80)]),
        ("literal_80_then_literal", [S.lit(80), S.lit(65, 5), S.lit(1), (S.C1, 4, 100), S.lit(79, 2)]),
        ("far_copy", [S.lit(200), (S.C2, 40, 190), (S.C4, 64, 130), (S.C1, 9, 121), S.lit(5, 5),
                      (S.C2, 3, 250), (S.C4, 64, 300)]),
        ("half_slot", [S.lit(129), (S.C2, 30, 120), (S.C2, 17, 124), (S.C4, 64, 128), (S.C2, 8, 127),
                       (S.C4, 21, 121), (S.C2, 64, 129)]),
        ("literal_65_short_copies", [S.lit(65), S.lit(1, 2), (S.C4, 1, 66), (S.C2, 3, 2), S.lit(66, 4),
                                     (S.C2, 2, 1)]),
    ]
    for i in range(3):
        prog = []
        for _ in range(24):
            prog.append(S.rand_element(rng, S.produced(prog)))
        probes.append((f"random_{i}", prog))
    return [S.case(name, prog, rng) for name, prog in probes]


def test_alignment(ctx):
    """Ten probe programs (literal-first, copy-heavy, 65-80 byte literals, literal -> literal, far
    copies, the ring's half-slot edge, random ones), each at all 64 values of its output start mod
    64 times all 16 values of its source start mod 16: the ring's lines, slots and funnels and the
    header window at every alignment. A two-element snappy block whose output is n bytes longer
    or shorter than its source sets the skew between the two positions, a tag-1 pad block of
    1..64 bytes (copied unchanged) the output start."""
    rng = random.Random(0x5A11)
    probes = probe_programs()
    assert len(probes) >= 8
    shifters = {n: S.case(f"shift_{n}", [S.lit(1), (S.C2, n, 1)], rng) for n in range(1, 17)}
    items, where = [], []
    s_pos = d_pos = 0
    for pi, pr in enumerate(probes):
        for ro in range(64):
            for rs in range(16):
                n = (s_pos - d_pos + 5 + ro - rs - 1) % 16 + 1
                sh = shifters[n]
                assert len(sh.stream) == 6 and len(sh.out) == n + 1
                pad = (ro - d_pos - (n + 2) - 1) % 64 + 1
                padb = rng.randbytes(pad - 1) + b"\x01"
                items += [(sh.name, block_of(sh), sh.out + b"\x01"), ("pad", padb, padb)]
                s_pos += 7 + pad
                d_pos += n + 2 + pad
                assert d_pos % 64 == ro and s_pos % 16 == rs
                where.append((pi, len(items)))
                items.append((pr.name, block_of(pr), pr.out + b"\x01"))
                s_pos += len(pr.stream) + 1
                d_pos += len(pr.out) + 1
    outs, st, ext, oext = run_codec(ctx, [b for _n, b, _w in items])
    for i, ((name, _b, want), o, s) in enumerate(zip(items, outs, st)):
        assert s == _lib.BLOCK_OK and o == want, (i, name, int(oext[i]) % 64, int(ext[i]) % 16)
    achieved = {(pi, int(oext[i]) % 64, int(ext[i]) % 16) for pi, i in where}
    assert achieved == {(pi, ro, rs) for pi in range(len(probes)) for ro in range(64)
                        for rs in range(16)}


def test_end_of_source(ctx):
    """Batches whose src_bytes is exactly ext[n]: the last block's final element is a literal of
    1..100 bytes (the ring's clamped loads near the end of the source, with the next header taken
    out of the literal's last piece or not), and the same with a copy as the final element."""
    rng = random.Random(0x5A12)
    prefixes = ([], [S.lit(30), (S.C2, 5, 30)], [S.lit(75), S.lit(3, 5)], [S.lit(16), (S.C4, 1, 16)])
    lead = [S.case(f"lead_{i}", [S.rand_element(rng, 0), S.lit(20), (S.C1, 7, 9)], rng)
            for i in range(2)]
    n_runs = 0
    for L in (1, 15, 16, 17, 64, 80, 81, 100):
        for pre in prefixes:
            for final_copy in (False, True):
                prog = list(pre) + [S.lit(L, rng.choice([h for h in range(S.min_hw(L), 6)]))]
                if final_copy:
                    prog.append(S.rand_copy(rng, S.produced(prog)))
                last = S.case(f"tail_{L}", prog, rng)
                for cases in ([last], lead + [last]):
                    blocks = [block_of(c) for c in cases]
                    if sum(map(len, blocks)) < 16:
                        continue                        # (tiny batches: test_tiny_batches)
                    outs, st = device_codec(ctx, blocks)
                    n_runs += 1
                    for c, o, s in zip(cases, outs, st):
                        assert s == _lib.BLOCK_OK and o == c.out + b"\x01", (L, pre, final_copy, c.name)
    assert n_runs >= 100


@pytest.fixture(scope="module")
def big_src(ctx):
    """One allocation of 0x7FFFFFF0 + 16 bytes and a MiB: a batch placed at its start and passed
    with the whole size as src_bytes is not the ring's. Never filled: a correct kernel reads only
    the batch."""
    free, _total = torch.cuda.mem_get_info()
    need = BIG_SRC + (2 << 30)
    assert free >= need, f"{free >> 20} MiB free on the device, the source span needs {need >> 20} MiB"
    buf = torch.empty(BIG_SRC, dtype=torch.uint8, device="cuda")
    yield buf
    del buf


def test_wave_side_routes(ctx, big_src, ring_result):
    """The same valid and invalid sets with the ring not live: snappy_decode in the small and in
    the big windows and snappy_decode_global, each with every ordered pair and every header width
    (test_snappy_cases.py::test_reach_of_each_wave_side_route), the offsets of 65,536 and more on
    the global decoder. Against the generator, and equal to the ring route's result."""
    items, ring_outs, ring_st = ring_result
    blocks = [b for _n, b, _w in items]
    data, ext = batch_of(blocks)
    n_bytes = int(ext[-1])
    big_src[:n_bytes].copy_(torch.from_numpy(np.ascontiguousarray(data).copy()))
    big_src[n_bytes:n_bytes + (1 << 20)].fill_(CANARY)
    routes = {k: 0 for k in ("small", "big", "global")}
    for c in S.valid_cases():
        routes[S.route_of(c)] += 1
    assert min(routes.values()) >= 30
    outs, st, _ext, _oext = run_codec(ctx, blocks, src=big_src, src_bytes=BIG_SRC)
    check_items(items, outs, st)
    np.testing.assert_array_equal(st, ring_st)
    for (name, _b, want), o, ro in zip(items, outs, ring_outs):
        if want is not None:
            assert o == ro, name


def test_tiny_batches(ctx):
    """A batch of one valid block whose source is shorter than 16 bytes, and one whose output is:
    the wave kernel's (the ring needs 16 bytes of each)."""
    rng = random.Random(0x5A13)
    short_src = S.case("short_src", [S.lit(3), (S.C1, 11, 3), (S.C2, 64, 2)], rng)
    assert len(block_of(short_src)) < 16 and len(short_src.out) + 1 >= 16
    short_out = S.case("short_out", [S.lit(3, 5), S.lit(2, 5), (S.C4, 4, 5), (S.C4, 1, 1)], rng)
    assert len(block_of(short_out)) >= 16 and len(short_out.out) + 1 < 16
    both = S.case("short_both", [S.lit(1), S.lit(1, 2), (S.C2, 3, 2), (S.C2, 1, 5)], rng)
    assert len(block_of(both)) < 16 and len(both.out) + 1 < 16
    for c in (short_src, short_out, both):
        outs, st, _ext, _oext = run_codec(ctx, [block_of(c)])
        assert st[0] == _lib.BLOCK_OK and outs[0] == c.out + b"\x01", c.name
        outs, st = device_codec(ctx, [block_of(c)])
        assert st[0] == _lib.BLOCK_OK and outs[0] == c.out + b"\x01", c.name

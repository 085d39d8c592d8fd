"""tpz_decode_blocks_host (the entry point the Rust facade calls, tpz_host_pipeline.cpp) against
the oracle, across chunks: every output column a caller reads, in the caller's layout, byte for
byte (tests/_host_columns.py), with every buffer at exactly the size the header asks for and a
guard region behind each.

Covered: the chunk geometry edges (chunks of 1, of n, past n, n no multiple of the chunk, a chunk
of empty blocks only, a batch that starts past byte 0, pageable and pinned buffers); batches that
mix Uncompress, snappy, lz4 and rejected streams; spill-resident blocks (OK_SPILLED, BAD_ENTRY)
in several chunks with the slot's device arena growing when a later chunk reuses it; a codec
chunk that expands past the pipeline's first guess and one that outgrows the regrown buffers;
the TPZ_ERR_NOMEM contract (the sizes reported, and a repeat with exactly those sizes); reuse of
one context's pooled buffers by calls of other shapes.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _oracle as O
import badentry_util as U
from _host_columns import (GUARD, PATTERN, Reference, assert_host_parity, check_outputs,
                           decode_host, probe_spill)
from test_gpu_decode import MG, _random_blocks
from test_gpu_snappy import batch_of
from test_gpu_spill import fuzz_blocks, repeated_offset_blocks
from topazdb_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def fresh_ctx():
    """A context whose host pipeline has no buffers yet: device arenas empty, codec buffers at
    their first guess."""
    c = _lib.Context(0)
    yield c
    c.close()


def split(src, ext):
    return [src[int(ext[i]):int(ext[i + 1])].tobytes() for i in range(len(ext) - 1)]


# ---- the batches (each built once, with its oracle answer) ------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_blocks():
    """120 blocks: random ones with a corrupted byte in every seventh, and three consecutive empty
    blocks at 9..11 (with chunk_blocks = 3 they are the whole of chunk 3)."""
    rng = np.random.default_rng(41)
    blocks = split(*_random_blocks(rng, 130, corrupt_every=7))[:117]
    assert len(blocks) == 117
    blocks[9:9] = [b"", b"", b""]
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def geometry_ref():
    return Reference(*batch_of(list(geometry_blocks())))


def codec_mix(blocks, seed, damage_snappy=True):
    """test_gpu_snappy.snappy_random_blocks' and test_gpu_lz4.lz4_random_blocks' i % 5 mix over
    given blocks: runs of five alternate between snappy and lz4, the fifth of a run stays
    Uncompress, and every seventh stream gets a flipped bit, a cut, or (lz4) a size prefix of 1,
    which the codec may reject. damage_snappy = False leaves the snappy streams whole."""
    rng = np.random.default_rng(seed)
    out = []
    for i, b in enumerate(blocks):
        lz4 = (i // 5) % 2 == 1
        if b and b[-1] == 1 and i % 5 < 4:
            b = O.lz4_block(b, 1 if i % 5 == 3 else 0) if lz4 else O.snappy_block(b, i % 5)
        if b and i % 7 == 3 and (damage_snappy or b[-1] != 2):
            b = bytearray(b)
            p = int(rng.integers(0, max(len(b) - 1, 1)))
            kind = i % 3
            if kind == 0:
                b[p] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1 or not lz4:
                b = b[:p] + b[-1:]
            else:
                b[0:4] = (1).to_bytes(4, "little")       # too small for the stream: an Err
            b = bytes(b)
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def mixed_codec_ref(damage_snappy=True):
    """The geometry blocks through codec_mix, with three repeated-offset blocks (spilled) and ten
    compressible blocks among them, so that the batch's decoded bytes exceed its compressed ones
    (the random blocks do not compress)."""
    blocks = list(geometry_blocks())
    rep = repeated_offset_blocks()
    blocks[20:20] = [rep[0]]
    blocks[61:61] = [rep[1]]
    blocks[100:100] = [rep[6]]
    blocks[40:40] = flat_blocks(4096, 10, 0)
    blocks = codec_mix(blocks, 42, damage_snappy)
    if damage_snappy:
        # the batch ends in two snappy Errs: a preamble past u32 (TooBig), and a stream cut in half
        sn = O.snappy_block(geometry_blocks()[5])
        blocks += [b"\xff\xff\xff\xff\x7fabc\x02", sn[:len(sn) // 2] + b"\x02"]
    ref = Reference(*batch_of(blocks))
    tags = {int(ref.src[int(e) - 1]) for s, e in zip(ref.ext[:-1], ref.ext[1:]) if e > s}
    assert {1, 2, 3} <= tags and (ref.o.status == O.CODEC).sum() >= 3
    assert (ref.o.status == O.OK).sum() >= 80
    return ref


@functools.lru_cache(maxsize=None)
def last_codec_ref():
    """Only the last block is a codec block: the decoded layout holds for the whole batch, though
    no chunk before the last one sees a codec block."""
    blocks = list(geometry_blocks())
    assert blocks[-1][-1] == 1
    blocks[-1] = O.snappy_block(blocks[-1])
    return Reference(*batch_of(blocks))


def spill_chunks():
    """Chunks of four blocks. Chunks 0, 1, 3 and 4 hold spill-resident blocks (OK_SPILLED and
    BAD_ENTRY), chunk 2 none; chunk 3's records (which reuse chunk 0's slot) and chunk 4's (chunk
    1's) are far larger than the earlier ones; fuzzed-offset blocks follow."""
    rng = np.random.default_rng(43)
    rep = repeated_offset_blocks()
    ents = [(U.key(i), b"value_%04d" % i) for i in range(20)]
    bad = [U.bad_block(ents, j, kind) for j, kind in ((0, "key_off"), (7, "key_len"), (19, "value"))]
    plain = split(*_random_blocks(rng, 24, max_target=3000))
    assert len(plain) >= 14
    p = iter(plain)
    blocks = [next(p), rep[6], bad[0], next(p),
              rep[0], next(p), rep[3], bad[1],
              next(p), rep[4], next(p), rep[5],
              rep[1], next(p), bad[2], rep[7],
              next(p), rep[2], next(p), next(p)]
    for f in fuzz_blocks(rng, 10):
        blocks += [f, next(p)] if len(blocks) % 3 else [f]
    return blocks


def as_codec(blocks, codec):
    enc = {None: lambda b: b, "snappy": O.snappy_block, "lz4": O.lz4_block}[codec]
    return [enc(b) if b and b[-1] == 1 else b for b in blocks]


@functools.lru_cache(maxsize=None)
def spill_ref(codec=None):
    return Reference(*batch_of(as_codec(spill_chunks(), codec)))


def chunk_record_bytes(probe, cb):
    """Spill bytes per chunk, from a probing call's record offsets (records lie in chunk order)."""
    st = probe.status
    res = np.nonzero((st == _lib.BLOCK_OK_SPILLED) | (st == _lib.BLOCK_BAD_ENTRY))[0]
    offs = probe.spill_off[res].astype(np.int64)
    order = np.argsort(offs)
    size = np.diff(np.concatenate([offs[order], [probe.spill_used]]))
    per = np.zeros((probe.n + cb - 1) // cb, np.int64)
    np.add.at(per, res[order] // cb, size)
    return per


# ---- chunk geometry ---------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("chunk", [1, 3, 7, 119, 120, 500, 0])
def test_chunk_geometry(ctx, chunk, pinned):
    ref = geometry_ref()
    assert ref.n == 120 and (np.diff(ref.ext[9:13].astype(np.int64)) == 0).all()
    assert (ref.ext.astype(np.int64)[1:] % 384 != 0).sum() > 100     # unaligned chunk starts
    out, g = assert_host_parity(ctx, ref.src, ref.ext, chunk, pinned=pinned, ref=ref)
    assert out.spill_used == 0
    assert (ref.o.status == O.CHECKSUM).sum() >= 10 and (ref.o.status == O.OK).sum() >= 90


@pytest.mark.parametrize("chunk", [7, 0])
def test_batch_starting_past_byte_zero(ctx, chunk):
    """h_ext[0] = 1000 with junk before it: the layout follows the extents as given."""
    base = geometry_ref()
    rng = np.random.default_rng(44)
    src = np.concatenate([np.frombuffer(rng.bytes(1000), np.uint8), base.src])
    ref = Reference(src, base.ext + np.uint64(1000))
    assert ref.ext[0] == 1000 and ref.dext[0] == 1000
    np.testing.assert_array_equal(ref.o.status, base.o.status)
    assert_host_parity(ctx, ref.src, ref.ext, chunk, ref=ref)


# ---- codecs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 0])
@pytest.mark.parametrize("batch", ["mixed", "mixed_snappy_whole", "last"])
def test_codec_batches(ctx, batch, chunk):
    ref = last_codec_ref() if batch == "last" else mixed_codec_ref(batch == "mixed")
    assert ref.codec
    assert_host_parity(ctx, ref.src, ref.ext, chunk, ref=ref)


# ---- spill and BAD_ENTRY across chunks --------------------------------------------------------
@pytest.mark.parametrize("codec", [None, "snappy", "lz4"])
def test_spill_records_across_chunks(ctx, fresh_ctx, codec):
    ref = spill_ref(codec)
    assert ref.codec == (codec is not None)
    probe = probe_spill(ctx, ref, 4)
    per = chunk_record_bytes(probe, 4)
    # chunk 0's arena is grown to 1.25 times its need; chunk 3 reuses it and must outgrow it
    assert per[0] > 0 and per[1] > 0 and per[2] == 0 and per[3] > 0 and per[4] > 0, per
    assert per[3] > per[0] + per[0] // 4 and per[4] > per[1] + per[1] // 4, per
    assert (ref.o.status == O.BAD_ENTRY).sum() >= 3
    out, g = assert_host_parity(fresh_ctx, ref.src, ref.ext, 4, spill_cap=probe.spill_used, ref=ref)
    assert out.spill_used == probe.spill_used == per.sum()
    assert (out.status == _lib.BLOCK_OK_SPILLED).sum() >= 6


# ---- a codec chunk past the first guess -------------------------------------------------------
def flat_blocks(target, n_blocks, start):
    """BlockBuilder(target) blocks whose values are 90 copies of one byte (the same byte within
    a block): they compress to about a tenth."""
    out, i = [], start
    for t in range(n_blocks):
        bb = MG.BlockBuilder(target)
        while bb.add(b"%08d" % i, bytes([t % 251]) * 90):
            i += 1
        out.append(MG.encode_block(*bb.build()))
    return out


@pytest.mark.parametrize("codec", ["snappy", "lz4"])
def test_codec_chunk_regrowth(fresh_ctx, codec):
    cb = 40
    blocks = (flat_blocks(4096, cb, 0) + flat_blocks(512, cb, 10 ** 5) + flat_blocks(1024, cb, 2 * 10 ** 5)
              + flat_blocks(8192, cb, 3 * 10 ** 5))
    ref = Reference(*batch_of(as_codec(blocks, codec)))
    ext = ref.ext.astype(np.int64)
    # the pipeline's first guess of a chunk's decoded bytes, and what each chunk needs
    # (tpz_host_pipeline.cpp: dst_guess and chunk_extents_kernel's need_dst)
    spans = [ext[min(ref.n, lo + cb)] - (ext[lo] - ext[lo] % 384) for lo in range(0, ref.n, cb)]
    cap = 2 * max(spans) + 65536 + 16
    need = [ref.dext[lo] % 384 + (ref.dext[lo + cb] - ref.dext[lo]) + 16 for lo in range(0, ref.n, cb)]
    assert need[0] > cap and need[3] > cap, (need, cap)
    assert need[3] > need[0] + need[0] // 4, need    # chunk 3 outgrows the slot chunk 0 regrew
    assert (ref.o.status == O.OK).all()
    # the only call on the fresh context: the one that overflows, regrows and is compared
    out, g = assert_host_parity(fresh_ctx, ref.src, ref.ext, cb, spill_cap=0, ref=ref)
    assert out.spill_used == 0


# ---- TPZ_ERR_NOMEM ----------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["spill", "mixed", "mixed_snappy_whole"])
def test_nomem_contract(ctx, batch):
    ref = spill_ref() if batch == "spill" else mixed_codec_ref(batch == "mixed")
    good = decode_host(ctx, ref.src, ref.ext, 4, ref=ref)      # exactly sufficient buffers
    check_outputs(good, ref)
    ends, spill, data = good.needs()
    assert (ends, data) == (ref.ends_need, ref.data_need) and spill == good.spill_cap > 0
    cases = {"data": dict(data_cap=data - 1), "ends": dict(ends_cap=ends - 1),
             "spill": dict(spill_cap=spill - 1),
             "all": dict(data_cap=1, ends_cap=0, spill_cap=0)}
    if ref.codec:
        # data_cap = 0 is the capacity of the compressed size, short for this batch
        assert _lib.data_capacity(int(ref.ext[-1]), ref.n) < data
        cases["data_default"] = dict(data_cap=0)
    for name, caps in cases.items():
        kw = dict(data_cap=data, ends_cap=ends, spill_cap=spill)
        kw.update(caps)
        short = decode_host(ctx, ref.src, ref.ext, 4, ref=ref, **kw)
        assert short.rc == _lib.ERR_NOMEM, name
        assert short.needs() == (ends, spill, data), name
        again = decode_host(ctx, ref.src, ref.ext, 4, ref=ref, ends_cap=short.needs()[0],
                            spill_cap=short.needs()[1], data_cap=short.needs()[2])
        assert again.rc == _lib.SUCCESS, name
        check_outputs(again, ref)


def test_verify_host_nomem(ctx):
    """tpz_verify_blocks_host with plain_cap one byte short: NOMEM and h_dext[n] = the need; with
    exactly the need: every block's Uncompress form."""
    ref = mixed_codec_ref()
    n, need = ref.n, int(ref.dext[-1])
    for cap, want in ((need - 1, _lib.ERR_NOMEM), (need, _lib.SUCCESS)):
        status, crc, count = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        dext = np.zeros(n + 1, np.uint64)
        plain = np.full(cap + GUARD, PATTERN, np.uint8)
        rc = _lib.lib().tpz_verify_blocks_host(
            ctx.handle, C.c_void_p(ref.src.ctypes.data), C.c_void_p(ref.ext.ctypes.data), n,
            C.c_void_p(status.ctypes.data), C.c_void_p(crc.ctypes.data),
            C.c_void_p(count.ctypes.data), C.c_void_p(plain.ctypes.data), cap,
            C.c_void_p(dext.ctypes.data), 4)
        assert rc == want
        assert (plain[cap:] == PATTERN).all()
        np.testing.assert_array_equal(dext.astype(np.int64), ref.dext)
    e = ref.ext.astype(np.int64)
    for b in range(n):
        st, p = O.decompress_block(ref.src[e[b]:e[b + 1]].tobytes())
        got = plain[int(ref.dext[b]):int(ref.dext[b + 1])].tobytes()
        assert got == (p if st == O.OK else b"\x00"), b          # an Err: the tag-0 stub
    np.testing.assert_array_equal(np.where(status == _lib.BLOCK_OK_SPILLED, _lib.BLOCK_OK, status),
                                  ref.o.status)


# ---- one context, calls of other shapes -------------------------------------------------------
def test_context_reuse(fresh_ctx):
    """Pooled buffers larger than a later call needs, and a codec call's chunk metadata, must not
    show in a later call: one large chunk, then small chunks, a codec batch after a plain one and
    a plain one after it."""
    geo, mixed, spill = geometry_ref(), mixed_codec_ref(), spill_ref()
    needs = [ref.spill_need for ref in (geo, mixed, spill, spill_ref("lz4"))]   # on other contexts
    assert needs[0] == 0 and min(needs[1:]) > 0
    # every call on fresh_ctx is compared with the oracle and follows the previous one directly
    for ref, chunk in ((spill, 0), (geo, 3), (mixed, 7), (geo, 0), (spill_ref("lz4"), 4),
                       (spill, 4), (mixed, 1)):
        assert_host_parity(fresh_ctx, ref.src, ref.ext, chunk, ref=ref)

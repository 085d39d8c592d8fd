"""tests/_open_model.py (the model the device open is tested against) against the golden SSTs'
recorded metas and against table.py's own pieces on malformed images. No GPU."""
import glob
import json
import os

import numpy as np
import pytest

import _open_model as M
from conftest import GOLDEN, read_golden
from topazdb_amd.table import BlockMeta, FileObject, ReferencePanic, SsTable

SSTS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.sst")))


def facade_parse(data: bytes):
    """SsTable.open's steps before the decode (table.py), on the same bytes: ("read_bloom" |
    "open", exception) where one of them raises, else (None, (metas, meta offset, Bloom | None))."""
    f = FileObject("image", data)
    try:
        offset, bloom = SsTable._read_bloom(f)
    except ReferencePanic as e:
        return "read_bloom", e
    try:
        if offset < 4:
            raise ReferencePanic("attempt to subtract with overflow")
        meta_offset = int.from_bytes(f.read(offset - 4, 4), "big")
        if meta_offset > offset - 4:
            raise ReferencePanic("attempt to subtract with overflow")
        metas = BlockMeta.decode_block_meta(f.read(meta_offset, offset - 4 - meta_offset))
        ext = np.array([m.offset for m in metas] + [meta_offset], np.uint64)
        if len(metas) and (np.diff(ext.astype(np.int64)) < 0).any():
            raise ReferencePanic("range start index out of range")
        if not metas:      # init_samllest_biggest_key
            raise ReferencePanic("index out of bounds: the len is 0 but the index is 0")
    except ReferencePanic as e:
        return "open", e
    return None, (metas, meta_offset, bloom)


# the stage that raises and the text, per status class
EXPECTED = {
    M.SHORT: ("read_bloom", ("attempt to subtract with overflow",)),
    M.BLOOM_RANGE: ("read_bloom", ("attempt to subtract with overflow",)),
    M.META_RANGE: ("open", ("attempt to subtract with overflow",)),
    M.META_TRUNCATED: ("open", ("advance out of bounds", "copy_to_bytes out of bounds")),
    M.BAD_EXTENTS: ("open", ("range start index out of range",)),
    M.NO_BLOCKS: ("open", ("index out of bounds: the len is 0 but the index is 0",)),
}


def test_facade_parse_restates_open():
    """facade_parse's inline checks are SsTable.open's own lines (guards the restatement)."""
    import inspect
    src = inspect.getsource(SsTable.open)
    for line in ("if offset < SIZEOF_U32:", "if meta_offset > offset - SIZEOF_U32:",
                 'raise ReferencePanic("range start index out of range")'):
        assert line in src


@pytest.mark.parametrize("name", SSTS)
def test_model_on_golden_ssts(name):
    data = read_golden(name + ".sst")
    j = json.load(open(os.path.join(GOLDEN, name + ".json")))
    r = M.parse(data)
    assert r.status == M.OK
    assert r.info[1] == len(data) - 4 == j["file_len"] - 4
    assert r.info[6] == len(j["blocks"]) == len(r.first_keys)
    assert [k.hex() for k in r.first_keys] == j["first_keys"]
    assert r.ext == j["ext"] and r.info[2] == j["meta_off"]
    assert (r.info[4] != M.NONE) == bool(j["bloom_len"]) and r.info[5] == j["bloom_len"]
    assert r.has_codec == ("snappy" in name or "lz4" in name)
    stage, got = facade_parse(data)
    assert stage is None
    assert [(m.offset, m.first_key) for m in got[0]] == list(zip(r.ext[:-1], r.first_keys))
    assert got[1] == r.info[2]
    assert got[2].filter == data[r.info[4]:r.info[4] + r.info[5]]


@pytest.mark.parametrize("name,image,status", M.boundary_cases(),
                         ids=[c[0] for c in M.boundary_cases()])
def test_model_class_matches_the_facade(name, image, status):
    r = M.parse(image)
    assert r.status == status
    stage, got = facade_parse(image)
    if status == M.OK:
        assert stage is None
        assert [(m.offset, m.first_key) for m in got[0]] == list(zip(r.ext[:-1], r.first_keys))
        assert (got[2] is None) == (r.info[4] == M.NONE)
        if got[2] is not None:
            assert got[2].filter == image[r.info[4]:r.info[4] + r.info[5]]
        return
    assert r.info[2:] == [0] * 6
    want_stage, texts = EXPECTED[status]
    assert stage == want_stage and isinstance(got, ReferencePanic) and str(got) in texts


def test_truncation_texts():
    """A cut header is get_u32 / get_u16's panic, a cut key copy_to_bytes': one class, two texts."""
    cases = {c[0]: c[1] for c in M.boundary_cases()}
    assert str(facade_parse(cases["header_cut_3"])[1]) == "advance out of bounds"
    assert str(facade_parse(cases["key_cut_by_one"])[1]) == "copy_to_bytes out of bounds"


def test_builder_round_trips():
    keys = [bytes([65 + i % 26]) * (i % 41) for i in range(200)]
    lens = [7 + i % 13 for i in range(200)]
    tags = [1] * 200
    tags[77] = 3
    img = M.build_image(M.regular_metas(lens, keys), b"\x01\x02\x03", lens, tags)
    r = M.parse(img)
    assert r.status == M.OK and r.first_keys == keys and r.has_codec
    assert r.ext[-1] == sum(lens) and r.info[5] == 3
    assert not M.parse(M.build_image(M.regular_metas(lens, keys), None, lens)).has_codec

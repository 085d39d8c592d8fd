"""tpz_wal_index (host code, no GPU) against the line-by-line WalIterator of
tests/_membuild_model.py: record starts, how the walk ended, and the reference's panics."""
import ctypes as C
import random

import numpy as np
import pytest

import _membuild_model as M
from topazdb_amd import _lib
from topazdb_amd.memtable import wal_encode, wal_index
from topazdb_amd.table import ReferencePanic


def index(image: bytes):
    """(rc, rec list, info list) of the two-call form, straight through ctypes."""
    buf = (C.c_uint8 * max(len(image), 1)).from_buffer_copy(image or b"\0")
    info = (C.c_uint64 * 4)()
    L = _lib.lib()
    rc0 = L.tpz_wal_index(buf, len(image), None, 0, info)
    counted = list(info)
    rec = np.full(counted[0] + 2, 0xABABABABABABABAB, np.uint64)       # one canary past the end
    rc = L.tpz_wal_index(buf, len(image), C.c_void_p(rec.ctypes.data), counted[0] + 1, info)
    assert rc == rc0 and list(info) == counted, "the count-only call reports the same"
    assert rec[-1] == 0xABABABABABABABAB
    return rc, [int(x) for x in rec[:-1]], [int(x) for x in info]


def check(image: bytes):
    rec, how, bad = M.wal_walk(image)
    rc, grec, info = index(image)
    assert grec == rec
    assert info == [len(rec) - 1, how, rec[-1], bad]
    assert rc == (_lib.ERR_SIZES if how == 2 else _lib.SUCCESS)
    return info


def rand_entries(rng, n, empty_at=()):
    return [(b"" if i in empty_at else bytes(rng.randrange(256) for _ in range(rng.randrange(1, 20))),
             bytes(rng.randrange(256) for _ in range(rng.randrange(0, 60)))) for i in range(n)]


@pytest.mark.parametrize("seed", range(6))
def test_random_batches(seed):
    rng = random.Random(seed)
    ent = rand_entries(rng, rng.randrange(1, 300))
    info = check(wal_encode(ent))
    assert info[0] == len(ent) and info[1] == _lib.WAL_END_IMAGE


def test_every_cut_of_a_six_record_image():
    rng = random.Random(7)
    ent = rand_entries(rng, 6)
    ent[2] = (ent[2][0], b"")                              # a tombstone among them
    img = wal_encode(ent)
    ends = {0}
    for k, v in ent:
        ends.add(max(ends) + 4 + len(k) + len(v))
    for cut in range(len(img) + 1):
        info = check(img[:cut])
        assert (info[1] == _lib.WAL_END_IMAGE) == (cut in ends), cut
        if cut not in ends:
            assert info[1] == _lib.WAL_TRUNCATED and info[3] == max(e for e in ends if e < cut)
            with pytest.raises(ReferencePanic):
                wal_index(img[:cut])


def test_empty_image():
    assert check(b"") == [0, _lib.WAL_END_IMAGE, 0, M.NONE]
    rec, info = wal_index(b"")
    assert list(rec) == [0] and info[0] == 0


def test_empty_key_in_the_middle_ends_the_walk():
    rng = random.Random(9)
    ent = rand_entries(rng, 9, empty_at=(4, 6))
    img = wal_encode(ent)
    info = check(img)
    assert info[0] == 5 and info[1] == _lib.WAL_END_EMPTY_KEY
    assert info[2] == len(wal_encode(ent[:5]))
    # what follows the terminator is never parsed: garbage there changes nothing
    assert check(img[:info[2]] + b"\xff\xff\xff")[:3] == info[:3]
    # the terminator's own value is parsed: cut inside it and next() panics
    assert check(img[:info[2] - 1])[1] == (_lib.WAL_TRUNCATED if ent[4][1] else _lib.WAL_END_EMPTY_KEY)


def test_a_65535_byte_value_and_key():
    ent = [(b"k", b"\x5a" * 65535), (b"\x01" * 65535, b""), (b"z", b"1")]
    img = wal_encode(ent)
    info = check(img)
    assert info[0] == 3 and info[2] == len(img)
    assert check(img[:65000])[1] == _lib.WAL_TRUNCATED


def test_count_only_and_arguments():
    img = wal_encode([(b"a", b"b"), (b"c", b"d")])
    rec, info = wal_index(img, count_only=True)
    assert rec is None and info[0] == 2
    L = _lib.lib()
    buf = (C.c_uint8 * len(img)).from_buffer_copy(img)
    out = (C.c_uint64 * 4)()
    small = np.zeros(2, np.uint64)
    assert L.tpz_wal_index(buf, len(img), C.c_void_p(small.ctypes.data), 2, out) == _lib.ERR_NOMEM
    assert L.tpz_wal_index(buf, len(img), None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.tpz_wal_index(None, len(img), None, 0, out) == _lib.ERR_INVALID_ARG
    assert L.tpz_wal_index(None, 0, None, 0, out) == _lib.SUCCESS

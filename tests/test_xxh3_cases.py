"""What the inputs of tests/test_gpu_xxh3_lengths.py reach (tests/_xxh3_cases.py), checked without
a GPU: every branch of hash64 has a length, the model filter holds every key and rejects every
mutant, so a device hash that is wrong for a key shows as a rejected key, and the library's filter
geometry is the model's at every size the GPU tests use.
"""
import numpy as np
import pytest

import _xxh3_cases as X
from topazdb_amd import _lib
from topazdb_amd.table import Bloom


def test_every_branch_has_a_length():
    assert X.LENGTHS[:2201] == list(range(2201)) and len(X.LENGTHS) == 2209
    assert len(set(X.LENGTHS)) == len(X.LENGTHS) and max(X.LENGTHS) == 0xFFFF
    seen = {}
    for n in X.LENGTHS:
        name, detail = X.branch(n)
        seen.setdefault(name, []).append(detail)
    assert set(seen) == {"0", "1-3", "4-8", "9-16", "17-32", "33-64", "65-96", "97-128", "129-240",
                         "long"}
    # the paths' edges, on both sides
    for n in (0, 1, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 240, 241):
        assert n in X.LENGTHS
    assert X.branch(128)[0] == "97-128" and X.branch(129) == ("129-240", 8)
    assert X.branch(240) == ("129-240", 15) and X.branch(241) == ("long", (0, 3))
    assert set(seen["129-240"]) == set(range(8, 16))             # every round count
    blocks = {nb for nb, _ in seen["long"]}
    assert blocks >= {0, 1, 2, 3, 4, 7, 8, 63}
    assert {ns for _, ns in seen["long"]} == set(range(16))      # every stripe count
    # no stripe after a whole block: the last-stripe read alone follows the scramble
    for nb, lo, hi in ((1, 1025, 1088), (2, 2049, 2112)):
        assert all(X.branch(n) == ("long", (nb, 0)) for n in range(lo, hi + 1))
        assert X.branch(lo - 1) == ("long", (nb - 1, 15)) and X.branch(hi + 1) == ("long", (nb, 1))
    assert X.branch(65535) == ("long", (63, 15)) and X.branch(8193) == ("long", (8, 0))
    assert set(X.SINGLE) <= set(X.LENGTHS)
    assert {X.branch(n)[0] for n in X.TABLE_LENGTHS} == set(seen) - {"0", "4-8"}


def test_keys_and_mutants():
    keys, muts = X.keys(), X.mutants()
    assert [len(k) for k in keys] == X.LENGTHS and sum(X.LENGTHS) < 2_600_000
    assert len(muts) == 13266 and len({m for _, _, m in muts}) == len(muts)
    per_key = {}
    for i, p, m in muts:
        assert len(m) == len(keys[i]) and m != keys[i]
        assert bytes(a ^ b for a, b in zip(m[p:p + 1], keys[i][p:p + 1])) == bytes([X.FLIP])
        assert m[:p] == keys[i][:p] and m[p + 1:] == keys[i][p + 1:]
        per_key.setdefault(i, []).append(p)
    assert set(per_key) == set(range(1, len(keys)))              # every non-empty key
    n = 65535
    assert per_key[X.LENGTHS.index(n)] == [0, 63, 1023, 1024, n // 2, n - 64, n - 1]
    assert per_key[X.LENGTHS.index(1)] == [0] and per_key[X.LENGTHS.index(1025)][-1] == 1024


def test_pack_reaches_every_alignment():
    keys = X.keys()
    for lead in X.LEADS:
        col, pos = X.pack(keys, lead)
        assert pos[0] == lead and len(pos) == len(keys) + 1 and len(col) == int(pos[-1])
        # key starts and key ends (the tail reads) on every residue of the 8-byte loads
        assert {int(p) % 8 for p in pos[:-1]} == set(range(8))
        for i in (0, 1, 17, 240, 1025, len(keys) - 1):
            assert col[int(pos[i]):int(pos[i + 1])].tobytes() == keys[i]
    starts = {int(X.pack(keys, lead)[1][-2]) % 16 for lead in X.LEADS}
    assert starts == set(range(16))                              # the 65,535-byte key's start


def test_vector_probe_is_bloom_may_contain():
    filt = X.model_filter(X.PROBE_FPP)
    hs = np.concatenate([X.key_hashes()[::40], X.mutant_hashes()[::60]])
    b = Bloom(filt)
    assert X.may_contain(filt, hs).tolist() == [b.may_contain(int(h)) for h in hs]


@pytest.mark.parametrize("fpp", [1e-300, X.PROBE_FPP, 1e-9])
def test_model_filter_holds_the_keys_and_no_mutant(fpp):
    """With no mutant accepted, a key whose device hash differs from the true one is, like a
    mutant, rejected: the probe test fails on it."""
    filt = X.model_filter(fpp)
    if fpp == X.PROBE_FPP:
        assert len(filt) == 39702 and filt[-1] == 15
    assert X.may_contain(filt, X.key_hashes()).all()
    accepted = X.may_contain(filt, X.mutant_hashes())
    assert len(accepted) == 13266 and int(accepted.sum()) == 0


def test_host_hash_of_the_table_keys():
    """The get tests' model probes with the library's host hash: it is xxhash's for every key the
    tables hold and every key the SST test writes."""
    _, held = X.table_sets()
    ks = held + [k for k, _ in X.sst_entries()]
    assert [_lib.xxh3_64(k) for k in ks] == X.hashes(ks).tolist()
    assert len(held) == 100 and sorted(len(k) for k in held) == sorted(X.TABLE_LENGTHS * 5)
    assert [len(k) for k, _ in X.sst_entries()] == (X.TABLE_LENGTHS * 3)[:X.SST_ENTRIES]
    assert [k for k, _ in X.sst_entries()] == sorted(k for k, _ in X.sst_entries())


def test_geometry_of_every_case():
    for n, fpp in X.GEOMETRIES:
        assert _lib.bloom_geometry(n, fpp) == Bloom.geometry(n, fpp), (n, fpp)
    assert X.reach(len(X.LENGTHS), X.TINY) == (7, 3, 819, 15)
    S, nwg, per_wg, k = X.reach(len(X.LENGTHS), 0.1)
    assert (S, nwg) == (1, 1) and k < 15 and per_wg == _lib.BLOOM_WG_PROBES // k > 819
    assert X.reach(1, X.TINY) == (1, 1, 819, 15) and Bloom.geometry(1, X.TINY)[0] == 181

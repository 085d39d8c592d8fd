"""The closed-form merge rule the device implements equals the reference's MergeIterator
(tests/_merge_model.py restates both; no GPU, no library)."""
import random

from _merge_model import merge_iterator, merge_rule, merged_entries


def random_runs(rng: random.Random, n_runs: int, max_len: int, alphabet: bytes, max_key: int,
                repeat: float):
    """Sorted runs over a tiny key space (so keys collide across runs); with probability `repeat`
    a key is repeated inside its run."""
    runs = []
    for r in range(n_runs):
        keys = []
        for _ in range(rng.randint(0, max_len)):
            k = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, max_key)))
            keys += [k] * (1 + (rng.random() < repeat) + (rng.random() < repeat / 2))
        keys.sort()
        runs.append([(k, b"%d.%d" % (r, j)) for j, k in enumerate(keys)])
    return runs


def test_rule_equals_iterator_on_random_inputs():
    rng = random.Random(20240607)
    for case in range(4000):
        runs = random_runs(rng, rng.randint(0, 6), rng.randint(0, 7), b"ab\x00\xff",
                           rng.randint(1, 3), rng.choice([0.0, 0.3]))
        assert merge_iterator(runs) == merge_rule(runs), runs


def test_rule_on_hand_cases():
    a, b, c = (b"a", b"A"), (b"b", b"B"), (b"c", b"C")
    # an empty first run does not take index 0 (create filters before enumerate)
    assert merge_rule([[], [a, c], [b]]) == merge_iterator([[], [a, c], [b]]) == [(1, 0), (2, 0), (1, 1)]
    # the lower run wins a key; its own repeats all come out, the loser's all go
    runs = [[(b"k", b"0"), (b"k", b"1")], [(b"j", b"x"), (b"k", b"2"), (b"k", b"3"), (b"l", b"y")]]
    assert merge_iterator(runs) == merge_rule(runs) == [(1, 0), (0, 0), (0, 1), (1, 3)]
    # a repeat inside a losing run, with the winner after it in run order
    runs = [[(b"k", b"")], [(b"k", b"v"), (b"k", b"w")], [(b"k", b"z")]]
    assert merge_iterator(runs) == merge_rule(runs) == [(0, 0)]
    # tombstones (empty values) are entries like any other
    assert merged_entries(runs) == [(b"k", b"")]
    # a proper prefix is smaller; bytes compare unsigned
    runs = [[(b"a\x00", b"1"), (b"\x80", b"2")], [(b"a", b"3"), (b"a\x00", b"4"), (b"\x7f", b"5")]]
    assert merge_iterator(runs) == merge_rule(runs) == [(1, 0), (0, 0), (1, 2), (0, 1)]
    assert merge_rule([]) == merge_iterator([]) == []

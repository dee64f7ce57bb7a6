"""tests/string_order_oracle.py against hyrise_amd.string_keys.StringRanks (the host path the device order replaces), a hand-written
example, and the property that makes the stand-in a well-formed DictionarySegment<int32>: a chunk's ranks ascend strictly."""
import numpy as np

from hyrise_amd.string_keys import StringRanks
import string_order_oracle as oracle


def random_dictionaries(rng, counts, alphabet=b"ab\x00\xff", longest=6):
    out = []
    for n in counts:
        entries = set()
        while len(entries) < n:
            entries.add(bytes(rng.choice(list(alphabet), rng.integers(0, longest + 1)).tolist()))
        out.append(sorted(entries))
    return out


def test_hand_written_three_chunks():
    dictionaries = [[b"", b"ab", b"b"], [], [b"a", b"ab", b"ab\x00", b"\x80"], [b"b"]]
    # distinct, in order: "" a ab ab\0 b \x80
    ranks, n_distinct = oracle.column_order(dictionaries)
    assert ranks == [[0, 2, 4], [], [1, 2, 3, 5], [4]] and n_distinct == 6
    assert oracle.column_order([]) == ([], 0) and oracle.column_order([[], []]) == ([[], []], 0)


def test_agrees_with_string_ranks():
    rng = np.random.default_rng(21)
    for counts in ((5,), (0, 7, 0), (63, 64, 65), (257, 1, 0, 100, 100)):
        dictionaries = random_dictionaries(rng, counts)
        host = StringRanks([entry for dictionary in dictionaries for entry in dictionary])
        ranks, n_distinct = oracle.column_order(dictionaries)
        assert n_distinct == len(host.sorted)
        for dictionary, chunk_ranks in zip(dictionaries, ranks):
            assert chunk_ranks == [host.rank(entry) for entry in dictionary]


def test_ranks_ascend_strictly_inside_a_chunk_and_are_dense():
    rng = np.random.default_rng(22)
    dictionaries = random_dictionaries(rng, (100, 0, 257, 64, 3))
    ranks, n_distinct = oracle.column_order(dictionaries)
    for chunk_ranks in ranks:
        assert all(a < b for a, b in zip(chunk_ranks, chunk_ranks[1:]))
    assert sorted({r for chunk_ranks in ranks for r in chunk_ranks}) == list(range(n_distinct))

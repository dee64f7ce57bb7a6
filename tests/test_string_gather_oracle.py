"""tests/string_gather_oracle.py against hand-written cases, and its rank path against tests/string_order_oracle.py's ranks."""
import string_gather_oracle as oracle
import string_order_oracle

NULL = (0xFFFFFFFF, 0xFFFFFFFF)


def test_hand_written_gathers():
    chunks = [[b"b", b"a", None], [b"a", b"", b"c"]]
    # one chunk: equal strings of two source chunks are one entry, the empty string sorts first, NULL holds the entry count
    assert oracle.column_gather(chunks, [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), NULL], 10) == ([[b"", b"a", b"b"]], [[2, 1, 1, 0, 3, 3]])
    # chunks of two rows, the last one shorter; a chunk of NULLs only has no entries
    assert oracle.column_gather(chunks, [(1, 2), (0, 0), NULL, (0, 2), (1, 2)], 2) == ([[b"b", b"c"], [], [b"c"]], [[1, 0], [0, 0], [0]])
    assert oracle.column_gather(chunks, [], 3) == ([], [])
    assert oracle.column_gather(chunks, [None], 1) == ([[]], [[0]])


def test_order_is_that_of_unsigned_bytes_with_prefixes_first():
    chunks = [[b"a\x00b", b"a", b"\xff", b"a\x00", b"ab", b"\x80"]]
    dictionaries, value_ids = oracle.column_gather(chunks, [(0, i) for i in range(6)], 6)
    assert dictionaries == [[b"a", b"a\x00", b"a\x00b", b"ab", b"\x80", b"\xff"]] and value_ids == [[2, 0, 5, 1, 3, 4]]


def test_uniform_sizes():
    assert oracle.uniform_sizes(0, 3) == [] and oracle.uniform_sizes(7, 3) == [3, 3, 1] and oracle.uniform_sizes(6, 3) == [3, 3]
    assert oracle.uniform_sizes(70_000, 65_535) == [65_535, 4_465]


def test_ranks_fed_back_give_the_strings():
    dictionaries = [[b"a", b"c"], [], [b"", b"b", b"c"]]
    ranks, n_distinct = string_order_oracle.column_order(dictionaries)
    assert n_distinct == 4
    got_dictionaries, got_ids = oracle.ranks_gather(dictionaries, ranks)
    assert got_dictionaries == dictionaries and got_ids == [[0, 1], [], [0, 1, 2]]
    # NULL ranks and ranks outside 0 .. n_distinct - 1 are NULL rows
    assert oracle.ranks_gather(dictionaries, [[3, None, -1, 4, 0]]) == ([[b"", b"c"]], [[1, 2, 2, 2, 0]])

"""tests/string_substr_oracle.py pinned: the reference's known answers, its branch structure transcribed literally, the identity window."""
import string_substr_oracle as oracle


def reference_substr(string, start, length):
    """_evaluate_substring's loop body (expression_evaluator.cpp:1597-1638), statement for statement; Python's integers do not overflow."""
    result = b""
    signed_string_size = len(string)
    if length <= 0:
        return result
    end = 0
    if start < 0:
        start += signed_string_size
    else:
        if start == 0:
            length -= 1
        else:
            start -= 1
    end = start + length
    start = max(0, start)
    end = min(end, signed_string_size)
    length = end - start
    if len(string) != 0 and start >= 0 and start < signed_string_size and length > 0:
        length = min(signed_string_size - start, length)
        result = string[start:start + length]
    return result


def test_known_answers():
    assert oracle.substr(b"HELLO", 0, 2) == b"H"
    assert oracle.substr(b"HELLO", -1, 2) == b"O"
    assert oracle.substr(b"HELLO", -8, 1) == b""
    assert oracle.substr(b"HELLO", -8, 5) == b"HE"


def test_sweep_against_the_reference_branches():
    for value in (b"", b"a", b"HELLO"):
        for start in range(-9, 10):
            for length in range(-1, 10):
                assert oracle.substr(value, start, length) == reference_substr(value, start, length), (value, start, length)


def test_identity():
    for value in (b"", b"a", b"HELLO", b"a\x00b", bytes(range(256))):
        assert oracle.substr(value, 1, 2**31 - 1) == value


def test_output_pair():
    chunks = [[b"1995-01-02", None, b"1996-01-02", b"1995-03-04"], [None, None], [b"x", b""]]
    dictionaries, value_ids = oracle.column_substr(chunks, 1, 4)
    assert dictionaries == [[b"1995", b"1996"], [], [b"", b"x"]]
    assert value_ids == [[0, 2, 1, 0], [0, 0], [1, 0]]
    dictionaries, value_ids = oracle.column_substr(chunks, 6, 2)
    assert dictionaries == [[b"01", b"03"], [], [b""]]
    assert value_ids == [[0, 2, 0, 1], [0, 0], [0, 0]]

"""tests/string_join_keys_oracle.py against what it restates: ids equal exactly when the strings are, low bits std::hash's, and the oracle's
hash join over these ids finds the pairs, in the order, that it finds over join_keys.StringJoinKeys' ids -- the number above bit 20 only
has to be unique."""
import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.join_keys import HASH_BITS, StringJoinKeys, std_hash_bytes
from hyrise_amd.storage import HostColumn, HostSegment
from hyrise_amd.string_keys import encode_string_column
from support import oracle_join
import string_join_keys_oracle as oracle


def words_table(seed, rows, n_words, chunk, null_fraction=0.08):
    rng = np.random.default_rng(seed)
    words = [b""] + [b"w%d" % i + b"x" * (i % 9) for i in range(n_words - 1)]
    strings = [words[i] for i in rng.integers(0, n_words, rows)]
    nulls = rng.random(rows) < null_fraction
    segments, dictionaries = encode_string_column(strings, nulls, chunk)
    return strings, nulls, segments, dictionaries


def key_column(segments, keys, data_type=abi.TYPE_LONG):
    """The segments' attribute vectors over per-chunk keys in place of the strings."""
    dtype = np.int64 if data_type == abi.TYPE_LONG else np.int32
    out = [HostSegment(abi.ENC_DICTIONARY, data_type, s.size, s.width, s.data, aux=np.array(k, dtype=dtype), aux_size=len(k)) for s, k in zip(segments, keys)]
    return HostColumn(out, data_type)


def test_ids_are_equal_exactly_when_the_strings_are():
    left = [[b"", b"a", b"ab", b"abc"], [], [b"a", b"b\x00", b"zz"]]
    right = [[b"ab", b"b", b"b\x00"], [b"", b"zz", b"zzz"]]
    left_ranks, right_ranks, n_distinct = oracle.joint_order(left, right)
    assert n_distinct == 8 and left_ranks == [[0, 1, 2, 3], [], [1, 5, 6]] and right_ranks == [[2, 4, 5], [0, 6, 7]]
    left_ids, right_ids = oracle.join_ids(left, right)
    flat = [(e, i) for d, ids in zip(left + right, left_ids + right_ids) for e, i in zip(d, ids)]
    for e, i in flat:
        for f, j in flat:
            assert (e == f) == (i == j)
        assert i & ((1 << HASH_BITS) - 1) == std_hash_bytes(e) & 0xFFFFF and i >> HASH_BITS >= 1


@pytest.mark.parametrize("mode", [abi.JOIN_INNER, abi.JOIN_LEFT])
@pytest.mark.parametrize("radix_bits", [0, 8])
def test_the_oracle_join_over_rank_ids_is_the_join_over_registry_ids(mode, radix_bits):
    _, _, left_segments, left_dicts = words_table(1, 400, 90, 128)
    _, _, right_segments, right_dicts = words_table(2, 600, 120, 150)
    registry = StringJoinKeys()
    want = oracle_join(registry.column(left_segments, left_dicts), registry.column(right_segments, right_dicts), mode, radix_bits)
    left_ids, right_ids = oracle.join_ids(left_dicts, right_dicts)
    got = oracle_join(key_column(left_segments, left_ids), key_column(right_segments, right_ids), mode, radix_bits)
    n = want.n_pairs
    assert n > 400 and got.n_pairs == n and got.c.n_slices == want.c.n_slices and got.c.left_is_build == want.c.left_is_build
    assert got.left[:n].tobytes() == want.left[:n].tobytes() and got.right[:n].tobytes() == want.right[:n].tobytes()
    assert np.array_equal(got.slice_offsets[:want.c.n_slices + 1], want.slice_offsets[:want.c.n_slices + 1])

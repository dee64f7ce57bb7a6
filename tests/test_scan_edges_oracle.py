"""The CPU oracle's ColumnVsValue scans (oracle/scan.c) against the plain truth of tests/scan_edge_truth.py, at the limits of every column
type: every limit value as the literal of the six comparisons, about thirty BETWEEN pairs per type in the four forms, IS [NOT] NULL and (float
types) NaN literals, over the limit columns in the layouts the oracle reads (Unencoded, Dictionary, FrameOfReference), nullable and not.

A disagreement means that one of the two misreads the reference (column_vs_value_table_scan_impl.cpp, column_between_table_scan_impl.cpp,
sorted_segment_search.hpp, the comparator lambdas of type_comparison.hpp).  Two were found this way and decided for the truth:
  - integer BETWEEN: the reference computes `right - left` and `upper_bound - lower_bound` in the column's SIGNED type
    (column_between_table_scan_impl.cpp:87, type_comparison.hpp:121-131), which overflows -- undefined behaviour -- once the bounds lie more
    than the type's maximum apart; the oracle had restated that with wrap-around, so BETWEEN MIN AND MAX matched nothing and BETWEEN MAX AND
    MIN matched both ends.  What the code means is `lower <= x <= upper`; the oracle now forms both differences in a wider type.
  - a NaN literal on a dictionary segment: std::lower_bound / upper_bound with a NaN are not a search in an ordered range (every comparison is
    false), and `<= NaN` / `>= NaN` / BETWEEN came out as "all rows"; the generic path of the same scan compares row by row and matches
    nothing.  Both follow IEEE now: nothing matches except <>, on every layout.
"""
import numpy as np
import pytest

import scan_edge_truth as T
from hyrise_amd import abi, storage
from hyrise_amd.operators import make_predicate
from support import oracle_scan

CONDITION_OF = {"=": abi.PRED_EQUALS, "<>": abi.PRED_NOT_EQUALS, "<": abi.PRED_LESS_THAN, "<=": abi.PRED_LESS_THAN_EQUALS, ">": abi.PRED_GREATER_THAN,
                ">=": abi.PRED_GREATER_THAN_EQUALS, "between_inclusive": abi.PRED_BETWEEN_INCLUSIVE, "between_lower_exclusive": abi.PRED_BETWEEN_LOWER_EXCLUSIVE,
                "between_upper_exclusive": abi.PRED_BETWEEN_UPPER_EXCLUSIVE, "between_exclusive": abi.PRED_BETWEEN_EXCLUSIVE, "is_null": abi.PRED_IS_NULL,
                "is_not_null": abi.PRED_IS_NOT_NULL}
ENCODING_OF = {"Unencoded": abi.ENC_UNENCODED, "Dictionary": abi.ENC_DICTIONARY, "FrameOfReference": abi.ENC_FRAME_OF_REFERENCE}
CASES = [(name, layout) for name in T.TYPES for layout in ENCODING_OF if layout != "FrameOfReference" or name == "int32"]


def predicate_of(name, condition, literal, literal2, nullable):
    return make_predicate(CONDITION_OF[condition], storage.TYPE_OF_NP[np.dtype(T.TYPES[name])], literal, literal2, nullable=nullable)


def column_of(chunks, encoding):
    """The truth's chunks [(values, nulls or None)] as a HostColumn of one encoding."""
    return storage.HostColumn([storage.encode_segment(values, nulls, encoding) for values, nulls in chunks], storage.TYPE_OF_NP[np.dtype(chunks[0][0].dtype)])


def all_rows(result):
    """Every matching RowID of a scan result as uint32 [n, 2]; a chunk in state "all" whose RowIDs were left out stands for all of its rows."""
    parts = []
    for c in range(result.n_chunks):
        if result.chunk_state[c] == abi.CHUNK_ALL_MATCH and result.offsets[c + 1] == result.offsets[c]:
            parts.append(np.stack([np.full(int(result.counts[c]), c, dtype=np.uint32), np.arange(int(result.counts[c]), dtype=np.uint32)], axis=1))
        else:
            parts.append(result.pos_list(c))
    return np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.uint32)


def assert_truth(result, chunks, host, condition, literal, literal2, context):
    """PosList, per-chunk counts, and the chunk states the truth implies.  "All" needs every row to match and a column that can hold no NULL,
    "none" needs no match; the reference decides a chunk before reading its rows only on dictionary segments (column_vs_value_table_scan_impl.cpp:
    124-160, column_between_table_scan_impl.cpp:131-170) -- there the state must be exactly that; elsewhere it must not contradict the truth."""
    pairs, counts = T.truth(chunks, condition, literal, literal2)
    assert [int(c) for c in result.counts[:len(counts)]] == counts, f"counts {context}"
    assert all_rows(result).tobytes() == pairs.tobytes(), f"PosList {context}"
    for c, ((values, nulls), count) in enumerate(zip(chunks, counts)):
        state = int(result.chunk_state[c])
        if state == abi.CHUNK_ALL_MATCH:
            assert count == len(values), f"state all {context} chunk {c}"
        if state == abi.CHUNK_NONE_MATCH:
            assert count == 0, f"state none {context} chunk {c}"
        if condition not in T.NULL_TESTS and host.segments[c].encoding == abi.ENC_DICTIONARY:
            if count == len(values) and nulls is None:
                assert state == abi.CHUNK_ALL_MATCH, f"state {state}, not all: {context} chunk {c}"
            if count == 0:
                assert state == abi.CHUNK_NONE_MATCH, f"state {state}, not none: {context} chunk {c}"


@pytest.mark.parametrize("name,layout", CASES, ids=[f"{n}-{l}" for n, l in CASES])
@pytest.mark.parametrize("nullable", [True, False], ids=["nullable", "not_null"])
def test_oracle_matches_truth(name, layout, nullable):
    values, nulls = T.limit_column(name, pool=3_000 if layout == "Dictionary" else None)
    nulls = nulls if nullable else None
    chunks = T.split(values, nulls)
    host = column_of(chunks, ENCODING_OF[layout])
    for condition, literal, literal2 in T.predicates(name, with_nan=T.is_float(name)):
        for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH):
            got = oracle_scan(host, predicate_of(name, condition, literal, literal2, nullable), flags=flags)
            assert_truth(got, chunks, host, condition, literal, literal2, f"{name} {layout} {condition} {literal!r} {literal2!r} flags {flags}")


@pytest.mark.parametrize("name", [n for n in T.TYPES if T.is_float(n)])
def test_oracle_matches_truth_nan_rows(name):
    """NaN rows (the default pattern, one with the sign bit, one with a payload) in the one layout the oracle reads that can hold them."""
    values, nulls = T.limit_column(name, nan=True)
    assert np.isnan(values).sum() > 300 and np.signbit(values[np.isnan(values)]).any()
    chunks = T.split(values, nulls)
    host = column_of(chunks, abi.ENC_UNENCODED)
    for condition, literal, literal2 in T.predicates(name, with_nan=True):
        got = oracle_scan(host, predicate_of(name, condition, literal, literal2, True))
        assert_truth(got, chunks, host, condition, literal, literal2, f"{name} NaN rows {condition} {literal!r} {literal2!r}")


def test_truth_rules():
    """The truth module against hand-written answers: its rules, stated once more on six rows."""
    values = np.array([-np.inf, -0.0, 0.0, np.nan, 1.0, 7.0], dtype=np.float32)
    nulls = np.array([False, False, False, False, False, True])
    chunk = [(values, nulls)]
    offsets = lambda *a: T.truth(chunk, *a)[0][:, 1].tolist()   # noqa: E731
    assert offsets("=", 0.0) == [1, 2] and offsets("=", -0.0) == [1, 2]
    assert offsets("<>", np.nan) == [0, 1, 2, 3, 4] and offsets("=", np.nan) == [] and offsets("<=", np.nan) == [] and offsets(">=", np.nan) == []
    assert offsets("<>", 1.0) == [0, 1, 2, 3] and offsets("<", 0.0) == [0] and offsets(">=", -np.inf) == [0, 1, 2, 4]
    assert offsets("between_inclusive", -0.0, 1.0) == [1, 2, 4] and offsets("between_exclusive", -0.0, 1.0) == []
    assert offsets("between_lower_exclusive", -np.inf, 0.0) == [1, 2] and offsets("between_inclusive", 1.0, 0.0) == []
    assert offsets("between_inclusive", np.nan, 1.0) == [] and offsets("is_null") == [5] and offsets("is_not_null") == [0, 1, 2, 3, 4]
    ints = [(np.array([np.iinfo(np.int32).min, -1, 0, np.iinfo(np.int32).max], dtype=np.int32), None)]
    assert T.truth(ints, "between_inclusive", np.iinfo(np.int32).min, np.iinfo(np.int32).max)[1] == [4]
    assert T.truth(ints, "between_exclusive", np.iinfo(np.int32).min, np.iinfo(np.int32).max)[1] == [2]
    assert T.truth(ints, "between_inclusive", np.iinfo(np.int32).max, np.iinfo(np.int32).min)[1] == [0]
    assert T.truth(ints, "<", np.iinfo(np.int32).min)[1] == [0] and T.truth(ints, "<=", np.iinfo(np.int32).max)[1] == [4]
    for name in T.TYPES:
        assert len(T.between_pairs(name)) >= 30 and len(set(T.limits(name).tolist())) == len(T.limits(name)) - (1 if T.is_float(name) else 0)   # (-0.0 == 0.0)

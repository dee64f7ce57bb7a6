"""hy_join_nested_loop's output restated with numpy: the reference's walk (join_nested_loop.cpp:141-236) chunk pair by chunk pair.  Per
(outer chunk, inner chunk) block np.nonzero of the boolean match matrix already is the (i, j) order of the two inner loops; the blocks are
cut out of one matrix by a stable sort.

Operands are compared in their common C++ type -- double if either is double, else float if either is float, else int64 -- which is what the
reference's generic comparator lambdas do.  numpy's own promotion is NOT that rule (int32 or int64 against float32 becomes float64 there), so
both sides are cast explicitly before they are compared."""
import numpy as np

from hyrise_amd import abi
from join_sort_merge_oracle import compare, row_ids  # noqa: F401  (row_ids: re-exported for the tests)

MODES = (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_RIGHT, abi.JOIN_FULL_OUTER, abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_FALSE, abi.JOIN_ANTI_NULL_AS_TRUE)
SEMI_ANTI = (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_FALSE, abi.JOIN_ANTI_NULL_AS_TRUE)
CONDITIONS = (abi.PRED_EQUALS, abi.PRED_NOT_EQUALS, abi.PRED_LESS_THAN, abi.PRED_LESS_THAN_EQUALS, abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS)
FLIPPED = {abi.PRED_LESS_THAN: abi.PRED_GREATER_THAN, abi.PRED_LESS_THAN_EQUALS: abi.PRED_GREATER_THAN_EQUALS, abi.PRED_GREATER_THAN: abi.PRED_LESS_THAN,
           abi.PRED_GREATER_THAN_EQUALS: abi.PRED_LESS_THAN_EQUALS, abi.PRED_EQUALS: abi.PRED_EQUALS, abi.PRED_NOT_EQUALS: abi.PRED_NOT_EQUALS}


def common_type(a, b):
    """The usual arithmetic conversions over int32 / int64 / float / double."""
    a, b = np.dtype(a), np.dtype(b)
    if np.float64 in (a, b):
        return np.float64
    if np.float32 in (a, b):
        return np.float32
    return np.int64


def _column(values, nulls):
    values = np.asarray(values)
    return values, np.zeros(len(values), dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)


def match_block(outer, inner, predicates, null_matches, o_range, i_range):
    """outer / inner: lists of (values, is_null); predicates: [(outer column, condition, inner column)] -> bool [o rows, i rows]."""
    (o_begin, o_end), (i_begin, i_end) = o_range, i_range
    match = np.ones((o_end - o_begin, i_end - i_begin), dtype=bool)
    for o_column, condition, i_column in predicates:
        (x, x_null), (y, y_null) = outer[o_column], inner[i_column]
        kind = common_type(x.dtype, y.dtype)
        compared = compare(condition, x[o_begin:o_end].astype(kind)[:, None], y[i_begin:i_end].astype(kind)[None, :])
        is_null = x_null[o_begin:o_end, None] | y_null[None, i_begin:i_end]
        match &= np.where(is_null, null_matches, compared)   # a NULL fails the predicate; under AntiNullAsTrue it satisfies it
    return match


def nested_loop_join(left_columns, right_columns, left_sizes, right_sizes, mode, predicates):
    """left_columns / right_columns: [(values, nulls or None), ...] of the two input tables, *_sizes their chunk sizes;
    predicates: [(left column index, condition, right column index), ...], the first one the primary.
    -> (left rows, right rows): flat row numbers in the reference's order, -1 = NULL_ROW_ID; Semi / Anti: right rows is None."""
    left = [_column(*c) for c in left_columns]
    right = [_column(*c) for c in right_columns]
    outer, inner, o_sizes, i_sizes = left, right, left_sizes, right_sizes
    walk = [(l, c, r) for l, c, r in predicates]
    if mode == abi.JOIN_RIGHT:   # join_nested_loop.cpp:130-139: the tables swapped, every predicate flipped
        outer, inner, o_sizes, i_sizes = right, left, right_sizes, left_sizes
        walk = [(r, FLIPPED[c], l) for l, c, r in predicates]
    o_base = np.concatenate([[0], np.cumsum(np.asarray(o_sizes, dtype=np.int64))]).astype(np.int64)
    i_base = np.concatenate([[0], np.cumsum(np.asarray(i_sizes, dtype=np.int64))]).astype(np.int64)
    null_matches = mode == abi.JOIN_ANTI_NULL_AS_TRUE
    outer_mode = mode in (abi.JOIN_LEFT, abi.JOIN_RIGHT, abi.JOIN_FULL_OUTER)
    # np.nonzero of the match matrix lists the matches by (i, j).  A STABLE sort of them by (chunk of i, chunk of j) is the walk's order: inside
    # one (co, ci) block it leaves what np.nonzero of that block alone gives.  (The matrix is built in bands of outer rows to bound its size.)
    n_o, n_i, n_ci = int(o_base[-1]), int(i_base[-1]), len(i_sizes)
    o_matched = np.zeros(n_o, dtype=bool)
    i_matched = np.zeros(n_i, dtype=bool)
    o_parts, i_parts = [], []
    band = max(1, (1 << 25) // max(1, n_i))
    for begin in range(0, n_o, band):
        end = min(n_o, begin + band)
        i, j = np.nonzero(match_block(outer, inner, walk, null_matches, (begin, end), (0, n_i)))
        o_matched[begin + i] = True
        i_matched[j] = True
        if mode not in SEMI_ANTI:
            o_parts.append(begin + i)
            i_parts.append(j)
    o_rows = np.concatenate(o_parts).astype(np.int64) if o_parts else np.zeros(0, dtype=np.int64)
    i_rows = np.concatenate(i_parts).astype(np.int64) if i_parts else np.zeros(0, dtype=np.int64)
    chunk_of_o = np.searchsorted(o_base, o_rows, side="right") - 1
    chunk_of_i = np.searchsorted(i_base, i_rows, side="right") - 1
    place = chunk_of_o * (n_ci + 1) + chunk_of_i
    if outer_mode:   # :191-199: behind all pairs of co its rows that matched nothing -- one more slot behind co's inner chunks
        unmatched = np.flatnonzero(~o_matched)
        o_rows = np.concatenate([o_rows, unmatched])
        i_rows = np.concatenate([i_rows, np.full(len(unmatched), -1, dtype=np.int64)])
        place = np.concatenate([place, (np.searchsorted(o_base, unmatched, side="right") - 1) * (n_ci + 1) + n_ci])
    order = np.argsort(place, kind="stable")
    o_rows, i_rows = o_rows[order], i_rows[order]
    if mode == abi.JOIN_FULL_OUTER:   # :206-219
        unmatched = np.flatnonzero(~i_matched)
        o_rows = np.concatenate([o_rows, np.full(len(unmatched), -1, dtype=np.int64)])
        i_rows = np.concatenate([i_rows, unmatched])
    if mode in SEMI_ANTI:   # :223-236
        return np.flatnonzero(o_matched != (mode != abi.JOIN_SEMI)).astype(np.int64), None
    return (i_rows, o_rows) if mode == abi.JOIN_RIGHT else (o_rows, i_rows)

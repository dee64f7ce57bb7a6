"""hy_join_sort_merge's output restated with numpy.  ordered_join is the order contract of include/hyrise_amd.h (stable argsort plus
searchsorted); nested_loop_pairs is an independent nested loop that yields the multiset of pairs -- the reference's JoinVerification
contract (join_test_runner.cpp), whose tests compare unordered."""
import numpy as np

from hyrise_amd import abi
from sort_oracle import positions_of

OUTER_LEFT = (abi.JOIN_LEFT, abi.JOIN_FULL_OUTER)
OUTER_RIGHT = (abi.JOIN_RIGHT, abi.JOIN_FULL_OUTER)
MODES = (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_RIGHT, abi.JOIN_FULL_OUTER)
CONDITIONS = (abi.PRED_EQUALS, abi.PRED_NOT_EQUALS, abi.PRED_LESS_THAN, abi.PRED_LESS_THAN_EQUALS, abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS)
ACCEPTED = [(mode, condition) for condition in CONDITIONS for mode in MODES if condition != abi.PRED_NOT_EQUALS or mode == abi.JOIN_INNER]


def compare(condition, left, right):
    return {abi.PRED_EQUALS: np.equal, abi.PRED_NOT_EQUALS: np.not_equal, abi.PRED_LESS_THAN: np.less, abi.PRED_LESS_THAN_EQUALS: np.less_equal,
            abi.PRED_GREATER_THAN: np.greater, abi.PRED_GREATER_THAN_EQUALS: np.greater_equal}[condition](left, right)


def _sorted_side(values, nulls):
    values = np.asarray(values)
    is_null = np.zeros(len(values), dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)
    present = np.flatnonzero(~is_null)
    keys = values[present]
    if keys.dtype.kind == "f":
        keys = keys + keys.dtype.type(0)   # -0.0 -> +0.0: one key
    order = np.argsort(keys, kind="stable")
    return present[order], keys[order], is_null


def ordered_join(left_values, left_nulls, right_values, right_nulls, mode, condition):
    """-> (left rows, right rows, n_matched, n_left_outer): flat row numbers (chunk order, then offset) in the contract's order, -1 = NULL."""
    left_rows, left_keys, left_is_null = _sorted_side(left_values, left_nulls)
    right_rows, right_keys, right_is_null = _sorted_side(right_values, right_nulls)
    m_right = len(right_keys)
    lower = np.searchsorted(right_keys, left_keys, side="left").astype(np.int64)
    upper = np.searchsorted(right_keys, left_keys, side="right").astype(np.int64)
    if condition == abi.PRED_EQUALS:
        first, count = lower, upper - lower
    elif condition == abi.PRED_LESS_THAN:
        first, count = upper, m_right - upper
    elif condition == abi.PRED_LESS_THAN_EQUALS:
        first, count = lower, m_right - lower
    elif condition == abi.PRED_GREATER_THAN:
        first, count = np.zeros_like(lower), lower
    elif condition == abi.PRED_GREATER_THAN_EQUALS:
        first, count = np.zeros_like(upper), upper
    else:
        first, count = np.zeros_like(lower), lower + (m_right - upper)   # below the key, then above it
    offsets = np.cumsum(count) - count
    n_matched = int(count.sum())
    j = np.arange(n_matched, dtype=np.int64) - np.repeat(offsets, count)
    at = np.repeat(first, count) + j
    if condition == abi.PRED_NOT_EQUALS:
        below = np.repeat(lower, count)
        at = np.where(j < below, j, j - below + np.repeat(upper, count))
    out_left = [np.repeat(left_rows, count)]
    out_right = [right_rows[at] if n_matched else np.zeros(0, dtype=np.int64)]
    n_left_outer = 0
    if mode in OUTER_LEFT:
        matched = np.zeros(len(left_is_null), dtype=bool)
        matched[left_rows[count > 0]] = True
        unmatched = np.flatnonzero(~matched)
        n_left_outer = len(unmatched)
        out_left.append(unmatched)
        out_right.append(np.full(n_left_outer, -1, dtype=np.int64))
    if mode in OUTER_RIGHT:
        # how many left keys satisfy the condition for every right key, from the sorted left keys
        below = np.searchsorted(left_keys, right_keys, side="left")
        up_to = np.searchsorted(left_keys, right_keys, side="right")
        partners = {abi.PRED_EQUALS: up_to - below, abi.PRED_LESS_THAN: below, abi.PRED_LESS_THAN_EQUALS: up_to,
                    abi.PRED_GREATER_THAN: len(left_keys) - up_to, abi.PRED_GREATER_THAN_EQUALS: len(left_keys) - below}[condition]
        matched = np.zeros(len(right_is_null), dtype=bool)
        matched[right_rows[partners > 0]] = True
        unmatched = np.flatnonzero(~matched)
        out_left.append(np.full(len(unmatched), -1, dtype=np.int64))
        out_right.append(unmatched)
    return np.concatenate(out_left).astype(np.int64), np.concatenate(out_right).astype(np.int64), n_matched, n_left_outer


def nested_loop_pairs(left_values, left_nulls, right_values, right_nulls, mode, condition):
    """The multiset of output pairs as a sorted list of (left row, right row), -1 = NULL: one loop over the left rows."""
    left_values, right_values = np.asarray(left_values), np.asarray(right_values)
    left_is_null = np.zeros(len(left_values), dtype=bool) if left_nulls is None else np.asarray(left_nulls, dtype=bool)
    right_is_null = np.zeros(len(right_values), dtype=bool) if right_nulls is None else np.asarray(right_nulls, dtype=bool)
    pairs = []
    right_matched = np.zeros(len(right_values), dtype=bool)
    for i in range(len(left_values)):
        hits = np.zeros(0, dtype=np.int64)
        if not left_is_null[i]:
            hits = np.flatnonzero(compare(condition, left_values[i], right_values) & ~right_is_null)
        right_matched[hits] = True
        pairs.extend((i, int(h)) for h in hits)
        if not len(hits) and mode in OUTER_LEFT:
            pairs.append((i, -1))
    if mode in OUTER_RIGHT:
        pairs.extend((-1, int(h)) for h in np.flatnonzero(~right_matched))
    return sorted(pairs)


def row_ids(rows, chunk_sizes):
    """Flat row numbers (-1 = NULL) -> RowIDs {chunk, offset} of a table with the given chunk sizes, NULL_ROW_ID = {~0, ~0}."""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.full((len(rows), 2), 0xFFFFFFFF, dtype=np.uint32)
    present = rows >= 0
    if present.any():
        out[present] = positions_of(rows[present], chunk_sizes)
    return out

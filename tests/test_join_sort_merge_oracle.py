"""tests/join_sort_merge_oracle.py against itself: on the reference's JoinTestRunner input tables the ordered restatement yields the nested
loop's multiset of pairs (the reference's JoinVerification contract) and every property of hy_join_sort_merge's order contract holds."""
import itertools

import numpy as np
import pytest

from hyrise_amd import abi
from join_sort_merge_oracle import ACCEPTED, OUTER_LEFT, OUTER_RIGHT, compare, nested_loop_pairs, ordered_join
from support import load_tbl

SIZES = (0, 10, 15)
TABLES = {(side, size): f"join_test_runner/input_table_{side}_{size}.tbl" for side in ("left", "right") for size in SIZES}


def numeric_column_pairs(left, right):
    for a, b in itertools.product(range(len(left.types)), range(len(right.types))):
        if left.types[a] == right.types[b] and left.types[a] != abi.TYPE_STRING:
            yield a, b


def key_of(values):
    return values + values.dtype.type(0) if values.dtype.kind == "f" else values


def check_order_contract(lv, ln, rv, rn, mode, condition, out):
    left, right, n_matched, n_left_outer = out
    ml, mr = left[:n_matched], right[:n_matched]
    assert (ml >= 0).all() and (mr >= 0).all()
    lk, rk = key_of(lv)[ml], key_of(rv)[mr]
    assert compare(condition, lk, rk).all()
    if ln is not None:
        assert not ln[ml].any()
    if rn is not None:
        assert not rn[mr].any()
    # 1. left rows ascending by key, ties by left position
    assert (lk[1:] >= lk[:-1]).all()
    assert (ml[1:][lk[1:] == lk[:-1]] >= ml[:-1][lk[1:] == lk[:-1]]).all()
    # 2. under one left row: ascending right key, ties by right position (3.: for <> that puts the keys below the left key before those above)
    same = ml[1:] == ml[:-1]
    assert (rk[1:][same] >= rk[:-1][same]).all()
    tie = same & (rk[1:] == rk[:-1])
    assert (mr[1:][tie] > mr[:-1][tie]).all()
    if condition == abi.PRED_NOT_EQUALS:
        above_then_below = same & (rk[:-1] > lk[:-1]) & (rk[1:] < lk[1:])
        assert not above_then_below.any()
    # a left row's pairs are consecutive
    starts = np.flatnonzero(np.concatenate([[True], ~same])) if n_matched else np.zeros(0, dtype=int)
    assert len(set(ml[starts].tolist())) == len(starts)
    # 4. / 5. the outer rows by position, NULL on the other side
    lo_l, lo_r = left[n_matched:n_matched + n_left_outer], right[n_matched:n_matched + n_left_outer]
    ro_l, ro_r = left[n_matched + n_left_outer:], right[n_matched + n_left_outer:]
    assert (lo_r == -1).all() and (lo_l >= 0).all() and (np.diff(lo_l) > 0).all()
    assert (ro_l == -1).all() and (ro_r >= 0).all() and (np.diff(ro_r) > 0).all()
    if mode not in OUTER_LEFT:
        assert n_left_outer == 0
    if mode not in OUTER_RIGHT:
        assert len(ro_r) == 0


@pytest.mark.parametrize("left_size", SIZES)
@pytest.mark.parametrize("right_size", SIZES)
def test_ordered_oracle_is_the_nested_loop_and_keeps_the_order_contract(left_size, right_size):
    left, right = load_tbl(TABLES[("left", left_size)]), load_tbl(TABLES[("right", right_size)])
    cases = 0
    for a, b in numeric_column_pairs(left, right):
        (lv, ln), (rv, rn) = left.column(a), right.column(b)
        for mode, condition in ACCEPTED:
            out = ordered_join(lv, ln, rv, rn, mode, condition)
            assert sorted(zip(out[0].tolist(), out[1].tolist())) == nested_loop_pairs(lv, ln, rv, rn, mode, condition), (left.names[a], right.names[b], mode, condition)
            check_order_contract(lv, ln, rv, rn, mode, condition, out)
            cases += 1
    assert cases == 16 * len(ACCEPTED)   # int, float, double, long x nullable or not, on both sides


def test_negative_zero_is_zero_and_not_equals_splits_around_the_key():
    lv, rv = np.array([-0.0, 1.0, 0.0], dtype=np.float32), np.array([0.0, -0.0, 2.0, -1.0], dtype=np.float32)
    left, right, n_matched, _ = ordered_join(lv, None, rv, None, abi.JOIN_INNER, abi.PRED_EQUALS)
    assert (left.tolist(), right.tolist(), n_matched) == ([0, 0, 2, 2], [0, 1, 0, 1], 4)
    left, right, n_matched, _ = ordered_join(lv, None, rv, None, abi.JOIN_INNER, abi.PRED_NOT_EQUALS)
    assert (left.tolist(), right.tolist()) == ([0, 0, 2, 2, 1, 1, 1, 1], [3, 2, 3, 2, 3, 0, 1, 2])

"""expression_scan_oracle.pos_list -- the reference's recursion over AND / OR with sorted-list intersection / union and per-leaf rules --
against {row : the ternary value of the predicate is TRUE}, which is what hy_table_scan_expression computes in one pass; BETWEEN's fast
path against its rewrite on the spine; and the tree where they differ, which is why BETWEEN stays refused below the spine."""
import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.operators import lower_between
import expression_scan_oracle as scan_oracle
import projection_expression_oracle as oracle

TYPES = (abi.TYPE_INT, abi.TYPE_LONG, abi.TYPE_FLOAT, abi.TYPE_DOUBLE)
CMP = (abi.PRED_EQUALS, abi.PRED_NOT_EQUALS, abi.PRED_LESS_THAN, abi.PRED_LESS_THAN_EQUALS, abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS)
BETWEENS = (abi.PRED_BETWEEN_INCLUSIVE, abi.PRED_BETWEEN_LOWER_EXCLUSIVE, abi.PRED_BETWEEN_UPPER_EXCLUSIVE, abi.PRED_BETWEEN_EXCLUSIVE)


class FakeColumn:
    handle = None


def columns(rng, rows):
    raw = {abi.TYPE_INT: rng.integers(-5, 6, rows).astype(np.int32), abi.TYPE_LONG: rng.integers(-5, 6, rows).astype(np.int64),
           abi.TYPE_FLOAT: (rng.integers(-10, 11, rows) / 2.0).astype(np.float32), abi.TYPE_DOUBLE: rng.integers(-10, 11, rows) / 2.0}
    out, resolve = {}, {}
    for t in TYPES:
        out[t] = FakeColumn()
        resolve[id(out[t])] = oracle.Column.of(raw[t], rng.random(rows) < 0.25)
    return out, resolve


def random_value(rng, cols, depth):
    pick = rng.integers(0, 5 if depth else 3)
    if pick == 0:
        return cols[TYPES[rng.integers(0, 4)]]
    if pick == 1:
        t = TYPES[rng.integers(0, 4)]
        return (t, int(rng.integers(-3, 4)) if t in (abi.TYPE_INT, abi.TYPE_LONG) else float(rng.integers(-6, 7)) / 2.0)
    if pick == 2:
        return ("neg", cols[TYPES[rng.integers(0, 4)]])
    if pick == 3:
        return ("arith", (abi.ARITH_ADD, abi.ARITH_SUB, abi.ARITH_MUL, abi.ARITH_DIV)[rng.integers(0, 4)], random_value(rng, cols, depth - 1), random_value(rng, cols, depth - 1))
    return ("case", random_predicate(rng, cols, depth - 1, False), random_value(rng, cols, depth - 1), random_value(rng, cols, depth - 1))


def random_predicate(rng, cols, depth, spine):
    pick = rng.integers(0, 5 if depth else 3)
    if pick == 0:
        return ("cmp", CMP[rng.integers(0, 6)], random_value(rng, cols, depth), random_value(rng, cols, depth))
    if pick == 1:
        return ("is_null" if rng.integers(0, 2) else "is_not_null", random_value(rng, cols, depth))
    if pick == 2:
        if not spine:
            return ("cmp", CMP[rng.integers(0, 6)], cols[abi.TYPE_INT], (abi.TYPE_DOUBLE, 0.5))
        t = TYPES[rng.integers(0, 4)]
        return ("between", BETWEENS[rng.integers(0, 4)], cols[t], (abi.TYPE_INT, -2), (abi.TYPE_DOUBLE, 1.5))
    return ("and" if pick == 3 else "or", random_predicate(rng, cols, depth - 1, spine), random_predicate(rng, cols, depth - 1, spine))


@pytest.mark.parametrize("seed", range(40))
def test_the_recursion_over_sorted_lists_is_the_rows_whose_ternary_value_is_true(seed):
    rng = np.random.default_rng(seed)
    rows = 97
    cols, resolve = columns(rng, rows)
    tree = random_predicate(rng, cols, 3, True)
    want = scan_oracle.true_rows(tree, resolve, rows, "fast")
    assert scan_oracle.pos_list(tree, resolve, rows, "fast") == want, tree
    # BETWEEN on the spine: the fast path (!null && in range), the rewrite, and the lowered tree the mirrors hand to the library agree
    assert scan_oracle.pos_list(tree, resolve, rows, "rewrite") == want, tree
    assert scan_oracle.true_rows(tree, resolve, rows, "rewrite") == want, tree
    lowered = lower_between(tree)
    assert "between" not in repr(lowered)
    assert scan_oracle.pos_list(lowered, resolve, rows) == want, tree


def test_between_under_is_null_shows_why_it_stays_refused_below_the_spine():
    rng = np.random.default_rng(1)
    rows = 50
    cols, resolve = columns(rng, rows)
    column = cols[abi.TYPE_INT]
    nulls = [i for i, c in enumerate(resolve[id(column)].cells) if c is None]
    assert nulls and len(nulls) < rows
    tree = ("is_null", ("between", abi.PRED_BETWEEN_INCLUSIVE, column, (abi.TYPE_INT, -1), (abi.TYPE_INT, 1)))
    assert scan_oracle.pos_list(tree, resolve, rows, "fast") == []          # the fast path's FALSE for a NULL operand is not NULL
    assert scan_oracle.pos_list(tree, resolve, rows, "rewrite") == nulls    # the rewrite's NULL is
    with pytest.raises(ValueError):
        lower_between(tree)
    with pytest.raises(ValueError):
        lower_between(("case", ("between", abi.PRED_BETWEEN_INCLUSIVE, column, (abi.TYPE_INT, -1), (abi.TYPE_INT, 1)), column, column))
    on_spine = ("or", ("is_null", column), ("between", abi.PRED_BETWEEN_EXCLUSIVE, column, (abi.TYPE_INT, -1), (abi.TYPE_INT, 1)))
    assert lower_between(on_spine) == ("or", ("is_null", column), ("and", ("cmp", abi.PRED_GREATER_THAN, column, (abi.TYPE_INT, -1)), ("cmp", abi.PRED_LESS_THAN, column, (abi.TYPE_INT, 1))))


def test_no_predicate_at_the_root_fails():
    rng = np.random.default_rng(2)
    cols, resolve = columns(rng, 5)
    for tree in (cols[abi.TYPE_INT], (abi.TYPE_INT, 1), ("neg", cols[abi.TYPE_INT]), ("arith", abi.ARITH_ADD, cols[abi.TYPE_INT], (abi.TYPE_INT, 1)),
                 ("case", ("is_null", cols[abi.TYPE_INT]), (abi.TYPE_INT, 1), (abi.TYPE_INT, 0))):
        with pytest.raises(ValueError):
            scan_oracle.pos_list(tree, resolve, 5)

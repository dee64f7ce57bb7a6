"""A literal restatement of ExpressionEvaluator::evaluate_expression_to_pos_list (expression_evaluator.cpp:1129-1311): the PosList of a
predicate tree over one chunk.  AND / OR recurse and intersect / unite the children's sorted lists (:1249-1265); every other node kind
is a leaf with its own rule; anything that is no predicate Fails (:1307).  Below the leaves the cells come from
projection_expression_oracle.evaluate.  Trees are what hyrise_amd.operators.table_scan_expression takes, ("between", condition, operand,
lower, upper) included; `between` picks how a BETWEEN is evaluated: "fast" (_evaluate_between_expression's fast path, :590-656: not NULL
and in range -- FALSE, not NULL, for a NULL operand) or "rewrite" (operand >= lower AND operand <= upper, rewrite_between_expression)."""
import numpy as np

from hyrise_amd import abi
from hyrise_amd.operators import BETWEEN_BOUNDS, ColumnTest
import projection_expression_oracle as oracle


class Cells:
    """Evaluated cells standing in for a subtree (looks like a column to projection_expression_oracle.evaluate)."""
    handle = None


def value(tree, resolve, rows, between="fast"):
    """(type, cells) of any tree: projection_expression_oracle.evaluate, plus BETWEEN as a value under either evaluation."""
    if not isinstance(tree, tuple) or not tree or not isinstance(tree[0], str):
        return oracle.evaluate(tree, resolve, rows)
    if tree[0] == "between":
        condition, operand, lower, upper = tree[1:]
        lower_condition, upper_condition = BETWEEN_BOUNDS[condition]
        (xt, xs), (lt, ls), (ut, us) = (value(t, resolve, rows, between) for t in (operand, lower, upper))
        cells = []
        for x, lo, hi in zip(xs, ls, us):
            above, below = oracle.comparison_cell(lower_condition, x, xt, lo, lt), oracle.comparison_cell(upper_condition, x, xt, hi, ut)
            if between == "fast":   # a bool per row, never NULL (the bounds of the fast path are non-NULL literals)
                cells.append(np.int32(1 if above is not None and below is not None and above != 0 and below != 0 else 0))
            else:
                cells.append(oracle.and_cell(above, below))
        return abi.TYPE_INT, cells
    first = 2 if tree[0] in ("arith", "cmp") else 1
    resolve = dict(resolve)
    stand_ins = []
    for t in tree[first:]:
        data_type, cells = value(t, resolve, rows, between)
        if data_type == abi.TYPE_NULL:
            stand_ins.append(None)
            continue
        stand_in = Cells()
        resolve[id(stand_in)] = oracle.Column(data_type, cells)
        stand_ins.append(stand_in)
    return oracle.evaluate(tree[:first] + tuple(stand_ins), resolve, rows)


def true_rows(tree, resolve, rows, between="fast"):
    """{row : the ternary value of the tree is TRUE}, ascending."""
    _, cells = value(tree, resolve, rows, between)
    return [i for i, c in enumerate(cells) if c is not None and c != 0]


def intersection(left, right):   # std::ranges::set_intersection of two sorted lists
    out, i, j = [], 0, 0
    while i < len(left) and j < len(right):
        if left[i] < right[j]:
            i += 1
        elif right[j] < left[i]:
            j += 1
        else:
            out.append(left[i])
            i, j = i + 1, j + 1
    return out


def union(left, right):   # std::ranges::set_union
    out, i, j = [], 0, 0
    while i < len(left) and j < len(right):
        if left[i] < right[j]:
            out.append(left[i])
            i += 1
        elif right[j] < left[i]:
            out.append(right[j])
            j += 1
        else:
            out.append(left[i])
            i, j = i + 1, j + 1
    return out + left[i:] + right[j:]


def pos_list(tree, resolve, rows, between="fast"):
    """evaluate_expression_to_pos_list over one chunk of `rows` rows -> ascending row numbers."""
    if isinstance(tree, ColumnTest):   # a ColumnVsValue / Between / Like / In / IsNull leaf: value != 0 && !null
        return [i for i, c in enumerate(oracle.evaluate(tree, resolve, rows)[1]) if c is not None and c != 0]
    if not isinstance(tree, tuple) or not tree or not isinstance(tree[0], str):
        raise ValueError("Expression type cannot be evaluated to PosList.")
    kind = tree[0]
    if kind in ("and", "or"):
        left, right = pos_list(tree[1], resolve, rows, between), pos_list(tree[2], resolve, rows, between)
        return intersection(left, right) if kind == "and" else union(left, right)
    if kind == "cmp":   # :1152-1190: rows where neither operand is NULL and the comparison holds
        (at, xs), (bt, ys) = value(tree[2], resolve, rows, between), value(tree[3], resolve, rows, between)
        out = []
        for i, (x, y) in enumerate(zip(xs, ys)):
            if x is None or y is None or abi.TYPE_NULL in (at, bt):
                continue
            if oracle.comparison_cell(tree[1], x, at, y, bt) != 0:
                out.append(i)
        return out
    if kind in ("is_null", "is_not_null"):   # :1210-1230
        _, xs = value(tree[1], resolve, rows, between)
        return [i for i, x in enumerate(xs) if (x is None) == (kind == "is_null")]
    if kind == "between":
        if between == "rewrite":   # :1200
            lower_condition, upper_condition = BETWEEN_BOUNDS[tree[1]]
            return pos_list(("and", ("cmp", lower_condition, tree[2], tree[3]), ("cmp", upper_condition, tree[2], tree[4])), resolve, rows, between)
        return [i for i, c in enumerate(value(tree, resolve, rows, "fast")[1]) if c != 0]   # !null && in range
    raise ValueError("Expression type cannot be evaluated to PosList.")

"""Cell-by-cell restatement of what the reference's ExpressionEvaluator computes for the node kinds of hy_projection_expression
(expression/evaluation/expression_evaluator.cpp, expression_functors.hpp, expression/expression_utils.cpp).  One Python function per
node kind, one cell at a time, no vectorised shortcut that could hide a NULL rule.  A cell is a numpy scalar of the node's type, or None
for NULL.  Floating point: numpy scalar operations are single IEEE operations in the scalar's type.  NaN is not among the inputs of any
test (the swapped > / >= differ from the direct forms only there).

A tree is what hyrise_amd.operators.projection_program takes; `resolve` maps id(column object) -> Column and id(ColumnTest) -> Test."""
import math

import numpy as np

from hyrise_amd import abi

NP = {abi.TYPE_INT: np.int32, abi.TYPE_LONG: np.int64, abi.TYPE_FLOAT: np.float32, abi.TYPE_DOUBLE: np.float64}
FLOATS = (abi.TYPE_FLOAT, abi.TYPE_DOUBLE)


class Column:
    def __init__(self, data_type, cells):
        self.data_type, self.cells = data_type, list(cells)

    @classmethod
    def of(cls, values, nulls=None):
        values = np.asarray(values)
        data_type = {np.dtype(v): k for k, v in NP.items()}[values.dtype]
        return cls(data_type, [None if nulls is not None and nulls[i] else values[i] for i in range(len(values))])


class Test:
    """A column test: cells (anything, None = NULL) and holds(cell) -> bool; null_test: None, "is_null" or "is_not_null"."""
    __test__ = False

    def __init__(self, cells, holds=None, null_test=None):
        self.cells, self.holds, self.null_test = list(cells), holds, null_test


def expression_common_type(lhs, rhs):   # expression_utils.cpp:172-204
    if lhs == abi.TYPE_NULL:
        return rhs
    if rhs == abi.TYPE_NULL:
        return lhs
    if abi.TYPE_DOUBLE in (lhs, rhs):
        return abi.TYPE_DOUBLE
    if abi.TYPE_LONG in (lhs, rhs):
        return abi.TYPE_DOUBLE if abi.TYPE_FLOAT in (lhs, rhs) else abi.TYPE_LONG
    if abi.TYPE_FLOAT in (lhs, rhs):
        return abi.TYPE_FLOAT
    return abi.TYPE_INT


def cxx_common_type(a, b):   # std::common_type_t: the usual arithmetic conversions
    for t in (abi.TYPE_DOUBLE, abi.TYPE_FLOAT, abi.TYPE_LONG):
        if t in (a, b):
            return t
    return abi.TYPE_INT


def wrap(x, data_type):
    """A Python int as the two's-complement int32 / int64 it wraps to."""
    bits = 32 if data_type == abi.TYPE_INT else 64
    x = (int(x) + (1 << (bits - 1))) % (1 << bits) - (1 << (bits - 1))
    return NP[data_type](x)


def cast(x, to):   # static_cast between the four numeric types
    if to in FLOATS:
        return NP[to](x)
    if isinstance(x, (np.floating, float)):
        return wrap(math.trunc(float(x)), to)
    return wrap(int(x), to)


def arithmetic_cell(op, x, at, y, bt):   # expression_functors.hpp:127-213
    rt = expression_common_type(at, bt)
    if x is None or y is None:
        return None
    if op in (abi.ARITH_DIV, abi.ARITH_MOD) and y == 0:   # :174,205
        return None
    with np.errstate(all="ignore"):
        if op == abi.ARITH_DIV:   # computed in the result type
            p, q = cast(x, rt), cast(y, rt)
            if rt in FLOATS:
                return NP[rt](p / q)
            p, q = int(p), int(q)
            quotient = abs(p) // abs(q)
            return wrap(quotient if (p < 0) == (q < 0) else -quotient, rt)
        if op == abi.ARITH_MOD:
            if at not in FLOATS and bt not in FLOATS:
                c = cxx_common_type(at, bt)
                p, q = int(x), int(y)
                remainder = 0 if q == -1 else (abs(p) % abs(q)) * (1 if p >= 0 else -1)
                return cast(wrap(remainder, c), rt)
            if at == abi.TYPE_FLOAT and bt == abi.TYPE_FLOAT:
                return cast(np.float32(math.fmod(float(x), float(y))), rt)   # (fmod is exact: computing it in double loses nothing)
            return cast(np.float64(math.fmod(float(x), float(y))), rt)
        c = cxx_common_type(at, bt)   # + - *: in the common C++ type, then cast to the result type
        p, q = cast(x, c), cast(y, c)
        if c in FLOATS:
            result = p + q if op == abi.ARITH_ADD else p - q if op == abi.ARITH_SUB else p * q
            return cast(NP[c](result), rt)
        p, q = int(p), int(q)
        return cast(wrap(p + q if op == abi.ARITH_ADD else p - q if op == abi.ARITH_SUB else p * q, c), rt)


def comparison_cell(condition, x, at, y, bt):   # expression_functors.hpp:90-116, expression_evaluator.cpp:73-90
    if x is None or y is None or abi.TYPE_NULL in (at, bt):
        return None
    if condition in (abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS):   # evaluated as the swapped < / <=
        x, at, y, bt = y, bt, x, at
        condition = abi.PRED_LESS_THAN if condition == abi.PRED_GREATER_THAN else abi.PRED_LESS_THAN_EQUALS
    c = cxx_common_type(at, bt)
    p, q = cast(x, c), cast(y, c)
    holds = {abi.PRED_EQUALS: p == q, abi.PRED_NOT_EQUALS: p != q, abi.PRED_LESS_THAN: p < q, abi.PRED_LESS_THAN_EQUALS: p <= q}[condition]
    return np.int32(1 if holds else 0)


def and_cell(a, b):   # TernaryAndEvaluator, expression_functors.hpp:61-84
    a_true, b_true = a is not None and a != 0, b is not None and b != 0
    is_null = (a is None and b is None) or (a_true and b is None) or (b_true and a is None)
    return None if is_null else np.int32(1 if a_true and b_true else 0)


def or_cell(a, b):   # TernaryOrEvaluator, expression_functors.hpp:41-56
    a_true, b_true = a is not None and a != 0, b is not None and b != 0
    value = a_true or b_true
    return None if (a is None or b is None) and not value else np.int32(1 if value else 0)


def case_cell(when, then, then_type, otherwise, otherwise_type):   # expression_evaluator.cpp:726-759
    result_type = expression_common_type(then_type, otherwise_type)
    chosen = then if when is not None and when != 0 else otherwise
    return None if chosen is None else cast(chosen, result_type)


def negate_cell(x, data_type):   # expression_evaluator.cpp:965-988
    if x is None:
        return None
    return NP[data_type](-x) if data_type in FLOATS else wrap(-int(x), data_type)


def test_cell(test, cell):
    if test.null_test is not None:
        return np.int32(1 if (cell is None) == (test.null_test == "is_null") else 0)
    return None if cell is None else np.int32(1 if test.holds(cell) else 0)   # the evaluator's rule: NULL where the cell is NULL


test_cell.__test__ = False


def evaluate(tree, resolve, rows):
    """-> (HY_TYPE_* of the result, [cell per row])"""
    from hyrise_amd.operators import ColumnTest
    if hasattr(tree, "handle"):
        column = resolve[id(tree)]
        return column.data_type, column.cells
    if isinstance(tree, ColumnTest):
        test = resolve[id(tree)]
        return abi.TYPE_INT, [test_cell(test, cell) for cell in test.cells]
    if tree is None:
        return abi.TYPE_NULL, [None] * rows
    if not isinstance(tree[0], str):
        return tree[0], [NP[tree[0]](tree[1])] * rows
    kind = tree[0]
    if kind in ("arith", "cmp"):
        (at, xs), (bt, ys) = evaluate(tree[2], resolve, rows), evaluate(tree[3], resolve, rows)
        if kind == "arith":
            return expression_common_type(at, bt), [arithmetic_cell(tree[1], x, at, y, bt) for x, y in zip(xs, ys)]
        return abi.TYPE_INT, [comparison_cell(tree[1], x, at, y, bt) for x, y in zip(xs, ys)]
    operands = [evaluate(t, resolve, rows) for t in tree[1:]]
    if kind in ("and", "or"):
        cell = and_cell if kind == "and" else or_cell
        return abi.TYPE_INT, [cell(a, b) for a, b in zip(operands[0][1], operands[1][1])]
    if kind in ("is_null", "is_not_null"):   # expression_evaluator.cpp:382-402
        return abi.TYPE_INT, [np.int32(1 if (x is None) == (kind == "is_null") else 0) for x in operands[0][1]]
    if kind == "neg":
        return operands[0][0], [negate_cell(x, operands[0][0]) for x in operands[0][1]]
    if kind == "case":
        (_, whens), (tt, thens), (ot, others) = operands
        return expression_common_type(tt, ot), [case_cell(w, t, tt, o, ot) for w, t, o in zip(whens, thens, others)]
    raise ValueError(f"node {kind}")


def as_arrays(data_type, cells):
    """(values with T{} in NULL cells, null mask): what ResultColumn.read() returns."""
    nulls = np.array([c is None for c in cells], dtype=bool)
    values = np.array([NP[data_type](0) if c is None else c for c in cells], dtype=NP[data_type])
    return values, nulls

"""Pins tests/projection_expression_oracle.py -- the cell rules the GPU tests of hy_projection_expression compare against -- to recorded
answers of the reference's own tests (src/test/lib/expression/expression_evaluator_to_values_test.cpp), restated as data in
tests/golden/expression/known_answers.json: every entry names the test and the line it was read from.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from hyrise_amd import abi
import projection_expression_oracle as oracle
from support import load_tbl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expression")
TYPES = {"int": abi.TYPE_INT, "long": abi.TYPE_LONG, "float": abi.TYPE_FLOAT, "double": abi.TYPE_DOUBLE}
ARITH = {"add": abi.ARITH_ADD, "sub": abi.ARITH_SUB, "mul": abi.ARITH_MUL, "div": abi.ARITH_DIV, "mod": abi.ARITH_MOD}
CMP = {"=": abi.PRED_EQUALS, "<>": abi.PRED_NOT_EQUALS, "<": abi.PRED_LESS_THAN, "<=": abi.PRED_LESS_THAN_EQUALS, ">": abi.PRED_GREATER_THAN,
       ">=": abi.PRED_GREATER_THAN_EQUALS}
DOCUMENT = json.load(open(os.path.join(GOLDEN, "known_answers.json")))


class Name:
    """Stands where a device column stands in a tree."""
    handle = None


def columns_of(entry):
    if "table" in entry:
        table = load_tbl(os.path.join(GOLDEN, entry["table"]))
        return {name: oracle.Column.of(*table.column(name)) for name, t in zip(table.names, table.types) if t != abi.TYPE_STRING}
    return {name: oracle.Column(TYPES[t], [None if c is None else oracle.NP[TYPES[t]](c) for c in cells]) for name, (t, cells) in entry["columns"].items()}


def tree_of(expr, names, resolve, columns):
    kind = expr[0]
    if kind == "col":
        if expr[1] not in names:
            names[expr[1]] = Name()
            resolve[id(names[expr[1]])] = columns[expr[1]]
        return names[expr[1]]
    if kind == "lit":
        return (TYPES[expr[1]], expr[2])
    if kind == "null":
        return None
    rest = [tree_of(e, names, resolve, columns) for e in expr[1:] if isinstance(e, list)]
    if kind == "arith":
        return ("arith", ARITH[expr[1]], *rest)
    if kind == "cmp":
        return ("cmp", CMP[expr[1]], *rest)
    return (kind, *rest)


def test_manifest_matches_the_fixtures():
    manifest = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    assert sorted(manifest) == sorted(name for name in os.listdir(GOLDEN) if name != "MANIFEST.json")
    for name, record in manifest.items():
        data = open(os.path.join(GOLDEN, name), "rb").read()
        assert len(data) == record["bytes"] and hashlib.sha256(data).hexdigest() == record["sha256"], name


def test_every_listed_test_is_restated():
    tests = {entry["test"] for entry in DOCUMENT["entries"]}
    assert tests == {"TernaryOrLiterals", "TernaryOrSeries", "TernaryAndLiterals", "TernaryAndSeries", "ArithmeticsSeries", "PredicatesSeries", "CaseSeries", "IsNullSeries",
                     "NegateSeries"}
    assert all(isinstance(entry["line"], int) for entry in DOCUMENT["entries"])


@pytest.mark.parametrize("entry", DOCUMENT["entries"], ids=lambda e: f"{e['test']}:{e['line']}")
def test_oracle_gives_the_recorded_answer(entry):
    columns = columns_of(entry)
    rows = len(next(iter(columns.values())).cells)
    resolve = {}
    tree = tree_of(entry["expr"], {}, resolve, columns)
    data_type, cells = oracle.evaluate(tree, resolve, rows)
    assert data_type == TYPES[DOCUMENT["result_type"]]
    assert [None if c is None else c.item() for c in cells] == entry["expected"]
    assert all(c is None or isinstance(c, np.int32) for c in cells)


def test_cell_rules_the_recorded_answers_do_not_reach():
    """Int against Float compares as float (16 777 217 rounds to 16 777 216.0f: equal); -0.0 equals 0.0; int32 arithmetic wraps; Long with Float
    computes in float and widens to double; division truncates; a CASE over Int and Double branches is Double."""
    assert oracle.comparison_cell(abi.PRED_EQUALS, np.int32(16_777_217), abi.TYPE_INT, np.float32(16_777_216.0), abi.TYPE_FLOAT) == 1
    assert oracle.comparison_cell(abi.PRED_EQUALS, np.int64(16_777_217), abi.TYPE_LONG, np.float32(16_777_216.0), abi.TYPE_FLOAT) == 1
    assert oracle.comparison_cell(abi.PRED_EQUALS, np.int32(16_777_217), abi.TYPE_INT, np.float64(16_777_216.0), abi.TYPE_DOUBLE) == 0
    assert oracle.comparison_cell(abi.PRED_EQUALS, np.float64(-0.0), abi.TYPE_DOUBLE, np.float32(0.0), abi.TYPE_FLOAT) == 1
    assert oracle.arithmetic_cell(abi.ARITH_ADD, np.int32(2**31 - 1), abi.TYPE_INT, np.int32(1), abi.TYPE_INT) == -2**31
    got = oracle.arithmetic_cell(abi.ARITH_MUL, np.int64(3), abi.TYPE_LONG, np.float32(0.1), abi.TYPE_FLOAT)
    assert isinstance(got, np.float64) and got == np.float64(np.float32(3) * np.float32(0.1))
    assert oracle.arithmetic_cell(abi.ARITH_DIV, np.int32(-7), abi.TYPE_INT, np.int32(2), abi.TYPE_INT) == -3
    assert oracle.arithmetic_cell(abi.ARITH_MOD, np.int32(-7), abi.TYPE_INT, np.int32(2), abi.TYPE_INT) == -1
    got = oracle.case_cell(np.int32(1), np.int32(5), abi.TYPE_INT, np.float64(0.5), abi.TYPE_DOUBLE)
    assert isinstance(got, np.float64) and got == 5.0
    assert oracle.case_cell(None, np.int32(5), abi.TYPE_INT, None, abi.TYPE_NULL) is None
    assert str(oracle.negate_cell(np.float32(0.0), abi.TYPE_FLOAT)) == "-0.0"

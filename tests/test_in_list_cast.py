"""hy_in_list_cast: the list handling in front of hy_table_scan_in_list (rewrite_in_list_expression's `=` terms under
lossless_predicate_cast): elements the column's type cannot hold exactly are dropped, NULLs are dropped and reported."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.operators import in_list_cast

INT, LONG, FLOAT, DOUBLE, STRING = abi.TYPE_INT, abi.TYPE_LONG, abi.TYPE_FLOAT, abi.TYPE_DOUBLE, abi.TYPE_STRING
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_int_column_mixed_list():
    literals = [(INT, 1), (DOUBLE, 2.0), (DOUBLE, 2.5), (LONG, 2 ** 40), None]
    kept, has_null = in_list_cast(INT, literals)
    assert kept == [1, 2] and has_null
    again, again_null = in_list_cast(INT, list(reversed(literals)))   # the result does not depend on the order
    assert sorted(again) == sorted(kept) and again_null
    kept, has_null = in_list_cast(INT, [(INT, 1), (DOUBLE, 2.0)])
    assert kept == [1, 2] and not has_null


def test_float_column_double_elements():
    kept, has_null = in_list_cast(FLOAT, [(DOUBLE, 0.1), (DOUBLE, 0.5)])   # no float equals the double 0.1
    assert kept == [0.5] and not has_null
    kept, _ = in_list_cast(FLOAT, [(DOUBLE, 0.5), (DOUBLE, 0.1)])
    assert kept == [0.5]
    kept, _ = in_list_cast(FLOAT, [(DOUBLE, float(np.float32(0.1)))])      # ... but the double that IS a float is kept
    assert kept == [float(np.float32(0.1))]
    kept, _ = in_list_cast(DOUBLE, [(FLOAT, float("nan")), (FLOAT, 1.5)])   # NaN equals no row
    assert kept == [1.5]


def test_long_column_int_elements():
    kept, has_null = in_list_cast(LONG, [(INT, -7), (INT, 2 ** 31 - 1), (LONG, 2 ** 40), None, (DOUBLE, 3.0), (FLOAT, 0.5)])
    assert kept == [-7, 2 ** 31 - 1, 2 ** 40, 3] and has_null


def test_string_against_numeric_column():
    for column_type in (INT, LONG, FLOAT, DOUBLE):
        kept, has_null = in_list_cast(column_type, [(STRING, "7"), (INT, 7)])
        assert kept == [7] and not has_null
        kept, has_null = in_list_cast(column_type, [(STRING, "7"), None])
        assert kept == [] and has_null


def test_arguments():
    lib = abi.load_library()
    n_out, has_null = C.c_uint32(9), C.c_uint32(9)
    assert lib.hy_in_list_cast(INT, None, None, 0, None, C.byref(n_out), C.byref(has_null)) == abi.OK   # the empty list: nothing kept
    assert n_out.value == 0 and has_null.value == 0
    types, values, out = (C.c_uint32 * 1)(INT), (abi.Value * 1)(), (abi.Value * 1)()
    assert lib.hy_in_list_cast(STRING, C.addressof(types), C.addressof(values), 1, C.addressof(out), C.byref(n_out), C.byref(has_null)) == abi.ERR_INVALID
    assert lib.hy_in_list_cast(INT, C.addressof(types), C.addressof(values), 1, C.addressof(out), None, C.byref(has_null)) == abi.ERR_INVALID
    types[0] = 17
    assert lib.hy_in_list_cast(INT, C.addressof(types), C.addressof(values), 1, C.addressof(out), C.byref(n_out), C.byref(has_null)) == abi.ERR_INVALID


def test_hy_in_list_layout_matches_the_header(tmp_path):
    """abi.InList field by field against the C compiler's layout of hy_in_list; HY_MAX_IN_LIST is abi.MAX_IN_LIST."""
    lines = ['  printf("size %zu\\n", sizeof(hy_in_list));\n', '  printf("max %d\\n", HY_MAX_IN_LIST);\n']
    lines += [f'  printf("{field[0]} %zu\\n", offsetof(hy_in_list, {field[0]}));\n' for field in abi.InList._fields_]
    source = tmp_path / "layout.c"
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    got = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.InList) and int(got["max"]) == abi.MAX_IN_LIST == 256
    for field in abi.InList._fields_:
        assert int(got[field[0]]) == getattr(abi.InList, field[0]).offset, field[0]
    assert abi.PRED_IN == 10 and abi.PRED_NOT_IN == 11

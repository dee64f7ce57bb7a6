"""tests/product_oracle.py against the reference's OperatorsProductTest (product_test.cpp:30-56): the three expected tables as multisets of
rows, the oracle's two statements against each other, the order contract written out for one small case, and the fixtures' manifest."""
import hashlib
import json
import os

import numpy as np

from hyrise_amd import abi, storage
from hyrise_amd.operators import make_predicate
from product_oracle import NULL_ROW_ID, entire_chunk, product, product_numpy
from support import GOLDEN, load_tbl, oracle_scan

PRODUCT_TBL = os.path.join(GOLDEN, "product")
NAMES = ["float.tbl", "int_filtered_float_product.tbl", "int_float_product.tbl", "int_int.tbl", "int_int_self_product.tbl"]


def chunk_sizes(rows, chunk):
    return [min(chunk, rows - begin) for begin in range(0, rows, chunk)]


def rows_of(table):
    """The rows of a TblTable as tuples of Python numbers (floats as the float32 the file's text rounds to)."""
    return [tuple(column[r].item() for column in table.columns) for r in range(table.rows)]


def joined_rows(left_rows, right_rows, left_list, right_list, left_chunk, right_chunk):
    """What the output table holds: the left table's row at every left RowID next to the right table's row at the right RowID."""
    return sorted(left_rows[int(l[0]) * left_chunk + int(l[1])] + right_rows[int(r[0]) * right_chunk + int(r[1])] for l, r in zip(left_list, right_list))


def test_value_segments():   # product_test.cpp:30-36: int.tbl in chunks of 5 x float.tbl in chunks of 2
    a, b = load_tbl("int.tbl"), load_tbl("product/float.tbl")
    left, right, offsets = product(chunk_sizes(a.rows, 5), chunk_sizes(b.rows, 2))
    assert offsets.tolist() == [0, 6, 12]   # 3 rows x chunks of 2 and 2 rows
    assert joined_rows(rows_of(a), rows_of(b), left, right, 5, 2) == sorted(rows_of(load_tbl("product/int_float_product.tbl")))


def test_reference_and_value_segments():   # :38-48: the left input is the scan `a >= 1234` of int.tbl
    a, b = load_tbl("int.tbl"), load_tbl("product/float.tbl")
    column = storage.make_column(a.columns[0], None, abi.ENC_UNENCODED, chunk_size=5)
    scanned = oracle_scan(column, make_predicate(abi.PRED_GREATER_THAN_EQUALS, abi.TYPE_INT, 1234), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    lists = [scanned.pos_list(c).copy() for c in range(column.n_chunks) if len(scanned.pos_list(c))]   # (one output chunk per chunk with matches)
    assert [len(p) for p in lists] == [2]
    left, right, _ = product([len(p) for p in lists], chunk_sizes(b.rows, 2), left_lists=lists)
    assert joined_rows(rows_of(a), rows_of(b), left, right, 5, 2) == sorted(rows_of(load_tbl("product/int_filtered_float_product.tbl")))


def test_self_product():   # :50-56: int_int.tbl in chunks of 2 with itself
    c = load_tbl("product/int_int.tbl")
    sizes = chunk_sizes(c.rows, 2)
    left, right, offsets = product(sizes, sizes)
    assert offsets.tolist() == [0, 4, 6, 8, 9]
    assert joined_rows(rows_of(c), rows_of(c), left, right, 2, 2) == sorted(rows_of(load_tbl("product/int_int_self_product.tbl")))


def test_order_written_out():
    """L = [2, 1], R = [3]: pair (0, 0) is l0r0 l0r1 l0r2 l1r0 l1r1 l1r2, pair (1, 0) follows; a reference input's entries replace (chunk, offset),
    NULL_ROW_ID included."""
    left, right, offsets = product([2, 1], [3])
    assert left.tolist() == [[0, 0]] * 3 + [[0, 1]] * 3 + [[1, 0]] * 3
    assert right.tolist() == [[0, 0], [0, 1], [0, 2]] * 3
    assert offsets.tolist() == [0, 6, 9]
    lists = [np.array([(7, 5), NULL_ROW_ID], dtype=np.uint32), np.array([(3, 1)], dtype=np.uint32)]
    left, right, _ = product([2, 1], [3], left_lists=lists, right_lists=[entire_chunk(4, 3)])
    assert left.tolist() == [[7, 5]] * 3 + [list(NULL_ROW_ID)] * 3 + [[3, 1]] * 3
    assert right.tolist() == [[4, 0], [4, 1], [4, 2]] * 3
    assert product([], [3])[2].tolist() == [0] and product([2, 0], [0, 1])[2].tolist() == [0, 0, 2, 2, 2]


def test_the_numpy_statement_is_the_loop():
    rng = np.random.default_rng(3)
    for left_sizes, right_sizes in (([5, 3, 1], [2, 2, 1]), ([1, 1], [1]), ([0, 4], [3, 0, 2]), ([], [2]), ([7], [])):
        for referenced in (False, True):
            left_lists = [rng.integers(0, 9, (n, 2)).astype(np.uint32) for n in left_sizes] if referenced else None
            right_lists = [rng.integers(0, 9, (n, 2)).astype(np.uint32) for n in right_sizes] if referenced else None
            want, got = product(left_sizes, right_sizes, left_lists, right_lists), product_numpy(left_sizes, right_sizes, left_lists, right_lists)
            for a, b in zip(want, got):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_product_fixtures_match_their_manifest():
    manifest = json.load(open(os.path.join(PRODUCT_TBL, "MANIFEST.json")))
    assert sorted(manifest) == sorted(f for f in os.listdir(PRODUCT_TBL) if f.endswith(".tbl")) == NAMES
    for name, entry in manifest.items():
        data = open(os.path.join(PRODUCT_TBL, name), "rb").read()
        assert len(data) < 400, name
        assert hashlib.sha256(data).hexdigest() == entry["sha256"], name

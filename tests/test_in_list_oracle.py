"""The two statements of IN / NOT IN the GPU tests compare against agree with each other: the union of the oracle's Equals scans
(tests/in_list_oracle.py union_of_equals) and the numpy brute force, on a small .tbl fixture with NULLs, -0.0, NaN rows and lists
with duplicates."""
import numpy as np
import pytest

from hyrise_amd import abi

from in_list_oracle import brute_force_in, union_of_equals
from support import build_column, load_tbl

TABLE = "in_list/float_int_null.tbl"
LISTS = {"f": [[0.0], [-0.0, 1.5, 1.5], [2.5, 0.1, -1.5, 9.0, 2.5, 0.0], [7.0]],
         "i": [[2], [2, 2, 1], [-2147483648, 2147483647, 7, 5, 1073741824], [100]],
         "d": [[0.0, 0.5], [-0.0], [1e300, 0.1, 0.1, 3.0, -7.5], [4.0]]}


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("chunk_size", [5, 100])
@pytest.mark.parametrize("negated", [False, True], ids=["in", "not_in"])
def test_union_of_equals_is_the_brute_force(name, chunk_size, negated):
    table = load_tbl(TABLE)
    values, nulls = table.column(name)
    if name == "f":
        assert np.isnan(values).any() and np.signbit(values[0]) and nulls.any()
    encodings = [abi.ENC_UNENCODED] if np.dtype(values.dtype).kind == "f" else [abi.ENC_UNENCODED, abi.ENC_DICTIONARY, abi.ENC_FRAME_OF_REFERENCE]   # (NaN rows: no dictionary)
    for encoding in encodings:
        host = build_column(values, nulls, chunk_size, encoding)
        for elements in LISTS[name]:
            per_chunk = union_of_equals(host, elements, negated=negated, nullable=nulls is not None)
            rows = np.concatenate([c * chunk_size + p.astype(np.int64) for c, p in enumerate(per_chunk)]) if per_chunk else np.zeros(0, np.int64)
            want = np.flatnonzero(brute_force_in(values, nulls, elements, negated))
            np.testing.assert_array_equal(rows, want, err_msg=f"{name} {elements} encoding {encoding}")
            for positions in per_chunk:
                assert np.all(np.diff(positions.astype(np.int64)) > 0)


def test_nan_rows_and_signed_zero():
    values = np.array([np.nan, -0.0, 0.0, 1.0], dtype=np.float32)
    assert brute_force_in(values, None, [0.0]).tolist() == [False, True, True, False]
    assert brute_force_in(values, None, [0.0], negated=True).tolist() == [True, False, False, True]
    assert brute_force_in(values, np.array([True, False, False, False]), [5.0], negated=True).tolist() == [False, True, True, True]

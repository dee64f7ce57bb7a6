"""hy_string_column_materialize (csrc/string_substr.hip) against tests/string_gather_oracle.py -- and tests/string_substr_oracle.py with the
arguments that keep every byte -- byte for byte after read-back, under both routes (HY_OPT_STRING_SPARSE_GATHER 0 and 2): over the data
column, and over reference columns of 1, 257 and 70 000 rows with PosLists in host memory, in the caller's device memory and as entire
chunks, chunked 1 / 256 / unevenly with an empty chunk among them.  The output's chunk layout is the input's.  The same columns through
hy_string_column_substr with a window that does not begin at byte 0 give the same bytes under both routes (the subset ranked from single
positions)."""
import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import string_column_materialize, string_column_substr
from hyrise_amd.storage import DeviceColumn
from placed_columns import PlacedColumn
from string_sparse_source import DENSE, NULL, SPARSE, SparseSource
from test_string_gather_gpu import assert_result
import string_gather_oracle as oracle
import string_substr_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def source(device):
    return SparseSource()


def check_column(source, column, chunks, context):
    """chunks: the column's rows per chunk as bytes / None."""
    want = oracle.encode_chunks([row for chunk in chunks for row in chunk], [len(chunk) for chunk in chunks])
    assert want == string_substr_oracle.column_substr(chunks, 1, 2**31 - 1)
    want_window = string_substr_oracle.column_substr(chunks, 3, 2)
    for route in (SPARSE, DENSE):
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            got = string_column_materialize(column, source.dev_dict)
            window = string_column_substr(column, source.dev_dict, 3, 2)
        assert got.n_chunks == len(chunks) and [len(ids) for ids in got.read_value_ids()] == [len(chunk) for chunk in chunks], f"{context}, route {route}: chunk layout"
        assert_result(got, want, f"{context}, route {route}")
        assert_result(window, want_window, f"{context}, SUBSTR(3, 2), route {route}")


def test_the_data_column(source):
    check_column(source, source.dev, source.chunks, "data column")


def reference_lists(source, sizes, seed):
    """PosLists of the given sizes over the whole source, some RowIDs NULL; the first list with rows stays inside one chunk."""
    rng = np.random.default_rng(seed)
    lists, common = [], []
    for k, size in enumerate(sizes):
        chunk_ids = rng.integers(1, 5, size)
        if k == 0 and size:
            chunk_ids[:] = 4
        lengths = np.array([len(chunk) for chunk in source.chunks])[chunk_ids]
        positions = np.stack([chunk_ids, (rng.random(size) * lengths).astype(np.int64)], axis=1).astype(np.uint32)
        if size > 2:
            positions[rng.random(size) < 0.05] = NULL
        lists.append(positions)
        common.append(4 if k == 0 and size and not (positions == NULL).any() else None)
    return lists, common


LAYOUTS = {"one_row": [1], "rows_of_one": [1] * 257, "chunks_of_256": [256, 0, 1], "uneven": [3, 0, 65_535, 4_462]}


@pytest.mark.parametrize("lists", ["host", "device"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_reference_columns(source, layout, lists):
    """1, 257 and 70 000 rows; a caller-owned list without rows has no buffer and names a chunk (it reads as an entire-chunk list of no rows)."""
    sizes = LAYOUTS[layout]
    pos_lists, common = reference_lists(source, sizes, len(sizes))
    if lists == "device":
        common = [c if len(p) else 0 for p, c in zip(pos_lists, common)]
    reference = storage.make_reference_column(source.host, pos_lists, common)
    if lists == "device":
        column = PlacedColumn(reference, "aligned", 0x00, refs={id(source.host): source.dev})
    else:
        column = DeviceColumn(reference, refs={id(source.host): source.dev})
    chunks = [[source.row(tuple(p)) for p in positions.tolist()] for positions in pos_lists]
    check_column(source, column, chunks, f"{layout}, {lists} PosLists")
    if lists == "device":
        column.assert_untouched()


def test_entire_chunk_lists_among_others(source):
    """EntireChunkPosLists of the bit-packed chunk, of the chunk without entries and of the chunk with the long entry, and a list over them."""
    positions = reference_lists(source, [257], 9)[0][0]
    pos_lists = [2, positions, 0, 3]
    reference = storage.make_reference_column(source.host, pos_lists, [2, None, 0, 3])
    column = DeviceColumn(reference, refs={id(source.host): source.dev})
    chunks = [source.chunks[2], [source.row(tuple(p)) for p in positions.tolist()], source.chunks[0], source.chunks[3]]
    check_column(source, column, chunks, "entire chunks")

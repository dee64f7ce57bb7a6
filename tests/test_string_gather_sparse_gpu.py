"""hy_string_column_gather on its sparse route (HY_OPT_STRING_SPARSE_GATHER = 2: the column read at the RowIDs, only the entries they
reference ranked) against tests/string_gather_oracle.py and against the dense route (= 0) in the same process, byte for byte after
read-back: attribute vectors, offsets and chars.  The source (string_sparse_source.py) has every attribute-vector width and a bit-packed
one; the cases are sizes around the workgroup, positions in one chunk, positions that skip chunks, one row many times, no non-NULL row at
all (an empty subset), equal strings of different chunks, output chunks of 1 and 256 rows and one larger than n, and positions in the
caller's memory between guard bytes.  The sparse route takes no temporary block of the size of the column's export; the dense route does."""
import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.like import LikeMatcher
from hyrise_amd.operators import column_string_ranks, sort, string_column_gather, table_scan_like
from placed_columns import PlacedArray
from support import result_rows
from string_sparse_source import DENSE, NULL, SPARSE, SparseSource, temporary_pool_largest_block
from test_string_gather_gpu import assert_result
import string_gather_oracle as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def source(device):
    return SparseSource()


def random_positions(source, n, seed, chunks=(1, 2, 3, 4), null_fraction=0.1):
    rng = np.random.default_rng(seed)
    chunk_ids = np.array(chunks)[rng.integers(0, len(chunks), n)]
    sizes = np.array([len(chunk) for chunk in source.chunks])[chunk_ids]
    positions = np.stack([chunk_ids, (rng.random(n) * sizes).astype(np.int64)], axis=1).astype(np.uint32)
    positions[rng.random(n) < null_fraction] = NULL
    return positions


def gather_both(source, positions, chunk_rows, context):
    """The gather under both routes against the oracle; returns the sparse route's result."""
    positions = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1, 2)
    rows = [source.row(tuple(p)) for p in positions.tolist()]
    want = oracle.encode_chunks(rows, oracle.uniform_sizes(len(rows), chunk_rows))
    results = {}
    for route in (SPARSE, DENSE):
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            results[route] = string_column_gather(source.dev, source.dev_dict, positions, chunk_rows)
        assert_result(results[route], want, f"{context}, route {route}")
    sparse, dense = results[SPARSE], results[DENSE]
    for c, (a, b) in enumerate(zip(sparse.read_value_ids(), dense.read_value_ids())):
        assert a.tobytes() == b.tobytes(), f"{context}: attribute vector of chunk {c}"
        (_, chars_a, offsets_a), (_, chars_b, offsets_b) = sparse.dictionary.read_chunk(c), dense.dictionary.read_chunk(c)
        assert chars_a.tobytes() == chars_b.tobytes() and offsets_a.tobytes() == offsets_b.tobytes(), f"{context}: chars / offsets of chunk {c}"
    dense.close()
    return sparse, rows


@pytest.mark.parametrize("chunk_rows", [1, 256, 5_000])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1_000])
def test_sizes(source, n, chunk_rows):
    positions = random_positions(source, n, n * 3 + chunk_rows)
    if n > 2:
        positions[0] = positions[-1] = NULL
    gather_both(source, positions, chunk_rows, f"n {n}, chunk_rows {chunk_rows}")


@pytest.mark.parametrize("chunk", [1, 2, 3, 4])
def test_all_positions_in_one_chunk(source, chunk):
    """Chunk 1 has one entry (u8), 2 is bit-packed, 3 holds the 100 000-byte entry (u16), 4 has u32 value ids."""
    positions = random_positions(source, 300, chunk, chunks=(chunk,))
    if chunk == 3:
        positions[7] = positions[200] = (3, source.chunks[3].index(max(source.chunks[3], key=lambda row: len(row or b""))))
    gather_both(source, positions, 256, f"chunk {chunk}")


def test_positions_that_skip_whole_chunks(source):
    """Chunks 0 (no entries) and 2 .. 3 are never referenced; then only chunk 0's NULL rows and chunk 4."""
    gather_both(source, random_positions(source, 500, 21, chunks=(1, 4)), 256, "chunks 1 and 4")
    gather_both(source, random_positions(source, 500, 22, chunks=(0, 4)), 256, "chunks 0 and 4")
    gather_both(source, random_positions(source, 257, 23, chunks=(2,), null_fraction=0), 1, "chunk 2, no NULLs")


def test_every_position_the_same_row(source):
    gather_both(source, [(4, 12_345)] * 700, 256, "one row 700 times")
    gather_both(source, [(3, 0)] * 257, 5_000, "another row 257 times")


def test_no_row_references_an_entry(source):
    """NULL rows, NULL RowIDs and RowIDs outside the table only: the subset is empty, every output chunk has no entries."""
    null_rows = [(c, o) for c, chunk in enumerate(source.chunks) for o, row in enumerate(chunk) if row is None]
    outside = [(5, 0), (9, 3), (1, len(source.chunks[1])), (4, 1_000_000), (0, NULL - 1)]
    positions = null_rows + outside + [(NULL, NULL)] * 250
    for chunk_rows in (1, 256, 5_000):
        got, rows = gather_both(source, positions, chunk_rows, f"no entries, chunk_rows {chunk_rows}")
        assert all(row is None for row in rows) and got.dictionary.n_entries == [0] * got.n_chunks


def test_equal_strings_of_different_chunks_are_one_entry(source):
    shared = b"s00042"
    positions = [(c, source.chunks[c].index(shared)) for c in (2, 3, 4)]
    assert len(positions) == 3
    got, rows = gather_both(source, positions[:2], 256, "two chunks")
    assert rows == [shared] * 2 and got.dictionary.n_entries == [1] and got.read_value_ids()[0].tolist() == [0, 0]
    got, _ = gather_both(source, positions + [(2, source.chunks[2].index(b""))] + positions, 5_000, "three chunks and the empty string")
    assert got.dictionary.n_entries == [2]
    got, _ = gather_both(source, positions, 1, "one row per output chunk")
    assert got.dictionary.n_entries == [1, 1, 1]


def test_caller_owned_positions_between_guards(source):
    """The positions at 8 modulo 16 inside a larger allocation; the guard bytes around them stay as they were."""
    positions = random_positions(source, 1_000, 31)
    placed = PlacedArray(8 * len(positions), 8, 0xA5, guard=64, contents=positions)
    rows = [source.row(tuple(p)) for p in positions.tolist()]
    want = oracle.encode_chunks(rows, oracle.uniform_sizes(len(rows), 256))
    for route in (SPARSE, DENSE):
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            got = string_column_gather(source.dev, source.dev_dict, (placed.pointer, len(positions)), 256)
        assert_result(got, want, f"caller-owned positions, route {route}")
        placed.assert_untouched()


def test_the_sparse_route_takes_no_block_of_the_size_of_the_export(source):
    """The dense route exports every source row (4 bytes of value and 1 of NULL flag each) into blocks of the thread's temporary pool, which
    keeps them; the sparse route's temporaries follow n.  hy_shutdown empties the pool of the calling thread (the library grows it again)."""
    lib = abi.load_library()
    positions = random_positions(source, 20, 41)
    export_bytes = 4 * source.rows
    largest = {}
    for route in (SPARSE, DENSE):
        abi.check(lib.hy_shutdown())
        assert temporary_pool_largest_block(lib) == 0
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            string_column_gather(source.dev, source.dev_dict, positions, 256).close()
        largest[route] = temporary_pool_largest_block(lib)
    assert 0 < largest[SPARSE] < export_bytes <= largest[DENSE], largest


def test_the_result_is_a_string_column_for_sort_and_like(source):
    """hy_column_string_ranks + hy_sort over the sparse route's result order the oracle's rows; hy_table_scan_like over it is the host matcher."""
    chunk_rows = 300
    got, rows = gather_both(source, random_positions(source, 1_000, 51), chunk_rows, "composition")
    stand_in = column_string_ranks(got, got.dictionary)
    order = sort([stand_in], [abi.SORT_ASCENDING_NULLS_FIRST]).numpy()
    flat = (order[:, 0].astype(np.int64) * chunk_rows + order[:, 1]).tolist()
    present = [i for i, row in enumerate(rows) if row is not None]
    assert flat == [i for i, row in enumerate(rows) if row is None] + sorted(present, key=lambda i: rows[i])
    stand_in.close()
    for condition, pattern in ((abi.PRED_LIKE, b"s%"), (abi.PRED_NOT_LIKE, b"%\x00%"), (abi.PRED_LIKE_INSENSITIVE, b"_")):
        matcher = LikeMatcher(pattern, condition)
        found = result_rows(table_scan_like(got, got.dictionary, pattern, condition, nullable=True))
        assert found == [(i // chunk_rows, i % chunk_rows) for i, row in enumerate(rows) if row is not None and matcher(row)], f"LIKE {pattern!r} ({condition})"

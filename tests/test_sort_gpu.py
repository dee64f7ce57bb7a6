"""Sort on the device (hy_sort, hy_column_gather): the order sort.cpp produces -- checked against tests/sort_oracle.py -- over every numeric
type, both NULLS FIRST directions, columns with and without NULLs, every encoding, reference inputs, string keys as ranks."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import SortedPositions, column_gather, join_hash, sort, string_rank_column
from hyrise_amd.storage import DeviceColumn
from hyrise_amd.string_keys import encode_string_column
from sort_oracle import positions_of, sorted_order

pytestmark = pytest.mark.gpu

ASC, DESC = abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST
TYPES = [np.int32, np.int64, np.float32, np.float64]
KINDS = ["value", "dictionary", "frame_of_reference", "run_length", "bit_packed"]


def edge_values(dtype):
    if np.dtype(dtype).kind == "f":
        return np.array([-0.0, 0.0, np.inf, -np.inf, np.finfo(dtype).max, -np.finfo(dtype).max, np.finfo(dtype).tiny], dtype=dtype)
    info = np.iinfo(dtype)
    return np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1], dtype=dtype)


def tied_values(rng, n, dtype, domain=40):
    """Few distinct values (heavy ties), the type's edge values among them."""
    pool = np.concatenate([rng.integers(-domain // 2, domain // 2, domain).astype(dtype), edge_values(dtype)])
    if np.dtype(dtype).kind == "f":
        pool = np.concatenate([pool, (pool[:domain] / 4).astype(dtype)])
    return pool[rng.integers(0, len(pool), n)].astype(dtype)


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    if kind in ("dictionary", "bit_packed"):
        segment = storage.encode_segment(values, nulls, abi.ENC_DICTIONARY)
    elif kind == "frame_of_reference" and values.dtype == np.int32:
        segment = storage.encode_segment(values, nulls, abi.ENC_FRAME_OF_REFERENCE)
    else:
        segment = storage.encode_segment(values, nulls, abi.ENC_UNENCODED)
    if kind == "bit_packed" and segment.size:
        segment = storage.bit_pack_segment(segment)
    return segment


def host_column(values, nulls, chunk, kind, nullable=False):
    """values split into chunks of `chunk` rows, each encoded as `kind`; nullable without NULLs: value segments keep an all-false null vector."""
    segments = []
    for begin in range(0, len(values), chunk):
        end = min(len(values), begin + chunk)
        chunk_nulls = nulls[begin:end] if nulls is not None else (np.zeros(end - begin, dtype=bool) if nullable else None)
        segments.append(segment_of(values[begin:end], chunk_nulls, kind))
    return storage.HostColumn(segments, storage.TYPE_OF_NP[np.dtype(values.dtype)])


def check_sort(columns, keys, modes, chunk_sizes, context=""):
    """columns: DeviceColumns of one table; keys: their (values, nulls) in row order."""
    got = sort(columns, modes)
    want = positions_of(sorted_order(keys, modes), chunk_sizes)
    result = got.numpy()
    assert result.shape == want.shape, context
    if result.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(np.any(result != want, axis=1))[0])
        pytest.fail(f"{context}: first difference at output row {bad}: got {result[bad]}, want {want[bad]}")
    return got


def chunk_sizes_of(n, chunk):
    return [min(chunk, n - b) for b in range(0, n, chunk)]


@pytest.mark.parametrize("dtype", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("kind", KINDS)
def test_one_key_every_type_encoding_mode_and_null_shape(device, dtype, kind):
    rng = np.random.default_rng(len(kind) * 7 + np.dtype(dtype).itemsize)
    n, chunk = 40_003, 7_000
    values = tied_values(rng, n, dtype)
    for nulls, nullable in ((None, False), (np.zeros(n, dtype=bool), True), (rng.random(n) < 0.1, True)):
        column = DeviceColumn(host_column(values, nulls, chunk, kind, nullable))
        for mode in (ASC, DESC):
            check_sort([column], [(values, nulls)], [mode], chunk_sizes_of(n, chunk), f"{np.dtype(dtype).name} {kind} nullable={nullable} mode={mode}")


@pytest.mark.parametrize("n", [0, 1, 2, 3, 8191, 8192, 8193, 65_537, 100_003])
def test_one_to_four_keys_and_row_counts(device, n):
    rng = np.random.default_rng(n)
    chunk = 6_000
    data = [(rng.integers(0, 4, n).astype(np.int32), rng.random(n) < 0.2, "frame_of_reference"),
            (tied_values(rng, n, np.float64, 10), None, "dictionary"),
            (rng.integers(-3, 3, n).astype(np.int64) * (1 << 40), rng.random(n) < 0.05, "value"),
            (tied_values(rng, n, np.float32, 8), rng.random(n) < 0.3, "run_length")]
    columns = [DeviceColumn(host_column(v, m, chunk, kind)) for v, m, kind in data]
    for n_keys in (1, 2, 3, 4):
        for modes in ([ASC] * n_keys, [DESC] * n_keys, [ASC, DESC, ASC, DESC][:n_keys]):
            order = list(range(n_keys))[::-1] if n_keys % 2 == 0 else list(range(n_keys))
            check_sort([columns[i] for i in order], [data[i][:2] for i in order], modes, chunk_sizes_of(n, chunk), f"n={n} keys={order} modes={modes}")


def test_negative_zero_infinities_and_integer_limits(device):
    """-0.0 and 0.0 tie (std::less) and keep input order; the infinities and the integer limits sort at the ends."""
    n = 9_000
    zeros = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)
    ints = np.tile(np.array([np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0, -1, 1], dtype=np.int32), n // 5)
    longs = np.tile(np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, -1, 1 << 32], dtype=np.int64), n // 5)
    infinities = np.tile(np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324], dtype=np.float64), n // 5)
    for values in (zeros.astype(np.float64), zeros.astype(np.float32), ints, longs, infinities, infinities.astype(np.float32)):
        for kind in ("value", "dictionary"):
            column = DeviceColumn(host_column(values, None, 4_000, kind))
            for mode in (ASC, DESC):
                got = check_sort([column], [(values, None)], [mode], chunk_sizes_of(len(values), 4_000), f"{values.dtype} {kind} {mode}")
                if np.all(values == 0):   # every row ties: input order
                    assert got.numpy().tobytes() == positions_of(np.arange(len(values)), chunk_sizes_of(len(values), 4_000)).tobytes()


def test_reference_input_from_scan_pos_lists(device):
    """A reference table (a scan's output: one PosList per chunk, some of them empty, one an entire chunk): positions are (chunk, position in
    the chunk's PosList), ties in PosList order."""
    rng = np.random.default_rng(5)
    n, chunk = 50_000, 8_000
    values = tied_values(rng, n, np.int64, 30)
    nulls = rng.random(n) < 0.1
    base = host_column(values, nulls, chunk, "dictionary")
    base_dev = DeviceColumn(base)
    pos_lists, flat = [], []
    for c, size in enumerate(chunk_sizes_of(n, chunk)):
        if c == 2:
            pos_lists.append(c)   # EntireChunkPosList
            flat.append(c * chunk + np.arange(size))
            continue
        keep = np.flatnonzero(rng.random(size) < (0.0 if c == 4 else 0.4))
        rng.shuffle(keep)   # (a PosList need not be ordered)
        pos_lists.append(np.stack([np.full(len(keep), c), keep], axis=1).astype(np.uint32))
        flat.append(c * chunk + keep)
    reference = storage.make_reference_column(base, pos_lists, list(range(len(pos_lists))))   # (every list references its own chunk)
    reference_dev = DeviceColumn(reference, refs={id(base): base_dev})
    rows = np.concatenate(flat)
    for mode in (ASC, DESC):
        check_sort([reference_dev], [(values[rows], nulls[rows])], [mode], [s.size for s in reference.segments], f"scan output {mode}")
    gathered = column_gather(reference_dev, sort([reference_dev], [DESC]), 3_333)
    order = sorted_order([(values[rows], nulls[rows])], [DESC])
    got_values, got_nulls = gathered.read()
    assert got_nulls.tobytes() == nulls[rows][order].tobytes()
    assert got_values[~got_nulls].tobytes() == values[rows][order][~got_nulls].tobytes()


def test_reference_input_from_a_multi_chunk_join(device):
    """A join's output: two reference columns into two data tables, cut into several chunks; sorted by a column of each side."""
    rng = np.random.default_rng(9)
    left_keys = rng.integers(0, 3_000, 20_000).astype(np.int32)
    right_keys = np.arange(3_000, dtype=np.int32)
    left_payload = tied_values(rng, 20_000, np.float32, 12)
    right_payload = rng.integers(0, 7, 3_000).astype(np.int32)
    left_nulls = rng.random(20_000) < 0.05
    hosts = [host_column(left_keys, None, 4_096, "frame_of_reference"), host_column(right_keys, None, 1_000, "value"),
             host_column(left_payload, left_nulls, 4_096, "dictionary"), host_column(right_payload, None, 1_000, "run_length")]
    devs = [DeviceColumn(h) for h in hosts]
    joined = join_hash(devs[0], devs[1], abi.JOIN_INNER)
    pairs_left, pairs_right = joined.left[:joined.n_pairs], joined.right[:joined.n_pairs]
    cut = list(range(0, joined.n_pairs, 6_500)) + [joined.n_pairs]
    left_lists = [pairs_left[b:e] for b, e in zip(cut[:-1], cut[1:])]
    right_lists = [pairs_right[b:e] for b, e in zip(cut[:-1], cut[1:])]
    left_ref = storage.make_reference_column(hosts[2], left_lists)
    right_ref = storage.make_reference_column(hosts[3], right_lists)
    left_ref_dev, right_ref_dev = DeviceColumn(left_ref, refs={id(hosts[2]): devs[2]}), DeviceColumn(right_ref, refs={id(hosts[3]): devs[3]})
    left_rows = pairs_left[:, 0].astype(np.int64) * 4_096 + pairs_left[:, 1]
    right_rows = pairs_right[:, 0].astype(np.int64) * 1_000 + pairs_right[:, 1]
    keys = [(right_payload[right_rows], None), (left_payload[left_rows], left_nulls[left_rows])]
    sizes = [len(p) for p in left_lists]
    for modes in ([ASC, DESC], [DESC, ASC]):
        check_sort([right_ref_dev, left_ref_dev], keys, modes, sizes, f"join output {modes}")


def test_dictionary_string_key_as_ranks(device):
    """A string column sorts as the ranks of its strings among the column's distinct strings in byte order (StringRanks)."""
    rng = np.random.default_rng(3)
    words = ["", "a", "ab", "abc", "b", "Zebra", "zebra", "éclair", "e", "ba", "a\u0000b"]
    n, chunk = 12_345, 2_000
    strings = [words[i] for i in rng.integers(0, len(words), n)]
    nulls = rng.random(n) < 0.08
    segments, dictionaries = encode_string_column(strings, nulls, chunk)
    ranks_host, _ = string_rank_column(segments, dictionaries)
    column = DeviceColumn(ranks_host)
    for mode in (ASC, DESC):
        got = sort([column], [mode]).numpy()
        rows = got[:, 0].astype(np.int64) * chunk + got[:, 1]
        present = [i for i in range(n) if not nulls[i]]
        # (sorted(reverse=True) keeps ties in input order too: std::stable_sort with std::greater)
        expected = [i for i in range(n) if nulls[i]] + sorted(present, key=lambda i: strings[i].encode("utf-8"), reverse=(mode == DESC))
        assert rows.tolist() == expected, f"mode {mode}"


def test_column_gather_every_type_and_encoding(device):
    """hy_column_gather: the rows at the sorted positions, cut into chunk_rows-row value segments with a null vector."""
    rng = np.random.default_rng(11)
    n = 30_001
    for dtype in TYPES:
        values = tied_values(rng, n, dtype)
        nulls = rng.random(n) < 0.15
        for kind in KINDS:
            column = DeviceColumn(host_column(values, nulls, 5_000, kind))
            positions = sort([column], [ASC])
            order = sorted_order([(values, nulls)], [ASC])
            for chunk_rows in (33, 65_535):
                gathered = column_gather(column, positions, chunk_rows)
                assert gathered.n_chunks == (n + chunk_rows - 1) // chunk_rows
                assert [int(gathered.lib.hy_column_chunk_rows(gathered.handle, c)) for c in range(gathered.n_chunks)] == chunk_sizes_of(n, chunk_rows)
                got_values, got_nulls = gathered.read()
                assert got_nulls.tobytes() == nulls[order].tobytes(), f"{np.dtype(dtype).name} {kind}"
                assert np.array_equal(got_values[~got_nulls], values[order][~got_nulls]), f"{np.dtype(dtype).name} {kind}"
                gathered.close()


def test_refusals(device):
    """NULLS LAST (sort.cpp:294-296), columns of different tables, too small an output, string dictionaries that are not on the device."""
    values = np.arange(100, dtype=np.int32)
    a = DeviceColumn(host_column(values, None, 30, "value"))
    b = DeviceColumn(host_column(values, None, 40, "value"))
    out = SortedPositions(100)
    n_out = C.c_uint64(0)

    def call(columns, modes, capacity=100):
        keys = (abi.SortKey * len(columns))()
        for i, (column, mode) in enumerate(zip(columns, modes)):
            keys[i].column, keys[i].mode = column.handle, mode
        return device.hy_sort(keys, len(columns), out.pointer, capacity, C.byref(n_out))

    assert call([a], [abi.SORT_ASCENDING_NULLS_LAST]) == abi.ERR_INVALID
    assert call([a], [abi.SORT_DESCENDING_NULLS_LAST]) == abi.ERR_INVALID
    assert call([a], [abi.SORT_NONE]) == abi.ERR_INVALID
    assert call([a, b], [ASC, ASC]) == abi.ERR_INVALID
    assert call([a], [ASC], capacity=99) == abi.ERR_CAPACITY and n_out.value == 100
    segments, dictionaries = encode_string_column([str(v) for v in values], None, 30)
    strings = DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))
    assert call([strings], [ASC]) == abi.ERR_UNSUPPORTED
    assert call([a], [ASC]) == abi.OK and n_out.value == 100


def test_sixty_million_rows(device):
    """SF10 lineitem's row count: one double key with ties and NULLs, then an int key."""
    rng = np.random.default_rng(60)
    n = 59_986_052
    prices = (rng.integers(90_000, 10_500_000, n) / 100.0)
    prices[rng.random(n) < 0.01] = 0.0
    nulls = np.zeros(n, dtype=bool)
    nulls[rng.integers(0, n, 1_000)] = True
    lines = rng.integers(1, 8, n).astype(np.int32)
    price_col = DeviceColumn(host_column(prices, nulls, abi.CHUNK_DEFAULT_SIZE, "value"))
    line_col = DeviceColumn(host_column(lines, None, abi.CHUNK_DEFAULT_SIZE, "frame_of_reference"))
    check_sort([line_col, price_col], [(lines, None), (prices, nulls)], [DESC, ASC], chunk_sizes_of(n, abi.CHUNK_DEFAULT_SIZE), "60M rows")

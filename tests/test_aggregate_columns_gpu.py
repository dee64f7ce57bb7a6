"""hy_aggregate_hash_columns: AggregateHash's output table as device-resident columns.  Every case reads the columns and the representative
RowIDs back (hy_column_read_chunk of every chunk) and compares them with hy_aggregate_hash (HY_MEM_HOST) on the same arguments -- byte for
byte: values, NULL flags, RowIDs, n_groups -- and with the CPU oracle (integers exact, float SUM / AVG within 1e-9 relative).  The float
inputs are multiples of 1/4 of moderate size: their sums are exact in any order of the f64 atomics, so two runs give the same bytes."""
import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import aggregate_hash, aggregate_hash_columns, join_hash, make_predicate, sort, table_scan
from hyrise_amd.storage import DeviceColumn
from hyrise_amd.string_keys import AggregateKeyNames, encode_string_column
from sort_oracle import positions_of, sorted_order
from support import build_column, oracle_aggregate

pytestmark = pytest.mark.gpu
FLOAT_TOLERANCE = 1e-9
CHUNK = abi.CHUNK_DEFAULT_SIZE
NP = {abi.TYPE_INT: np.int32, abi.TYPE_LONG: np.int64, abi.TYPE_FLOAT: np.float32, abi.TYPE_DOUBLE: np.float64}
STAGED_GROUPS = 4096   # aggregate.hip: results up to this size are finished on the host


class Col:
    """A column of the test table: its rows (values, nulls) and the HostColumn made of them."""

    def __init__(self, values, nulls=None, encoding=abi.ENC_UNENCODED, chunk=CHUNK):
        self.values, self.nulls, self.chunk = values, nulls, chunk
        self.host = build_column(values, nulls, chunk, encoding)


def finished_on_device(lib):
    lib.hy_debug_aggregate_finished_on_device.restype = int
    return lib.hy_debug_aggregate_finished_on_device()


def read_chunks(lib, column, n_rows, chunk_rows):
    """Every chunk through hy_column_read_chunk: (values, nulls) of the column; checks the chunking and that the bitmaps' tail bits are zero."""
    assert column.rows == n_rows and column.n_chunks == (n_rows + chunk_rows - 1) // chunk_rows
    values, nulls = [], []
    for k in range(column.n_chunks):
        rows = int(lib.hy_column_chunk_rows(column.handle, k))
        assert rows == min(chunk_rows, n_rows - k * chunk_rows), f"chunk {k} holds {rows} rows"
        v = np.zeros(rows, dtype=NP[column.data_type])
        words = np.full((rows + 63) // 64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        abi.check(lib.hy_column_read_chunk(column.handle, k, v.ctypes.data, words.ctypes.data))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert not bits[rows:].any(), f"chunk {k}: bits behind the last row are set"
        values.append(v)
        nulls.append(bits[:rows].astype(bool))
    if not values:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    return np.concatenate(values), np.concatenate(nulls)


def typed_values(result, a, n):
    return np.frombuffer(result.raw[a].tobytes(), dtype=NP[result.columns[a].data_type])[:n]


def assert_oracle_equal(host, want, n_aggregates, context):
    assert host.n_groups == want.n_groups, f"group count {context}"
    n = want.n_groups
    np.testing.assert_array_equal(host.row_ids[:n], want.row_ids[:n], err_msg=f"group order / representative rows {context}")
    for a in range(n_aggregates if n else 0):   # (cells, as test_aggregate_gpu.py compares them: the oracle cannot type a column of a table without chunks)
        nulls = want.nulls[a][:n].astype(bool)
        np.testing.assert_array_equal(host.nulls[a][:n].astype(bool), nulls, err_msg=f"NULL mismatch aggregate {a} {context}")
        x, y = typed_values(host, a, n)[~nulls], typed_values(want, a, n)[~nulls]
        if y.dtype.kind == "f":
            assert np.all(np.abs(x - y) <= FLOAT_TOLERANCE * np.maximum(1.0, np.abs(y))), f"aggregate {a} {context}"
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"aggregate {a} {context}")


def compare_with_host_call(lib, got, host, n_aggregates, chunk_rows, context):
    """The columns and RowIDs of hy_aggregate_hash_columns against hy_aggregate_hash's host arrays, byte for byte."""
    n = host.n_groups
    assert got.n_groups == n, f"n_groups {context}"
    assert got.row_ids.numpy().tobytes() == host.row_ids[:n].tobytes(), f"representative RowIDs {context}"
    for a in range(n_aggregates):
        column = got.aggregates[a]
        if n:
            assert column.data_type == host.columns[a].data_type, f"aggregate {a}: result type {context}"
        values, nulls = read_chunks(lib, column, n, chunk_rows)
        want = typed_values(host, a, n) if n else np.zeros(0, dtype=np.int64)
        assert values.tobytes() == want.tobytes(), f"aggregate {a}: values {context}"
        np.testing.assert_array_equal(nulls, host.nulls[a][:n].astype(bool), err_msg=f"aggregate {a}: NULL flags {context}")


def check(lib, groupby, aggregates, chunk_rows=CHUNK, context=""):
    """groupby: [Col], aggregates: [(function, Col or None)] -> (host result, columns result), compared three ways."""
    cache = {}

    def dev(col):
        return cache.setdefault(id(col), DeviceColumn(col.host))

    device_groupby = [dev(c) for c in groupby]
    device_aggregates = [(f, dev(c) if c is not None else None) for f, c in aggregates]
    host = aggregate_hash(device_groupby, device_aggregates)
    host_finished = finished_on_device(lib)
    got = aggregate_hash_columns(device_groupby, device_aggregates, chunk_rows)
    assert finished_on_device(lib) == host_finished, f"the two entry points took different finishes {context}"
    compare_with_host_call(lib, got, host, len(aggregates), chunk_rows, context)
    want = oracle_aggregate([c.host for c in groupby], [(f, c.host if c is not None else None) for f, c in aggregates])
    assert_oracle_equal(host, want, len(aggregates), context)
    rows = got.row_ids.numpy().astype(np.int64)
    for g, col in enumerate(groupby):   # the GROUP BY columns at the representative rows
        flat = rows[:, 0] * col.chunk + rows[:, 1]
        values, nulls = read_chunks(lib, got.groupby[g], host.n_groups, chunk_rows)
        expected_nulls = col.nulls[flat] if col.nulls is not None else np.zeros(len(flat), dtype=bool)
        np.testing.assert_array_equal(nulls, expected_nulls, err_msg=f"GROUP BY column {g}: NULL flags {context}")
        np.testing.assert_array_equal(values[~nulls], col.values[flat][~nulls], err_msg=f"GROUP BY column {g}: values {context}")
    got.keep = cache
    return host, got


def quarters(rng, n, dtype, limit=4000):
    return (rng.integers(-limit, limit, n) / 4.0).astype(dtype)


def grouped_table(n_groups, seed, rows_per_group=2, dense=True, key_nulls=False, key_chunk=CHUNK):
    """n_groups keys in shuffled rows; every 64th, every 65th and the last group see only NULL inputs.  dense: an int key whose order is the
    result's (immediate keys); otherwise sparse keys, first-occurrence order."""
    rng = np.random.default_rng(seed)
    group = rng.permutation(np.repeat(np.arange(n_groups, dtype=np.int64), rows_per_group))
    n = len(group)
    key = group.astype(np.int32) if dense else (group * 7919 - 1_000_000).astype(np.int32)
    knull = None
    if key_nulls:
        knull = np.zeros(n, dtype=bool)
        knull[rng.choice(n, 5, replace=False)] = True
    only_nulls = (group % 64 == 0) | (group % 65 == 0) | (group == n_groups - 1)
    vnull = only_nulls | (rng.random(n) < 0.1)
    table = {"key": Col(key, knull, chunk=key_chunk),
             "int": Col(rng.integers(-1000, 1000, n).astype(np.int32), vnull, chunk=key_chunk),
             "long": Col(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), vnull, chunk=key_chunk),
             "float": Col(quarters(rng, n, np.float32), vnull, chunk=key_chunk),
             "double": Col(quarters(rng, n, np.float64, 4_000_000), vnull, chunk=key_chunk)}
    return table


def eight_aggregates(t):
    """MIN / MAX / SUM / AVG / COUNT / COUNT(*) over int, long, float and double inputs: result widths 4 and 8 side by side."""
    return [(abi.AGG_MIN, t["int"]), (abi.AGG_MAX, t["long"]), (abi.AGG_SUM, t["float"]), (abi.AGG_AVG, t["double"]), (abi.AGG_COUNT, t["int"]),
            (abi.AGG_COUNT, None), (abi.AGG_SUM, t["int"]), (abi.AGG_MIN, t["float"])]


@pytest.mark.parametrize("n_groups,on_device", [(STAGED_GROUPS, 0), (STAGED_GROUPS + 1, 1)])
def test_staged_groups_boundary(device, n_groups, on_device):
    t = grouped_table(n_groups, seed=n_groups)
    host, got = check(device, [t["key"]], eight_aggregates(t), CHUNK, f"{n_groups} groups")
    assert got.n_groups == n_groups
    assert finished_on_device(device) == on_device


@pytest.mark.parametrize("n_groups", [65_535, 65_536, 131_071])
def test_chunk_boundaries(device, n_groups):
    t = grouped_table(n_groups, seed=n_groups)
    host, got = check(device, [t["key"]], eight_aggregates(t), CHUNK, f"{n_groups} groups")
    assert got.n_groups == n_groups and finished_on_device(device) == 1
    assert got.aggregates[0].n_chunks == (n_groups + CHUNK - 1) // CHUNK


@pytest.mark.parametrize("chunk_rows,n_groups", [(100, 6_401), (64, 4_160)])
def test_small_chunk_rows(device, chunk_rows, n_groups):
    """100: word tails inside every chunk and a 1-row last chunk; 64: exact words.  Every 64th and 65th group and the last one are all-NULL:
    whole words without a NULL, mixed words and the tail bit."""
    t = grouped_table(n_groups, seed=chunk_rows)
    host, got = check(device, [t["key"]], eight_aggregates(t), chunk_rows, f"chunk_rows {chunk_rows}")
    assert got.n_groups == n_groups and finished_on_device(device) == 1
    assert got.aggregates[0].n_chunks == (n_groups + chunk_rows - 1) // chunk_rows
    assert host.nulls[0][n_groups - 1] == 1 and host.nulls[4][:n_groups].sum() == 0   # the last group: MIN is NULL; COUNT never is


def test_all_null_groups_and_the_null_group_of_a_nullable_key(device):
    t = grouped_table(5_000, seed=3, key_nulls=True, dense=False)
    host, got = check(device, [t["key"]], eight_aggregates(t), 100, "NULL groups")
    assert got.n_groups == 5_001 and finished_on_device(device) == 1
    key_values, key_is_null = read_chunks(device, got.groupby[0], got.n_groups, 100)
    assert key_is_null.sum() == 1
    for a, never_null in enumerate([False, False, False, False, True, True, False, False]):
        nulls = host.nulls[a][:got.n_groups]
        assert (nulls.sum() == 0) if never_null else (155 <= nulls.sum() < 300)   # 155 groups see only NULLs by construction, some more by chance


@pytest.mark.parametrize("order", ["immediate_key", "first_occurrence"])
def test_group_order(device, order):
    t = grouped_table(5_000, seed=11, dense=order == "immediate_key")
    second = Col(np.zeros(len(t["key"].values), dtype=np.int64))
    groupby = [t["key"]] if order == "immediate_key" else [t["key"], second]
    host, got = check(device, groupby, eight_aggregates(t)[:3], CHUNK, order)
    rows = got.row_ids.numpy().astype(np.int64)
    flat = rows[:, 0] * CHUNK + rows[:, 1]
    keys = t["key"].values[flat]
    if order == "immediate_key":
        assert np.all(np.diff(keys) > 0)
    else:
        assert np.all(np.diff(flat) > 0) and not np.all(np.diff(keys) > 0)


def test_host_finished_functions(device):
    """COUNT(DISTINCT), STDDEV_SAMP and ANY are finished on the host and uploaded: 5 000 groups, two chunk sizes."""
    t = grouped_table(5_000, seed=5, rows_per_group=3)
    aggregates = [(abi.AGG_COUNT_DISTINCT, t["int"]), (abi.AGG_STDDEV_SAMP, t["double"]), (abi.AGG_ANY, t["long"]), (abi.AGG_SUM, t["int"]), (abi.AGG_ANY, t["float"])]
    for chunk_rows in (CHUNK, 100):
        host, got = check(device, [t["key"]], aggregates, chunk_rows, f"host finish, chunk_rows {chunk_rows}")
        assert got.n_groups == 5_000 and finished_on_device(device) == 0


def test_more_aggregates_than_one_pass(device):
    t = grouped_table(5_000, seed=6)
    aggregates = eight_aggregates(t) + [(abi.AGG_MAX, t["int"]), (abi.AGG_STDDEV_SAMP, t["int"])]
    host, got = check(device, [t["key"]], aggregates, 1000, "ten aggregates")
    assert got.n_groups == 5_000


def test_no_group_by(device):
    t = grouped_table(500, seed=7)
    aggregates = eight_aggregates(t)
    host, got = check(device, [], aggregates, CHUNK, "no GROUP BY, 1000 rows")
    assert got.n_groups == 1 and got.column(5) == [1000]
    empty = {name: Col(col.values[:0], None if col.nulls is None else col.nulls[:0]) for name, col in t.items()}
    host, got = check(device, [], eight_aggregates(empty), CHUNK, "no GROUP BY, no rows")
    assert got.n_groups == 1 and got.aggregates[0].n_chunks == 1
    assert got.column(0) == [None] and got.column(4) == [0] and got.column(5) == [0]
    host, got = check(device, [empty["key"]], eight_aggregates(empty), CHUNK, "GROUP BY, no rows")
    assert got.n_groups == 0 and got.aggregates[0].n_chunks == 0 and got.groupby[0].n_chunks == 0 and got.row_ids.rows == 0


def test_reference_input_with_device_pos_lists(device):
    """The aggregate over the reference table a scan leaves in HBM (HY_MEM_DEVICE reference columns): 200 000 rows, 5 000 groups."""
    import torch
    from hyrise_amd.distributed import HipExecutor
    rng = np.random.default_rng(21)
    n, chunk, n_groups = 200_000, 40_000, 5_000
    key = rng.integers(0, n_groups, n).astype(np.int32) * 3
    pick = (rng.random(n) < 0.7).astype(np.int32)
    value = rng.integers(-1000, 1000, n).astype(np.int32)
    price = quarters(rng, n, np.float64)
    vnull = rng.random(n) < 0.1
    host = {"key": storage.make_column(key, None, abi.ENC_DICTIONARY, chunk), "value": storage.make_column(value, vnull, abi.ENC_UNENCODED, chunk),
            "price": storage.make_column(price, None, abi.ENC_UNENCODED, chunk), "pick": storage.make_column(pick, None, abi.ENC_UNENCODED, chunk)}
    data = {name: DeviceColumn(column) for name, column in host.items()}
    predicate = make_predicate(abi.PRED_EQUALS, abi.TYPE_INT, 1)
    ex = HipExecutor(torch.device("cuda:0"))
    lists = ex.scan_chunked(data["pick"], predicate)
    ref = {name: ex.reference_column_chunked(column, lists) for name, column in data.items()}
    on_host = table_scan(data["pick"], predicate)
    host_lists = [on_host.pos_list(c).copy() for c in range(data["pick"].n_chunks)]
    host_ref = {name: storage.make_reference_column(column, host_lists, list(range(column.n_chunks))) for name, column in host.items()}

    def aggregates(columns):
        return [(abi.AGG_SUM, columns["value"]), (abi.AGG_AVG, columns["price"]), (abi.AGG_COUNT, None), (abi.AGG_MIN, columns["value"]), (abi.AGG_MAX, columns["price"])]

    result = aggregate_hash([ref["key"]], aggregates(ref))
    got = aggregate_hash_columns([ref["key"]], aggregates(ref), 1000)
    assert finished_on_device(device) == 1 and got.n_groups == n_groups
    compare_with_host_call(device, got, result, 5, 1000, "reference input")
    assert_oracle_equal(result, oracle_aggregate([host_ref["key"]], aggregates(host_ref)), 5, "reference input")
    sizes = np.array([len(rows) for rows in host_lists], dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(sizes)])
    rows = got.row_ids.numpy().astype(np.int64)
    kept = np.flatnonzero(pick == 1)
    key_values, key_nulls = read_chunks(device, got.groupby[0], n_groups, 1000)
    np.testing.assert_array_equal(key_values, key[kept[base[rows[:, 0]] + rows[:, 1]]])
    assert not key_nulls.any()


@pytest.mark.parametrize("n_columns", [6, 10])
def test_wide_group_by(device, n_columns):
    """Six and ten GROUP BY columns: the nine- and seventeen-word builds behind the same entry point."""
    t = grouped_table(5_000, seed=n_columns, dense=False)
    n = len(t["key"].values)
    others = [Col(np.zeros(n, dtype=np.int32 if i % 2 else np.int64) + i) for i in range(n_columns - 1)]
    host, got = check(device, [t["key"]] + others, eight_aggregates(t)[:4], 1000, f"{n_columns} GROUP BY columns")
    assert got.n_groups == 5_000 and finished_on_device(device) == 1


def test_seventeen_group_by_columns_are_unsupported(device):
    t = grouped_table(10, seed=1)
    columns = [DeviceColumn(t["key"].host) for _ in range(17)]
    with pytest.raises(abi.HyriseAmdError):
        aggregate_hash_columns(columns, [(abi.AGG_COUNT, None)])


def test_string_group_by_column_as_key_names(device):
    """A string GROUP BY column passed as key names gets no output column (its handle is NULL: the adapter reads the strings through the
    representative rows); the other columns are there and the RowIDs are the host call's."""
    rng = np.random.default_rng(9)
    n, n_groups, chunk = 12_000, 5_000, 5_000
    group = rng.permutation(np.repeat(np.arange(n_groups), 3))[:n]
    strings = np.array([f"name{g:05d}" for g in group], dtype=object)
    segments, dictionaries = encode_string_column(strings, None, chunk)
    names = AggregateKeyNames().dictionary_column(segments, dictionaries)
    other = Col((group % 7).astype(np.int32), chunk=chunk)
    value = Col(rng.integers(0, 100, n).astype(np.int32), chunk=chunk)
    device_names, device_other, device_value = DeviceColumn(names), DeviceColumn(other.host), DeviceColumn(value.host)
    aggregates = [(abi.AGG_SUM, device_value), (abi.AGG_COUNT, None)]
    host = aggregate_hash([device_names, device_other], aggregates)
    got = aggregate_hash_columns([device_names, device_other], aggregates, 1000, key_name_columns=[0])
    assert got.n_groups == len(np.unique(group)) > STAGED_GROUPS
    compare_with_host_call(device, got, host, 2, 1000, "string key")
    assert got.groupby[0] is None and got.groupby[1] is not None
    rows = got.row_ids.numpy().astype(np.int64)
    flat = rows[:, 0] * chunk + rows[:, 1]
    assert np.all(np.diff(flat) > 0), "first-occurrence order"
    assert len(set(strings[flat])) == got.n_groups
    other_values, _ = read_chunks(device, got.groupby[1], got.n_groups, 1000)
    np.testing.assert_array_equal(other_values, other.values[flat])
    sums = {}
    for s, v in zip(strings, value.values):
        sums[s] = sums.get(s, 0) + int(v)
    assert got.column(0) == [sums[s] for s in strings[flat]]


@pytest.fixture(scope="module")
def chained(device):
    """One aggregate whose columns the chaining tests read: GROUP BY key, SUM(int), COUNT(*) over 6 000 groups, 1000-row chunks."""
    lib = device
    t = grouped_table(6_000, seed=31, rows_per_group=4, key_nulls=True)
    host, got = check(lib, [t["key"]], [(abi.AGG_SUM, t["int"]), (abi.AGG_COUNT, None)], 1000, "chaining")
    n = got.n_groups
    sums = np.frombuffer(host.raw[0].tobytes(), dtype=np.int64)[:n].copy()
    sum_nulls = host.nulls[0][:n].astype(bool)
    rows = host.row_ids[:n].astype(np.int64)
    flat = rows[:, 0] * CHUNK + rows[:, 1]
    yield {"table": t, "got": got, "n": n, "sums": sums, "sum_nulls": sum_nulls, "keys": t["key"].values[flat], "key_nulls": t["key"].nulls[flat]}
    for column in got.aggregates + got.groupby:
        column.close()
    got.row_ids.close()


def test_chain_having_scan(device, chained):
    result = table_scan(chained["got"].aggregates[0], make_predicate(abi.PRED_GREATER_THAN, abi.TYPE_LONG, 500))
    matches = result.matches[:result.total].astype(np.int64)
    np.testing.assert_array_equal(matches[:, 0] * 1000 + matches[:, 1], np.flatnonzero((chained["sums"] > 500) & ~chained["sum_nulls"]))
    assert result.total > 100


@pytest.mark.parametrize("limit", [None, 10])
def test_chain_sort(device, chained, limit):
    got, n = chained["got"], chained["n"]
    modes = [abi.SORT_DESCENDING_NULLS_FIRST, abi.SORT_ASCENDING_NULLS_FIRST]
    positions = sort([got.aggregates[0], got.groupby[0]], modes, limit=limit)
    order = sorted_order([(chained["sums"], chained["sum_nulls"]), (chained["keys"], chained["key_nulls"])], modes)
    want = positions_of(order[:limit], [min(1000, n - b) for b in range(0, n, 1000)])
    assert positions.numpy().tobytes() == want.tobytes()


def test_chain_join(device, chained):
    """The gathered key column as build side against the original key column: every input row with a key finds its group."""
    key = chained["table"]["key"]
    pairs = join_hash(chained["got"].groupby[0], DeviceColumn(key.host), abi.JOIN_INNER)
    assert pairs.n_pairs == int((~key.nulls).sum())

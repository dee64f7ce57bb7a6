"""JoinSortMerge on the device (hy_join_sort_merge, hy_join_sort_merge_count): both lists, n_pairs, n_matched and n_left_outer byte for byte
against tests/join_sort_merge_oracle.py's restatement of the order contract, with host-memory and device-memory results."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import join_hash, join_sort_merge, make_predicate, table_scan
from hyrise_amd.storage import DeviceColumn
from join_sort_merge_oracle import ACCEPTED, CONDITIONS, MODES, ordered_join, row_ids

pytestmark = pytest.mark.gpu

EQ, NE, LT, LE, GT, GE = CONDITIONS
INNER, LEFT, RIGHT, FULL = MODES
MEMS = [abi.MEM_HOST, abi.MEM_DEVICE]
SENTINEL = 0xA5A5A5A5


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    encoding = {"value": abi.ENC_UNENCODED, "dictionary": abi.ENC_DICTIONARY, "frame_of_reference": abi.ENC_FRAME_OF_REFERENCE}[kind]
    return storage.encode_segment(values, nulls, encoding)


def sizes_of(n, chunk):
    """chunk: rows per chunk, or the list of chunk sizes itself."""
    return list(chunk) if isinstance(chunk, (list, tuple)) else [min(chunk, n - b) for b in range(0, n, chunk)]


class Side:
    """One join input: its values and NULL flags in row order, the chunk sizes, and the column on the device."""

    def __init__(self, values, nulls=None, chunk=1000, kind="value"):
        self.values, self.nulls, self.sizes = values, nulls, sizes_of(len(values), chunk)
        segments, begin = [], 0
        for size in self.sizes:
            segments.append(segment_of(values[begin:begin + size], None if nulls is None else nulls[begin:begin + size], kind))
            begin += size
        if not segments:   # no rows: one empty chunk, so that the column still has its type
            segments, self.sizes = [segment_of(values, None if nulls is None else nulls, kind)], [0]
        self.host = storage.HostColumn(segments, storage.TYPE_OF_NP[np.dtype(values.dtype)])
        self.column = DeviceColumn(self.host)


def call(lib, left, right, mode, condition, mem, capacity):
    """hy_join_sort_merge into lists of `capacity` RowIDs pre-filled with SENTINEL -> (status, result struct, left list, right list)."""
    lists = [np.full((max(1, capacity), 2), SENTINEL, dtype=np.uint32) for _ in range(2)]
    result = abi.SortMergeResult()
    result.mem, result.capacity = mem, capacity
    pointers = []
    if mem == abi.MEM_DEVICE:
        for host in lists:
            pointer = C.c_void_p()
            abi.check(lib.hy_device_malloc(C.byref(pointer), host.nbytes))
            abi.check(lib.hy_memcpy_h2d(pointer, host.ctypes.data, host.nbytes))
            pointers.append(pointer)
        result.left_pos, result.right_pos = pointers[0].value, pointers[1].value
    else:
        result.left_pos, result.right_pos = lists[0].ctypes.data, lists[1].ctypes.data
    status = lib.hy_join_sort_merge(left.handle, right.handle, mode, condition, C.byref(result))
    for host, pointer in zip(lists, pointers):
        abi.check(lib.hy_memcpy_d2h(host.ctypes.data, pointer, host.nbytes))
        abi.check(lib.hy_device_free(pointer))
    return status, result, lists[0], lists[1]


def check(lib, left, right, mode, condition, context="", mems=MEMS, columns=None):
    """left / right: Side.  The call's five outputs against the oracle's bytes; hy_join_sort_merge_count agrees.  -> the oracle's output."""
    want = ordered_join(left.values, left.nulls, right.values, right.nulls, mode, condition)
    want_left, want_right = row_ids(want[0], left.sizes), row_ids(want[1], right.sizes)
    n = len(want[0])
    left_column, right_column = columns or (left.column, right.column)
    counted = C.c_uint64(0)
    abi.check(lib.hy_join_sort_merge_count(left_column.handle, right_column.handle, mode, condition, C.byref(counted)))
    assert counted.value == n, f"{context}: hy_join_sort_merge_count"
    for mem in mems:
        where = f"{context} mode={mode} condition={condition} mem={mem}"
        status, result, got_left, got_right = call(lib, left_column, right_column, mode, condition, mem, n)
        assert status == abi.OK, f"{where}: {lib.hy_last_error().decode()}"
        print(f"{where}: n_pairs {result.n_pairs} n_matched {result.n_matched} n_left_outer {result.n_left_outer}")
        assert (result.n_pairs, result.n_matched, result.n_left_outer) == (n, want[2], want[3]), where
        for name, got, expected in (("left_pos", got_left[:n], want_left), ("right_pos", got_right[:n], want_right)):
            if got.tobytes() != expected.tobytes():
                bad = int(np.flatnonzero(np.any(got != expected, axis=1))[0])
                pytest.fail(f"{where}: {name} differs first at output row {bad}: got {got[bad]}, want {expected[bad]}")
    return want


def modes_of(condition):
    return [mode for mode, c in ACCEPTED if c == condition]


@pytest.fixture(scope="module")
def general():
    rng = np.random.default_rng(42)
    return rng.integers(0, 64, 3000).astype(np.int32), rng.integers(0, 64, 2000).astype(np.int32)


@pytest.mark.parametrize("condition", CONDITIONS)
def test_general_every_condition_and_mode(device, general, condition):
    """3 000 x 2 000 rows, keys uniform in [0, 64): about 3 M pairs for <; chunks of 1 000, 1 999 and 1 rows."""
    left_values, right_values = general
    left, right = Side(left_values, chunk=1000), Side(right_values, chunk=[1999, 1])
    for mode in modes_of(condition):
        check(device, left, right, mode, condition, "general")
    if condition in (EQ, LT):   # (the chunk layout only changes the written RowIDs)
        check(device, Side(left_values, chunk=1999), Side(right_values, chunk=1), FULL if condition == EQ else INNER, condition, "general, 1-row chunks")
        check(device, Side(left_values, chunk=1), Side(right_values, chunk=1000), LEFT, condition, "general, 1-row chunks left")


def test_one_row_with_many_partners(device):
    """5 left rows x 40 000 right rows, >=, all match: every left row's range spans 20 emit tiles."""
    left = Side(np.array([7, 9, 8, 9, 7], dtype=np.int32))
    right = Side(np.random.default_rng(1).integers(0, 8, 40_000).astype(np.int32), chunk=9_001)
    want = check(device, left, right, INNER, GE, "many partners")
    assert want[2] == 200_000


def test_long_stretch_of_left_rows_without_partners(device):
    """50 000 left rows of which 10 have 3 partners each and the others none."""
    rng = np.random.default_rng(2)
    left_values = np.arange(50_000, dtype=np.int32) * 2
    lucky = np.sort(rng.choice(50_000, 10, replace=False))
    right_values = np.concatenate([np.repeat(left_values[lucky], 3), np.full(5, -1, dtype=np.int32)]).astype(np.int32)
    rng.shuffle(right_values)
    left, right = Side(left_values, chunk=8_192), Side(right_values, chunk=7)
    for mode in (INNER, FULL):
        want = check(device, left, right, mode, EQ, "empty stretch")
        assert want[2] == 30 and (mode == INNER or (want[3], len(want[0])) == (49_990, 30 + 49_990 + 5))


def test_one_run_of_duplicates(device):
    """300 x 300 rows of one key: =, <=, >= give 90 000 pairs, <, > and <> none."""
    left, right = Side(np.full(300, 5, dtype=np.int32), chunk=128), Side(np.full(300, 5, dtype=np.int32), chunk=299)
    for mode, condition in ACCEPTED:
        want = check(device, left, right, mode, condition, "one key")
        assert want[2] == (90_000 if condition in (EQ, LE, GE) else 0)


def test_duplicate_run_longer_than_the_lds_window(device):
    """20 000 equal right keys under a tile of left keys: the bounds search leaves LDS for global memory; neighbours on both sides."""
    rng = np.random.default_rng(3)
    left = Side(rng.integers(9, 12, 40).astype(np.int32))
    right = Side(np.concatenate([np.full(20_000, 10), rng.integers(0, 20, 500)]).astype(np.int32), chunk=4_096)
    for condition in (EQ, LT, NE):
        check(device, left, right, INNER, condition, "long run")
    left64 = Side(left.values.astype(np.int64) << 33)
    right64 = Side(right.values.astype(np.int64) << 33, chunk=4_096)
    check(device, left64, right64, FULL, EQ, "long run, int64")


@pytest.mark.parametrize("mode", [LEFT, RIGHT, FULL])
def test_nulls_on_both_sides(device, mode):
    rng = np.random.default_rng(4)
    left = Side(rng.integers(0, 300, 20_000).astype(np.int32), rng.random(20_000) < 0.2, chunk=8_191)
    right = Side(rng.integers(100, 400, 9_000).astype(np.int32), rng.random(9_000) < 0.2, chunk=3_000)
    for condition in (EQ, LE, GT):
        check(device, left, right, mode, condition, "20 % NULLs")


def test_all_null_and_empty_sides(device):
    rng = np.random.default_rng(5)
    some = Side(rng.integers(0, 10, 100).astype(np.int32), rng.random(100) < 0.2, chunk=33)
    all_null = Side(np.zeros(70, dtype=np.int32), np.ones(70, dtype=bool), chunk=64)
    empty = Side(np.zeros(0, dtype=np.int32))
    one = Side(np.array([3], dtype=np.int32))
    one_null = Side(np.array([3], dtype=np.int32), np.array([True]))
    for left, right in ((some, all_null), (all_null, some), (all_null, all_null), (some, empty), (empty, some), (empty, empty), (one, some), (some, one), (one_null, one),
                        (one, one)):
        for mode, condition in ACCEPTED:
            if condition in (EQ, LT, GE, NE):
                check(device, left, right, mode, condition, "degenerate sides")


def test_types(device):
    rng = np.random.default_rng(6)
    high = (rng.integers(-3, 4, 5_000).astype(np.int64) << 32) + 5             # differ only in the high word
    negative = rng.integers(-50, 50, 4_000).astype(np.int64) * 1_000_003 - (1 << 40)
    zeros = np.array([-0.0, 0.0, 1.5, -1.5, 0.0, -0.0, np.inf, -np.inf] * 40)
    doubles = np.round(rng.normal(0, 3, 3_000), 0)
    nulls = rng.random(3_000) < 0.1
    cases = [(Side(high, chunk=999), Side(high[:1_200][::-1].copy(), chunk=500)),
             (Side(negative, chunk=4_000), Side(np.concatenate([negative[:900], high[:100]]), chunk=512)),
             (Side(rng.integers(-40, 40, 2_000).astype(np.int32)), Side(rng.integers(-40, 40, 1_500).astype(np.int32))),
             (Side(zeros.astype(np.float32), chunk=100), Side(zeros[::-1].astype(np.float32), chunk=77)),
             (Side(zeros.astype(np.float64), chunk=100), Side(zeros[::3].astype(np.float64), chunk=77)),
             (Side(doubles, nulls, chunk=1_024), Side((doubles[:2_000] * -1 + 0.0), nulls[:2_000], chunk=700))]
    for left, right in cases:
        for mode, condition in ((INNER, EQ), (FULL, EQ), (FULL, LT), (LEFT, GE), (INNER, NE), (RIGHT, GT)):
            check(device, left, right, mode, condition, str(left.values.dtype))


@pytest.mark.parametrize("kind,dtype,domain", [("value", np.int32, 50), ("dictionary", np.int32, 100), ("dictionary", np.int64, 700), ("frame_of_reference", np.int32, 300),
                                               ("run_length", np.float64, 20)])
def test_encodings(device, kind, dtype, domain):
    """Dictionary with 1- and 2-byte value ids (100 / 700 distinct values per chunk)."""
    rng = np.random.default_rng(domain)
    left = Side(rng.integers(0, domain, 6_000).astype(dtype), rng.random(6_000) < 0.05, chunk=3_000, kind=kind)
    right = Side(rng.integers(0, domain, 5_000).astype(dtype), None, chunk=2_500, kind=kind)
    if kind == "dictionary":
        assert {s.width for s in left.host.segments} == {1 if domain < 255 else 2}
    for mode, condition in ((FULL, EQ), (INNER, LT) if domain >= 300 else (LEFT, GT)):
        check(device, left, right, mode, condition, kind)


def test_reference_column_over_a_scan_s_device_pos_lists(device):
    """The left input is the reference table a hy_table_scan leaves in HBM: one PosList per chunk that has matches, read in place."""
    import torch
    from hyrise_amd.distributed import HipExecutor
    rng = np.random.default_rng(8)
    n, chunk = 30_000, 7_000
    keys = rng.integers(0, 500, n).astype(np.int32)
    key_nulls = rng.random(n) < 0.1
    pick = (rng.random(n) < 0.3).astype(np.int32)
    pick[chunk:2 * chunk] = 0   # (a chunk without matches: no output chunk)
    data = {"key": DeviceColumn(storage.make_column(keys, key_nulls, abi.ENC_DICTIONARY, chunk)), "pick": DeviceColumn(storage.make_column(pick, None, abi.ENC_UNENCODED, chunk))}
    ex = HipExecutor(torch.device("cuda:0"))
    lists = ex.scan_chunked(data["pick"], make_predicate(abi.PRED_EQUALS, abi.TYPE_INT, 1))
    reference = ex.reference_column_chunked(data["key"], lists)
    assert reference.n_chunks == 4
    kept = np.flatnonzero(pick == 1)
    left = Side.__new__(Side)
    left.values, left.nulls, left.sizes = keys[kept], key_nulls[kept], [int(c) for c in lists.count if c]
    right = Side(rng.integers(0, 500, 4_000).astype(np.int32), rng.random(4_000) < 0.1, chunk=1_500)
    for mode, condition in ((FULL, EQ), (LEFT, LT), (INNER, NE)):
        check(device, left, right, mode, condition, "scan output", columns=(reference, right.column))
        mirrored = {LT: GT, EQ: EQ, NE: NE}[condition]
        check(device, right, left, {LEFT: RIGHT}.get(mode, mode), mirrored, "scan output on the right", columns=(right.column, reference))


def test_inner_equals_finds_join_hash_s_pairs(device, general):
    left, right = Side(general[0], chunk=1000), Side(general[1], chunk=[1999, 1])
    hashed = join_hash(left.column, right.column, abi.JOIN_INNER)
    merged = join_sort_merge(left.column, right.column, abi.JOIN_INNER, abi.PRED_EQUALS)
    merged_left, merged_right = merged.numpy()
    assert merged.n_pairs == merged.n_matched == hashed.n_pairs and merged.n_left_outer == 0

    def ordered(left_list, right_list):
        rows = np.concatenate([left_list, right_list], axis=1).astype(np.int64)
        return rows[np.lexsort(rows.T[::-1])]

    assert ordered(merged_left, merged_right).tobytes() == ordered(hashed.left[:hashed.n_pairs], hashed.right[:hashed.n_pairs]).tobytes()
    merged.close()


@pytest.mark.parametrize("mem", MEMS)
def test_capacity(device, general, mem):
    """capacity = needed - 1: HY_ERR_CAPACITY, the needed counts reported, both lists untouched."""
    left = Side(general[0][:500], np.arange(500) % 7 == 0, chunk=200)
    right = Side(general[1][:400] + 30, np.arange(400) % 5 == 0, chunk=150)
    for mode, condition in ((INNER, LT), (FULL, EQ), (LEFT, GE), (RIGHT, EQ)):
        want = ordered_join(left.values, left.nulls, right.values, right.nulls, mode, condition)
        needed = len(want[0])
        status, result, got_left, got_right = call(device, left.column, right.column, mode, condition, mem, needed - 1)
        assert status == abi.ERR_CAPACITY and device.hy_last_error()
        assert (result.n_pairs, result.n_matched, result.n_left_outer) == (needed, want[2], want[3])
        assert (got_left == SENTINEL).all() and (got_right == SENTINEL).all()
    status, result, _, _ = call(device, left.column, right.column, FULL, EQ, mem, 0)
    assert status == abi.ERR_CAPACITY and result.n_pairs > 0


def test_refusals(device):
    ints, longs = Side(np.arange(10, dtype=np.int32)), Side(np.arange(10, dtype=np.int64))
    segments, _ = __import__("hyrise_amd.string_keys", fromlist=["encode_string_column"]).encode_string_column(["a", "b", "c"], np.zeros(3, dtype=bool), 3)
    strings = DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))
    refused = [(ints.column, ints.column, mode, EQ) for mode in (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE, abi.JOIN_CROSS)]
    refused += [(ints.column, ints.column, mode, NE) for mode in (LEFT, RIGHT, FULL)]
    refused += [(ints.column, longs.column, INNER, EQ), (longs.column, ints.column, FULL, LT), (strings, strings, INNER, EQ), (ints.column, strings, INNER, LT)]
    for left, right, mode, condition in refused:
        status, result, _, _ = call(device, left, right, mode, condition, abi.MEM_HOST, 100)
        assert status == abi.ERR_UNSUPPORTED, (mode, condition)
        assert device.hy_last_error()
        counted = C.c_uint64(0)
        assert device.hy_join_sort_merge_count(left.handle, right.handle, mode, condition, C.byref(counted)) == abi.ERR_UNSUPPORTED
        assert device.hy_last_error()


def test_refuses_a_side_of_two_to_the_32_rows(device):
    """65 538 chunks of 65 535 rows over ONE device buffer (HY_MEM_DEVICE: nothing is copied): 2^32 + 65 534 rows, refused before any kernel."""
    import torch
    values = torch.zeros(65_535, dtype=torch.int32, device="cuda:0")
    n_chunks = 65_538
    segments = (abi.Segment * n_chunks)()
    for s in segments:
        s.encoding, s.data_type, s.size, s.width, s.data, s.ref_chunk_id = abi.ENC_UNENCODED, abi.TYPE_INT, 65_535, 4, values.data_ptr(), abi.INVALID_CHUNK_ID
    handle = C.c_void_p()
    abi.check(device.hy_column_create(segments, n_chunks, abi.MEM_DEVICE, C.byref(handle)))
    small = Side(np.arange(10, dtype=np.int32))
    try:
        for left, right in ((handle, small.column.handle), (small.column.handle, handle)):
            counted = C.c_uint64(0)
            assert device.hy_join_sort_merge_count(left, right, INNER, EQ, C.byref(counted)) == abi.ERR_UNSUPPORTED
            assert b"rows" in device.hy_last_error()
    finally:
        device.hy_column_destroy(handle)


def test_a_column_without_chunks_joins_with_any_type(device):
    """An input table without rows has no chunks, and its column no type of its own: every row of the other side is unmatched."""
    handle = C.c_void_p()
    abi.check(device.hy_column_create((abi.Segment * 1)(), 0, abi.MEM_HOST, C.byref(handle)))

    class Empty:
        pass

    empty = Empty()
    empty.handle = handle
    some = Side(np.array([1.5, -0.0, 2.5], dtype=np.float32), np.array([False, True, False]), chunk=2)
    try:
        for mem in MEMS:
            status, result, left, right = call(device, empty, some.column, FULL, LT, mem, 3)
            assert status == abi.OK, device.hy_last_error()
            assert (result.n_pairs, result.n_matched, result.n_left_outer) == (3, 0, 0)
            assert left.tolist() == [[0xFFFFFFFF] * 2] * 3 and right.tolist() == [[0, 0], [0, 1], [1, 0]]
            status, result, left, right = call(device, some.column, empty, LEFT, EQ, mem, 3)
            assert status == abi.OK and (result.n_pairs, result.n_matched, result.n_left_outer) == (3, 0, 3)
            assert right.tolist() == [[0xFFFFFFFF] * 2] * 3 and left.tolist() == [[0, 0], [0, 1], [1, 0]]
            status, result, _, _ = call(device, some.column, empty, INNER, GE, mem, 3)
            assert status == abi.OK and result.n_pairs == 0
    finally:
        device.hy_column_destroy(handle)

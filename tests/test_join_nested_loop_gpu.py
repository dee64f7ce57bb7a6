"""JoinNestedLoop on the device (hy_join_nested_loop, hy_join_nested_loop_count): both lists and n_pairs byte for byte against
tests/join_nested_loop_oracle.py's restatement of the reference's walk, with host-memory and device-memory results."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import join_nested_loop, join_predicates, make_predicate
from hyrise_amd.storage import DeviceColumn
from join_nested_loop_oracle import CONDITIONS, MODES, SEMI_ANTI, nested_loop_join, row_ids

pytestmark = pytest.mark.gpu

EQ, NE, LT, LE, GT, GE = CONDITIONS
INNER, LEFT, RIGHT, FULL, SEMI, ANTI_FALSE, ANTI_TRUE = MODES
MEMS = [abi.MEM_HOST, abi.MEM_DEVICE]
SENTINEL = 0xA5A5A5A5
NP_TYPES = [np.int32, np.int64, np.float32, np.float64]


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    if kind.startswith("bit_packed_"):
        return storage.bit_pack_segment(segment_of(values, nulls, kind[len("bit_packed_"):]))
    encoding = {"value": abi.ENC_UNENCODED, "dictionary": abi.ENC_DICTIONARY, "frame_of_reference": abi.ENC_FRAME_OF_REFERENCE}[kind]
    return storage.encode_segment(values, nulls, encoding)


def sizes_of(n, chunk):
    """chunk: rows per chunk, or the list of chunk sizes itself."""
    return list(chunk) if isinstance(chunk, (list, tuple)) else [min(chunk, n - b) for b in range(0, n, chunk)]


class Table:
    """One join input: columns [(values, nulls or None), ...] in row order, the chunk sizes, and every column on the device."""

    def __init__(self, columns, chunk=1000, kind="value"):
        self.columns = [(np.asarray(values), nulls) for values, nulls in columns]
        n = len(self.columns[0][0])
        self.sizes = sizes_of(n, chunk) or [0]   # no rows: one empty chunk, so that the columns still have their types
        self.device, self.host = [], []
        for values, nulls in self.columns:
            segments, begin = [], 0
            for size in self.sizes:
                segments.append(segment_of(values[begin:begin + size], None if nulls is None else nulls[begin:begin + size], kind))
                begin += size
            self.host.append(storage.HostColumn(segments, storage.TYPE_OF_NP[np.dtype(values.dtype)]))
            self.device.append(DeviceColumn(self.host[-1]))


def call(lib, left, right, mode, predicates, mem, capacity):
    """left / right: Table; predicates: [(left column index, condition, right column index)], the first one the primary.  hy_join_nested_loop
    into lists of `capacity` RowIDs pre-filled with SENTINEL -> (status, result struct, left list, right list)."""
    lists = [np.full((max(1, capacity), 2), SENTINEL, dtype=np.uint32) for _ in range(2)]
    result = abi.NestedLoopResult()
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
    secondary, n_secondary = join_predicates([(left.device[l], c, right.device[r]) for l, c, r in predicates[1:]])
    primary = predicates[0]
    status = lib.hy_join_nested_loop(left.device[primary[0]].handle, right.device[primary[2]].handle, mode, primary[1], secondary, n_secondary, C.byref(result))
    for host, pointer in zip(lists, pointers):
        abi.check(lib.hy_memcpy_d2h(host.ctypes.data, pointer, host.nbytes))
        abi.check(lib.hy_device_free(pointer))
    return status, result, lists[0], lists[1]


def count(lib, left, right, mode, predicates):
    secondary, n_secondary = join_predicates([(left.device[l], c, right.device[r]) for l, c, r in predicates[1:]])
    primary = predicates[0]
    counted = C.c_uint64(0)
    abi.check(lib.hy_join_nested_loop_count(left.device[primary[0]].handle, right.device[primary[2]].handle, mode, primary[1], secondary, n_secondary, C.byref(counted)))
    return counted.value


def check(lib, left, right, mode, predicates, context="", mems=MEMS, oracle_tables=None):
    """The call's lists against the oracle's bytes; hy_join_nested_loop_count agrees.  -> the oracle's output."""
    if isinstance(predicates, int):
        predicates = [(0, predicates, 0)]
    oracle_left, oracle_right = oracle_tables or (left, right)
    want = nested_loop_join(oracle_left.columns, oracle_right.columns, oracle_left.sizes, oracle_right.sizes, mode, predicates)
    want_left = row_ids(want[0], oracle_left.sizes)
    want_right = None if want[1] is None else row_ids(want[1], oracle_right.sizes)
    n = len(want[0])
    assert count(lib, left, right, mode, predicates) == n, f"{context}: hy_join_nested_loop_count, mode={mode} predicates={predicates}"
    for mem in mems:
        where = f"{context} mode={mode} predicates={predicates} mem={mem}"
        status, result, got_left, got_right = call(lib, left, right, mode, predicates, mem, n)
        assert status == abi.OK, f"{where}: {lib.hy_last_error().decode()}"
        assert result.n_pairs == n, where
        for name, got, expected in (("left_pos", got_left[:n], want_left), ("right_pos", got_right[:n], want_right)):
            if expected is None:   # Semi / Anti: right_pos is not written
                assert (got_right == SENTINEL).all(), where
            elif got.tobytes() != expected.tobytes():
                bad = int(np.flatnonzero(np.any(got != expected, axis=1))[0])
                pytest.fail(f"{where}: {name} differs first at output row {bad} of {n}: got {got[bad]}, want {expected[bad]}")
    return want


@pytest.fixture(scope="module")
def general():
    """257 x 130 rows of int, 10 % NULLs on each side, chunks of 100 (left) and 64 (right): a partial outer tile, a partial strip, an exact
    strip and several chunk pairs.  Columns 1 .. 4: secondary operands of four types."""
    rng = np.random.default_rng(42)
    left = [(rng.integers(0, 40, 257).astype(np.int32), rng.random(257) < 0.1), (rng.integers(0, 6, 257).astype(np.int64), rng.random(257) < 0.1),
            (rng.integers(0, 6, 257).astype(np.float32), None), (rng.integers(0, 6, 257).astype(np.float64), rng.random(257) < 0.05), (rng.integers(0, 3, 257).astype(np.int32), None)]
    right = [(rng.integers(0, 40, 130).astype(np.int32), rng.random(130) < 0.1), (rng.integers(0, 6, 130).astype(np.int32), rng.random(130) < 0.1),
             (rng.integers(0, 6, 130).astype(np.float64), None), (rng.integers(0, 6, 130).astype(np.int64), rng.random(130) < 0.05), (rng.integers(0, 3, 130).astype(np.float32), None)]
    return Table(left, chunk=100), Table(right, chunk=64)


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_and_condition(device, general, mode):
    for condition in CONDITIONS:
        check(device, general[0], general[1], mode, condition, "general")


@pytest.fixture(scope="module")
def edge_values():
    rng = np.random.default_rng(7)
    return rng.integers(0, 50, 1025).astype(np.int32), rng.integers(0, 50, 4097).astype(np.int32)


@pytest.fixture(scope="module")
def edge_right_tables(edge_values):
    return {(rows, chunk): Table([(edge_values[1][:rows], None)], chunk=chunk) for rows in (0, 1, 63, 64, 65, 4097) for chunk in (5000, 7)}


@pytest.mark.parametrize("left_rows", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_tile_edges(device, edge_values, edge_right_tables, left_rows):
    """Left rows around the wave and the tile, right rows around the strip, in one chunk each and in chunks of 3 and 7."""
    for left_chunk, right_chunk in ((2000, 5000), (3, 7)):
        left = Table([(edge_values[0][:left_rows], None)], chunk=left_chunk)
        for right_rows in (0, 1, 63, 64, 65, 4097):
            right = edge_right_tables[right_rows, right_chunk]
            check(device, left, right, INNER, LT, f"{left_rows} x {right_rows}", mems=[abi.MEM_DEVICE])
            check(device, left, right, FULL, EQ, f"{left_rows} x {right_rows}", mems=[abi.MEM_DEVICE])


def test_dense_and_empty_matches(device):
    """Every pair matches (>= against a constant column, 300 x 200): full 64-lane stores, running counts across strips.  And nothing matches."""
    left, right = Table([(np.full(300, 5, dtype=np.int32), None)], chunk=128), Table([(np.full(200, 5, dtype=np.int32), None)], chunk=77)
    for mode in MODES:
        want = check(device, left, right, mode, GE, "dense")
        assert len(want[0]) == {SEMI: 300, ANTI_FALSE: 0, ANTI_TRUE: 0}.get(mode, 60_000)
        want = check(device, left, right, mode, LT, "nothing")
        assert len(want[0]) == {INNER: 0, LEFT: 300, RIGHT: 200, FULL: 500, SEMI: 0}.get(mode, 300)


def test_nulls(device):
    """An all-NULL chunk on either side; AntiNullAsTrue with NULLs in the primary and in a secondary column."""
    rng = np.random.default_rng(5)
    left_nulls = rng.random(200) < 0.1
    left_nulls[64:128] = True
    right_nulls = rng.random(150) < 0.1
    right_nulls[:50] = True
    left = Table([(rng.integers(0, 10, 200).astype(np.int32), left_nulls), (rng.integers(0, 4, 200).astype(np.int32), rng.random(200) < 0.2)], chunk=64)
    right = Table([(rng.integers(0, 10, 150).astype(np.int32), right_nulls), (rng.integers(0, 4, 150).astype(np.int32), rng.random(150) < 0.2)], chunk=50)
    for mode in MODES:
        for condition in (EQ, LT, NE):
            check(device, left, right, mode, condition, "NULL chunks")
            check(device, left, right, mode, [(0, condition, 0), (1, LE, 1)], "NULL chunks, secondary")
    all_null = Table([(np.zeros(70, dtype=np.int32), np.ones(70, dtype=bool))], chunk=64)
    empty = Table([(np.zeros(0, dtype=np.int32), None)])
    some = Table([(rng.integers(0, 10, 100).astype(np.int32), rng.random(100) < 0.2)], chunk=33)
    for a, b in ((some, all_null), (all_null, some), (all_null, all_null), (some, empty), (empty, some), (empty, empty)):
        for mode in MODES:
            check(device, a, b, mode, LE, "degenerate sides")


@pytest.mark.parametrize("left_type", NP_TYPES)
def test_key_types(device, left_type):
    """Each of the 16 type pairs, with the values that tell the common types apart: int64 above 2^53 against double, 2^24 + 1 against float."""
    rng = np.random.default_rng(6)
    special = np.array([(1 << 24) + 1, 1 << 24, (1 << 24) - 1, (1 << 53) + 1, 1 << 53, -(1 << 53) - 1, 0, -1, 7, (1 << 31) - 1], dtype=np.int64)
    base = np.concatenate([special, rng.integers(-20, 20, 90)])

    def column(kind, values):
        if kind == np.int32:
            values = np.clip(values, -(1 << 31), (1 << 31) - 1)
        return values.astype(kind)

    for right_type in NP_TYPES:
        left = Table([(column(left_type, base), rng.random(100) < 0.05)], chunk=37)
        right = Table([(column(right_type, base[::-1].copy()), rng.random(100) < 0.05)], chunk=64)
        for mode, condition in ((INNER, EQ), (FULL, LE), (LEFT, NE), (RIGHT, GT), (SEMI, LT), (ANTI_TRUE, GE)):
            check(device, left, right, mode, condition, f"{np.dtype(left_type)} x {np.dtype(right_type)}", mems=[abi.MEM_DEVICE])


@pytest.mark.parametrize("kind,domain", [("dictionary", 100), ("dictionary", 700), ("frame_of_reference", 300), ("run_length", 20), ("bit_packed_dictionary", 100),
                                         ("bit_packed_frame_of_reference", 300)])
def test_encodings(device, kind, domain):
    """Dictionary with 1- and 2-byte value ids (100 / 700 distinct values per chunk), FrameOfReference, RunLength, BitPacking: key and secondary."""
    rng = np.random.default_rng(domain)
    left = Table([(rng.integers(0, domain, 1500).astype(np.int32), rng.random(1500) < 0.05), (rng.integers(0, domain, 1500).astype(np.int32), None)], chunk=800, kind=kind)
    right = Table([(rng.integers(0, domain, 1200).astype(np.int32), None), (rng.integers(0, domain, 1200).astype(np.int32), rng.random(1200) < 0.05)], chunk=1200, kind=kind)
    if kind == "dictionary":
        assert {s.width for s in left.host[0].segments} == {1 if domain < 255 else 2}
    for mode, predicates in ((FULL, [(0, EQ, 0), (1, LT, 1)]), (SEMI, [(0, GT, 0), (1, EQ, 1)]), (INNER, [(0, EQ, 0)])):
        check(device, left, right, mode, predicates, kind)


def test_reference_column_over_a_scan_s_device_pos_lists(device):
    """The left input is the reference table a hy_table_scan leaves in HBM: one PosList per chunk that has matches, read in place."""
    import torch
    from hyrise_amd.distributed import HipExecutor
    rng = np.random.default_rng(8)
    n, chunk = 3_000, 700
    keys = rng.integers(0, 500, n).astype(np.int32)
    key_nulls = rng.random(n) < 0.1
    other = rng.integers(0, 5, n).astype(np.int64)
    pick = (rng.random(n) < 0.3).astype(np.int32)
    pick[chunk:2 * chunk] = 0   # (a chunk without matches: no output chunk)
    data = {"key": DeviceColumn(storage.make_column(keys, key_nulls, abi.ENC_DICTIONARY, chunk)), "other": DeviceColumn(storage.make_column(other, None, abi.ENC_UNENCODED, chunk)),
            "pick": DeviceColumn(storage.make_column(pick, None, abi.ENC_UNENCODED, chunk))}
    ex = HipExecutor(torch.device("cuda:0"))
    lists = ex.scan_chunked(data["pick"], make_predicate(abi.PRED_EQUALS, abi.TYPE_INT, 1))
    kept = np.flatnonzero(pick == 1)
    left = Table.__new__(Table)
    left.columns, left.sizes = [(keys[kept], key_nulls[kept]), (other[kept], None)], [int(c) for c in lists.count if c]
    left.device = [ex.reference_column_chunked(data["key"], lists), ex.reference_column_chunked(data["other"], lists)]
    assert left.device[0].n_chunks == 4
    right = Table([(rng.integers(0, 500, 400).astype(np.int32), rng.random(400) < 0.1), (rng.integers(0, 5, 400).astype(np.int32), None)], chunk=150)
    for mode, predicates in ((FULL, [(0, EQ, 0)]), (LEFT, [(0, LT, 0), (1, EQ, 1)]), (ANTI_FALSE, [(0, GT, 0), (1, NE, 1)])):
        check(device, left, right, mode, predicates, "scan output")
        mirrored = [(r, {LT: GT, GT: LT}.get(c, c), l) for l, c, r in predicates]
        check(device, right, left, {LEFT: RIGHT}.get(mode, mode), mirrored, "scan output on the right")


@pytest.mark.parametrize("mode", [INNER, LEFT, FULL, SEMI, ANTI_FALSE])
def test_secondary_predicates(device, general, mode):
    """One and four secondary predicates, all six conditions."""
    left, right = general
    for condition in CONDITIONS:
        check(device, left, right, mode, [(0, LE, 0), (1, condition, 1)], "one secondary", mems=[abi.MEM_DEVICE])
        check(device, left, right, mode, [(0, NE, 0), (1, condition, 1), (2, GE, 2), (3, NE, 3), (4, LE, 4)], "four secondaries", mems=[abi.MEM_DEVICE])


def test_what_join_sort_merge_refuses_or_flips(device, general):
    """<> under an outer mode; Right with a secondary predicate (both flipped with the tables); AntiNullAsTrue with secondary predicates."""
    left, right = general
    for mode in (LEFT, RIGHT, FULL):
        check(device, left, right, mode, NE, "<> outer")
    for condition in CONDITIONS:
        check(device, left, right, RIGHT, [(0, condition, 0), (1, LT, 1)], "Right with a secondary")
    check(device, left, right, ANTI_TRUE, [(0, LT, 0), (1, EQ, 1), (3, GT, 3)], "AntiNullAsTrue with secondaries")
    pairs = join_nested_loop(left.device[0], right.device[0], abi.JOIN_SEMI, LT, [(left.device[1], GE, right.device[1])])   # (the wrapper of operators.py)
    want = nested_loop_join(left.columns, right.columns, left.sizes, right.sizes, SEMI, [(0, LT, 0), (1, GE, 1)])
    assert pairs.numpy()[0].tobytes() == row_ids(want[0], left.sizes).tobytes()
    pairs.close()


@pytest.mark.parametrize("mem", MEMS)
def test_capacity(device, general, mem):
    """capacity = needed - 1: HY_ERR_CAPACITY, the need reported, both lists untouched."""
    left, right = general
    for mode, predicates in ((INNER, [(0, LT, 0)]), (FULL, [(0, EQ, 0)]), (RIGHT, [(0, GE, 0), (1, NE, 1)]), (SEMI, [(0, LT, 0)]), (ANTI_FALSE, [(0, EQ, 0)])):
        want = nested_loop_join(left.columns, right.columns, left.sizes, right.sizes, mode, predicates)
        needed = len(want[0])
        assert needed > 1
        status, result, got_left, got_right = call(device, left, right, mode, predicates, mem, needed - 1)
        assert status == abi.ERR_CAPACITY and device.hy_last_error()
        assert result.n_pairs == needed
        assert (got_left == SENTINEL).all() and (got_right == SENTINEL).all()
    status, result, _, _ = call(device, left, right, FULL, [(0, EQ, 0)], mem, 0)
    assert status == abi.ERR_CAPACITY and result.n_pairs > 0


def test_unaligned_lists_are_refused(device, general):
    left, right = general
    result = abi.NestedLoopResult()
    buffer = np.zeros(4096, dtype=np.uint8)
    result.mem, result.capacity, result.left_pos, result.right_pos = abi.MEM_HOST, 100, buffer.ctypes.data + 4, buffer.ctypes.data + 2048
    assert device.hy_join_nested_loop(left.device[0].handle, right.device[0].handle, INNER, EQ, None, 0, C.byref(result)) == abi.ERR_INVALID
    assert not buffer.any()


def test_count_beyond_32_bits(device):
    """70 000 x 70 000 Inner <> over distinct keys: 70 000 x 69 999 pairs (> 2^32) -- the counting passes only, nothing is written."""
    keys = np.arange(70_000, dtype=np.int32)
    left, right = Table([(keys, None)], chunk=65_535), Table([(keys[::-1].copy(), None)], chunk=65_535)
    assert count(device, left, right, INNER, [(0, NE, 0)]) == 70_000 * 69_999


def test_segment_scan_with_output(device):
    """4 097 x 4 097 Inner <=: 17 tiles, about 8.4 M pairs written behind 64-bit offsets."""
    keys = np.random.default_rng(9).permutation(4_097).astype(np.int32)
    left, right = Table([(keys, None)], chunk=5_000), Table([(keys[::-1].copy(), None)], chunk=1_500)
    want = check(device, left, right, INNER, LE, "4097 x 4097", mems=[abi.MEM_DEVICE])
    assert len(want[0]) == 4_097 * 4_098 // 2


def test_refusals(device, general):
    left, right = general
    status, _, _, _ = call(device, left, right, abi.JOIN_CROSS, [(0, EQ, 0)], abi.MEM_HOST, 100)
    assert status == abi.ERR_UNSUPPORTED and device.hy_last_error()
    segments, _ = __import__("hyrise_amd.string_keys", fromlist=["encode_string_column"]).encode_string_column(["a", "b", "c"], np.zeros(3, dtype=bool), 3)
    strings = Table.__new__(Table)
    strings.device = [DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING)), Table([(np.arange(3, dtype=np.int32), None)]).device[0]]
    for predicates in ([(0, EQ, 0)], [(1, EQ, 1), (0, LT, 0)]):   # a string key, a string column in a secondary predicate
        status, _, _, _ = call(device, strings, strings, INNER, predicates, abi.MEM_HOST, 100)
        assert status == abi.ERR_UNSUPPORTED and device.hy_last_error(), predicates
    counted = C.c_uint64(0)
    assert device.hy_join_nested_loop_count(strings.device[0].handle, strings.device[0].handle, INNER, EQ, None, 0, C.byref(counted)) == abi.ERR_UNSUPPORTED
    other_layout = Table([(np.arange(257, dtype=np.int32), None)], chunk=101)
    mixed = Table.__new__(Table)
    mixed.device = [left.device[0], other_layout.device[0]]
    status, _, _, _ = call(device, mixed, right, INNER, [(0, EQ, 0), (1, LT, 1)], abi.MEM_HOST, 100)
    assert status == abi.ERR_INVALID and b"chunk layout" in device.hy_last_error()
    status, _, _, _ = call(device, left, right, INNER, [(0, EQ, 0)] + [(1, LT, 1)] * 5, abi.MEM_HOST, 100)
    assert status == abi.ERR_UNSUPPORTED


def test_refuses_more_than_the_comparison_limit(device):
    """33 chunks of 65 535 rows over ONE device buffer on each side (HY_MEM_DEVICE: nothing is copied): 2.16 M x 2.16 M rows are 4.7 * 10^12
    comparisons, above HY_NLJ_MAX_COMPARISONS; refused before any kernel."""
    import torch
    values = torch.zeros(65_535, dtype=torch.int32, device="cuda:0")
    n_chunks = 33
    assert (n_chunks * 65_535) ** 2 > abi.NLJ_MAX_COMPARISONS
    segments = (abi.Segment * n_chunks)()
    for s in segments:
        s.encoding, s.data_type, s.size, s.width, s.data, s.ref_chunk_id = abi.ENC_UNENCODED, abi.TYPE_INT, 65_535, 4, values.data_ptr(), abi.INVALID_CHUNK_ID
    handle = C.c_void_p()
    abi.check(device.hy_column_create(segments, n_chunks, abi.MEM_DEVICE, C.byref(handle)))
    try:
        counted = C.c_uint64(0)
        assert device.hy_join_nested_loop_count(handle, handle, INNER, LT, None, 0, C.byref(counted)) == abi.ERR_UNSUPPORTED
        assert b"comparisons" in device.hy_last_error()
    finally:
        device.hy_column_destroy(handle)

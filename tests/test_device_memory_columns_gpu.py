"""Caller-owned device columns (HY_MEM_DEVICE) at every alignment, through every operator.

Every parity test uploads through storage.DeviceColumn: the library's arena puts each buffer on a 256-byte boundary with 16 spare bytes
behind it.  Here every buffer of a column sits at a chosen address modulo 16 inside one tensor, surrounded by filler bytes (0x00: value id 0,
row 0, not NULL; 0xFF: the NULL value id, a NULL RowID, set null bits) -- tests/placed_columns.py.  Each case computes its expectation with
the CPU oracle over the HOST column, runs the operator over the uploaded column and over the placed ones, and asserts the oracle's bytes for
all of them; afterwards no byte of a placed input may have changed.

Shapes: three ragged chunks of 8 203 (an 8192-row slice, a partial group, an odd tail), 2 051 (a FrameOfReference block plus 3) and 5 rows."""
import ctypes as C

import numpy as np
import pytest

import fused_cases
from hyrise_amd import abi, storage
from hyrise_amd.operators import (aggregate_hash, aggregate_hash_columns, column_gather, join_hash, make_predicate, projection_arithmetic, scan_project_aggregate, sort,
                                  table_scan, table_scan_columns, validate)
from hyrise_amd.storage import DeviceColumn
from placed_columns import FILLS, PLACEMENTS, PlacedArray, PlacedColumn, residue
from sort_oracle import positions_of, sorted_order
from support import (DeviceArray, assert_scan_equal, oracle_aggregate, oracle_arithmetic, oracle_chain, oracle_join, oracle_scan, oracle_scan_columns, oracle_validate)
from test_aggregate_gpu import assert_aggregate_equal
from test_fused_gpu import assert_matches_chain
from test_join_gpu import assert_join_equal
from test_projection_gpu import assert_same
from test_scan_gpu import CONDITIONS, device_pos_list, expected_pos_list
from test_sort_gpu import check_sort
from test_sort_limit_gpu import check_limits

pytestmark = pytest.mark.gpu

SIZES = (8_203, 2_051, 5)
N = sum(SIZES)
COMBOS = [(placement, fill) for placement in PLACEMENTS for fill in FILLS]
TYPES = [np.int32, np.int64, np.float32, np.float64]
KINDS = ["value", "dictionary1", "dictionary2", "dictionary4", "frame_of_reference1", "frame_of_reference2", "frame_of_reference4", "run_length", "bit_packed"]
DOMAIN = {"value": 3_000, "dictionary1": 200, "dictionary2": 3_000, "dictionary4": 3_000, "frame_of_reference1": 200, "frame_of_reference2": 50_000,
          "frame_of_reference4": 1 << 29, "run_length": 40, "bit_packed": 3_000}


def widen(segment, width):
    """The same Dictionary segment with `width`-byte value ids (a chunk of these sizes never needs four bytes on its own)."""
    return storage.HostSegment(segment.encoding, segment.data_type, segment.size, width, segment.data.astype({2: np.uint16, 4: np.uint32}[width]), aux=segment.aux,
                               aux_size=segment.aux_size, nulls=segment.nulls, sorted_by=segment.sorted_by)


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    if kind.startswith("frame_of_reference"):
        return storage.encode_segment(values, nulls, abi.ENC_FRAME_OF_REFERENCE if values.dtype == np.int32 else abi.ENC_UNENCODED)
    if kind == "value":
        return storage.encode_segment(values, nulls, abi.ENC_UNENCODED)
    segment = storage.encode_segment(values, nulls, abi.ENC_DICTIONARY)
    if kind == "bit_packed":
        return storage.bit_pack_segment(segment)
    want = int(kind[-1])
    return widen(segment, want) if segment.width < want else segment


def column_of(values, nulls, kind, sizes=SIZES, nullable=None):
    nullable = nulls is not None if nullable is None else nullable
    segments, begin = [], 0
    for size in sizes:
        chunk_nulls = nulls[begin:begin + size] if nulls is not None else (np.zeros(size, dtype=bool) if nullable and kind == "value" else None)
        segments.append(segment_of(values[begin:begin + size], chunk_nulls, kind))
        begin += size
    assert begin == len(values)
    return storage.HostColumn(segments, storage.TYPE_OF_NP[np.dtype(values.dtype)])


def values_of(rng, kind, dtype, n=N):
    domain = DOMAIN[kind]
    if kind == "run_length":
        base = np.repeat(rng.integers(0, domain, n // 7 + 1), 7)[:n]
    else:
        base = rng.integers(0, domain, n)
    base = base - domain // 2
    return (base * 0.25).astype(dtype) if np.dtype(dtype).kind == "f" else base.astype(dtype)


def applicable(kind, dtype):
    return not (kind.startswith("frame_of_reference") and dtype != np.int32)   # FrameOfReference is int32 only


def layouts(host, combos=COMBOS, refs_of=None):
    """The uploaded column first (the control of the control), then the placed ones.  refs_of(placement, fill) -> refs for reference columns."""
    yield "uploaded", DeviceColumn(host, refs=refs_of("uploaded", None) if refs_of else None)
    for placement, fill in combos:
        yield f"{placement}/{fill:#04x}", PlacedColumn(host, placement, fill, refs=refs_of(placement, fill) if refs_of else None)


def untouched(*columns):
    for column in columns:
        if isinstance(column, (PlacedColumn, PlacedArray)):
            column.assert_untouched()


def test_placements_take_effect(device):
    """The addresses the library is handed, modulo 16, for every buffer of a column of every kind."""
    rng = np.random.default_rng(1)
    for kind in KINDS:
        host = column_of(values_of(rng, kind, np.int32), rng.random(N) < 0.1, kind)
        for placement, fill in COMBOS:
            placed = PlacedColumn(host, placement, fill)
            assert placed.addresses
            for b in placed.buffers:
                assert placed.addresses[(b.chunk, b.field)] % 16 == residue(placement, b.role, b.w)
            image = placed.tensor.cpu().numpy()
            assert np.array_equal(image, placed.image) and image[0] == fill and image[-1] == fill
            placed.assert_untouched()


# ---- hy_table_scan ------------------------------------------------------------------------------------------------------------------
def device_scan(lib, column, predicate, flags):
    """hy_table_scan into device memory under HY_SCAN_CHUNK_REGIONS -> (counts, chunk states, the written prefix of every chunk's region)."""
    rows, n_chunks = max(1, column.rows), column.n_chunks
    regions, offsets, counts, states = (DeviceArray(lib, (rows, 2), np.uint32), DeviceArray(lib, (n_chunks + 1,), np.uint64), DeviceArray(lib, (max(1, n_chunks),), np.uint32),
                                        DeviceArray(lib, (max(1, n_chunks),), np.uint8))
    result = abi.ScanResult()
    result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | flags
    result.matches, result.capacity, result.offsets, result.counts, result.chunk_state = regions.pointer, rows, offsets.pointer, counts.pointer, states.pointer
    abi.check(lib.hy_table_scan(column.handle, C.byref(predicate), None, 0, C.byref(result)))
    abi.check(lib.hy_synchronize())
    return counts.numpy()[:n_chunks], states.numpy()[:n_chunks], regions.numpy(), offsets.numpy()


def scan_matrix(lib, host, data_type, nullable, literals, combos, context):
    columns = list(layouts(host, combos))
    for condition in CONDITIONS:
        for value, value2 in literals:
            predicate = make_predicate(condition, data_type, value, value2, nullable=nullable)
            want = {flags: oracle_scan(host, predicate, flags=flags) for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH)}
            want_list = expected_pos_list(host, predicate)
            for name, column in columns:
                where = f"{context} {name} cond {condition} lit {value},{value2}"
                for flags in want:
                    assert_scan_equal(table_scan(column, predicate, flags=flags), want[flags], f"{where} flags {flags}")
                got_list, _ = device_pos_list(lib, host, column, predicate)
                assert got_list.tobytes() == want_list.tobytes(), f"{where}: device-memory PosList"
                # without MATERIALIZE_ALL_MATCH: the counts and states are the oracle's, scanned chunks hold the oracle's RowIDs
                counts, states, regions, offsets = device_scan(lib, column, predicate, 0)
                plain = want[0]
                np.testing.assert_array_equal(counts, plain.counts[:host.n_chunks], err_msg=f"{where}: device-memory counts")
                np.testing.assert_array_equal(states, plain.chunk_state[:host.n_chunks], err_msg=f"{where}: device-memory states")
                for c in range(host.n_chunks):
                    expected = plain.pos_list(c)
                    begin = int(offsets[c])
                    assert regions[begin:begin + len(expected)].tobytes() == expected.tobytes(), f"{where}: device-memory region of chunk {c}"
    untouched(*[column for _, column in columns])


def literal_pairs(values, dtype):
    low, high = np.quantile(values.astype(np.float64), [0.3, 0.6])
    top = float(values.max())
    cast = (lambda v: float(v)) if np.dtype(dtype).kind == "f" else (lambda v: int(v))
    return [(cast(low), cast(high)), (cast(top + 5), cast(top + 9))]


@pytest.mark.parametrize("kind,dtype", [(kind, dtype) for kind in KINDS for dtype in TYPES if applicable(kind, dtype)], ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_table_scan(device, kind, dtype):
    rng = np.random.default_rng(len(kind) * 11 + np.dtype(dtype).itemsize)
    values = values_of(rng, kind, dtype)
    data_type = storage.TYPE_OF_NP[np.dtype(dtype)]
    for nulls in (None, rng.random(N) < 0.1):
        host = column_of(values, nulls, kind, nullable=nulls is not None)
        scan_matrix(device, host, data_type, nulls is not None, literal_pairs(values, dtype), COMBOS, f"{kind} {np.dtype(dtype).name} nulls={nulls is not None}")


def test_table_scan_sorted_and_null_only_chunks(device):
    rng = np.random.default_rng(77)
    values = np.sort(rng.integers(-500, 500, N)).astype(np.int32)
    sorted_host = column_of(values, None, "dictionary2")
    for segment in sorted_host.segments:
        segment.sorted_by = abi.SORT_ASCENDING_NULLS_FIRST
    scan_matrix(device, sorted_host, abi.TYPE_INT, False, literal_pairs(values, np.int32), COMBOS, "sorted_by")
    nulls = rng.random(N) < 0.05
    nulls[SIZES[0]:SIZES[0] + SIZES[1]] = True     # chunk 1: a dictionary segment with an empty dictionary
    shuffled = rng.permutation(values)
    scan_matrix(device, column_of(shuffled, nulls, "dictionary1"), abi.TYPE_INT, True, literal_pairs(values, np.int32), COMBOS, "NULL-only chunk")


# ---- hy_table_scan_columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_columns", [1, 0], ids=["two_stream", "generic"])
def test_table_scan_columns(device, options, two_columns):
    options.set(abi.OPT_SCAN_TWO_COLUMNS, two_columns)
    rng = np.random.default_rng(5)
    pairs = []
    for dtype, kinds in ((np.int32, ("value", "dictionary1", "dictionary4", "frame_of_reference2")), (np.float32, ("value", "dictionary2"))):
        left, right = values_of(rng, "dictionary1", dtype), values_of(rng, "dictionary1", dtype)
        for lkind in kinds:
            for rkind in kinds[:2]:
                pairs.append((column_of(left, rng.random(N) < 0.1, lkind), column_of(right, None, rkind), f"{np.dtype(dtype).name} {lkind} x {rkind}"))
    wide_left, wide_right = values_of(rng, "dictionary1", np.int64), values_of(rng, "dictionary1", np.float64)
    pairs.append((column_of(wide_left, rng.random(N) < 0.1, "value"), column_of(wide_right, rng.random(N) < 0.1, "dictionary1"), "int64 x float64 (row by row)"))
    for left, right, name in pairs:
        want = {condition: oracle_scan_columns(left, right, condition) for condition in CONDITIONS[:6]}
        lefts = dict(layouts(left))
        rights = dict(layouts(right))
        # the two columns at different placements: every left layout against the right layout three places on (the uploaded one among them),
        # and the uploaded pair
        names = list(lefts)
        for i, lname in enumerate(names):
            rname = names[(i + 3) % len(names)] if lname != "uploaded" else "uploaded"
            for condition, expected in want.items():
                assert_scan_equal(table_scan_columns(lefts[lname], rights[rname], condition), expected, f"{name}: left {lname} right {rname} cond {condition}")
        untouched(*lefts.values(), *rights.values())


# ---- reference columns --------------------------------------------------------------------------------------------------------------
def reference_shapes(rng, base):
    first = oracle_scan(base, make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, 0, nullable=True), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    single = [first.pos_list(c).copy() for c in range(base.n_chunks)] + [1]
    single_host = storage.make_reference_column(base, single, list(range(base.n_chunks)) + [1])
    many = []
    for size in (1, 65, 4_097, 3):
        rows = rng.integers(0, N, size)
        chunk = np.searchsorted(np.cumsum(SIZES), rows, side="right")
        pos = np.stack([chunk, rows - np.concatenate([[0], np.cumsum(SIZES)])[chunk]], axis=1).astype(np.uint32)
        pos[rng.random(size) < 0.05] = 0xFFFFFFFF
        many.append(pos)
    return single_host, storage.make_reference_column(base, many, [None] * len(many))


@pytest.mark.parametrize("kind", ["value", "dictionary2", "frame_of_reference1"])
def test_reference_columns(device, kind):
    """PosLists at 8 mod 16 (and everywhere else) over a placed base column: scanned, exported, sorted, projected and aggregated."""
    rng = np.random.default_rng(len(kind))
    values, nulls = values_of(rng, kind, np.int32), rng.random(N) < 0.1
    base = column_of(values, nulls, kind)
    bases = dict(layouts(base))
    flat = np.concatenate([[0], np.cumsum(SIZES)])
    for shape, host in zip(("single-chunk and EntireChunk PosLists", "multi-chunk PosLists with NULL RowIDs"), reference_shapes(rng, base)):
        columns = dict(layouts(host, refs_of=lambda placement, fill: {id(base): bases["uploaded" if fill is None else f"{placement}/{fill:#04x}"]}))
        # what the reference column holds, row by row
        cells, cell_nulls = [], []
        for segment in host.segments:
            rows = np.stack([np.full(segment.size, segment.ref_chunk_id), np.arange(segment.size)], axis=1) if segment.data is None else segment.data.astype(np.int64)
            is_null = rows[:, 1] == 0xFFFFFFFF
            index = np.where(is_null, 0, flat[np.where(is_null, 0, rows[:, 0])] + rows[:, 1])
            cells.append(values[index])
            cell_nulls.append(is_null | nulls[index])
        cells, cell_nulls = np.concatenate(cells), np.concatenate(cell_nulls)
        sizes = [s.size for s in host.segments]
        predicates = [make_predicate(condition, abi.TYPE_INT, -20, 30, nullable=True) for condition in CONDITIONS]
        want_scans = [oracle_scan(host, p) for p in predicates]
        want_sum = oracle_aggregate([host], [(abi.AGG_SUM, host), (abi.AGG_COUNT, None)])
        want_plus = oracle_arithmetic(abi.ARITH_ADD, (cells, cell_nulls), (abi.TYPE_INT, 3))
        for name, column in columns.items():
            where = f"{kind}, {shape}, {name}"
            for predicate, want in zip(predicates, want_scans):
                assert_scan_equal(table_scan(column, predicate), want, f"{where} cond {predicate.condition}")
            out_values, out_nulls = PlacedArray(4 * column.rows, 8, 0xFF), PlacedArray(column.rows, 8, 0xFF)
            abi.check(device.hy_column_export(column.handle, out_values.pointer, out_nulls.pointer))
            got_values, guards = out_values.read(np.int32)
            got_nulls, null_guards = out_nulls.read(np.uint8)
            assert guards and null_guards, f"{where}: hy_column_export wrote outside its outputs"
            assert got_nulls.astype(bool).tobytes() == cell_nulls.tobytes() and got_values.tobytes() == np.where(cell_nulls, 0, cells).astype(np.int32).tobytes(), f"{where}: export"
            for mode in (abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST):
                check_sort([column], [(cells, cell_nulls)], [mode], sizes, f"{where} sort {mode}").close()
            assert_same(projection_arithmetic(abi.ARITH_ADD, column, (abi.TYPE_INT, 3)), want_plus, f"{where}: projection")
            assert_aggregate_equal(aggregate_hash([column], [(abi.AGG_SUM, column), (abi.AGG_COUNT, None)]), want_sum, 2, f"{where}: aggregate")
        untouched(*columns.values())
    untouched(*bases.values())


# ---- hy_validate --------------------------------------------------------------------------------------------------------------------
def test_validate(device):
    from test_oracle_validate import TRUTH_TABLE
    tids, begins, ends = (np.array([row[i] for row in TRUTH_TABLE], dtype=np.uint32) for i in (1, 2, 3))
    rng = np.random.default_rng(41)
    more = (rng.integers(0, 6, N).astype(np.uint32), np.where(rng.random(N) < 0.05, storage.MAX_COMMIT_ID, rng.integers(1, 40, N)).astype(np.uint32),
            np.where(rng.random(N) < 0.25, rng.integers(1, 50, N), storage.MAX_COMMIT_ID).astype(np.uint32))
    for host, cases in ((storage.make_mvcc_column(tids, begins, ends, chunk_size=10, mutable_chunks=(0,)), [(2, 2)]),
                        (storage.make_mvcc_column(*more, chunk_size=SIZES[0], mutable_chunks=(1,)), [(2, 20), (0, 5), (9, 0)])):
        columns = list(layouts(host))
        for our_tid, snapshot in cases:
            for shortcut in (True, False):
                for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH):
                    want = oracle_validate(host, our_tid, snapshot, shortcut, flags)
                    for name, column in columns:
                        assert_scan_equal(validate(column, our_tid, snapshot, shortcut, flags), want, f"validate {name} tid {our_tid} snapshot {snapshot} shortcut {shortcut} flags {flags}")
        untouched(*[column for _, column in columns])


# ---- hy_join_hash -------------------------------------------------------------------------------------------------------------------
PROBE_SIZES = (8_203, 8_203, 5)
JOIN_MODES = [abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE]


def join_hooks(lib):
    for hook in (lib.hy_debug_join_used_pkfk, lib.hy_debug_join_used_rank_table, lib.hy_debug_join_build_was_hinted):
        hook.restype = C.c_int
    return int(lib.hy_debug_join_used_pkfk()), int(lib.hy_debug_join_used_rank_table()), int(lib.hy_debug_join_build_was_hinted())


def join_shapes():
    rng = np.random.default_rng(300)
    n_build, n_probe = 3_000, sum(PROBE_SIZES)
    keys = np.arange(n_build, dtype=np.int32) * 2 - 1_000
    probe = rng.choice(keys, n_probe).astype(np.int32)
    outside = rng.random(n_probe) < 0.05
    probe[outside] = rng.integers(-1_300, 5_300, int(outside.sum())).astype(np.int32)
    build_sizes = (1_024, 1_024, 952)
    yield "pk-fk, unencoded probe", column_of(keys, None, "value", build_sizes), column_of(probe, None, "value", PROBE_SIZES)
    yield "pk-fk, FrameOfReference probe", column_of(keys, None, "value", build_sizes), column_of(np.sort(probe), None, "frame_of_reference2", PROBE_SIZES)
    yield "unique shuffled build side", column_of(rng.permutation(keys), None, "value", build_sizes), column_of(probe, None, "dictionary2", PROBE_SIZES)
    yield "duplicate build side", column_of(rng.integers(0, 900, n_build).astype(np.int32), None, "value", build_sizes), column_of((probe // 4).astype(np.int32), None, "value", PROBE_SIZES)
    yield ("NULL keys", column_of(rng.integers(0, 2_000, n_build).astype(np.int32), rng.random(n_build) < 0.1, "dictionary2", build_sizes),
           column_of((probe // 2).astype(np.int32), rng.random(n_probe) < 0.1, "value", PROBE_SIZES))


@pytest.mark.parametrize("mode", JOIN_MODES)
def test_join_hash(device, mode):
    semi = mode in (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_LEFT)
    for shape, build, probe in join_shapes():
        left, right = (probe, build) if semi else (build, probe)
        want = oracle_join(left, right, mode)
        hooks = {}
        for (name, left_column), (_, right_column) in zip(layouts(left), layouts(right)):
            for attempt in (0, 1):   # the second join over the resident build column: the hinted fill
                assert_join_equal(join_hash(left_column, right_column, mode), want, mode, f"{shape} mode {mode} {name} join {attempt}")
                hooks[(name, attempt)] = join_hooks(device)
            untouched(left_column, right_column)
        for fill in FILLS:
            for attempt in (0, 1):
                assert hooks[(f"aligned/{fill:#04x}", attempt)] == hooks[("uploaded", attempt)], f"{shape} mode {mode}: the aligned control left the uploaded column's path (pkfk, rank table, hinted)"


def test_join_hash_predicates(device):
    rng = np.random.default_rng(12)
    n_build, n_probe = 3_000, sum(PROBE_SIZES)
    build_sizes = (1_024, 1_024, 952)
    build, probe = column_of(rng.integers(0, 1_500, n_build).astype(np.int32), None, "value", build_sizes), column_of(rng.integers(0, 1_500, n_probe).astype(np.int32), None, "frame_of_reference2", PROBE_SIZES)
    build_extra = column_of(rng.integers(0, 50, n_build).astype(np.int32), rng.random(n_build) < 0.1, "dictionary1", build_sizes)
    probe_extra = column_of(rng.integers(0, 50, n_probe).astype(np.int64), rng.random(n_probe) < 0.1, "value", PROBE_SIZES)
    want = oracle_join(build, probe, abi.JOIN_INNER, secondary=[(build_extra, abi.PRED_LESS_THAN, probe_extra)])
    for columns in zip(layouts(build), layouts(probe), layouts(build_extra), layouts(probe_extra)):
        name = columns[0][0]
        b, p, be, pe = (column for _, column in columns)
        assert_join_equal(join_hash(b, p, abi.JOIN_INNER, secondary=[(be, abi.PRED_LESS_THAN, pe)]), want, abi.JOIN_INNER, f"secondary predicate, {name}")
        untouched(b, p, be, pe)


# ---- hy_aggregate_hash / hy_aggregate_hash_columns ----------------------------------------------------------------------------------
class ColumnsAsResult:
    """hy_aggregate_hash_columns' output in the shape assert_aggregate_equal reads."""

    def __init__(self, out):
        self.n_groups, self.row_ids, self.out = out.n_groups, out.row_ids.numpy(), out

    def column(self, a):
        return self.out.column(a)


def small_domain_hook(lib):
    lib.hy_debug_aggregate_small_domain.restype = int
    return lib.hy_debug_aggregate_small_domain()


def aggregate_shapes():
    rng = np.random.default_rng(91)
    flags, status = rng.integers(0, 2, N).astype(np.int32), rng.integers(0, 2, N).astype(np.int64)
    quantity, discount = rng.integers(1, 51, N).astype(np.float32), (rng.integers(0, 11, N) / 100.0).astype(np.float64)
    small = [column_of(flags, rng.random(N) < 0.01, "dictionary1"), column_of(status, None, "dictionary1")]
    q, d = column_of(quantity, None, "dictionary1"), column_of(discount, rng.random(N) < 0.03, "dictionary1")
    qi = column_of(rng.integers(-40, 41, N).astype(np.int32), rng.random(N) < 0.05, "dictionary1")
    yield "small domain", small[1:], [(abi.AGG_SUM, q), (abi.AGG_AVG, q), (abi.AGG_MIN, d), (abi.AGG_MAX, d), (abi.AGG_COUNT, d), (abi.AGG_COUNT, None)]
    yield "small domain, four groups", [column_of(flags, None, "dictionary1"), small[1]], [(abi.AGG_SUM, qi), (abi.AGG_AVG, q), (abi.AGG_MIN, qi), (abi.AGG_MAX, q), (abi.AGG_COUNT, None)]
    ints, floats = rng.integers(-1_000, 1_000, N).astype(np.int32), (rng.integers(0, 4_000, N) * 0.25).astype(np.float32)
    longs, doubles = rng.integers(-3, 4, N).astype(np.int64) * (1 << 40), rng.integers(0, 4_000, N) * 0.125
    for width in (1, 2, 4):
        keys = column_of(rng.integers(0, 200 if width == 1 else 900, N).astype(np.int32), rng.random(N) < 0.02, f"dictionary{width}")
        for nullable in (False, True):
            four = [column_of(ints, rng.random(N) < 0.1 if nullable else None, "value"), column_of(floats, rng.random(N) < 0.1 if nullable else None, "value")]
            yield (f"{width}-byte keys, 4-byte inputs, bitmap {nullable}", [keys],
                   [(abi.AGG_MIN, four[0]), (abi.AGG_MAX, four[1]), (abi.AGG_SUM, four[0]), (abi.AGG_SUM, four[1]), (abi.AGG_AVG, four[1]), (abi.AGG_COUNT, four[0]), (abi.AGG_COUNT, None)])
        eight = [column_of(longs, rng.random(N) < 0.1, "value"), column_of(doubles, None, "value")]
        yield (f"{width}-byte keys, 8-byte inputs", [keys],
               [(abi.AGG_MIN, eight[0]), (abi.AGG_MAX, eight[1]), (abi.AGG_SUM, eight[0]), (abi.AGG_SUM, eight[1]), (abi.AGG_AVG, eight[0]), (abi.AGG_COUNT, eight[0]), (abi.AGG_COUNT, None)])
    many = column_of(rng.permutation(np.arange(N) % 5_000).astype(np.int32), None, "value")
    yield "5 000 groups", [many], [(abi.AGG_SUM, column_of(ints, None, "frame_of_reference2")), (abi.AGG_MAX, column_of(doubles, None, "dictionary2")), (abi.AGG_COUNT, None)]


@pytest.mark.parametrize("entry", ["hy_aggregate_hash", "hy_aggregate_hash_columns"])
def test_aggregate_hash(device, entry):
    for shape, groupby, aggregates in aggregate_shapes():
        want = oracle_aggregate(groupby, aggregates)
        hosts = {id(c): c for c in groupby + [c for _, c in aggregates if c is not None]}
        hooks = {}
        for name in ["uploaded"] + [f"{placement}/{fill:#04x}" for placement, fill in COMBOS]:
            made = {key: (DeviceColumn(host) if name == "uploaded" else PlacedColumn(host, name.split("/")[0], int(name.split("/")[1], 16))) for key, host in hosts.items()}
            keys, specs = [made[id(c)] for c in groupby], [(f, made[id(c)] if c is not None else None) for f, c in aggregates]
            got = aggregate_hash(keys, specs) if entry == "hy_aggregate_hash" else ColumnsAsResult(aggregate_hash_columns(keys, specs, chunk_rows=1_000))
            hooks[name] = small_domain_hook(device)
            assert_aggregate_equal(got, want, len(aggregates), f"{entry}: {shape}, {name}")
            untouched(*made.values())
        if shape.startswith("small domain"):
            assert hooks["uploaded"] == 1, f"{shape}: the uploaded columns did not take the small-domain kernel"
        for fill in FILLS:
            assert hooks[f"aligned/{fill:#04x}"] == hooks["uploaded"], f"{shape}: the aligned control left the uploaded columns' kernel"


# ---- hy_scan_project_aggregate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoded", [True, False], ids=["encoded", "unencoded"])
@pytest.mark.parametrize("with_nulls", [False, True], ids=["not_null", "nullable"])
def test_scan_project_aggregate(device, encoded, with_nulls):
    _, _, hosts = fused_cases.lineitem(n=20_000, chunk=8_203, encoded=encoded, with_nulls=with_nulls)
    plans = fused_cases.plans(with_nulls)
    chains = [oracle_chain(*plan.on(hosts)) for plan in plans]
    for name in ["uploaded"] + [f"{placement}/{fill:#04x}" for placement, fill in COMBOS]:
        made = {key: (DeviceColumn(host) if name == "uploaded" else PlacedColumn(host, name.split("/")[0], int(name.split("/")[1], 16))) for key, host in hosts.items()}
        for plan, chain in zip(plans, chains):
            assert_matches_chain(scan_project_aggregate(*plan.on(made)), chain, len(plan.aggregates), f"plan {plan.name}, {name}")
        untouched(*made.values())


def test_scan_project_aggregate_small_domain(device):
    import test_fused_small_gpu as small
    hosts = small.table(20_000, 8_203)
    plans = [plan for plan in small.plans() if plan.name in ("q1", "one_key_two_filters", "no_groups")]
    chains = [oracle_chain(*plan.on(hosts)) for plan in plans]
    kernels = {}
    for name in ["uploaded"] + [f"{placement}/{fill:#04x}" for placement, fill in COMBOS]:
        made = {key: (DeviceColumn(host) if name == "uploaded" else PlacedColumn(host, name.split("/")[0], int(name.split("/")[1], 16))) for key, host in hosts.items()}
        for plan, chain in zip(plans, chains):
            got = scan_project_aggregate(*plan.on(made))
            kernels[(name, plan.name)] = small_domain_hook(device)
            assert_matches_chain(got, chain, len(plan.aggregates), f"plan {plan.name}, {name}")
        untouched(*made.values())
    for plan in plans:
        assert kernels[("uploaded", plan.name)] == 2, f"plan {plan.name}: the uploaded columns did not take fused_small_domain"
        for fill in FILLS:
            assert kernels[(f"aligned/{fill:#04x}", plan.name)] == 2, f"plan {plan.name}: the aligned control left fused_small_domain"


# ---- hy_projection_arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_nulls", [False, True], ids=["not_null", "bitmaps"])
def test_projection_arithmetic(device, with_nulls):
    rng = np.random.default_rng(62)
    raw = {abi.TYPE_INT: rng.integers(-2**31, 2**31 - 1, N).astype(np.int32), abi.TYPE_LONG: rng.integers(-2**62, 2**62, N).astype(np.int64),
           abi.TYPE_FLOAT: rng.normal(0, 1e6, N).astype(np.float32), abi.TYPE_DOUBLE: rng.normal(0, 1e12, N)}
    nulls = {t: (rng.random(N) < 0.07 if with_nulls else None) for t in raw}
    hosts = {t: column_of(values, nulls[t], "value") for t, values in raw.items()}
    small = rng.integers(-9, 10, N).astype(np.int32)     # (zeroes among them: x / 0 and x % 0 are NULL)
    small_nulls = rng.random(N) < 0.07 if with_nulls else None
    encoded = {"dictionary2": column_of(small * 100, small_nulls, "dictionary2"), "frame_of_reference1": column_of(small, small_nulls, "frame_of_reference1"), "value": column_of(small, small_nulls, "value")}
    encoded_values = {"dictionary2": small * 100, "frame_of_reference1": small, "value": small}
    literal = {abi.TYPE_INT: -7, abi.TYPE_LONG: 5_000_000_000, abi.TYPE_FLOAT: 0.3, abi.TYPE_DOUBLE: 0.95}
    want = {}
    for op in (abi.ARITH_ADD, abi.ARITH_MUL):
        for lt in raw:
            for rt in raw:
                want[("pair", op, lt, rt)] = oracle_arithmetic(op, (raw[lt], nulls[lt]), (raw[rt], nulls[rt]))
            want[("right literal", op, lt)] = oracle_arithmetic(op, (raw[lt], nulls[lt]), (lt, literal[lt]))
            want[("left literal", op, lt)] = oracle_arithmetic(op, (abi.TYPE_DOUBLE, literal[abi.TYPE_DOUBLE]), (raw[lt], nulls[lt]))
    for op in (abi.ARITH_DIV, abi.ARITH_MOD):
        want[("ints", op)] = oracle_arithmetic(op, (raw[abi.TYPE_INT], nulls[abi.TYPE_INT]), (small, small_nulls))
    for kind, values in encoded_values.items():
        want[("encoded", kind)] = oracle_arithmetic(abi.ARITH_ADD, (values, small_nulls), (raw[abi.TYPE_FLOAT], nulls[abi.TYPE_FLOAT]))
    inner = oracle_arithmetic(abi.ARITH_SUB, (abi.TYPE_INT, 1), (raw[abi.TYPE_FLOAT], nulls[abi.TYPE_FLOAT]))
    want["chained"] = oracle_arithmetic(abi.ARITH_MUL, (raw[abi.TYPE_DOUBLE], nulls[abi.TYPE_DOUBLE]), (inner[0], inner[1] if with_nulls else None))
    for name in ["uploaded"] + [f"{placement}/{fill:#04x}" for placement, fill in COMBOS]:
        place = (lambda host: DeviceColumn(host)) if name == "uploaded" else (lambda host: PlacedColumn(host, name.split("/")[0], int(name.split("/")[1], 16)))
        devs = {t: place(host) for t, host in hosts.items()}
        others = {kind: place(host) for kind, host in encoded.items()}
        for op in (abi.ARITH_ADD, abi.ARITH_MUL):
            for lt in raw:
                for rt in raw:
                    assert_same(projection_arithmetic(op, devs[lt], devs[rt]), want[("pair", op, lt, rt)], f"{name}: op {op} types {lt},{rt}")
                assert_same(projection_arithmetic(op, devs[lt], (lt, literal[lt])), want[("right literal", op, lt)], f"{name}: op {op} {lt} x literal")
                assert_same(projection_arithmetic(op, (abi.TYPE_DOUBLE, literal[abi.TYPE_DOUBLE]), devs[lt]), want[("left literal", op, lt)], f"{name}: op {op} literal x {lt}")
        for op in (abi.ARITH_DIV, abi.ARITH_MOD):
            assert_same(projection_arithmetic(op, devs[abi.TYPE_INT], others["value"]), want[("ints", op)], f"{name}: int {op} int")
        for kind in ("dictionary2", "frame_of_reference1"):
            assert_same(projection_arithmetic(abi.ARITH_ADD, others[kind], devs[abi.TYPE_FLOAT]), want[("encoded", kind)], f"{name}: {kind} operand")
        one_minus = projection_arithmetic(abi.ARITH_SUB, (abi.TYPE_INT, 1), devs[abi.TYPE_FLOAT])
        assert_same(projection_arithmetic(abi.ARITH_MUL, devs[abi.TYPE_DOUBLE], one_minus), want["chained"], f"{name}: a result column as an operand")
        untouched(*devs.values(), *others.values())


# ---- hy_sort / hy_sort_limit / hy_column_gather ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype", [(kind, dtype) for kind in KINDS for dtype in (np.int32, np.float64) if applicable(kind, dtype)], ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_sort_limit_and_gather(device, kind, dtype):
    rng = np.random.default_rng(len(kind) * 7 + np.dtype(dtype).itemsize)
    values, nulls = values_of(rng, kind, dtype), rng.random(N) < 0.1
    host = column_of(values, nulls, kind)
    modes = (abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST)
    orders = {mode: sorted_order([(values, nulls)], [mode]) for mode in modes}
    for name, column in layouts(host):
        for mode in modes:
            where = f"{kind} {np.dtype(dtype).name} {name} mode {mode}"
            positions = check_sort([column], [(values, nulls)], [mode], list(SIZES), where)
            check_limits([column], [(values, nulls)], [mode], list(SIZES), [1, 100, N], where)
            gathered = column_gather(column, positions, 1_000)
            got_values, got_nulls = gathered.read()
            order = orders[mode]
            assert got_nulls.tobytes() == nulls[order].tobytes(), f"{where}: gathered NULLs"
            assert got_values[~got_nulls].tobytes() == values[order][~got_nulls].tobytes(), f"{where}: gathered values"
            gathered.close()
            positions.close()
        untouched(column)


# ---- hy_join_sort_merge / hy_union_positions ------------------------------------------------------------------------------------------
def test_join_sort_merge(device):
    import test_join_sort_merge_gpu as smj
    rng = np.random.default_rng(2)
    left = smj.Side(rng.integers(0, 60, 2_056).astype(np.int32), rng.random(2_056) < 0.1, chunk=[2_051, 5], kind="dictionary")
    right = smj.Side(rng.integers(0, 60, 300).astype(np.int32), rng.random(300) < 0.1, chunk=[295, 5], kind="value")
    for mode, condition in ((smj.INNER, smj.EQ), (smj.LEFT, smj.LT)):
        for (name, left_column), (_, right_column) in zip(layouts(left.host), layouts(right.host)):
            smj.check(device, left, right, mode, condition, f"sort-merge {name}", columns=(left_column, right_column))
            untouched(left_column, right_column)


def test_union_positions(device):
    import test_union_positions_gpu as union
    table = union.Table(N, 4_096)
    left_rows, right_rows = np.flatnonzero(table.values % 3 != 0), np.flatnonzero(table.values % 5 < 3)
    sides = []
    for rows in (left_rows, right_rows):
        positions = table.positions(rows)
        sizes = [int(n) for n in np.bincount(rows // table.chunk, minlength=table.host.n_chunks)]
        sides.append((positions, storage.make_reference_column(table.host, union.split(positions, sizes))))
    for (name, left_column), (_, right_column) in zip(layouts(sides[0][1], refs_of=lambda p, f: {id(table.host): table.device}),
                                                      layouts(sides[1][1], refs_of=lambda p, f: {id(table.host): table.device})):
        for force_sort in (False, True):
            union.check_union([left_column], [right_column], [sides[0][0]], [sides[1][0]], force_sort=force_sort, context=f"union {name} force_sort {force_sort}")
        untouched(left_column, right_column)


# ---- hy_gather_row_ids / hy_poslist_gather ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4_095, 4_096, 4_097, 20_001])
def test_gather_row_ids_and_poslist_gather(device, n):
    """The table, positions and output arrays each at 0 and at 8 modulo 16, independently, with 64 guard bytes around the output."""
    rng = np.random.default_rng(n)
    table_rows, chunk_rows = 9_001, 4_096
    table = rng.integers(0, 1 << 31, (table_rows, 2)).astype(np.uint32)
    flat = rng.integers(0, table_rows + 50, n)
    positions = np.stack([flat // chunk_rows, flat % chunk_rows], axis=1).astype(np.uint32)
    null_positions = rng.random(n) < 0.02
    positions[null_positions] = 0xFFFFFFFF
    want = np.full((n, 2), 0xFFFFFFFF, dtype=np.uint32)
    ok = ~null_positions & (flat < table_rows)
    want[ok] = table[flat[ok]]
    # hy_poslist_gather: positions of a reference table (two PosLists and an EntireChunkPosList over a data table) -> the RowIDs held there
    base = column_of(np.arange(N, dtype=np.int32), None, "value")
    base_device = DeviceColumn(base)
    lists = [np.stack([rng.integers(0, 3, k), rng.integers(0, 5, k)], axis=1).astype(np.uint32) for k in (5_000, 3)] + [1]
    lists[0][rng.random(5_000) < 0.05] = 0xFFFFFFFF
    reference = storage.make_reference_column(base, lists, [None, None, 1])
    through = np.stack([rng.integers(0, 4, n), rng.integers(0, 5_010, n)], axis=1).astype(np.uint32)     # (some chunks and offsets past the end)
    through[rng.random(n) < 0.02] = 0xFFFFFFFF
    want_through = np.full((n, 2), 0xFFFFFFFF, dtype=np.uint32)
    for i, (chunk, offset) in enumerate(through.tolist()):
        if offset != 0xFFFFFFFF and chunk < 3 and offset < reference.segments[chunk].size:
            want_through[i] = (1, offset) if chunk == 2 else lists[chunk][offset]
    for fill in FILLS:
        for table_at in (0, 8):
            for positions_at in (0, 8):
                for out_at in (0, 8):
                    where = f"n {n} fill {fill:#04x} table {table_at} positions {positions_at} out {out_at}"
                    d_table, d_positions, out = PlacedArray(table.nbytes, table_at, fill, contents=table), PlacedArray(positions.nbytes, positions_at, fill, contents=positions), PlacedArray(8 * n, out_at, fill)
                    abi.check(device.hy_gather_row_ids(d_table.pointer, table_rows, chunk_rows, d_positions.pointer, n, out.pointer))
                    got, guards = out.read(np.uint32)
                    assert guards, f"hy_gather_row_ids wrote outside its output, {where}"
                    assert got.tobytes() == want.tobytes(), f"hy_gather_row_ids, {where}"
                    untouched(d_table, d_positions)
                    lists_column = PlacedColumn(reference, "aligned" if table_at == 0 else "natural", fill, refs={id(base): base_device})
                    d_through, out = PlacedArray(through.nbytes, positions_at, fill, contents=through), PlacedArray(8 * n, out_at, fill)
                    abi.check(device.hy_poslist_gather(lists_column.handle, d_through.pointer, n, out.pointer))
                    got, guards = out.read(np.uint32)
                    assert guards, f"hy_poslist_gather wrote outside its output, {where}"
                    assert got.tobytes() == want_through.tobytes(), f"hy_poslist_gather, {where}"
                    untouched(lists_column, d_through)


# ---- output buffers in caller device memory, off the 16-byte grid -----------------------------------------------------------------------
def test_sort_output_off_the_grid(device):
    rng = np.random.default_rng(4)
    values = values_of(rng, "value", np.int32)
    column = DeviceColumn(column_of(values, None, "value"))
    want = positions_of(sorted_order([(values, None)], [abi.SORT_ASCENDING_NULLS_FIRST]), list(SIZES))
    keys = (abi.SortKey * 1)()
    keys[0].column, keys[0].mode = column.handle, abi.SORT_ASCENDING_NULLS_FIRST
    for fill in FILLS:
        out = PlacedArray(8 * N, 8, fill)
        n_out = C.c_uint64(0)
        abi.check(device.hy_sort(keys, 1, out.pointer, N, C.byref(n_out)))
        got, guards = out.read(np.uint32)
        assert guards and n_out.value == N and got.tobytes() == want.tobytes(), f"hy_sort into an output at 8 mod 16, fill {fill:#04x}"
        out = PlacedArray(8 * 100, 8, fill)
        path = C.c_uint32(0)
        abi.check(device.hy_sort_limit(keys, 1, 100, 0, out.pointer, 100, C.byref(n_out), C.byref(path)))
        got, guards = out.read(np.uint32)
        assert guards and n_out.value == 100 and got.tobytes() == want[:100].tobytes(), f"hy_sort_limit into an output at 8 mod 16, fill {fill:#04x}"


def device_scan_into(lib, column, predicate, n_chunks, matches, offsets, counts, states):
    result = abi.ScanResult()
    result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH
    result.matches, result.capacity, result.offsets, result.counts, result.chunk_state = matches.pointer, N, offsets.pointer, counts.pointer, states.pointer
    status = lib.hy_table_scan(column.handle, C.byref(predicate), None, 0, C.byref(result))
    abi.check(lib.hy_synchronize())
    return status, result


def test_scan_and_translate_outputs_off_the_grid(device):
    """hy_table_scan's device-memory result: the regions are written two RowIDs per store, so `matches` off a 16-byte boundary (and offsets /
    counts off their element size) is refused with nothing written; on it -- with chunk states at 1 modulo 16 and 64 guard bytes around
    every array -- the result is the oracle's.  hy_poslist_translate writes RowID by RowID: its `out` at 8 modulo 16."""
    rng = np.random.default_rng(6)
    values = values_of(rng, "dictionary2", np.int32)
    host = column_of(values, None, "dictionary2")
    predicate = make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, 100)
    want = oracle_scan(host, predicate, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    want_list = expected_pos_list(host, predicate)
    n_chunks = host.n_chunks
    for fill in FILLS:
        column = PlacedColumn(host, "last", fill)
        for at in ((8, 0, 0), (0, 4, 0), (0, 0, 2)):   # one array off its boundary at a time
            arrays = PlacedArray(8 * N, at[0], fill), PlacedArray(8 * (n_chunks + 1), at[1], fill), PlacedArray(4 * n_chunks, at[2], fill), PlacedArray(n_chunks, 1, fill)
            status, _ = device_scan_into(device, column, predicate, n_chunks, *arrays)
            assert status == abi.ERR_INVALID, f"scan result at {at} modulo 16"
            untouched(*arrays)   # nothing was written
        matches, offsets, counts, states = PlacedArray(8 * N, 0, fill), PlacedArray(8 * (n_chunks + 1), 8, fill), PlacedArray(4 * n_chunks, 4, fill), PlacedArray(n_chunks, 1, fill)
        status, result = device_scan_into(device, column, predicate, n_chunks, matches, offsets, counts, states)
        assert status == abi.OK
        (got_matches, g0), (got_offsets, g1), (got_counts, g2), (got_states, g3) = matches.read(np.uint32), offsets.read(np.uint64), counts.read(np.uint32), states.read(np.uint8)
        assert g0 and g1 and g2 and g3, f"hy_table_scan wrote outside its device-memory outputs, fill {fill:#04x}"
        np.testing.assert_array_equal(got_counts, want.counts[:n_chunks])
        np.testing.assert_array_equal(got_states, want.chunk_state[:n_chunks])
        got_matches = got_matches.reshape(-1, 2)
        for c in range(n_chunks):
            expected = want.pos_list(c)
            assert got_matches[int(got_offsets[c]):int(got_offsets[c]) + len(expected)].tobytes() == expected.tobytes(), f"chunk {c}, fill {fill:#04x}"
        for layout in (abi.POSLIST_DENSE, abi.POSLIST_CHUNK_REGIONS):
            out = PlacedArray(8 * N, 8, fill)
            written = C.c_uint64(0)
            abi.check(device.hy_poslist_translate(column.handle, C.byref(result), layout, out.pointer, N, C.byref(written)))
            abi.check(device.hy_synchronize())
            got, guards = out.read(np.uint32)
            got = got.reshape(-1, 2)
            assert guards and written.value == len(want_list), f"hy_poslist_translate layout {layout}, fill {fill:#04x}"
            if layout == abi.POSLIST_DENSE:
                got = got[:written.value]
            else:
                got = np.concatenate([got[int(got_offsets[c]):int(got_offsets[c]) + int(got_counts[c])] for c in range(n_chunks)])
            assert got.tobytes() == want_list.tobytes(), f"hy_poslist_translate layout {layout}, fill {fill:#04x}"
        untouched(column)


def test_join_output_off_the_grid(device):
    """hy_join_hash's device-memory result: the emitting kernels store two pairs at a time, so lists off a 16-byte boundary are refused
    before any launch with nothing written; lists on one (64 guard bytes around them, slice offsets at 8 modulo 16) hold the oracle's pairs."""
    shape, build, probe = next(join_shapes())
    want = oracle_join(build, probe, abi.JOIN_INNER)
    b, p = DeviceColumn(build), DeviceColumn(probe)
    capacity, slice_capacity = probe.rows, 700
    for fill in FILLS:
        for left_at, right_at, slices_at, refused in ((8, 0, 0, True), (0, 8, 0, True), (0, 0, 4, True), (0, 0, 8, False)):
            left, right, slices = PlacedArray(8 * capacity, left_at, fill), PlacedArray(8 * capacity, right_at, fill), PlacedArray(8 * (slice_capacity + 2), slices_at, fill)
            r = abi.JoinResult()
            r.mem, r.radix_bits, r.left_pos, r.right_pos, r.capacity, r.slice_offsets, r.slice_capacity = abi.MEM_DEVICE, 0xFFFFFFFF, left.pointer, right.pointer, capacity, slices.pointer, slice_capacity
            status = device.hy_join_hash(b.handle, p.handle, abi.JOIN_INNER, C.byref(r))
            abi.check(device.hy_synchronize())
            where = f"lists at {left_at}, {right_at}, slice offsets at {slices_at} modulo 16, fill {fill:#04x}"
            if refused:
                assert status == abi.ERR_INVALID, where
                untouched(left, right, slices)
                continue
            assert status == abi.OK, where
            n, n_slices = int(r.n_pairs), int(r.n_slices)
            (got_left, g0), (got_right, g1), (got_slices, g2) = left.read(np.uint32), right.read(np.uint32), slices.read(np.uint64)
            assert g0 and g1 and g2, f"hy_join_hash wrote outside its device-memory outputs, {where}"
            assert n == want.n_pairs and n_slices == want.c.n_slices
            assert got_left[:2 * n].tobytes() == want.left[:n].tobytes() and got_right[:2 * n].tobytes() == want.right[:n].tobytes(), where
            np.testing.assert_array_equal(got_slices[:n_slices + 1], want.slice_offsets[:n_slices + 1])


def test_aggregate_output_off_the_grid(device):
    """hy_aggregate_hash's device-memory result is copied into place: RowIDs at 8, 8-byte values at 8, 4-byte values at 4, NULL flags at 1 modulo 16."""
    rng = np.random.default_rng(17)
    keys = column_of(rng.integers(0, 300, N).astype(np.int32), rng.random(N) < 0.01, "dictionary2")
    ints = column_of(rng.integers(-1000, 1000, N).astype(np.int32), rng.random(N) < 0.1, "frame_of_reference2")
    floats = column_of(rng.random(N).astype(np.float32), None, "value")
    spec = [(abi.AGG_SUM, ints), (abi.AGG_AVG, floats), (abi.AGG_MIN, ints), (abi.AGG_MAX, floats), (abi.AGG_COUNT, None)]
    want = oracle_aggregate([keys], spec)
    made = {id(c): DeviceColumn(c) for c in (keys, ints, floats)}
    capacity = 512
    for fill in FILLS:
        rows = PlacedArray(8 * capacity, 8, fill)
        values = [PlacedArray(8 * capacity, 4 if function in (abi.AGG_MIN, abi.AGG_MAX) else 8, fill) for function, _ in spec]
        nulls = [PlacedArray(capacity, 1, fill) for _ in spec]
        columns = (abi.AggregateColumn * len(spec))()
        for a in range(len(spec)):
            columns[a].values, columns[a].is_null = values[a].pointer, nulls[a].pointer
        result = abi.AggregateResult()
        result.mem, result.group_capacity, result.group_row_ids, result.columns = abi.MEM_DEVICE, capacity, rows.pointer, columns
        garr = (C.c_void_p * 1)(made[id(keys)].handle)
        specs = (abi.AggregateSpec * len(spec))()
        for i, (function, column) in enumerate(spec):
            specs[i].function, specs[i].column = function, made[id(column)].handle if column is not None else None
        abi.check(device.hy_aggregate_hash(garr, 1, specs, len(spec), C.byref(result)))
        groups = int(result.n_groups)
        got_rows, guards = rows.read(np.uint32)
        assert guards and groups == want.n_groups and got_rows[:2 * groups].tobytes() == want.row_ids[:groups].tobytes()

        class Got:
            n_groups, row_ids = groups, got_rows.reshape(-1, 2)

            @staticmethod
            def column(a):
                raw, value_guards = values[a].read(np.uint8)
                flags, null_guards = nulls[a].read(np.uint8)
                assert value_guards and null_guards, f"aggregate {a}: written outside the output"
                cells = raw.view({abi.TYPE_INT: np.int32, abi.TYPE_LONG: np.int64, abi.TYPE_FLOAT: np.float32, abi.TYPE_DOUBLE: np.float64}[columns[a].data_type])[:groups]
                return [None if flags[i] else cells[i].item() for i in range(groups)]

        assert_aggregate_equal(Got, want, len(spec), f"device-memory aggregate result, fill {fill:#04x}")


def test_sort_merge_and_union_outputs_off_the_grid(device):
    """hy_join_sort_merge and hy_union_positions write RowID by RowID: lists at 8 modulo 16 hold the oracle's rows between intact guards; lists
    off an 8-byte boundary are refused with HY_ERR_INVALID and nothing written."""
    import test_join_sort_merge_gpu as smj
    import test_union_positions_gpu as union
    from union_positions_oracle import union_positions as oracle_union
    rng = np.random.default_rng(2)
    left = smj.Side(rng.integers(0, 60, 2_056).astype(np.int32), rng.random(2_056) < 0.1, chunk=[2_051, 5], kind="dictionary")
    right = smj.Side(rng.integers(0, 60, 300).astype(np.int32), None, chunk=[295, 5], kind="value")
    want = smj.ordered_join(left.values, left.nulls, right.values, right.nulls, smj.INNER, smj.EQ)
    want_left, want_right = smj.row_ids(want[0], left.sizes), smj.row_ids(want[1], right.sizes)
    n = len(want[0])
    table = union.Table(N, 4_096)
    sides = [table.positions(np.flatnonzero(table.values % 3 != 0)), table.positions(np.flatnonzero(table.values % 5 < 3))]
    union_columns = [union.host_lists(table, union.split(side, [int(k) for k in np.bincount(side[:, 0], minlength=table.host.n_chunks)])) for side in sides]
    want_union = oracle_union([sides[0]], [sides[1]])[0]
    for fill in FILLS:
        for at, refused in ((8, False), (4, True)):
            lists = [PlacedArray(8 * n, at, fill) for _ in range(2)]
            result = abi.SortMergeResult()
            result.mem, result.capacity, result.left_pos, result.right_pos = abi.MEM_DEVICE, n, lists[0].pointer, lists[1].pointer
            status = device.hy_join_sort_merge(left.column.handle, right.column.handle, smj.INNER, smj.EQ, C.byref(result))
            abi.check(device.hy_synchronize())
            if refused:
                assert status == abi.ERR_INVALID
                untouched(*lists)
            else:
                assert status == abi.OK and int(result.n_pairs) == n
                (got_left, g0), (got_right, g1) = lists[0].read(np.uint32), lists[1].read(np.uint32)
                assert g0 and g1 and got_left.tobytes() == want_left.tobytes() and got_right.tobytes() == want_right.tobytes(), f"hy_join_sort_merge lists at 8 modulo 16, fill {fill:#04x}"
            capacity = len(sides[0]) + len(sides[1])
            out = PlacedArray(8 * capacity, at, fill)
            handles = [(C.c_void_p * 1)(column.handle) for column in union_columns]
            pointers = (C.c_void_p * 1)(out.pointer)
            n_out, path = C.c_uint64(0), C.c_uint32(0)
            status = device.hy_union_positions(handles[0], handles[1], 1, 0, pointers, capacity, C.byref(n_out), C.byref(path))
            abi.check(device.hy_synchronize())
            if refused:
                assert status == abi.ERR_INVALID
                untouched(out)
            else:
                got, guards = out.read(np.uint32)
                assert status == abi.OK and guards and n_out.value == len(want_union) and got[:2 * len(want_union)].tobytes() == want_union.tobytes(), f"hy_union_positions out at 8 modulo 16, fill {fill:#04x}"


# ---- hy_star_join_aggregate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [2, 1, 0], ids=["fused_finish", "fused_probe", "join_by_join"])
@pytest.mark.parametrize("case", ["filtered", "dangling_foreign_keys"])
def test_star_join_aggregate(device, options, case, fused):
    """The `filtered` and `dangling_foreign_keys` tables of test_ssb_gpu.test_star_join_aggregate_small_tables with every fact and dimension
    column placed; which path ran is asserted for the uploaded and the `aligned` columns."""
    from hyrise_amd.operators import star_join_aggregate
    from test_ssb_gpu import star_was_fused
    rng = np.random.default_rng(len(case))
    n_fact, n_a, n_b = sum(PROBE_SIZES), 3_000, 500
    a_key = np.arange(1, n_a + 1, dtype=np.int32) * 3
    a_group, a_filter = rng.integers(0, 7, n_a).astype(np.int32), rng.integers(0, 10, n_a).astype(np.int32)
    b_key = rng.permutation(n_b).astype(np.int32) + 100
    b_group, b_filter = rng.integers(0, 5, n_b).astype(np.int32), rng.integers(0, 4, n_b).astype(np.int32)
    fk_a, fk_b = a_key[rng.integers(0, n_a, n_fact)].copy(), b_key[rng.integers(0, n_b, n_fact)].copy()
    if case == "dangling_foreign_keys":
        fk_a[rng.random(n_fact) < 0.3] = 1
        fk_b[rng.random(n_fact) < 0.2] = 99
    x, y = rng.integers(-1000, 1000, n_fact).astype(np.int32), rng.integers(0, 50, n_fact).astype(np.int32)
    a_sizes, b_sizes = (1_024, 1_024, 952), (200, 200, 100)
    hosts = {"a_key": column_of(a_key, None, "value", a_sizes), "a_group": column_of(a_group, None, "dictionary1", a_sizes), "a_filter": column_of(a_filter, None, "frame_of_reference1", a_sizes),
             "b_key": column_of(b_key, None, "value", b_sizes), "b_group": column_of(b_group, None, "frame_of_reference1", b_sizes), "b_filter": column_of(b_filter, None, "dictionary1", b_sizes),
             "fk_a": column_of(fk_a, None, "frame_of_reference2", PROBE_SIZES), "fk_b": column_of(fk_b, None, "frame_of_reference2", PROBE_SIZES),
             "x": column_of(x, None, "frame_of_reference2", PROBE_SIZES), "y": column_of(y, None, "dictionary1", PROBE_SIZES)}
    a_of, b_of = {int(k): i for i, k in enumerate(a_key)}, {int(k): i for i, k in enumerate(b_key)}
    ia, ib = np.array([a_of.get(int(k), -1) for k in fk_a]), np.array([b_of.get(int(k), -1) for k in fk_b])
    keep = (ia >= 0) & (ib >= 0) & (a_filter[np.maximum(ia, 0)] < 3) & (b_filter[np.maximum(ib, 0)] != 2)
    want = {}
    for ga, gb, xv, yv in zip(a_group[ia[keep]], b_group[ib[keep]], x[keep].astype(np.int64), y[keep].astype(np.int64)):
        cell = want.setdefault((int(ga), int(gb)), [0, 0, 0])
        cell[0] += int(xv)
        cell[1] += int(xv) * int(yv)
        cell[2] += 1
    options.set(abi.OPT_STAR_FUSED_PROBE, 1 if fused else 0)
    options.set(abi.OPT_STAR_FUSED_FINISH, 1 if fused == 2 else 0)
    paths = {}
    for name in ["uploaded"] + [f"{placement}/{fill:#04x}" for placement, fill in COMBOS]:
        c = {key: (DeviceColumn(host) if name == "uploaded" else PlacedColumn(host, name.split("/")[0], int(name.split("/")[1], 16))) for key, host in hosts.items()}
        dimensions = [(c["a_key"], c["a_filter"], make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, 3), c["fk_a"]), (c["b_key"], c["b_filter"], make_predicate(abi.PRED_NOT_EQUALS, abi.TYPE_INT, 2), c["fk_b"])]
        groupby = [(1, c["a_group"]), (2, c["b_group"])]
        aggregates = [(abi.AGG_SUM, (0, c["x"]), None, None), (abi.AGG_SUM, (0, c["x"]), abi.ARITH_MUL, (0, c["y"])), (abi.AGG_COUNT, None, None, None),
                      (abi.AGG_MIN, groupby[0], None, None), (abi.AGG_MIN, groupby[1], None, None)]
        result, joined = star_join_aggregate(dimensions, groupby, aggregates)
        paths[name] = star_was_fused()
        assert joined == int(keep.sum()), f"{case} {name}: rows of the join result"
        cells = [result.column(a) for a in range(5)]
        got = {(cells[3][i], cells[4][i]): [cells[0][i], cells[1][i], cells[2][i]] for i in range(result.n_groups)}
        assert got == want, f"{case} {name}"
        untouched(*c.values())
    assert paths["uploaded"] == fused, f"{case}: the uploaded columns did not take path {fused}"
    for fill in FILLS:
        assert paths[f"aligned/{fill:#04x}"] == fused, f"{case}: the aligned control left path {fused}"

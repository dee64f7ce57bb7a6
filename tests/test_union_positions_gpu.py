"""UnionPositions on the device (hy_union_positions): every case byte-equal to tests/union_positions_oracle.py, all n_clusters output lists
compared.  The kernels' boundaries: 64 rows per wave, 256 per workgroup step and 8 192 per slice in union_flatten; 2 048 merged rows per tile
in union_merge / union_emit."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import make_predicate, table_scan, union_positions
from hyrise_amd.storage import DeviceColumn
from support import DeviceArray
from union_positions_oracle import NULL_ROW_ID, union_positions as oracle_union

pytestmark = pytest.mark.gpu

TILE, SLICE, STEP, WAVE = 2048, 8192, 256, 64


class Table:
    """A data table of one int32 column in chunks of `chunk` rows, on the device: what the PosLists of the tests point into."""

    def __init__(self, rows, chunk, values=None):
        self.values = np.arange(rows, dtype=np.int32) if values is None else values
        self.chunk = chunk
        self.host = storage.make_column(self.values, None, abi.ENC_UNENCODED, chunk_size=chunk)
        self.device = DeviceColumn(self.host)

    def positions(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return np.stack([rows // self.chunk, rows % self.chunk], axis=1).astype(np.uint32)


def split(positions, chunk_sizes):
    """An (n, 2) list cut into the chunks of a reference table."""
    assert sum(chunk_sizes) == len(positions)
    out, at = [], 0
    for size in chunk_sizes:
        out.append(positions[at:at + size])
        at += size
    return out


def chunks_of(n, size):
    return [min(size, n - b) for b in range(0, n, size)] or [0]


def host_lists(table, pos_lists):
    """A reference column whose PosLists arrive in host memory (int k: the EntireChunkPosList of chunk k)."""
    return DeviceColumn(storage.make_reference_column(table.host, pos_lists), refs={id(table.host): table.device})


class DeviceLists:
    """A reference column whose PosLists already lie in device memory (HY_MEM_DEVICE): back to back in one buffer (`gap` = 0, the dense
    output of an operator, which the library reads in place) or `gap` RowIDs apart."""

    def __init__(self, lib, table, pos_lists, gap=0):
        self.lib = lib
        sizes = [len(p) for p in pos_lists]
        starts = np.concatenate([[0], np.cumsum([s + gap for s in sizes])]).astype(np.int64)
        staged = np.zeros((max(1, int(starts[-1])), 2), dtype=np.uint32)
        for p, s in zip(pos_lists, starts):
            staged[s:s + len(p)] = p
        self.buffer = DeviceArray(lib, staged.shape, np.uint32)
        abi.check(lib.hy_memcpy_h2d(self.buffer.pointer, staged.ctypes.data, staged.nbytes))
        self.segments = (abi.Segment * max(1, len(sizes)))()
        for i, size in enumerate(sizes):
            d = self.segments[i]
            d.encoding, d.data_type, d.size, d.width = abi.ENC_REFERENCE, table.host.data_type, size, 8
            d.data = self.buffer.pointer + 8 * int(starts[i])
            d.ref_chunk_id = abi.INVALID_CHUNK_ID
            d.ref = table.device.handle
        self.handle = C.c_void_p()
        abi.check(lib.hy_column_create(self.segments, len(sizes), abi.MEM_DEVICE, C.byref(self.handle)))
        self.rows, self.n_chunks = sum(sizes), len(sizes)

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None


def check_union(left_columns, right_columns, left_lists, right_lists, path=None, force_sort=False, context=""):
    """left_lists / right_lists: per cluster the side's RowIDs in table order, for the oracle."""
    got = union_positions(left_columns, right_columns, force_sort=force_sort)
    want = oracle_union(left_lists, right_lists)
    assert got.rows == len(want[0]), f"{context}: {got.rows} rows, want {len(want[0])}"
    for c in range(len(want)):
        result = got.numpy(c)
        if result.tobytes() != want[c].tobytes():
            bad = int(np.flatnonzero(np.any(result != want[c], axis=1))[0])
            pytest.fail(f"{context}: cluster {c}, first difference at output row {bad}: got {result[bad]}, want {want[c][bad]}")
    if path is not None:
        assert got.path == path, f"{context}: path {got.path}, want {path}"
    got.close()
    return want


def scan_lists(table, mask):
    """What a TableScan hands on: per chunk of the table the ascending positions of the matching rows."""
    rows = np.flatnonzero(mask)
    per_chunk = np.bincount(rows // table.chunk, minlength=table.host.n_chunks)
    return table.positions(rows), [int(n) for n in per_chunk]


SCAN_PAIRS = {
    "disjoint": (lambda v: v % 4 == 0, lambda v: v % 4 == 1),
    "overlapping": (lambda v: v % 3 != 0, lambda v: v % 5 < 3),
    "identical": (lambda v: v % 7 < 3, lambda v: v % 7 < 3),
    "left_empty": (lambda v: v < 0, lambda v: v % 2 == 0),
    "right_empty": (lambda v: v % 2 == 0, lambda v: v < 0),
    "both_empty": (lambda v: v < 0, lambda v: v < 0),
}


@pytest.mark.parametrize("force_sort", [False, True], ids=["in_order", "force_sort"])
@pytest.mark.parametrize("lists", ["host", "device"])
@pytest.mark.parametrize("case", list(SCAN_PAIRS))
def test_two_scans_of_one_table(device, case, lists, force_sort):
    table = Table(50_000, 7_000)
    p, q = SCAN_PAIRS[case]
    sides = []
    for predicate in (p, q):
        positions, sizes = scan_lists(table, predicate(table.values))
        pos_lists = split(positions, sizes)
        sides.append((host_lists(table, pos_lists) if lists == "host" else DeviceLists(device, table, pos_lists), positions))
    want = check_union([sides[0][0]], [sides[1][0]], [sides[0][1]], [sides[1][1]], path=3 if force_sort else 0, force_sort=force_sort, context=case)
    np.testing.assert_array_equal(want[0], table.positions(np.flatnonzero(p(table.values) | q(table.values))))


@pytest.mark.parametrize("seed", range(4))
def test_union_of_two_real_scans_is_the_scan_of_the_disjunction(device, seed):
    """Without the oracle: union(scan(p), scan(q)) == the positions of flatnonzero(p | q), the scans being hy_table_scan's."""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 1000, 200_000).astype(np.int32)
    table = Table(len(values), 20_011, values)
    a, b, c = sorted(int(x) for x in rng.integers(0, 1000, 3))
    scans = [(make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, a), values < a),
             (make_predicate(abi.PRED_BETWEEN_UPPER_EXCLUSIVE, abi.TYPE_INT, b, c + 1), (values >= b) & (values < c + 1))]
    columns, keep = [], []
    for predicate, mask in scans:
        result = table_scan(table.device, predicate)
        assert result.total == int(mask.sum())
        pos_lists = [result.pos_list(k).copy() for k in range(table.host.n_chunks)]
        columns.append(DeviceLists(device, table, pos_lists) if seed % 2 else host_lists(table, pos_lists))
        keep.append(pos_lists)
    got = union_positions([columns[0]], [columns[1]])
    assert got.path == 0
    np.testing.assert_array_equal(got.numpy(0), table.positions(np.flatnonzero(scans[0][1] | scans[1][1])))
    got.close()


def random_side(rng, n, n_clusters, domain, nulls=0.0):
    """n rows of n_clusters RowIDs drawn from few values (many duplicates), in no order."""
    out = []
    for _ in range(n_clusters):
        pos = np.stack([rng.integers(0, domain, n), rng.integers(0, domain, n)], axis=1).astype(np.uint32)
        if nulls:
            pos[rng.random(n) < nulls] = NULL_ROW_ID
        out.append(pos)
    return out


@pytest.mark.parametrize("n_clusters", [1, 2, 3, 8])
def test_shuffled_sides_with_duplicates_and_null_row_ids(device, n_clusters):
    """A join's output on both sides: no order, duplicates within a side (m < n, m = n, m > n all occur), NULL_ROW_ID rows; host lists on the
    left, device lists (apart and back to back) on the right."""
    rng = np.random.default_rng(n_clusters)
    table = Table(64, 8)
    left, right = random_side(rng, 9_000, n_clusters, 3, nulls=0.1), random_side(rng, 7_000, n_clusters, 3, nulls=0.1)
    left_columns = [host_lists(table, split(pos, chunks_of(9_000, 1_000))) for pos in left]
    right_columns = [DeviceLists(device, table, split(pos, chunks_of(7_000, 3_000)), gap=(c % 2) * 5) for c, pos in enumerate(right)]
    check_union(left_columns, right_columns, left, right, path=3, context=f"{n_clusters} clusters")


@pytest.mark.parametrize("n_clusters", [1, 2, 3, 8])
def test_only_the_last_cluster_differs(device, n_clusters):
    rng = np.random.default_rng(10 + n_clusters)
    table = Table(64, 8)

    def side(n):
        same = [np.tile(np.array([[c, 5]], dtype=np.uint32), (n, 1)) for c in range(n_clusters - 1)]
        return same + [np.stack([rng.integers(0, 4, n), rng.integers(0, 50, n)], axis=1).astype(np.uint32)]

    left, right = side(5_000), side(6_000)
    columns = [[host_lists(table, split(pos, chunks_of(len(pos), 1_500))) for pos in s] for s in (left, right)]
    check_union(columns[0], columns[1], left, right, path=3)
    # ... and in order: the same rows sorted by the last cluster are sorted rows
    ordered = []
    for s in (left, right):
        keys = (s[-1][:, 0].astype(np.uint64) << np.uint64(32)) | s[-1][:, 1]
        ordered.append([pos[np.argsort(keys, kind="stable")] for pos in s])
    columns = [[host_lists(table, split(pos, chunks_of(len(pos), 1_500))) for pos in s] for s in ordered]
    check_union(columns[0], columns[1], ordered[0], ordered[1], path=0)


def test_nine_clusters_are_refused(device):
    table = Table(64, 8)
    column = host_lists(table, [table.positions(np.arange(8))])
    with pytest.raises(abi.HyriseAmdError) as error:
        union_positions([column] * 9, [column] * 9)
    assert error.value.status == abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("m,n", [(1, 3), (3, 3), (3, 1), (0, 2), (2, 0), (TILE + 5, 3 * TILE), (3 * TILE, TILE + 5), (2 * TILE, 2 * TILE)])
def test_runs_of_equal_rows(device, m, n):
    """One row m times on the left and n times on the right, between other rows: max(m, n) copies -- runs longer than a tile included."""
    table = Table(64, 8)
    other = table.positions(np.arange(0, 64, 3))
    run = np.array([[3, 4]], dtype=np.uint32)   # (row 28: not among `other`)
    left = np.concatenate([other[:10], np.repeat(run, m, axis=0), other[10:]])
    right = np.concatenate([np.repeat(run, n, axis=0), other[5:]])
    for shuffle in (False, True):
        if shuffle:
            rng = np.random.default_rng(m * 7 + n)
            left, right = left[rng.permutation(len(left))], right[rng.permutation(len(right))]
        else:
            left, right = (s[np.lexsort((s[:, 1], s[:, 0]))] for s in (left, right))
        columns = [host_lists(table, split(s, chunks_of(len(s), 1_000))) for s in (left, right)]
        want = check_union([columns[0]], [columns[1]], [left], [right], path=3 if shuffle else 0, context=f"m {m} n {n} shuffled {shuffle}")
        assert int(np.sum(np.all(want[0] == run, axis=1))) == max(m, n)


@pytest.mark.parametrize("rows", [(1, 0), (0, 1), (1, 1), (5 * TILE, 4 * TILE)])
def test_every_row_is_the_same_row(device, rows):
    table = Table(64, 8)
    for row in ((2, 1), NULL_ROW_ID):
        left, right = (np.tile(np.array([row], dtype=np.uint32), (n, 1)) for n in rows)
        columns = [host_lists(table, split(s, chunks_of(len(s), 3_000))) for s in (left, right)]
        for force_sort in (False, True):
            got = check_union([columns[0]], [columns[1]], [left], [right], path=3 if force_sort else 0, force_sort=force_sort)
            assert len(got[0]) == max(rows)


def test_entire_chunk_host_and_device_lists_mixed(device):
    """Left: cluster 0 = EntireChunkPosLists and host lists mixed within one column, cluster 1 = device lists back to back (read in place);
    right: the other way round, device lists apart."""
    rng = np.random.default_rng(5)
    table = Table(40, 8)   # chunks of 8 rows
    entire = lambda k: table.positions(np.arange(8 * k, 8 * k + 8))
    left0 = [1, table.positions([3, 4, 17]), 0, 4]
    left0_rows = np.concatenate([entire(1), left0[1], entire(0), entire(4)])
    left1_rows = random_side(rng, len(left0_rows), 1, 4)[0]
    right1 = [2, 2, table.positions([39, 0])]
    right1_rows = np.concatenate([entire(2), entire(2), right1[2]])
    right0_rows = np.concatenate([left0_rows[:10], left0_rows[:8]])
    left1_rows[:10] = right1_rows[:10]   # (some rows on both sides)
    sizes_left, sizes_right = [8, 3, 8, 8], [8, 8, 2]
    left_columns = [host_lists(table, left0), DeviceLists(device, table, split(left1_rows, sizes_left))]
    right_columns = [DeviceLists(device, table, split(right0_rows, sizes_right), gap=3), host_lists(table, right1)]
    check_union(left_columns, right_columns, [left0_rows, left1_rows], [right0_rows, right1_rows], path=3)
    # in order, single cluster: entire-chunk lists of ascending chunks are a scan's all-match chunks
    ascending = [0, table.positions([8, 9, 15]), 3, 4]
    rows = np.concatenate([entire(0), ascending[1], entire(3), entire(4)])
    other = table.positions(np.arange(5, 30))
    check_union([host_lists(table, ascending)], [DeviceLists(device, table, split(other, [20, 5]))], [rows], [other], path=0)


BOUNDARIES = sorted({b + d for b in (WAVE, STEP, TILE, 2 * TILE, SLICE, 2 * SLICE) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", BOUNDARIES)
def test_sizes_around_every_boundary(device, n):
    """A side of n rows (wave, workgroup step, slice) and n merged rows in all (tile), in one chunk and in chunks that end off the boundaries."""
    table = Table(3 * SLICE + 10, 5_000)
    rng = np.random.default_rng(n)
    left_rows = np.sort(rng.choice(3 * SLICE, n, replace=False))
    right_rows = np.sort(rng.choice(3 * SLICE, n // 2, replace=False))
    for left, right in ((left_rows, right_rows), (left_rows[:n - n // 2], right_rows)):   # n rows on the left; n merged rows
        lists = [table.positions(left), table.positions(right)]
        for chunk in (1 << 30, 1_000):
            columns = [host_lists(table, split(s, chunks_of(len(s), chunk))) for s in lists]
            check_union([columns[0]], [columns[1]], [lists[0]], [lists[1]], path=0, context=f"n {n} chunk {chunk}")
            check_union([columns[1]], [columns[0]], [lists[1]], [lists[0]], path=3, force_sort=True, context=f"n {n} chunk {chunk} forced")


@pytest.mark.parametrize("lists", ["host", "device"])
@pytest.mark.parametrize("descent", [1, WAVE, STEP, SLICE, 2 * SLICE, 1_000, 3 * SLICE + 99])
def test_a_side_out_of_order_at_one_boundary_only(device, descent, lists):
    """Ascending but for ONE row that is smaller than its predecessor, which sits at the first row of a wave / a workgroup step / a slice / a
    chunk (chunks of 1 000 rows) or at the last row: the side must be found unordered (path bit 1 only) and the result be right."""
    table = Table(4 * SLICE, 5_000)
    n = 3 * SLICE + 100
    ascending = np.arange(n) + 50
    right_rows = np.concatenate([ascending[n - descent:], ascending[:n - descent]])   # row `descent` is the smallest, all others ascend
    assert np.flatnonzero(np.diff(right_rows) < 0).tolist() == [descent - 1]
    left, right = table.positions(np.arange(0, 4 * SLICE, 3)), table.positions(right_rows)
    make = (lambda pos, chunk: host_lists(table, split(pos, chunks_of(len(pos), chunk)))) if lists == "host" else \
        (lambda pos, chunk: DeviceLists(device, table, split(pos, chunks_of(len(pos), chunk))))
    check_union([make(left, 1_000)], [make(right, 1_000)], [left], [right], path=2, context=f"descent at {descent}")


def test_capacity_and_argument_errors(device):
    table = Table(1_000, 300)
    left, right = table.positions(np.arange(0, 600)), table.positions(np.arange(400, 1_000))
    columns = [host_lists(table, split(s, chunks_of(len(s), 250))) for s in (left, right)]
    with pytest.raises(abi.HyriseAmdError) as error:
        union_positions([columns[0]], [columns[1]], capacity=999)
    assert error.value.status == abi.ERR_CAPACITY
    got = union_positions([columns[0]], [columns[1]], capacity=1_000)   # (exactly the output's rows)
    np.testing.assert_array_equal(got.numpy(0), table.positions(np.arange(1_000)))
    got.close()
    with pytest.raises(abi.HyriseAmdError) as error:   # a data column is no reference table
        union_positions([table.device], [columns[1]])
    assert error.value.status == abi.ERR_INVALID
    shorter = host_lists(table, split(left[:500], [250, 250]))
    with pytest.raises(abi.HyriseAmdError) as error:   # clusters of different row counts
        union_positions([columns[0], shorter], [columns[1], columns[1]])
    assert error.value.status == abi.ERR_INVALID and "rows" in str(error.value)


def test_full_size_two_scans_of_a_60m_row_column(device):
    """Two scans over a 60 M-row, 916-chunk column that select about half the rows each: device lists as the scans leave them."""
    rows = 60_000_000
    rng = np.random.default_rng(77)
    values = rng.integers(0, 100, rows, dtype=np.int32)
    table = Table(rows, abi.CHUNK_DEFAULT_SIZE, values)
    assert table.host.n_chunks == 916
    masks = [values < 50, (values >= 30) & (values < 80)]
    columns, lists = [], []
    for mask in masks:
        positions, sizes = scan_lists(table, mask)
        columns.append(DeviceLists(device, table, split(positions, sizes)))
        lists.append(positions)
    want = table.positions(np.flatnonzero(masks[0] | masks[1]))
    for force_sort in (False, True):
        got = union_positions([columns[0]], [columns[1]], force_sort=force_sort)
        assert got.path == (3 if force_sort else 0) and got.rows == len(want)
        assert got.numpy(0).tobytes() == want.tobytes()
        got.close()
    oracle = oracle_union([lists[0]], [lists[1]])
    assert oracle[0].tobytes() == want.tobytes()
    with pytest.raises(abi.HyriseAmdError) as error:
        union_positions([columns[0]], [columns[1]], capacity=len(want) - 1)
    assert error.value.status == abi.ERR_CAPACITY

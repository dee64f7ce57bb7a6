"""Product on the device (hy_product, hy_product_count): both lists and pair_offsets byte for byte against tests/product_oracle.py, with
host-memory and device-memory results, the device lists on 16-byte boundaries and 8 bytes off them, canary rows around every list.
The kernel's boundaries: 2 rows per 16-byte store, 512 rows per workgroup step, tiles cut at multiples of 8 192 output rows and at every
pair's end."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import make_predicate, product, product_count, table_scan
from hyrise_amd.storage import DeviceColumn
from product_oracle import NULL_ROW_ID, product_numpy
from support import DeviceArray

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
CANARY = 16   # rows in front of and behind every list


def carrier(sizes, dtype=np.int32):
    """A data column with these chunk sizes: only its layout matters."""
    return DeviceColumn(storage.HostColumn([storage.encode_segment(np.zeros(n, dtype=dtype), None, abi.ENC_UNENCODED) for n in sizes], storage.TYPE_OF_NP[np.dtype(dtype)]))


class Lists:
    """One result buffer per list, SENTINEL everywhere: CANARY rows, `off` more (0 or 1: the list then lies 8 bytes off a 16-byte boundary),
    `capacity` rows for the list, CANARY rows."""

    def __init__(self, lib, mem, capacity, off):
        self.lib, self.mem, self.capacity, self.start = lib, mem, capacity, CANARY + off
        self.host = [np.full((self.start + capacity + CANARY, 2), SENTINEL, dtype=np.uint32) for _ in range(2)]
        self.device = []
        if mem == abi.MEM_DEVICE:
            for host in self.host:
                self.device.append(DeviceArray(lib, host.shape, np.uint32))
                assert self.device[-1].pointer % 16 == 0
                abi.check(lib.hy_memcpy_h2d(self.device[-1].pointer, host.ctypes.data, host.nbytes))

    def pointer(self, side):
        base = self.device[side].pointer if self.mem == abi.MEM_DEVICE else self.host[side].ctypes.data
        return base + 8 * self.start

    def fetch(self):
        for host, device in zip(self.host, self.device):
            abi.check(self.lib.hy_memcpy_d2h(host.ctypes.data, device.pointer, host.nbytes))

    def rows(self, side, n):
        return self.host[side][self.start:self.start + n]

    def untouched_outside(self, side, n):
        return bool((self.host[side][:self.start] == SENTINEL).all() and (self.host[side][self.start + n:] == SENTINEL).all())


def call(lib, left, right, mem, capacity, off=0, want=(True, True)):
    lists = Lists(lib, mem, capacity, off)
    offsets = np.full(left.n_chunks * right.n_chunks + 1, SENTINEL, dtype=np.uint64)
    result = abi.ProductResult()
    result.mem, result.capacity, result.pair_offsets = mem, capacity, offsets.ctypes.data
    result.left_pos, result.right_pos = (lists.pointer(0) if want[0] else None), (lists.pointer(1) if want[1] else None)
    status = lib.hy_product(left.handle, right.handle, C.byref(result))
    lists.fetch()
    return status, result, lists, offsets


def check(lib, left, right, want, context, variants=((abi.MEM_HOST, 0), (abi.MEM_DEVICE, 0), (abi.MEM_DEVICE, 1))):
    """want: the oracle's (left list, right list, pair_offsets)."""
    n = len(want[0])
    assert product_count(left, right) == n, context
    for mem, off in variants:
        where = f"{context} mem={mem} off={off}"
        status, result, lists, offsets = call(lib, left, right, mem, n, off)
        assert status == abi.OK, f"{where}: {lib.hy_last_error().decode()}"
        assert result.n_rows == n, where
        assert offsets.tobytes() == want[2].tobytes(), f"{where}: pair_offsets {offsets.tolist()[:8]}, want {want[2].tolist()[:8]}"
        for side, name in ((0, "left_pos"), (1, "right_pos")):
            got = lists.rows(side, n)
            if got.tobytes() != want[side].tobytes():
                bad = int(np.flatnonzero(np.any(got != want[side], axis=1))[0])
                pytest.fail(f"{where}: {name} differs first at output row {bad} of {n}: got {got[bad]}, want {want[side][bad]}")
            assert lists.untouched_outside(side, n), f"{where}: {name}: a canary row was written"


@pytest.mark.parametrize("left_sizes,right_sizes", [([5, 3, 1], [2, 2, 1]), ([1, 1], [1]), ([1], [513, 1, 64]), ([300, 7], [257, 3]), ([3], [65_535]), ([65_535], [3]),
                                                    ([0, 4, 0], [3, 0, 2]), ([2], [8_191, 2, 8_193])])
def test_data_inputs(device, left_sizes, right_sizes):
    """The reference's own chunking; rows(cr) = 1 (a wrap on every element); one pair over several steps and tiles, regions that start at odd
    row indices and tails shorter than a store; Hyrise's chunk size as a long run and as a long period; empty chunks; cuts around a tile."""
    check(device, carrier(left_sizes), carrier(right_sizes), product_numpy(left_sizes, right_sizes), f"{left_sizes} x {right_sizes}")


def test_a_side_without_chunks(device):
    for left_sizes, right_sizes in (([], [3, 2]), ([4], []), ([], [])):
        left, right = carrier(left_sizes), carrier(right_sizes)
        want = product_numpy(left_sizes, right_sizes)
        assert len(want[0]) == 0 and want[2].tolist() == [0]
        check(device, left, right, want, f"{left_sizes} x {right_sizes}")


class Table:
    """A data table of one int32 column in chunks of `chunk` rows: what the tests' PosLists point into."""

    def __init__(self, rows, chunk):
        self.values, self.chunk = np.arange(rows, dtype=np.int32), chunk
        self.host = storage.make_column(self.values, None, abi.ENC_UNENCODED, chunk_size=chunk)
        self.device = DeviceColumn(self.host)


def host_lists(table, pos_lists, single_chunk_ids=None):
    """A reference column whose PosLists arrive in host memory (int k: the EntireChunkPosList of chunk k)."""
    return DeviceColumn(storage.make_reference_column(table.host, pos_lists, single_chunk_ids), refs={id(table.host): table.device})


class DeviceLists:
    """A reference column whose PosLists already lie in device memory (HY_MEM_DEVICE), back to back in one buffer; int k: an entire-chunk list."""

    def __init__(self, lib, table, pos_lists, single_chunk_ids=None):
        self.lib = lib
        sizes = [table.host.segments[p].size if isinstance(p, int) else len(p) for p in pos_lists]
        staged, starts, at = np.zeros((max(1, sum(sizes)), 2), dtype=np.uint32), [], 0
        for p, size in zip(pos_lists, sizes):
            starts.append(at)
            if not isinstance(p, int):
                staged[at:at + size] = p
                at += size
        self.buffer = DeviceArray(lib, (len(staged) + 2, 2), np.uint32)   # (16 readable bytes behind the last list)
        abi.check(lib.hy_memcpy_h2d(self.buffer.pointer, staged.ctypes.data, staged.nbytes))
        self.segments = (abi.Segment * max(1, len(sizes)))()
        for i, (p, size) in enumerate(zip(pos_lists, sizes)):
            d = self.segments[i]
            d.encoding, d.data_type, d.size, d.width, d.ref = abi.ENC_REFERENCE, table.host.data_type, size, 8, table.device.handle
            d.data = None if isinstance(p, int) else self.buffer.pointer + 8 * starts[i]
            d.ref_chunk_id = p if isinstance(p, int) else abi.INVALID_CHUNK_ID if single_chunk_ids is None else single_chunk_ids[i]
        self.handle = C.c_void_p()
        abi.check(lib.hy_column_create(self.segments, len(sizes), abi.MEM_DEVICE, C.byref(self.handle)))
        self.rows, self.n_chunks = sum(sizes), len(sizes)

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None


def expanded(table, pos_lists):
    """The lists as RowIDs, for the oracle."""
    return [np.stack([np.full(table.host.segments[p].size, p, dtype=np.uint32), np.arange(table.host.segments[p].size, dtype=np.uint32)], axis=1) if isinstance(p, int)
            else np.asarray(p, dtype=np.uint32).reshape(-1, 2) for p in pos_lists]


@pytest.fixture(scope="module")
def reference_inputs(device):
    """Three kinds of PosLists over a table of 2 000 rows in chunks of 700: a real scan's single-chunk lists (50, all 700 and 151 rows of the
    three chunks), a multi-chunk list with NULL_ROW_IDs in it next to a short one, and entire-chunk lists next to a materialised one."""
    table = Table(2_000, 700)
    rng = np.random.default_rng(12)
    scanned = table_scan(table.device, make_predicate(abi.PRED_BETWEEN_INCLUSIVE, abi.TYPE_INT, 650, 1_550), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    scan_chunks = [c for c in range(table.host.n_chunks) if len(scanned.pos_list(c))]
    scan = ([scanned.pos_list(c).copy() for c in scan_chunks], scan_chunks)
    assert [len(p) for p in scan[0]] == [50, 700, 151]
    rows = rng.integers(0, 2_000, 333)
    multi = np.stack([rows // 700, rows % 700], axis=1).astype(np.uint32)
    multi[rng.random(333) < 0.1] = NULL_ROW_ID
    multi[0] = multi[-1] = NULL_ROW_ID
    joined = ([multi, np.array([(2, 599), NULL_ROW_ID, (0, 0)], dtype=np.uint32)], None)
    entire = ([0, np.array([(1, 5), (1, 9), (1, 11)], dtype=np.uint32), 2], [0, 1, 2])
    return table, {"scan": scan, "multi_chunk_with_nulls": joined, "entire_chunk": entire}


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("kind", ["scan", "multi_chunk_with_nulls", "entire_chunk"])
def test_reference_inputs(device, reference_inputs, kind, memory):
    """A reference column on the left, on the right, and on both sides at once, over PosLists in host and in device memory."""
    table, kinds = reference_inputs
    pos_lists, single = kinds[kind]
    column = host_lists(table, pos_lists, single) if memory == "host" else DeviceLists(device, table, pos_lists, single)
    lists = expanded(table, pos_lists)
    sizes = [len(p) for p in lists]
    other_sizes = [3, 130]
    other = carrier(other_sizes)
    variants = ((abi.MEM_DEVICE, 0), (abi.MEM_DEVICE, 1), (abi.MEM_HOST, 0))
    check(device, column, other, product_numpy(sizes, other_sizes, left_lists=lists), f"{kind} ({memory}) x data", variants)
    check(device, other, column, product_numpy(other_sizes, sizes, right_lists=lists), f"data x {kind} ({memory})", variants)
    short_lists, short_single = kinds["multi_chunk_with_nulls"] if kind != "multi_chunk_with_nulls" else kinds["entire_chunk"]
    short_lists, short_single = short_lists[1:2], None if short_single is None else short_single[1:2]
    short = host_lists(table, short_lists, short_single) if memory == "device" else DeviceLists(device, table, short_lists, short_single)   # (the other memory)
    short_rows = expanded(table, short_lists)
    check(device, column, short, product_numpy(sizes, [3], left_lists=lists, right_lists=short_rows), f"{kind} ({memory}) x reference", variants[:2])
    check(device, short, column, product_numpy([3], sizes, left_lists=short_rows, right_lists=lists), f"reference x {kind} ({memory})", variants[:2])


def test_one_side_only(device):
    """left_pos only and right_pos only are the two-list call's halves; the list that is not wanted is not touched."""
    left_sizes, right_sizes = [300, 7], [257, 3]
    left, right = carrier(left_sizes), carrier(right_sizes)
    want = product_numpy(left_sizes, right_sizes)
    n = len(want[0])
    for mem, off in ((abi.MEM_DEVICE, 1), (abi.MEM_DEVICE, 0), (abi.MEM_HOST, 0)):
        for side in (0, 1):
            status, result, lists, offsets = call(device, left, right, mem, n, off, want=(side == 0, side == 1))
            assert status == abi.OK and result.n_rows == n
            assert lists.rows(side, n).tobytes() == want[side].tobytes() and lists.untouched_outside(side, n)
            assert (lists.host[1 - side] == SENTINEL).all()
            assert offsets.tobytes() == want[2].tobytes()
    wrapped = product(left, right, want_left=False)
    assert wrapped.numpy()[0] is None and wrapped.numpy()[1].tobytes() == want[1].tobytes() and wrapped.pair_offsets.tobytes() == want[2].tobytes()
    wrapped.close()
    both = product(left, right)
    assert both.n_rows == n and both.numpy()[0].tobytes() == want[0].tobytes() and both.numpy()[1].tobytes() == want[1].tobytes()
    both.close()


@pytest.mark.parametrize("mem", [abi.MEM_HOST, abi.MEM_DEVICE])
def test_capacity(device, mem):
    """capacity = needed - 1: HY_ERR_CAPACITY, the need reported, nothing written anywhere."""
    left, right = carrier([300, 7]), carrier([257, 3])
    needed = 307 * 260
    assert product_count(left, right) == needed
    status, result, lists, offsets = call(device, left, right, mem, needed - 1)
    assert status == abi.ERR_CAPACITY and device.hy_last_error()
    assert result.n_rows == needed
    assert (lists.host[0] == SENTINEL).all() and (lists.host[1] == SENTINEL).all() and (offsets == SENTINEL).all()


def test_refusals(device):
    left, right = carrier([4, 2]), carrier([3])
    status, result, lists, offsets = call(device, left, right, abi.MEM_DEVICE, 100, want=(False, False))
    assert status == abi.ERR_INVALID and device.hy_last_error()
    assert (lists.host[0] == SENTINEL).all() and (lists.host[1] == SENTINEL).all() and (offsets == SENTINEL).all()
    buffer = np.zeros(4096, dtype=np.uint8)   # lists 4 bytes off an 8-byte boundary
    result = abi.ProductResult()
    result.mem, result.capacity, result.left_pos, result.right_pos = abi.MEM_HOST, 100, buffer.ctypes.data + 4, buffer.ctypes.data + 2048
    assert device.hy_product(left.handle, right.handle, C.byref(result)) == abi.ERR_INVALID
    assert not buffer.any()
    # one chunk pair whose rows do not fit a ChunkOffset: 65 537 chunks' worth of rows in ONE descriptor each side, over one small device buffer
    # (HY_MEM_DEVICE: nothing is copied, and nothing is read: the call is refused before any kernel)
    values = DeviceArray(device, (16,), np.int32)
    handles = []
    for size in (65_537, 65_535):
        segment = (abi.Segment * 1)()
        segment[0].encoding, segment[0].data_type, segment[0].size, segment[0].width, segment[0].data = abi.ENC_UNENCODED, abi.TYPE_INT, size, 4, values.pointer
        segment[0].ref_chunk_id = abi.INVALID_CHUNK_ID
        handle = C.c_void_p()
        abi.check(device.hy_column_create(segment, 1, abi.MEM_DEVICE, C.byref(handle)))
        handles.append(handle)
    try:
        counted = C.c_uint64(7)
        assert 65_537 * 65_535 == 2 ** 32 - 1
        assert device.hy_product_count(handles[0], handles[1], C.byref(counted)) == abi.ERR_UNSUPPORTED and b"ChunkOffset" in device.hy_last_error()
        assert device.hy_product_count(handles[1], handles[1], C.byref(counted)) == abi.OK and counted.value == 65_535 ** 2   # (2^32 - 131 071: fits)
    finally:
        for handle in handles:
            device.hy_column_destroy(handle)
    mvcc = DeviceColumn(storage.make_mvcc_column(np.zeros(5), np.zeros(5), np.full(5, storage.MAX_COMMIT_ID), chunk_size=5))
    counted = C.c_uint64(0)
    assert device.hy_product_count(mvcc.handle, right.handle, C.byref(counted)) == abi.ERR_UNSUPPORTED


def test_a_string_column_carries_the_layout(device):
    from hyrise_amd.string_keys import encode_string_column
    segments, _ = encode_string_column(["a", "b", "c", "d", "e", "f", "g"], np.zeros(7, dtype=bool), 3)
    strings = DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))
    assert strings.n_chunks == 3
    right_sizes = [2, 5]
    want = product_numpy([3, 3, 1], right_sizes)
    check(device, strings, carrier(right_sizes, np.float64), want, "string x double")
    check(device, carrier([3, 3, 1]), carrier(right_sizes), want, "int x int")
    check(device, carrier(right_sizes, np.int64), strings, product_numpy(right_sizes, [3, 3, 1]), "long x string")

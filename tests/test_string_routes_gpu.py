"""Every entry point of the string operators (csrc/string_order.hip, string_gather.hip, string_substr.hip, string_join_keys.hip) through every
route of its host side once, at the smallest shapes that still cross the boundaries, against the existing oracles (string_gather_oracle,
string_substr_oracle, string_order_oracle, string_join_keys_oracle, string_columns_oracle) byte for byte after read-back.  The route of the
producers of string columns is forced with HY_OPT_STRING_SPARSE_GATHER (0: dense, 2: sparse).

The source has 254 .. 257 dictionary entries in three chunks -- one in the offsets layout (with the empty string, a '\\0' inside an entry,
bytes above 0x7F and one entry of COPY_TILE * 4 + 1 bytes), one in the fixed-slot layout (one entry fills its slot), one without rows --,
forty strings shared by the two, a NULL row, and rows that are not in dictionary order.  The columns over it: the data column, a reference
column of one uploaded PosList, and one of three PosLists in the caller's device memory (one of them without rows).

Not reached, because no test can build the input: 2^31 dictionary entries behind real buffers (the refusal itself is reached with counts
alone: test_string_gather_abi.py), 2^32 rows, 4 GiB of chars in one output chunk, and a dictionary or column that lives on a second device
(the suite runs on one)."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import (column_string_join_keys, column_string_ranks, string_column_gather, string_column_materialize, string_column_substr,
                                  string_dictionary_join_ids, string_dictionary_order, string_dictionary_order_pair, string_dictionary_ranks, string_ranks_gather)
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn
from placed_columns import PlacedArray, PlacedColumn
from string_sparse_source import DENSE, NULL, SPARSE
from test_string_gather_gpu import Source, assert_result, ranks_column
import string_columns_oracle
import string_gather_oracle
import string_join_keys_oracle
import string_order_oracle
import string_substr_oracle

pytestmark = pytest.mark.gpu

ROUTES = (DENSE, SPARSE)
SIZES = (254, 255, 256, 257)   # dictionary entries; the data column has one row more, the reference columns and the gathers as many rows
KINDS = ("data", "uploaded_list", "device_lists")
LONG_ENTRY = bytes(np.random.default_rng(17).integers(1, 256, 4 * 1024 + 1, dtype=np.uint8))   # COPY_TILE * 4 + 1 bytes
# start 0 and 1 keep a chunk's entries ascending, 3 and a negative start do not (the merge starts from single positions); length <= 0: ""
SUBSTR_ARGUMENTS = ((0, 3), (1, 2), (3, 2), (-2, 2), (2, 0), (1, -5))


class Sources:
    """The sources and the columns over them, made once per module (or once per run of a tool that walks the cases)."""

    def __init__(self):
        self.sources, self.columns = {}, {}

    def source(self, n_entries):
        if n_entries not in self.sources:
            shared = [b"s%02d" % i for i in range(40)]
            slots = shared + [b"12345678"] + [b"f%05d" % i for i in range(59)]                             # chunk 1: slots of 8 bytes
            own = [b"", b"a\x00b", b"\xff\x80", LONG_ENTRY] + [b"o%04d\x80" % i for i in range(n_entries - len(slots) - len(shared) - 4)]
            rng = np.random.default_rng(n_entries)
            first = [(shared + own)[i] for i in rng.permutation(len(shared) + len(own))] + [None]
            source = Source([first, [slots[i] for i in rng.permutation(len(slots))], []], fixed_lengths=(None, 8, None))
            assert sum(map(len, source.dictionaries)) == n_entries and source.dictionaries[2] == []
            self.sources[n_entries] = source
        return self.sources[n_entries]

    def column(self, n_entries, kind):
        """(the column, its rows per chunk as bytes / None)"""
        if (n_entries, kind) not in self.columns:
            self.columns[n_entries, kind] = self.make_column(n_entries, kind)
        return self.columns[n_entries, kind][:2]

    def make_column(self, n_entries, kind):
        source = self.source(n_entries)
        if kind == "data":
            return source.dev, source.chunks, None
        rng = np.random.default_rng(n_entries + len(kind))
        sizes = [len(chunk) for chunk in source.chunks]
        chunk_ids = rng.integers(0, 2, n_entries)
        positions = np.stack([chunk_ids, (rng.random(n_entries) * np.array(sizes)[chunk_ids]).astype(np.int64)], axis=1).astype(np.uint32)
        positions[rng.random(n_entries) < 0.05] = NULL
        positions[0] = positions[-1] = NULL
        if kind == "uploaded_list":
            pos_lists = [positions]
            reference = storage.make_reference_column(source.host, pos_lists, [None])
            column = DeviceColumn(reference, refs={id(source.host): source.dev})
        else:   # (a caller-owned list without rows has no buffer and names a chunk: it reads as an entire-chunk list of no rows)
            pos_lists = [positions[:-200], positions[:0], positions[-200:]]
            reference = storage.make_reference_column(source.host, pos_lists, [None, 0, None])
            column = PlacedColumn(reference, "aligned", 0x00, refs={id(source.host): source.dev})
        rows = [[source.chunks[c][o] if o != NULL else None for c, o in p.tolist()] for p in pos_lists]
        return column, rows, reference

    def clear(self):
        self.columns.clear()
        self.sources.clear()


@pytest.fixture(scope="module")
def sources(device):
    made = Sources()
    yield made
    made.clear()


def positions_into(chunks, n, seed):
    """n RowIDs into a column of these chunks, NULL RowIDs at both ends and among the others"""
    rng = np.random.default_rng(seed)
    sizes = np.array([len(chunk) for chunk in chunks])
    filled = np.flatnonzero(sizes)
    chunk_ids = filled[rng.integers(0, len(filled), n)]
    positions = np.stack([chunk_ids, (rng.random(n) * sizes[chunk_ids]).astype(np.int64)], axis=1).astype(np.uint32)
    positions[rng.random(n) < 0.1] = NULL
    positions[0] = positions[-1] = NULL
    return positions


def flat(chunks):
    return [row for chunk in chunks for row in chunk]


# ---- gather, substr, materialize: dense and sparse, data and reference columns ------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_entries", SIZES)
def test_gather_substr_and_materialize_on_both_routes(device, sources, n_entries, kind):
    source = sources.source(n_entries)
    column, chunks = sources.column(n_entries, kind)
    n = n_entries
    positions = positions_into(chunks, n, n)
    want_rows = string_gather_oracle.encode_chunks(flat(chunks), [len(chunk) for chunk in chunks])
    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            context = f"{n_entries} entries, {kind}, route {route}"
            for chunk_rows in (1, 100, n + 1):   # one row per chunk; several chunks; one chunk (no chunk sort)
                got = string_column_gather(column, source.dev_dict, positions, chunk_rows)
                assert_result(got, string_gather_oracle.column_gather(chunks, [tuple(p) for p in positions.tolist()], chunk_rows), f"{context}: gather, chunk_rows {chunk_rows}")
                got.close()
            got = string_column_materialize(column, source.dev_dict)
            assert_result(got, want_rows, f"{context}: materialize")
            got.close()
            for start, length in SUBSTR_ARGUMENTS:
                got = string_column_substr(column, source.dev_dict, start, length)
                assert_result(got, string_substr_oracle.column_substr(chunks, start, length), f"{context}: SUBSTR({start}, {length})")
                got.close()
    if kind == "device_lists":
        column.assert_untouched()


def test_equal_strings_of_both_layouts_are_one_entry_and_the_long_entry_is_copied(device, sources):
    source = sources.source(256)
    first, second = source.chunks[0], source.chunks[1]
    positions = [(0, first.index(b"s07")), (1, second.index(b"s07")), (0, first.index(LONG_ENTRY)), (1, second.index(b"12345678")), (0, first.index(LONG_ENTRY))]
    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            got = string_column_gather(source.dev, source.dev_dict, np.array(positions, dtype=np.uint32), 8)
        assert_result(got, string_gather_oracle.column_gather(source.chunks, positions, 8), f"route {route}")
        assert got.dictionary.n_entries == [3]


# ---- empty and NULL cases -----------------------------------------------------------------------------------------------------------------
def test_no_rows_and_a_column_without_chunks_give_empty_results(device, sources):
    source = sources.source(256)
    no_chunks, no_dictionary = DeviceColumn(HostColumn([], abi.TYPE_STRING)), DeviceStringDictionary([])
    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            results = [string_column_gather(source.dev, source.dev_dict, np.zeros((0, 2), dtype=np.uint32), 4),
                       string_column_materialize(no_chunks, no_dictionary), string_column_substr(no_chunks, no_dictionary, 1, 2),
                       string_ranks_gather(source.dev_dict, ranks_column([]))]
        for got in results:
            assert (got.n_chunks, got.rows, got.dictionary.n_chunks) == (0, 0, 0), f"route {route}"


def test_empty_chunks_no_entries_and_no_referenced_entry(device, sources):
    """A column of chunks without rows; a dictionary without entries (every row NULL); and on the sparse route requested rows that are all
    NULL, so that the subset is empty."""
    for chunks in ([[], []], [[None, None], [], [None]]):
        source = Source(chunks)
        assert sum(map(len, source.dictionaries)) == 0
        for route in ROUTES:
            with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
                context = f"{chunks}, route {route}"
                want = string_gather_oracle.encode_chunks(flat(chunks), [len(chunk) for chunk in chunks])
                assert_result(string_column_materialize(source.dev, source.dev_dict), want, f"{context}: materialize")
                assert_result(string_column_substr(source.dev, source.dev_dict, 3, 2), want, f"{context}: substr")
                positions = [(0, 0), (NULL, NULL), (2, 0), (7, 7), (1, 0)]
                got = string_column_gather(source.dev, source.dev_dict, np.array(positions, dtype=np.uint32), 2)
                assert_result(got, ([[], [], []], [[0, 0], [0, 0], [0]]), f"{context}: gather")
    source = sources.source(255)
    null_rows = [(c, o) for c, chunk in enumerate(source.chunks) for o, row in enumerate(chunk) if row is None]
    positions = null_rows + [(NULL, NULL)] * 3 + [(5, 0), (2, 0), (1, len(source.chunks[1]))]
    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            for chunk_rows in (1, 4, 100):
                got = string_column_gather(source.dev, source.dev_dict, np.array(positions, dtype=np.uint32), chunk_rows)
                assert got.read() == [None] * len(positions) and got.dictionary.n_entries == [0] * got.n_chunks, f"route {route}, chunk_rows {chunk_rows}"


def test_a_subset_smaller_than_the_number_of_source_chunks(device, sources):
    """Nine source chunks, two referenced entries: the sparse route's merge starts from single positions.  The two are equal strings or not."""
    chunks = [[b"w%d" % (c % 4), b"x%d" % c, None] for c in range(9)]
    source = Source(chunks)
    for positions in ([(8, 0), (2, 1), (8, 0)], [(0, 0), (4, 0), (NULL, NULL)], [(3, 1)]):
        want = string_gather_oracle.column_gather(chunks, positions, 2)
        for route in ROUTES:
            with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
                assert_result(string_column_gather(source.dev, source.dev_dict, np.array(positions, dtype=np.uint32), 2), want, f"{positions}, route {route}")
    reference = storage.make_reference_column(source.host, [np.array([(7, 1), (1, 0), (5, 0)], dtype=np.uint32)], [None])
    column = DeviceColumn(reference, refs={id(source.host): source.dev})
    rows = [[b"x7", b"w1", b"w1"]]
    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            assert_result(string_column_materialize(column, source.dev_dict), string_gather_oracle.encode_chunks(rows[0], [3]), f"materialize, route {route}")
            assert_result(string_column_substr(column, source.dev_dict, 2, 1), string_substr_oracle.column_substr(rows, 2, 1), f"substr, route {route}")


# ---- hy_string_ranks_gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_entries", SIZES)
def test_ranks_gather(device, sources, n_entries):
    """A NULL rank, ranks that no entry has (-1, n_distinct, the ends of int32), every rank of a dictionary with duplicates across chunks."""
    source = sources.source(n_entries)
    n_distinct = len({entry for dictionary in source.dictionaries for entry in dictionary})
    assert n_distinct == n_entries - 40
    rng = np.random.default_rng(n_entries)
    ranks = [None, -1, n_distinct, 2**31 - 1, -2**31] + rng.permutation(n_distinct).tolist() + [int(r) for r in rng.integers(0, n_distinct, n_entries - n_distinct - 5)]
    assert len(ranks) == n_entries
    for rank_chunks in ([ranks], [ranks[:100], [], ranks[100:]], [[r] for r in ranks[:7]]):
        got = string_ranks_gather(source.dev_dict, ranks_column(rank_chunks))
        assert_result(got, string_gather_oracle.ranks_gather(source.dictionaries, rank_chunks), f"{n_entries} entries, {len(rank_chunks)} chunks")


# ---- the rankings of dictionaries: to host and to device memory, with and without n_distinct ---------------------------------------------------
def device_output(n, width, fill=0xA5):
    return PlacedArray(width * n, width, fill, guard=64)


def flat_keys(per_chunk, dtype):
    return np.array([x for chunk in per_chunk for x in chunk], dtype=dtype)


def order_to_device(lib, dev_dict, want, want_distinct, with_distinct, context):
    out = device_output(sum(dev_dict.n_entries), 4)
    n = C.c_uint32(0xFFFFFFFF)
    abi.check(lib.hy_string_dictionary_order(dev_dict.handle, abi.MEM_DEVICE, out.pointer, C.byref(n) if with_distinct else None))
    if with_distinct:
        assert n.value == want_distinct, context
    abi.check(lib.hy_synchronize())   # (without n_distinct there was no host round trip: stream order)
    inside, guards_intact = out.read(np.int32)
    assert guards_intact and np.array_equal(inside, flat_keys(want, np.int32)), context


@pytest.mark.parametrize("n_entries", SIZES)
def test_dictionary_order_and_ranks(device, sources, n_entries):
    lib = device
    source = sources.source(n_entries)
    want, want_distinct = string_order_oracle.column_order(source.dictionaries)
    got, n_distinct = string_dictionary_order(source.dev_dict)
    assert n_distinct == want_distinct and [g.tolist() for g in got] == want
    host = np.zeros(n_entries, dtype=np.int32)
    abi.check(lib.hy_string_dictionary_order(source.dev_dict.handle, abi.MEM_HOST, host.ctypes.data, None))
    assert host.tolist() == flat_keys(want, np.int32).tolist()
    for with_distinct in (True, False):
        order_to_device(lib, source.dev_dict, want, want_distinct, with_distinct, f"{n_entries} entries, n_distinct {with_distinct}")
    # hy_string_dictionary_ranks: chunk by chunk against a dictionary of as many chunks
    others = [sorted(set(source.dictionaries[1][::2] + [b"", b"zz"])), source.dictionaries[0][1::3], [b"q"]]
    other_dict = DeviceStringDictionary(others)
    want_ranks = string_columns_oracle.column_ranks(source.dictionaries, others)
    assert [g.tolist() for g in string_dictionary_ranks(source.dev_dict, other_dict)] == [list(w) for w in want_ranks]
    out = device_output(n_entries, 4)
    abi.check(lib.hy_string_dictionary_ranks(source.dev_dict.handle, other_dict.handle, abi.MEM_DEVICE, out.pointer))
    abi.check(lib.hy_synchronize())
    inside, guards_intact = out.read(np.int32)
    assert guards_intact and inside.tolist() == [r for w in want_ranks for r in w]


@pytest.mark.parametrize("empty", [[], [[]], [[], []]], ids=["no_chunks", "one_empty_chunk", "two_empty_chunks"])
def test_totals_of_zero(device, sources, empty):
    """No entry on either side: nothing is written, n_distinct is 0; hy_string_dictionary_ranks of no entries returns at once."""
    lib = device
    dev_dict = DeviceStringDictionary(empty)
    untouched = np.full(4, 77, dtype=np.int64)
    for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        n = C.c_uint32(0xFFFFFFFF)
        abi.check(lib.hy_string_dictionary_order(dev_dict.handle, mem, untouched.ctypes.data, C.byref(n)))
        assert n.value == 0
        abi.check(lib.hy_string_dictionary_order(dev_dict.handle, mem, untouched.ctypes.data, None))
        n = C.c_uint32(0xFFFFFFFF)
        abi.check(lib.hy_string_dictionary_order_pair(dev_dict.handle, dev_dict.handle, mem, untouched.ctypes.data, untouched.ctypes.data, C.byref(n)))
        assert n.value == 0
        abi.check(lib.hy_string_dictionary_join_ids(dev_dict.handle, dev_dict.handle, mem, untouched.ctypes.data, untouched.ctypes.data))
        abi.check(lib.hy_string_dictionary_ranks(dev_dict.handle, dev_dict.handle, mem, untouched.ctypes.data))
    assert (untouched == 77).all()


def pair_to_device(lib, left_dev, right_dev, want_left, want_right, ids, want_distinct, context):
    width, dtype = (8, np.int64) if ids else (4, np.int32)
    left_out, right_out = device_output(sum(left_dev.n_entries), width), device_output(sum(right_dev.n_entries), width)
    if ids:
        abi.check(lib.hy_string_dictionary_join_ids(left_dev.handle, right_dev.handle, abi.MEM_DEVICE, left_out.pointer, right_out.pointer))
    else:
        for with_distinct in (True, False):
            n = C.c_uint32(0xFFFFFFFF)
            abi.check(lib.hy_string_dictionary_order_pair(left_dev.handle, right_dev.handle, abi.MEM_DEVICE, left_out.pointer, right_out.pointer, C.byref(n) if with_distinct else None))
            assert not with_distinct or n.value == want_distinct, context
    abi.check(lib.hy_synchronize())
    for out, want in ((left_out, want_left), (right_out, want_right)):
        inside, guards_intact = out.read(dtype)
        assert guards_intact and np.array_equal(inside, flat_keys(want, dtype)), context


@pytest.mark.parametrize("right", ["other", "none", "empty_chunks"])
@pytest.mark.parametrize("n_entries", (255, 257))
def test_order_pair_and_join_ids(device, sources, n_entries, right):
    lib = device
    source = sources.source(n_entries)
    right_dicts = {"other": [source.dictionaries[1][::3], [], sorted(source.dictionaries[0][5:70] + [b"right only"])], "none": [], "empty_chunks": [[], []]}[right]
    right_dev = DeviceStringDictionary(right_dicts)
    for left_dicts, left_dev, rd, rdev in ((source.dictionaries, source.dev_dict, right_dicts, right_dev), (right_dicts, right_dev, source.dictionaries, source.dev_dict)):
        context = f"{n_entries} entries, right {right}, left chunks {len(left_dicts)}"
        want_left, want_right, want_distinct = string_join_keys_oracle.joint_order(left_dicts, rd)
        got_left, got_right, n_distinct = string_dictionary_order_pair(left_dev, rdev)
        assert n_distinct == want_distinct and [g.tolist() for g in got_left] == want_left and [g.tolist() for g in got_right] == want_right, context
        want_left_ids, want_right_ids = string_join_keys_oracle.join_ids(left_dicts, rd)
        got_left, got_right = string_dictionary_join_ids(left_dev, rdev)
        assert [g.tolist() for g in got_left] == want_left_ids and [g.tolist() for g in got_right] == want_right_ids, context
        pair_to_device(lib, left_dev, rdev, want_left, want_right, False, want_distinct, context)
        pair_to_device(lib, left_dev, rdev, want_left_ids, want_right_ids, True, want_distinct, context)


def test_an_order_over_more_entries_than_one_lane_per_tile_of_the_scan(device, sources):
    """Five chunks of 65 535 entries: 1 280 tiles of 256 positions, so a lane of the one-workgroup tile scan (1 024 lanes) owns two."""
    n = 65_535
    dictionaries = [[b"%07d" % (5 * i + (c % 4)) for i in range(n)] for c in range(5)]   # (chunk 4 = chunk 0: duplicates)
    dev_dict = DeviceStringDictionary(dictionaries)
    ranks, n_distinct = string_dictionary_order(dev_dict)
    assert n_distinct == 4 * n and sum(map(len, ranks)) > 262_144
    for c in range(5):
        assert np.array_equal(ranks[c], 4 * np.arange(n, dtype=np.int32) + c % 4), f"chunk {c}"


# ---- the stand-in columns -------------------------------------------------------------------------------------------------------------------
def export(column, dtype):
    import torch
    lib = abi.load_library()
    values = torch.full((max(1, column.rows),), -7, dtype=torch.int64 if dtype == np.int64 else torch.int32, device="cuda")
    nulls = torch.full((max(1, column.rows),), 9, dtype=torch.uint8, device="cuda")
    abi.check(lib.hy_column_export(column.handle, values.data_ptr(), nulls.data_ptr()))
    abi.check(lib.hy_synchronize())
    return values.cpu().numpy()[:column.rows].tolist(), nulls.cpu().numpy()[:column.rows].astype(bool).tolist()


def assert_stand_in(stand_in, rows, key_of, dtype, context):
    values, nulls = export(stand_in, dtype)
    assert nulls == [row is None for row in rows], context
    assert [v for v, null in zip(values, nulls) if not null] == [key_of[row] for row in rows if row is not None], context


@pytest.mark.parametrize("kind", KINDS)
def test_column_string_ranks_and_join_keys(device, sources, kind):
    """The stand-ins row for row, on a data column and on reference columns; the other side is a reference column whose one uploaded
    PosList has no rows (no device buffer, no common chunk)."""
    source = sources.source(257)
    column, chunks = sources.column(257, kind)
    rows = flat(chunks)
    ranks, _ = string_order_oracle.column_order(source.dictionaries)
    rank_of = {entry: rank for dictionary, chunk_ranks in zip(source.dictionaries, ranks) for entry, rank in zip(dictionary, chunk_ranks)}
    stand_in = column_string_ranks(column, source.dev_dict)
    assert (stand_in.rows, stand_in.n_chunks) == (len(rows), len(chunks))
    assert_stand_in(stand_in, rows, rank_of, np.int32, f"{kind}: ranks")
    stand_in.close()
    other = Source([[b"s03", b"other", None], [b"12345678", b""]])
    without_rows = DeviceColumn(storage.make_reference_column(other.host, [np.zeros((0, 2), dtype=np.uint32)], [None]), refs={id(other.host): other.dev})
    for key_kind, dtype in ((abi.STRING_KEYS_RANKS, np.int32), (abi.STRING_KEYS_HASH_IDS, np.int64)):
        if key_kind == abi.STRING_KEYS_RANKS:
            left_keys, right_keys, _ = string_join_keys_oracle.joint_order(source.dictionaries, other.dictionaries)
        else:
            left_keys, right_keys = string_join_keys_oracle.join_ids(source.dictionaries, other.dictionaries)
        key_of = {e: k for d, keys in zip(source.dictionaries + other.dictionaries, left_keys + right_keys) for e, k in zip(d, keys)}
        left_in, right_in = column_string_join_keys(column, source.dev_dict, other.dev, other.dev_dict, key_kind)
        assert_stand_in(left_in, rows, key_of, dtype, f"{kind}, keys {key_kind}: left")
        assert_stand_in(right_in, flat(other.chunks), key_of, dtype, f"{kind}, keys {key_kind}: right")
        left_in.close()
        right_in.close()
        left_in, right_in = column_string_join_keys(without_rows, other.dev_dict, column, source.dev_dict, key_kind)
        assert (left_in.rows, left_in.n_chunks) == (0, 1)
        assert_stand_in(right_in, rows, key_of, dtype, f"{kind}, keys {key_kind}: right of a column without rows")
        left_in.close()
        right_in.close()
    if kind == "device_lists":
        column.assert_untouched()


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(device, sources):
    """Status and, where another test pins it already, the message; outputs stay NULL and nothing is written."""
    import torch
    lib = device
    source = sources.source(254)
    column, dev_dict = source.dev.handle, source.dev_dict.handle
    ints = DeviceColumn(storage.make_column(np.arange(9, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    of_another_column = DeviceStringDictionary(source.dictionaries[:2])
    block = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    pointer = block.data_ptr()
    assert pointer % 16 == 0

    def producer(call, *arguments, give=(True, True)):
        result, result_dict = C.c_void_p(1), C.c_void_p(1)
        status = call(*arguments, C.byref(result) if give[0] else None, C.byref(result_dict) if give[1] else None)
        assert status != abi.OK and (not give[0] or not result.value) and (not give[1] or not result_dict.value)
        return status, lib.hy_last_error()

    for route in ROUTES:
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, route):
            # null arguments
            for give in ((False, True), (True, False)):
                assert producer(lib.hy_string_column_gather, column, dev_dict, pointer, 4, 2, give=give)[0] == abi.ERR_INVALID
                assert producer(lib.hy_string_column_substr, column, dev_dict, 1, 2, give=give)[0] == abi.ERR_INVALID
                assert producer(lib.hy_string_column_materialize, column, dev_dict, give=give)[0] == abi.ERR_INVALID
                assert producer(lib.hy_string_ranks_gather, dev_dict, ints.handle, give=give)[0] == abi.ERR_INVALID
            for c, d in ((None, dev_dict), (column, None)):
                for status, message in (producer(lib.hy_string_column_gather, c, d, pointer, 4, 2), producer(lib.hy_string_column_substr, c, d, 1, 2),
                                        producer(lib.hy_string_column_materialize, c, d), producer(lib.hy_string_ranks_gather, d, c)):
                    assert status == abi.ERR_INVALID and b"null argument" in message
            assert producer(lib.hy_string_column_gather, column, dev_dict, None, 4, 2)[0] == abi.ERR_INVALID
            assert producer(lib.hy_string_column_gather, column, dev_dict, pointer, 4, 0)[0] == abi.ERR_INVALID
            # misaligned positions
            for off in (1, 4):
                status, message = producer(lib.hy_string_column_gather, column, dev_dict, pointer + off, 4, 2)
                assert status == abi.ERR_INVALID and b"8-byte" in message
            # wrong column type, a dictionary of another column (check_dictionary), too many rows
            for status, message in (producer(lib.hy_string_column_gather, ints.handle, dev_dict, pointer, 4, 2), producer(lib.hy_string_column_substr, ints.handle, dev_dict, 1, 2),
                                    producer(lib.hy_string_column_materialize, ints.handle, dev_dict)):
                assert status == abi.ERR_INVALID and b"string column" in message
            assert producer(lib.hy_string_column_gather, column, of_another_column.handle, pointer, 4, 2)[0] == abi.ERR_INVALID
            assert producer(lib.hy_string_column_substr, column, of_another_column.handle, 1, 2)[0] == abi.ERR_INVALID
            assert producer(lib.hy_string_column_materialize, column, of_another_column.handle)[0] == abi.ERR_INVALID
            status, message = producer(lib.hy_string_column_gather, column, dev_dict, pointer, 1 << 32, 65_535)
            assert status == abi.ERR_UNSUPPORTED and b"32-bit" in message
            # ranks that are no int32 data column of unencoded segments
            assert producer(lib.hy_string_ranks_gather, dev_dict, column)[0] == abi.ERR_INVALID
            assert producer(lib.hy_string_ranks_gather, dev_dict, ints.handle)[0] == abi.ERR_INVALID

    # the rankings: null arguments, a bad memory space, misaligned device outputs, chunk counts that differ
    host = np.full(600, 77, dtype=np.int64)
    out = host.ctypes.data
    n = C.c_uint32(77)
    assert lib.hy_string_dictionary_order(None, abi.MEM_HOST, out, C.byref(n)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_order(dev_dict, abi.MEM_HOST, None, C.byref(n)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_order(dev_dict, 2, out, C.byref(n)) == abi.ERR_INVALID and b"memory space" in lib.hy_last_error()
    assert lib.hy_string_dictionary_order(dev_dict, abi.MEM_DEVICE, pointer + 2, C.byref(n)) == abi.ERR_INVALID and b"4-byte" in lib.hy_last_error()
    assert lib.hy_string_dictionary_ranks(None, dev_dict, abi.MEM_HOST, out) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_ranks(dev_dict, dev_dict, abi.MEM_HOST, None) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_ranks(dev_dict, dev_dict, 7, out) == abi.ERR_INVALID and b"memory space" in lib.hy_last_error()
    assert lib.hy_string_dictionary_ranks(dev_dict, dev_dict, abi.MEM_DEVICE, pointer + 1) == abi.ERR_INVALID and b"4-byte" in lib.hy_last_error()
    assert lib.hy_string_dictionary_ranks(dev_dict, of_another_column.handle, abi.MEM_HOST, out) == abi.ERR_INVALID and b"chunks" in lib.hy_last_error()
    for call, width, tail in ((lib.hy_string_dictionary_order_pair, 4, (C.byref(n),)), (lib.hy_string_dictionary_join_ids, 8, ())):
        assert call(None, dev_dict, abi.MEM_HOST, out, out, *tail) == abi.ERR_INVALID
        assert call(dev_dict, dev_dict, abi.MEM_HOST, None, out, *tail) == abi.ERR_INVALID
        assert call(dev_dict, dev_dict, abi.MEM_HOST, out, None, *tail) == abi.ERR_INVALID
        assert call(dev_dict, dev_dict, 2, out, out, *tail) == abi.ERR_INVALID and b"memory space" in lib.hy_last_error()
        assert call(dev_dict, dev_dict, abi.MEM_DEVICE, pointer + width // 2, pointer + 2048, *tail) == abi.ERR_INVALID and (b"%d-byte" % width) in lib.hy_last_error()
        assert call(dev_dict, dev_dict, abi.MEM_DEVICE, pointer, pointer + 2048 + width // 2, *tail) == abi.ERR_INVALID and (b"%d-byte" % width) in lib.hy_last_error()
    assert n.value == 77 and (host == 77).all()
    abi.check(lib.hy_synchronize())
    assert not block.cpu().numpy().any()

    # the stand-ins: null arguments, an unknown kind of keys, wrong column type, a dictionary of another column
    stand_in = C.c_void_p(1)
    assert lib.hy_column_string_ranks(column, dev_dict, None) == abi.ERR_INVALID
    for c, d in ((None, dev_dict), (column, None), (ints.handle, dev_dict), (column, of_another_column.handle)):
        stand_in.value = 1
        assert lib.hy_column_string_ranks(c, d, C.byref(stand_in)) == abi.ERR_INVALID and not stand_in.value
    assert b"hy_column_string_ranks" in lib.hy_last_error()

    def join_keys(left, left_dict, right, right_dict, kind):
        a, b = C.c_void_p(1), C.c_void_p(1)
        status = lib.hy_column_string_join_keys(left, left_dict, right, right_dict, kind, C.byref(a), C.byref(b))
        assert status != abi.OK and not a.value and not b.value
        return status

    assert lib.hy_column_string_join_keys(column, dev_dict, column, dev_dict, abi.STRING_KEYS_RANKS, None, C.byref(stand_in)) == abi.ERR_INVALID
    assert join_keys(None, dev_dict, column, dev_dict, abi.STRING_KEYS_RANKS) == abi.ERR_INVALID
    assert join_keys(column, dev_dict, column, None, abi.STRING_KEYS_HASH_IDS) == abi.ERR_INVALID
    assert join_keys(column, dev_dict, column, dev_dict, 2) == abi.ERR_INVALID
    assert join_keys(ints.handle, dev_dict, column, dev_dict, abi.STRING_KEYS_RANKS) == abi.ERR_INVALID and b"string column" in lib.hy_last_error()
    assert join_keys(column, dev_dict, column, of_another_column.handle, abi.STRING_KEYS_HASH_IDS) == abi.ERR_INVALID

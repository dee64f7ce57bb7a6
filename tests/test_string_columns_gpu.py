"""ColumnVsColumn on two string columns: hy_string_dictionary_ranks (csrc/string_order.hip) against tests/string_columns_oracle.py, and
hy_table_scan_columns_strings against the row-by-row oracle and -- for counts, offsets and chunk states, bit for bit -- against the numeric
ColumnVsColumn oracle over the int32 stand-ins the oracle's ranks describe."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import HostScanResult, string_dictionary_ranks, table_scan_columns_strings
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn, HostSegment
from placed_columns import PlacedArray
from support import DeviceArray, assert_scan_equal, load_tbl, oracle_scan_columns
from test_like_device_gpu import BYTE_ENTRIES, PlacedDictionary, device_result_as_host
import string_columns_oracle as oracle

pytestmark = pytest.mark.gpu

ENTRY_COUNTS = (0, 1, 63, 64, 65, 257)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


# ---- the ranking kernel ------------------------------------------------------------------------------------------------------------------
def random_entries(rng, n, alphabet=b"ab\x00\xff", longest=6):
    """n distinct sorted entries (the alphabet is small and the strings short: two such dictionaries share many entries)."""
    out = set()
    while len(out) < n:
        out.add(bytes(rng.choice(list(alphabet), rng.integers(0, longest + 1)).tolist()))
    return sorted(out)


def assert_ranks(left, right, context, left_fixed=None, right_fixed=None):
    got = string_dictionary_ranks(DeviceStringDictionary(left, fixed_length=left_fixed), DeviceStringDictionary(right, fixed_length=right_fixed))
    want = oracle.column_ranks(left, right)
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.tolist() == w, f"{context}: chunk {c} ({len(left[c])} x {len(right[c])} entries)"


def every_count_pair(rng, **kwargs):
    pairs = [(l, r) for l in ENTRY_COUNTS for r in ENTRY_COUNTS]
    return [random_entries(rng, l, **kwargs) for l, _ in pairs], [random_entries(rng, r, **kwargs) for _, r in pairs]


def test_ranks_for_every_pair_of_entry_counts(device):
    left, right = every_count_pair(np.random.default_rng(1))
    assert_ranks(left, right, "offsets x offsets")


@pytest.mark.parametrize("left_fixed,right_fixed", [(None, 6), (6, None), (6, 6), (9, 6)])
def test_ranks_with_fixed_length_layouts(device, left_fixed, right_fixed):
    """Slots of 6 bytes hold entries of 0 .. 6 bytes: some fill the whole slot, and a slot's entry ends at its first \\0."""
    left, right = every_count_pair(np.random.default_rng(2), alphabet=b"ab\xff")
    assert any(len(e) == 6 for d in left for e in d) and any(len(e) == 6 for d in right for e in d)
    assert_ranks(left, right, f"fixed {left_fixed} x {right_fixed}", left_fixed, right_fixed)


def test_ranks_of_bytes(device):
    """The empty string, \\x00 inside an entry, 0x80-0xFF against ASCII (signed bytes would order them first), a / ab / aab, two 400-byte
    entries that differ in the last byte only, one of them the other's prefix."""
    entries = sorted(set(BYTE_ENTRIES))
    assert entries[0] == b"" and b"a\x00b" in entries and b"a" * 400 in entries and b"a" * 400 + b"b" in entries
    others = sorted(set(entries[::2] + [b"a" * 400 + b"a", b"a" * 399, b"\x7f", b"\x80", b"aa", b"\x00\x00\x00"]))
    left = [entries, entries, others, entries[::3], [b"a" * 400 + b"b"], [b"a" * 400]]
    right = [entries, others, entries, entries[1::3], [b"a" * 400], [b"a" * 400 + b"b"]]
    assert_ranks(left, right, "byte entries")


def test_ranks_equal_disjoint_below_and_above(device):
    rng = np.random.default_rng(3)
    base = [e for e in random_entries(rng, 301, alphabet=b"bcd", longest=8) if e][:300]       # (the empty string lies below everything)
    below = sorted({b"a" + e for e in base})
    above = sorted({b"e" + e for e in base})
    interleaved = sorted({e + b"\x00" for e in base})          # disjoint, every entry right behind its twin
    assert_ranks([base, base, base, base, base], [base, interleaved, below, above, []], "equal / disjoint / below / above / empty")
    assert string_dictionary_ranks(DeviceStringDictionary([base]), DeviceStringDictionary([base]))[0].tolist() == list(range(0, 600, 2))
    assert set(string_dictionary_ranks(DeviceStringDictionary([base]), DeviceStringDictionary([above]))[0].tolist()) == {-1}
    assert set(string_dictionary_ranks(DeviceStringDictionary([base]), DeviceStringDictionary([below]))[0].tolist()) == {2 * len(below) - 1}


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_device_ranks_on_four_bytes_and_caller_owned_dictionaries(device, fill):
    """HY_MEM_DEVICE ranks at 4 modulo 16 with guards around them, over caller-owned dictionaries whose chars begin at odd addresses."""
    lib = abi.load_library()
    left, right = every_count_pair(np.random.default_rng(4))
    want = np.array([r for chunk in oracle.column_ranks(left, right) for r in chunk], dtype=np.int32)
    placed_left, placed_right = PlacedDictionary(left, 3, fill), PlacedDictionary(right, 1, fill)
    for l, r in ((placed_left, placed_right), (DeviceStringDictionary(left), placed_right)):
        ranks = PlacedArray(4 * len(want), 4, fill, guard=64)
        abi.check(lib.hy_string_dictionary_ranks(l.handle, r.handle, abi.MEM_DEVICE, ranks.pointer))
        abi.check(lib.hy_synchronize())
        inside, guards_intact = ranks.read(np.int32)
        assert guards_intact and np.array_equal(inside, want)
    placed_left.assert_untouched()
    placed_right.assert_untouched()
    host = np.full(len(want) + 8, 0x5A5A5A5A, dtype=np.int32)
    abi.check(lib.hy_string_dictionary_ranks(placed_left.handle, placed_right.handle, abi.MEM_HOST, host[4:].ctypes.data))
    assert np.array_equal(host[4:4 + len(want)], want) and (host[:4] == 0x5A5A5A5A).all() and (host[4 + len(want):] == 0x5A5A5A5A).all()


def test_ranks_refusals(device):
    lib = abi.load_library()
    three, two = DeviceStringDictionary([[b"a"], [], [b"b"]]), DeviceStringDictionary([[b"a"], [b"b"]])
    ranks = np.full(8, 0x5A5A5A5A, dtype=np.int32)
    assert lib.hy_string_dictionary_ranks(three.handle, two.handle, abi.MEM_HOST, ranks.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_ranks(None, two.handle, abi.MEM_HOST, ranks.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_ranks(two.handle, two.handle, abi.MEM_HOST, None) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_ranks(two.handle, two.handle, 7, ranks.ctypes.data) == abi.ERR_INVALID
    placed = PlacedArray(64, 0, 0x5A)
    for off in (1, 2, 3):
        assert lib.hy_string_dictionary_ranks(two.handle, two.handle, abi.MEM_DEVICE, placed.pointer + off) == abi.ERR_INVALID
    placed.assert_untouched()
    assert (ranks == 0x5A5A5A5A).all()


# ---- the scan ----------------------------------------------------------------------------------------------------------------------------
def random_chunk(rng, rows, n_entries, null_fraction, **kwargs):
    """(dictionary, value ids, NULL id): every id of the dictionary may occur, NULLs with the given probability."""
    dictionary = random_entries(rng, n_entries, **kwargs)
    ids = rng.integers(0, n_entries, rows) if n_entries else np.zeros(rows, dtype=np.int64)
    nulls = rng.random(rows) < null_fraction if n_entries else np.ones(rows, dtype=bool)
    return dictionary, np.where(nulls, n_entries, ids).tolist(), n_entries


def string_column(chunks, width=None):
    """DictionarySegment<pmr_string> chunks with a chosen attribute vector width (FixedWidthInteger picks the narrowest; a wider one is legal)."""
    segments = []
    for dictionary, ids, null_id in chunks:
        w = width or storage.fixed_width(null_id)
        segments.append(HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, len(ids), w, np.asarray(ids, dtype=UINT[w]), aux=None, aux_size=len(dictionary)))
    return HostColumn(segments, abi.TYPE_STRING)


def stand_ins(left_host, right_host, left_chunks, right_chunks):
    """The int32 dictionary columns of the issue: the oracle's ranks on the left, 0, 2, 4, ... on the right, over the same attribute vectors."""
    def column(host, tables):
        return HostColumn([HostSegment(abi.ENC_DICTIONARY, abi.TYPE_INT, s.size, s.width, s.data, aux=np.asarray(t, dtype=np.int32), aux_size=s.aux_size)
                           for s, t in zip(host.segments, tables)], abi.TYPE_INT)
    rank_tables = oracle.column_ranks([c[0] for c in left_chunks], [c[0] for c in right_chunks])
    return column(left_host, rank_tables), column(right_host, [list(range(0, 2 * len(c[0]), 2)) for c in right_chunks])


class Pair:
    def __init__(self, left_chunks, right_chunks, left_width=None, right_width=None):
        self.left_chunks, self.right_chunks = left_chunks, right_chunks
        self.left_host, self.right_host = string_column(left_chunks, left_width), string_column(right_chunks, right_width)
        self.left_dev, self.right_dev = DeviceColumn(self.left_host), DeviceColumn(self.right_host)
        self.left_dict, self.right_dict = DeviceStringDictionary([c[0] for c in left_chunks]), DeviceStringDictionary([c[0] for c in right_chunks])
        self.twins = stand_ins(self.left_host, self.right_host, left_chunks, right_chunks)

    def want(self, condition):
        """The numeric ColumnVsColumn oracle over the stand-ins, its RowIDs checked against the row-by-row string oracle."""
        want = oracle_scan_columns(self.twins[0], self.twins[1], condition)
        for c, offsets in enumerate(oracle.scan(self.left_chunks, self.right_chunks, condition)):
            assert want.pos_list(c)[:, 1].tolist() == offsets and (want.pos_list(c)[:, 0] == c).all()
        return want

    def scan(self, condition, **kwargs):
        return table_scan_columns_strings(self.left_dev, self.left_dict, self.right_dev, self.right_dict, condition, **kwargs)

    def check(self, context, device_results=True):
        row_base = np.concatenate([[0], np.cumsum([s.size for s in self.left_host.segments])]).astype(np.uint64)
        n_chunks = self.left_host.n_chunks
        for condition in oracle.CONDITIONS:
            want = self.want(condition)
            assert_scan_equal(self.scan(condition), want, f"{context} cond {condition}")
            if not device_results:
                continue
            matches, offsets, counts, chunk_state = device_result_as_host(self.scan(condition, device=True), n_chunks)
            assert np.array_equal(counts, want.counts[:n_chunks]) and np.array_equal(chunk_state, want.chunk_state[:n_chunks]), f"{context} cond {condition}"
            assert np.array_equal(offsets, row_base), f"{context} cond {condition}"
            for c in range(n_chunks):
                assert np.array_equal(matches[int(row_base[c]):int(row_base[c]) + int(counts[c])], want.pos_list(c)), f"{context} cond {condition} chunk {c}"


CHUNK_ROWS = (1, 63, 64, 65, 256, 257)


@pytest.mark.parametrize("left_nulls,right_nulls", [(0.0, 0.0), (0.2, 0.0), (0.0, 0.2), (0.1, 0.3)])
def test_scan_chunk_sizes_and_nulls(device, left_nulls, right_nulls):
    """Chunks of 1 .. 257 rows, NULLs on neither, one or both sides, and NULL-only chunks without any dictionary entry on either side."""
    rng = np.random.default_rng(int(100 * left_nulls + 10 * right_nulls))
    left = [random_chunk(rng, rows, 40, left_nulls) for rows in CHUNK_ROWS] + [random_chunk(rng, 70, 0, 1.0), random_chunk(rng, 70, 5, left_nulls), random_chunk(rng, 33, 0, 1.0)]
    right = [random_chunk(rng, rows, 30, right_nulls) for rows in CHUNK_ROWS] + [random_chunk(rng, 70, 5, right_nulls), random_chunk(rng, 70, 0, 1.0), random_chunk(rng, 33, 0, 1.0)]
    Pair(left, right).check(f"nulls {left_nulls} / {right_nulls}")


@pytest.mark.parametrize("left_width,right_width", [(1, 1), (2, 2), (4, 4), (1, 2), (2, 1), (4, 2)])
def test_scan_attribute_vector_widths(device, left_width, right_width):
    """Equal widths take scan_two_columns, different ones the generic kernel; one chunk is longer than a scan slice (8 192 rows), one longer
    than a part (65 536 rows), which sends the whole pair to the generic kernel."""
    rng = np.random.default_rng(10 * left_width + right_width)
    for sizes in ((9_000, 300), (70_000, 9_000, 65)):
        left = [random_chunk(rng, rows, 200, 0.05) for rows in sizes]
        right = [random_chunk(rng, rows, 180, 0.05) for rows in sizes]
        pair = Pair(left, right, left_width, right_width)
        for condition in (abi.PRED_LESS_THAN, abi.PRED_EQUALS, abi.PRED_GREATER_THAN_EQUALS):
            assert_scan_equal(pair.scan(condition), pair.want(condition), f"widths {left_width} / {right_width} sizes {sizes} cond {condition}")


def test_scan_of_a_column_against_itself(device):
    rng = np.random.default_rng(8)
    chunks = [random_chunk(rng, rows, 50, 0.1) for rows in (300, 65)]
    pair = Pair(chunks, chunks)
    pair.check("a column against itself", device_results=False)
    same = table_scan_columns_strings(pair.left_dev, pair.left_dict, pair.left_dev, pair.left_dict, abi.PRED_EQUALS)
    assert [int(c) for c in same.counts[:2]] == [sum(1 for v in ids if v != null) for _, ids, null in chunks]


def test_materialized_chunk_regions_and_poslist_translate(device):
    lib = abi.load_library()
    rng = np.random.default_rng(9)
    sizes = (257, 0, 64, 9_000)
    pair = Pair([random_chunk(rng, rows, 60, 0.1) for rows in sizes], [random_chunk(rng, rows, 60, 0.1) for rows in sizes])
    rows, n_chunks = sum(sizes), len(sizes)
    for condition in (abi.PRED_LESS_THAN_EQUALS, abi.PRED_NOT_EQUALS):
        want = pair.want(condition)
        want_list = np.concatenate([want.pos_list(c) for c in range(n_chunks)])
        for layout in (abi.POSLIST_DENSE, abi.POSLIST_CHUNK_REGIONS):
            regions, offsets, counts = DeviceArray(lib, (rows, 2), np.uint32), DeviceArray(lib, (n_chunks + 1,), np.int64), DeviceArray(lib, (n_chunks,), np.int32)
            result = abi.ScanResult()
            result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH
            result.matches, result.capacity, result.offsets, result.counts = regions.pointer, rows, offsets.pointer, counts.pointer
            abi.check(lib.hy_table_scan_columns_strings(pair.left_dev.handle, pair.left_dict.handle, pair.right_dev.handle, pair.right_dict.handle, condition, C.byref(result)))
            out = DeviceArray(lib, (rows, 2), np.uint32)
            written = C.c_uint64(0)
            abi.check(lib.hy_poslist_translate(pair.left_dev.handle, C.byref(result), layout, out.pointer, rows, C.byref(written)))
            assert written.value == len(want_list)
            if layout == abi.POSLIST_DENSE:
                got = out.numpy()[:written.value]
            else:
                begin, count = offsets.numpy(), counts.numpy()
                got = np.concatenate([out.numpy()[int(begin[c]):int(begin[c]) + int(count[c])] for c in range(n_chunks)])
            assert got.tobytes() == want_list.tobytes(), f"cond {condition} layout {layout}"


@pytest.mark.parametrize("multi_chunk", [False, True], ids=["single_chunk_poslists", "multi_chunk_poslists"])
def test_scan_behind_the_poslists_of_a_previous_scan(device, multi_chunk):
    """Both columns as reference columns over the same PosLists: what a first scan leaves (one referenced chunk per PosList, and an
    EntireChunkPosList), and PosLists that span the chunks, with NULL RowIDs."""
    rng = np.random.default_rng(11 + multi_chunk)
    sizes = (300, 65, 1_000, 40)
    left = [random_chunk(rng, rows, 40, 0.1) for rows in sizes[:3]] + [random_chunk(rng, sizes[3], 0, 1.0)]
    right = [random_chunk(rng, rows, 40, 0.1) for rows in sizes]
    base = Pair(left, right)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    if multi_chunk:
        pos_lists, common = [], None
        for size in (0, 1, 65, 2_049):
            rows = rng.integers(0, starts[-1], size)
            chunk = np.searchsorted(starts, rows, side="right") - 1
            pos = np.stack([chunk, rows - starts[chunk]], axis=1).astype(np.uint32)
            pos[rng.random(size) < 0.05] = 0xFFFFFFFF
            pos_lists.append(pos)
    else:
        keep = [np.flatnonzero(rng.random(size) < 0.6) for size in sizes]
        pos_lists = [np.stack([np.full(len(k), c), k], axis=1).astype(np.uint32) for c, k in enumerate(keep)] + [2]
        common = list(range(len(sizes))) + [2]
    left_ref_host = storage.make_reference_column(base.left_host, pos_lists, common)
    right_ref_host = storage.make_reference_column(base.right_host, pos_lists, common)
    left_ref = DeviceColumn(left_ref_host, refs={id(base.left_host): base.left_dev})
    right_ref = DeviceColumn(right_ref_host, refs={id(base.right_host): base.right_dev})
    twin_refs = [storage.make_reference_column(twin, pos_lists, common) for twin in base.twins]
    for condition in oracle.CONDITIONS:
        got = table_scan_columns_strings(left_ref, base.left_dict, right_ref, base.right_dict, condition)
        assert_scan_equal(got, oracle_scan_columns(twin_refs[0], twin_refs[1], condition), f"multi {multi_chunk} cond {condition}")
        compare = oracle.COMPARISONS[condition]
        for c, pos in enumerate(pos_lists):
            rows = [(pos, i) for i in range(sizes[pos])] if isinstance(pos, int) else [tuple(r) for r in pos.tolist()]
            want = []
            for position, (chunk, offset) in enumerate(rows):
                if offset == 0xFFFFFFFF:
                    continue
                (ld, li, ln), (rd, ri, rn) = left[chunk], right[chunk]
                if li[offset] != ln and ri[offset] != rn and compare(ld[li[offset]], rd[ri[offset]]):
                    want.append(position)
            assert sorted(got.pos_list(c)[:, 1].tolist()) == want, f"multi {multi_chunk} cond {condition} chunk {c}"
    with pytest.raises(abi.HyriseAmdError) as refused:      # a data column against a reference column
        table_scan_columns_strings(base.left_dev, base.left_dict, right_ref, base.right_dict, abi.PRED_EQUALS)
    assert refused.value.status == abi.ERR_INVALID


def test_lineitem_commitdate_before_receiptdate(device):
    table = load_tbl("tpch/sf-0.001/lineitem.tbl")
    commit = [v.encode() for v in table.columns[table.names.index("l_commitdate")]]
    receipt = [v.encode() for v in table.columns[table.names.index("l_receiptdate")]]
    left, right = [], []
    for begin in range(0, len(commit), 1000):
        for values, chunks in ((commit, left), (receipt, right)):
            segment, dictionary = storage.encode_string_dictionary(values[begin:begin + 1000])
            chunks.append((dictionary, [int(v) for v in segment.data], len(dictionary)))
    pair = Pair(left, right)
    got = pair.scan(abi.PRED_LESS_THAN)
    assert_scan_equal(got, pair.want(abi.PRED_LESS_THAN), "l_commitdate < l_receiptdate")
    rows = [1000 * int(c) + int(o) for c, o in got.matches[:got.total].tolist()]
    assert rows == [i for i, (l, r) in enumerate(zip(commit, receipt)) if l < r] and 0 < len(rows) < len(commit)


def test_scan_refusals_write_nothing(device):
    lib = abi.load_library()
    rng = np.random.default_rng(12)
    left = [random_chunk(rng, rows, 10, 0.1) for rows in (100, 65, 7)]
    right = [random_chunk(rng, rows, 12, 0.1) for rows in (100, 65, 7)]
    pair = Pair(left, right)
    dictionaries = [c[0] for c in left]

    def scan(left_dev=pair.left_dev, left_dict=pair.left_dict, right_dev=pair.right_dev, right_dict=pair.right_dict, condition=abi.PRED_LESS_THAN):
        result = HostScanResult(left_dev.n_chunks, left_dev.rows)
        for array in (result.matches, result.offsets, result.counts, result.chunk_state):
            array.view(np.uint8)[:] = 0x5A
        status = lib.hy_table_scan_columns_strings(left_dev.handle, left_dict.handle, right_dev.handle, right_dict.handle, condition, C.byref(result.c))
        assert status == abi.OK or all((array.view(np.uint8) == 0x5A).all() for array in (result.matches, result.offsets, result.counts, result.chunk_state))
        return status

    assert scan() == abi.OK
    ints = DeviceColumn(storage.make_column(np.arange(165, dtype=np.int32) % 7, None, abi.ENC_DICTIONARY, chunk_size=100))
    assert ints.n_chunks == 2
    two_chunks = Pair(left[:2], right[:2])
    assert scan(left_dev=ints, left_dict=two_chunks.left_dict, right_dev=two_chunks.right_dev, right_dict=two_chunks.right_dict) == abi.ERR_INVALID   # strings and non-strings
    assert b"strings and non-strings" in lib.hy_last_error()
    assert scan(right_dev=ints) == abi.ERR_INVALID                                                      # chunk counts of the columns
    assert scan(left_dict=DeviceStringDictionary(dictionaries[:2])) == abi.ERR_INVALID                  # chunk count of a dictionary
    assert scan(right_dict=DeviceStringDictionary([c[0] for c in right] + [[b"x"]])) == abi.ERR_INVALID
    assert scan(left_dict=DeviceStringDictionary([dictionaries[0], dictionaries[1][:-1], dictionaries[2]])) == abi.ERR_INVALID   # n_entries against aux_size
    assert scan(right_dict=pair.left_dict) == abi.ERR_INVALID
    for condition in (abi.PRED_BETWEEN_INCLUSIVE, abi.PRED_IS_NULL, abi.PRED_LIKE, abi.PRED_IN):
        assert scan(condition=condition) == abi.ERR_INVALID                                             # the six binary conditions only
    result = HostScanResult(3, pair.left_dev.rows)
    for arguments in ((None, pair.left_dict.handle, pair.right_dev.handle, pair.right_dict.handle), (pair.left_dev.handle, None, pair.right_dev.handle, pair.right_dict.handle),
                      (pair.left_dev.handle, pair.left_dict.handle, None, pair.right_dict.handle), (pair.left_dev.handle, pair.left_dict.handle, pair.right_dev.handle, None)):
        assert lib.hy_table_scan_columns_strings(*arguments, abi.PRED_EQUALS, C.byref(result.c)) == abi.ERR_INVALID
    # hy_table_scan_columns still has no dictionaries to read, and says where to go
    assert lib.hy_table_scan_columns(pair.left_dev.handle, pair.right_dev.handle, abi.PRED_EQUALS, C.byref(result.c)) == abi.ERR_UNSUPPORTED
    assert b"hy_table_scan_columns_strings" in lib.hy_last_error()
    # unencoded string segments never become a column: hy_column_create refuses them, so the scan's own refusal of them is a second line
    unencoded = HostColumn([HostSegment(abi.ENC_UNENCODED, abi.TYPE_STRING, 4, 4, np.zeros(4, dtype=np.uint32))], abi.TYPE_STRING)
    with pytest.raises(abi.HyriseAmdError) as refused:
        DeviceColumn(unencoded)
    assert refused.value.status == abi.ERR_UNSUPPORTED

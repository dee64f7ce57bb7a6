"""hy_string_column_substr (csrc/string_substr.hip) against tests/string_substr_oracle.py, byte for byte after read-back: every output
chunk's dictionary (entries, chars, offsets, entry count) and attribute vector.  Shapes are the smallest at which each mechanism can go
wrong: windows at every misalignment against the copy's 16-byte spans, results that collapse and reorder the source dictionary, more
entries than a copy tile and a scan tile hold, NULL rows and a chunk of them, fixed slots beside offsets, every attribute vector kind,
reference columns, the identity window against the gather, and the result as the input of the operators that read string columns."""
import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.like import LikeMatcher
from hyrise_amd.operators import aggregate_hash_columns, column_string_ranks, sort, string_column_gather, string_column_substr, table_scan_like
from hyrise_amd.storage import DeviceColumn, HostColumn
from placed_columns import PlacedColumn
from support import result_rows
from test_like_device_gpu import BYTE_ENTRIES
from test_string_gather_gpu import Source, assert_result, byte_source
import string_substr_oracle as oracle

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF
ALL = 2**31 - 1


def check_substr(source, start, length, context, column=None, chunks=None):
    got = string_column_substr(column or source.dev, source.dev_dict, start, length)
    assert_result(got, oracle.column_substr(chunks or source.chunks, start, length), f"{context}: SUBSTR({start}, {length})")
    return got


def draw(rng, entries, n, null_fraction=0.0):
    return [None if rng.random() < null_fraction else entries[i] for i in rng.integers(0, len(entries), n)]


@pytest.fixture(scope="module")
def span_source(device):
    """Three chunks of 1 000 rows over entries of 0, 1, 15, 16, 17, 31, 32, 33 and 100 bytes from a two-letter alphabet: windows of
    different entries are often equal."""
    rng = np.random.default_rng(1)
    entries = sorted({bytes(rng.choice(list(b"ab"), length).tolist()) for length in (0, 1, 15, 16, 17, 31, 32, 33, 100) for _ in range(40)})
    return Source([draw(rng, entries, 1_000) for _ in range(3)])


@pytest.mark.parametrize("length", [ALL, 16, 17, 1])
@pytest.mark.parametrize("start", [1, 2, 8, 16], ids=lambda s: f"byte_{s - 1}")
def test_copy_spans_and_misaligned_windows(span_source, start, length):
    check_substr(span_source, start, length, "spans")


@pytest.fixture(scope="module")
def date_source(device):
    """2 500 distinct YYYY-MM-DD strings, 1992-01-01 .. 1998-11-04, every one of them in each of two chunks."""
    days = [str(day).encode() for day in np.datetime64("1992-01-01") + np.arange(2_500)]
    rng = np.random.default_rng(2)
    return Source([[days[i] for i in rng.permutation(2_500)] + draw(rng, days, 300) for _ in range(2)])


@pytest.mark.parametrize("start,length", [(1, 4), (6, 2), (9, 2), (-2, 2), (0, 5), (20, 3), (1, 0), (-30, 25)])
def test_dates_collapse_and_reorder(date_source, start, length):
    got = check_substr(date_source, start, length, "dates")
    n_entries = {(1, 4): 7, (6, 2): 12, (20, 3): 1, (1, 0): 1}.get((start, length))
    if n_entries:
        assert got.dictionary.n_entries == [n_entries] * 2
    if (start, length) in ((20, 3), (1, 0)):
        assert got.dictionary.read_chunk(0)[0] == [b""]


@pytest.mark.parametrize("start,length", [(1, 5), (2, 4), (-6, 4)])
def test_seventy_thousand_rows_and_three_thousand_results(device, start, length):
    """One chunk; 6 000 source entries k0000-0 .. k2999-1: more output entries than COPY_TILE and more rows than one scan tile."""
    entries = [b"k%04d-%d" % (i % 3_000, i // 3_000) for i in range(6_000)]
    source = Source([draw(np.random.default_rng(3), entries, 70_000)])
    got = check_substr(source, start, length, "70 000 rows")
    assert got.dictionary.n_entries == [3_000]


def test_null_rows_and_a_chunk_of_nulls(device):
    rng = np.random.default_rng(4)
    chunks = [draw(rng, BYTE_ENTRIES, 500, 0.1), [None] * 70, draw(rng, BYTE_ENTRIES, 333, 0.1)]
    source = Source(chunks)
    for start, length in ((1, 2), (2, ALL), (-2, 2), (3, 0)):
        got = check_substr(source, start, length, "NULLs")
        assert got.dictionary.n_entries[1] == 0 and got.read_value_ids()[1].tolist() == [0] * 70
        assert [row is None for row in got.read()] == [row is None for chunk in chunks for row in chunk]


@pytest.mark.parametrize("fixed_lengths", [(12, None), (None, 9)], ids=["slot_12", "slot_9"])
def test_fixed_slots_beside_offsets(device, fixed_lengths):
    """Slots hold entries of 0 .. slot bytes, some filling the slot (slots of 12 lie on 4-byte boundaries, slots of 9 mostly not); windows
    reach past strnlen; the offsets chunk has entries with '\\0' inside, which is data there."""
    rng = np.random.default_rng(5)
    slot = next(length for length in fixed_lengths if length)
    plain = sorted({bytes(rng.choice(list(b"abc"), length).tolist()) for length in range(slot + 1) for _ in range(6)})
    with_zero = plain + [b"a\x00bc", b"\x00", b"ab\x00\x00", b"abcabcabcabc\x00x"]
    chunks = [draw(rng, plain if length else with_zero, 400, 0.05) for length in fixed_lengths]
    source = Source(chunks, fixed_lengths=fixed_lengths)
    assert any(len(e) == slot for e in source.dictionaries[0 if fixed_lengths[0] else 1])
    for start, length in ((1, ALL), (3, 20), (1, slot), (-4, 3), (slot, 5), (slot + 1, 5), (2, 2)):
        check_substr(source, start, length, f"slots of {slot}")


@pytest.mark.parametrize("width", [1, 2, 4, "bits"], ids=lambda w: f"width_{w}")
def test_attribute_vector_widths(device, width):
    source = byte_source(width)
    for start, length in ((1, 2), (2, 3)):
        check_substr(source, start, length, f"width {width}")


@pytest.mark.parametrize("lists", ["host", "device"])
def test_reference_columns(device, lists):
    """PosLists in host memory (uploaded) and in device memory (where a scan leaves them): the matches of a LIKE scan, an entire chunk, an
    empty list, and a list that points into all three source chunks and holds NULL RowIDs.  Equal substrings of different source chunks are
    one entry; a NULL RowID is a NULL row."""
    rng = np.random.default_rng(6)
    days = [str(day).encode() for day in np.datetime64("1995-11-01") + np.arange(200)]
    source = Source([draw(rng, days, 300, 0.05) for _ in range(3)])
    scanned = np.array(result_rows(table_scan_like(source.dev, source.dev_dict, b"%-1_-%", abi.PRED_LIKE, nullable=True)), dtype=np.uint32).reshape(-1, 2)
    assert len(set(scanned[:, 0].tolist())) == 3
    spanning = np.stack([rng.integers(0, 3, 400), rng.integers(0, 300, 400)], axis=1).astype(np.uint32)
    spanning[rng.random(400) < 0.1] = NULL
    spanning[0] = NULL
    pos_lists = [scanned, 1, spanning[:0], spanning]
    reference = storage.make_reference_column(source.host, pos_lists, [None, 1, 2 if lists == "device" else None, None])
    if lists == "device":
        reference_dev = PlacedColumn(reference, "aligned", 0x00, refs={id(source.host): source.dev})
    else:
        reference_dev = DeviceColumn(reference, refs={id(source.host): source.dev})
    rows = [[source.chunks[c][o] if c != NULL else None for c, o in ([(pos, o) for o in range(300)] if isinstance(pos, int) else pos.tolist())] for pos in pos_lists]
    for start, length in ((1, 4), (6, 2), (-2, 2)):
        got = check_substr(source, start, length, f"{lists} PosLists", column=reference_dev, chunks=rows)
        assert got.read()[len(rows[0]) + 300] is None
    assert len(oracle.column_substr(rows, 1, 4)[0][3]) == 2   # (1995 and 1996, each from all three source chunks)
    if lists == "device":
        reference_dev.assert_untouched()


def test_the_identity_window_is_the_gather(span_source):
    """(1, 2^31 - 1) over a data column: hy_string_column_gather at the identity positions, byte for byte; and arguments at the ends of
    int32 are answered."""
    source = span_source
    got = check_substr(source, 1, ALL, "identity")
    positions = np.array([(c, o) for c in range(3) for o in range(1_000)], dtype=np.uint32)
    gathered = string_column_gather(source.dev, source.dev_dict, positions, 1_000)
    assert [ids.tobytes() for ids in got.read_value_ids()] == [ids.tobytes() for ids in gathered.read_value_ids()]
    for c in range(3):
        (_, chars, offsets), (_, want_chars, want_offsets) = got.dictionary.read_chunk(c), gathered.dictionary.read_chunk(c)
        assert chars.tobytes() == want_chars.tobytes() and offsets.tobytes() == want_offsets.tobytes()
    assert got.dictionary.n_entries == gathered.dictionary.n_entries
    check_substr(source, 2, ALL, "ends of int32")
    check_substr(source, -2**31, ALL, "ends of int32")
    check_substr(source, ALL, ALL, "ends of int32")
    check_substr(source, -2**31, -2**31, "ends of int32")


def test_the_result_feeds_like_sort_and_aggregate(date_source):
    """hy_table_scan_like, hy_column_string_ranks -> hy_sort, and hy_aggregate_hash_columns grouped by the ranks with a SUM, each over the
    result pair of SUBSTR(date, 1, 7) with NULL rows."""
    rng = np.random.default_rng(7)
    chunks = [[None if rng.random() < 0.1 else row for row in chunk[:1_500]] for chunk in date_source.chunks]
    source = Source(chunks)
    got = check_substr(source, 1, 7, "consumers")
    rows = [row for chunk in chunks for row in oracle.substr_rows(chunk, 1, 7)]
    for condition, pattern in ((abi.PRED_LIKE, b"1996-0%"), (abi.PRED_NOT_LIKE, b"%-1_")):
        matcher = LikeMatcher(pattern, condition)
        found = result_rows(table_scan_like(got, got.dictionary, pattern, condition, nullable=True))
        assert found == [(i // 1_500, i % 1_500) for i, row in enumerate(rows) if row is not None and matcher(row)], f"LIKE {pattern!r} ({condition})"
    stand_in = column_string_ranks(got, got.dictionary)
    order = sort([stand_in], [abi.SORT_ASCENDING_NULLS_FIRST]).numpy()
    flat = (order[:, 0].astype(np.int64) * 1_500 + order[:, 1]).tolist()
    present = [i for i, row in enumerate(rows) if row is not None]
    assert flat == [i for i, row in enumerate(rows) if row is None] + sorted(present, key=lambda i: rows[i])
    amounts = rng.integers(-1_000, 1_000, len(rows)).astype(np.int32)
    amount_column = DeviceColumn(HostColumn([storage.encode_segment(amounts[begin:begin + 1_500], None, abi.ENC_UNENCODED) for begin in (0, 1_500)], abi.TYPE_INT))
    result = aggregate_hash_columns([stand_in], [(abi.AGG_SUM, amount_column)], chunk_rows=50)
    ranks, rank_nulls = result.groupby[0].read()
    sums = result.column(0)
    distinct = sorted({row for row in rows if row is not None})
    want = {}
    for row, amount in zip(rows, amounts.tolist()):
        want[row] = want.get(row, 0) + amount
    assert result.n_groups == len(want)
    assert {None if rank_nulls[g] else distinct[ranks[g]]: sums[g] for g in range(result.n_groups)} == want
    stand_in.close()

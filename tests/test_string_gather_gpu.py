"""hy_string_column_gather and hy_string_ranks_gather (csrc/string_gather.hip) against tests/string_gather_oracle.py, byte for byte after
read-back: every output chunk's dictionary (entries, chars, offsets) and attribute vector -- sizes around the wave and the tile, NULL
RowIDs and NULL rows, bytes as bytes, a 100 000-byte entry, entries so short that a copy workgroup's stretch overflows its LDS tile, every
attribute vector width, both dictionary layouts mixed, reference columns, caller-owned positions between guards; and the result as the
input of the operators that read string columns."""
import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.like import LikeMatcher
from hyrise_amd.operators import (aggregate_hash_columns, column_string_ranks, sort, string_column_gather, string_dictionary_order, string_ranks_gather,
                                  table_scan_like)
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn
from placed_columns import PlacedArray, PlacedColumn
from support import result_rows
from test_like_device_gpu import BYTE_ENTRIES
from test_string_order_gpu import MixedDictionary
from test_string_rank_column_gpu import widened
import string_gather_oracle as oracle
import string_order_oracle

pytestmark = pytest.mark.gpu

NULL = 0xFFFFFFFF


class Source:
    """A string column from per-chunk lists of bytes / None, its dictionaries uploaded (fixed_lengths[c]: that chunk in the fixed-slot layout)."""

    def __init__(self, chunks, width=None, fixed_lengths=None):
        self.chunks = chunks
        encoded = [storage.encode_string_dictionary([v if v is not None else b"" for v in chunk], [v is None for v in chunk]) for chunk in chunks]
        self.dictionaries = [dictionary for _, dictionary in encoded]
        self.host = HostColumn(widened([segment for segment, _ in encoded], width), abi.TYPE_STRING)
        self.dev = DeviceColumn(self.host)
        self.dev_dict = MixedDictionary(self.dictionaries, fixed_lengths) if fixed_lengths else DeviceStringDictionary(self.dictionaries)


def assert_result(got, want, context):
    """got: a StringResultColumn; want: the oracle's (dictionaries, value ids)."""
    want_dictionaries, want_ids = want
    assert got.n_chunks == len(want_dictionaries) and got.rows == sum(map(len, want_ids)), context
    ids = got.read_value_ids()
    for c, dictionary in enumerate(want_dictionaries):
        entries, chars, offsets = got.dictionary.read_chunk(c)
        assert entries == dictionary, f"{context}: dictionary of chunk {c}"
        assert chars.tobytes() == b"".join(dictionary) and offsets.tolist() == np.cumsum([0] + [len(e) for e in dictionary]).tolist(), f"{context}: chars / offsets of chunk {c}"
        assert ids[c].dtype == np.uint32 and ids[c].tolist() == want_ids[c], f"{context}: value ids of chunk {c}"


def check_gather(source, positions, chunk_rows, context, column=None, chunks=None):
    positions = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1, 2)
    got = string_column_gather(column or source.dev, source.dev_dict, positions, chunk_rows)
    assert_result(got, oracle.column_gather(chunks or source.chunks, [tuple(p) for p in positions.tolist()], chunk_rows), context)
    return got


def random_positions(rng, chunks, n, null_fraction=0.1):
    sizes = np.array([len(chunk) for chunk in chunks])
    filled = np.flatnonzero(sizes)
    chunk_ids = filled[rng.integers(0, len(filled), n)]
    positions = np.stack([chunk_ids, (rng.random(n) * sizes[chunk_ids]).astype(np.int64)], axis=1).astype(np.uint32)
    positions[rng.random(n) < null_fraction] = NULL
    return positions


def byte_source(width=None, fixed_lengths=None, entries=BYTE_ENTRIES):
    """Three chunks that share entries: the empty string, \\0 inside entries, 0x80-0xFF, prefixes; NULL rows in every chunk."""
    short = [e for e in entries if fixed_lengths is None or (len(e) <= 8 and b"\x00" not in e)]   # (a slot's entry ends at its first \0)
    chunks = [short[c::3] + short[(c + 1) % 3::5] + [None, short[c]] + [None] * c for c in range(3)]
    return Source(chunks, width, fixed_lengths)


@pytest.fixture(scope="module")
def shared_source(device):
    return byte_source()


@pytest.mark.parametrize("chunk_rows", [1, 3, 64, 1000])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_sizes(shared_source, n, chunk_rows):
    """NULL RowIDs at the start, at the end, and filling a whole output chunk (rows 3 .. 5 and 64 .. 127)."""
    positions = random_positions(np.random.default_rng(n * 7 + chunk_rows), shared_source.chunks, n)
    positions[:1] = NULL
    positions[-1:] = NULL
    positions[3:6] = NULL
    positions[64:128] = NULL
    check_gather(shared_source, positions, chunk_rows, f"n {n}, chunk_rows {chunk_rows}")


def test_seventy_thousand_rows_over_three_chunks_of_seventy_thousand_entries(device):
    """u32 attribute vectors on both sides; two output chunks of 65 535 and 4 465 rows; half of every chunk's entries are shared."""
    shared = [b"s%06d" % i for i in range(35_000)]
    chunks = [shared + [b"%c%06d" % (0x61 + c, 3 * i + c) for i in range(35_000)] for c in range(3)]
    source = Source(chunks)
    assert all(len(d) == 70_000 for d in source.dictionaries) and all(s.width == 4 for s in source.host.segments)
    got = check_gather(source, random_positions(np.random.default_rng(1), chunks, 70_000, 0.01), 65_535, "70 000 rows")
    assert got.n_chunks == 2 and got.read_value_ids()[1].shape == (4_465,)


def test_one_long_entry_among_short_ones(device):
    long_entry = bytes(np.random.default_rng(2).integers(0, 256, 100_000, dtype=np.uint8))
    chunks = [[b"a", long_entry, b"zz", None], [b"b", long_entry[:99_999], b""]]
    source = Source(chunks)
    positions = [(0, 1), (1, 1), (0, 0), (1, 2), (0, 1), (NULL, NULL), (1, 0), (0, 2)]
    check_gather(source, positions, 100, "one chunk")
    check_gather(source, positions, 3, "the long entries in two chunks")


def test_entries_too_short_for_the_copy_tile(device):
    """2- and 3-byte entries: a workgroup's 4 KiB of output hold more entry starts than it stages in LDS; and a run of empty-string twins
    (fixed slots that begin with \\0) cannot occur in one output chunk, but 5 000 entries in a chunk can."""
    entries = sorted({bytes(e) for e in np.random.default_rng(3).integers(0x30, 0x7B, (6_000, 3), dtype=np.uint8)} | {b"%c%c" % (a, b) for a in range(0x41, 0x5B) for b in range(0x41, 0x5B)})
    source = Source([entries[0::2] + [b""], entries[1::2]])
    positions = [(c, o) for c in range(2) for o in range(len(source.chunks[c]))]
    check_gather(source, positions, 100_000, "all entries, one output chunk")
    check_gather(source, positions[::-1], 4_097, "all entries backwards, chunks of 4 097")


@pytest.mark.parametrize("width", [1, 2, 4, "bits"], ids=lambda w: f"width_{w}")
def test_attribute_vector_widths(device, width):
    source = byte_source(width)
    check_gather(source, random_positions(np.random.default_rng(4), source.chunks, 500), 128, f"width {width}")


@pytest.mark.parametrize("fixed_lengths", [(8, 8, 8), (8, None, 9), (None, 8, None)], ids=["fixed", "mixed", "mixed_other"])
def test_fixed_slot_and_offsets_chunks_mixed(device, fixed_lengths):
    """Slots of 8 bytes hold entries of 0 .. 8 bytes, some filling the slot; equal strings of a fixed-slot and an offsets chunk are one entry."""
    source = byte_source(fixed_lengths=fixed_lengths, entries=BYTE_ENTRIES + [b"12345678", b"1234567"])
    assert any(len(e) == 8 for d in source.dictionaries for e in d)
    check_gather(source, random_positions(np.random.default_rng(5), source.chunks, 700), 256, f"layouts {fixed_lengths}")


@pytest.mark.parametrize("n_chunks", [1, 2, 33])
def test_source_chunk_counts_and_empty_source_chunks(device, n_chunks):
    rng = np.random.default_rng(n_chunks)
    words = sorted({bytes(rng.choice(list(b"ab\x00\xff"), rng.integers(0, 7)).tolist()) for _ in range(400)})
    chunks = [[] if n_chunks > 2 and c % 5 == 1 else [None if rng.random() < 0.1 else words[i] for i in rng.integers(0, len(words), 1 + 40 * (c % 4))] for c in range(n_chunks)]
    source = Source(chunks)
    check_gather(source, random_positions(rng, chunks, 777), 100, f"{n_chunks} source chunks")


@pytest.mark.parametrize("lists", ["host", "device"])
def test_reference_columns_and_caller_owned_positions(device, lists):
    """PosLists in host memory (uploaded) and in the caller's device memory, one of them an entire chunk, one empty, one with NULL RowIDs;
    the positions at 8 modulo 16 between guard bytes that stay as they were."""
    source = byte_source()
    rng = np.random.default_rng(6)
    sizes = [len(chunk) for chunk in source.chunks]
    spanning = random_positions(rng, source.chunks, 300)
    pos_lists = [np.stack([np.zeros(sizes[0] // 2), np.arange(sizes[0] // 2) * 2], axis=1).astype(np.uint32), 1, spanning[:0], spanning]
    # (a caller-owned list without rows has no buffer and reads as an entire-chunk list: it names a chunk; an uploaded one need not)
    reference = storage.make_reference_column(source.host, pos_lists, [0, 1, 2 if lists == "device" else None, None])
    if lists == "device":
        reference_dev = PlacedColumn(reference, "aligned", 0x00, refs={id(source.host): source.dev})
    else:
        reference_dev = DeviceColumn(reference, refs={id(source.host): source.dev})
    # the reference table's rows as lists of strings
    rows = [[source.chunks[c][o] if c != NULL else None for c, o in ([(pos, o) for o in range(sizes[pos])] if isinstance(pos, int) else pos.tolist())] for pos in pos_lists]
    positions = random_positions(rng, rows, 500)
    placed = PlacedArray(8 * len(positions), 8, 0xA5, guard=64, contents=positions)
    got = string_column_gather(reference_dev, source.dev_dict, (placed.pointer, len(positions)), 128)
    assert_result(got, oracle.column_gather(rows, [tuple(p) for p in positions.tolist()], 128), f"{lists} PosLists")
    placed.assert_untouched()
    if lists == "device":
        reference_dev.assert_untouched()


def test_the_result_is_a_string_column_for_sort_and_like(device):
    """hy_column_string_ranks + hy_sort over a gathered column order the oracle's rows; hy_table_scan_like over it is the host matcher."""
    source = byte_source()
    positions = random_positions(np.random.default_rng(7), source.chunks, 1_000)
    chunk_rows = 300
    got = check_gather(source, positions, chunk_rows, "composition")
    rows = oracle.gathered_rows(source.chunks, [tuple(p) for p in positions.tolist()])
    stand_in = column_string_ranks(got, got.dictionary)
    order = sort([stand_in], [abi.SORT_ASCENDING_NULLS_FIRST]).numpy()
    flat = (order[:, 0].astype(np.int64) * chunk_rows + order[:, 1]).tolist()
    present = [i for i, row in enumerate(rows) if row is not None]
    assert flat == [i for i, row in enumerate(rows) if row is None] + sorted(present, key=lambda i: rows[i])
    stand_in.close()
    for condition, pattern in ((abi.PRED_LIKE, b"a%"), (abi.PRED_NOT_LIKE, b"%\x00%"), (abi.PRED_LIKE_INSENSITIVE, b"_")):
        matcher = LikeMatcher(pattern, condition)
        found = result_rows(table_scan_like(got, got.dictionary, pattern, condition, nullable=True))
        assert found == [(i // chunk_rows, i % chunk_rows) for i, row in enumerate(rows) if row is not None and matcher(row)], f"LIKE {pattern!r} ({condition})"


def test_the_inputs_may_die_before_the_result_is_read(device):
    source = byte_source()
    positions = random_positions(np.random.default_rng(8), source.chunks, 200)
    want = oracle.column_gather(source.chunks, [tuple(p) for p in positions.tolist()], 64)
    got = string_column_gather(source.dev, source.dev_dict, positions, 64)
    again = string_column_gather(source.dev, source.dev_dict, positions, 64)
    source.dev_dict.close()
    source.dev.close()
    assert_result(got, want, "after the inputs died")
    assert_result(again, want, "the second call")


# ---- hy_string_ranks_gather -----------------------------------------------------------------------------------------------------------------
def ranks_column(rank_chunks):
    """An int32 data column of unencoded segments with null vectors, one segment per list of ranks / None."""
    segments = [storage.encode_segment(np.array([0 if r is None else r for r in chunk], dtype=np.int32), np.array([r is None for r in chunk], dtype=bool), abi.ENC_UNENCODED)
                for chunk in rank_chunks]
    return DeviceColumn(HostColumn(segments, abi.TYPE_INT))


def test_ranks_fed_back_give_the_strings(device):
    source = byte_source(fixed_lengths=(8, None, 8), entries=BYTE_ENTRIES + [b"12345678"])
    ranks, n_distinct = string_dictionary_order(source.dev_dict)
    rank_chunks = [chunk.tolist() for chunk in ranks]
    assert [r for chunk in rank_chunks for r in chunk] == [r for chunk in string_order_oracle.column_order(source.dictionaries)[0] for r in chunk]
    got = string_ranks_gather(source.dev_dict, ranks_column(rank_chunks))
    assert_result(got, oracle.ranks_gather(source.dictionaries, rank_chunks), "ranks fed back")
    assert [got.dictionary.read_chunk(c)[0] for c in range(3)] == source.dictionaries
    # NULL ranks, -1, n_distinct and far outside: NULL rows; chunks of every size around the wave, one of them empty
    rng = np.random.default_rng(9)
    odd = [[None, -1, n_distinct, 2**31 - 1, -2**31, 0, n_distinct - 1], [], [None] * 5] + [[None if rng.random() < 0.2 else int(r) for r in rng.integers(-2, n_distinct + 2, n)] for n in (63, 64, 65, 1000)]
    assert_result(string_ranks_gather(source.dev_dict, ranks_column(odd)), oracle.ranks_gather(source.dictionaries, odd), "odd ranks")


def test_min_and_max_of_a_string_column_per_group(device):
    """MIN / MAX over the stand-in through hy_aggregate_hash_columns, then one gather: Python's min / max over bytes per group."""
    source = byte_source()
    rows = [row for chunk in source.chunks for row in chunk]
    sizes = [len(chunk) for chunk in source.chunks]
    rng = np.random.default_rng(10)
    keys = rng.integers(0, 7, len(rows)).astype(np.int32)
    key_column = DeviceColumn(HostColumn([storage.encode_segment(keys[begin:begin + size], None, abi.ENC_UNENCODED) for begin, size in zip(np.cumsum([0] + sizes[:-1]), sizes)], abi.TYPE_INT))
    stand_in = column_string_ranks(source.dev, source.dev_dict)
    result = aggregate_hash_columns([key_column], [(abi.AGG_MIN, stand_in), (abi.AGG_MAX, stand_in)], chunk_rows=4)
    group_keys = result.groupby[0].read()[0].tolist()
    for a, pick in ((0, min), (1, max)):
        got = string_ranks_gather(source.dev_dict, result.aggregates[a]).read()
        for key, value in zip(group_keys, got):
            members = [row for row, k in zip(rows, keys.tolist()) if k == key and row is not None]
            assert value == (pick(members) if members else None), f"group {key}, aggregate {a}"
    stand_in.close()


def test_a_ranks_column_of_chunks_without_rows(device):
    """Chunks but no rows (an aggregate over no groups): the same chunks without entries, and nothing is launched."""
    source = byte_source()
    for rank_chunks in ([[]], [[], [], []]):
        got = string_ranks_gather(source.dev_dict, ranks_column(rank_chunks))
        assert_result(got, oracle.ranks_gather(source.dictionaries, rank_chunks), f"{len(rank_chunks)} empty chunks")
        assert got.dictionary.n_entries == [0] * len(rank_chunks) and got.read() == []


def test_every_row_id_into_a_column_without_rows_is_a_null_row(device):
    source = Source([[]])
    positions = [(0, 0), (NULL, NULL), (3, 7), (0, 1), (0, NULL)]
    got = string_column_gather(source.dev, source.dev_dict, np.array(positions, dtype=np.uint32), 2)
    assert_result(got, ([[], [], []], [[0, 0], [0, 0], [0]]), "an empty column")
    assert got.read() == [None] * 5


def test_string_ranks_of_a_reference_column_with_an_uploaded_list_without_rows(device):
    """hy_column_string_ranks itself: an uploaded PosList without rows and without a common chunk id has no device buffer."""
    from test_string_rank_column_gpu import export
    source = byte_source()
    pos_lists = [np.zeros((0, 2), dtype=np.uint32), np.array([[1, 0], [NULL, NULL], [0, 2]], dtype=np.uint32)]
    reference = storage.make_reference_column(source.host, pos_lists, [None, None])
    reference_dev = DeviceColumn(reference, refs={id(source.host): source.dev})
    stand_in = column_string_ranks(reference_dev, source.dev_dict)
    values, nulls = export(stand_in)
    rank_of = {}
    for dictionary, ranks in zip(source.dictionaries, string_order_oracle.column_order(source.dictionaries)[0]):
        rank_of.update(zip(dictionary, ranks))
    assert stand_in.n_chunks == 2 and nulls.tolist() == [False, True, False]
    assert [values[0], values[2]] == [rank_of[source.chunks[1][0]], rank_of[source.chunks[0][2]]]
    stand_in.close()


def test_ranks_over_a_dictionary_without_entries(device):
    """E == 0 (a column of NULLs only): no rank exists, every row is NULL, whatever it holds."""
    source = Source([[None, None], [None]])
    assert source.dictionaries == [[], []]
    rank_chunks = [[0, None, -1], [], [5]]
    got = string_ranks_gather(source.dev_dict, ranks_column(rank_chunks))
    assert_result(got, ([[], [], []], [[0, 0, 0], [], [0]]), "no entries")
    assert got.read() == [None] * 4

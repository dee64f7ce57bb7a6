"""hy_column_string_ranks: the int32 stand-in of a string column as an ordinary column -- exported row by row against the oracle's ranks,
and as a key of hy_sort / hy_sort_limit against the same calls over string_rank_column's host-made int64 column, byte for byte: data
columns of every attribute vector width (bit-packed too), reference columns over host, device and entire-chunk PosLists."""
import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import column_string_ranks, sort, string_rank_column
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn, HostSegment
from hyrise_amd.string_keys import encode_string_column
from placed_columns import PlacedColumn
import string_order_oracle as oracle

pytestmark = pytest.mark.gpu

ASC, DESC = abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST
CHUNK, ROWS = 1_000, 4_000
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def string_table(seed, distinct=300, null_fraction=0.1):
    """4 chunks x 1 000 rows drawn from `distinct` strings (equal strings in every chunk), with NULLs."""
    rng = np.random.default_rng(seed)
    words = sorted({bytes(rng.choice(list(b"ab\x00\xff"), rng.integers(0, 7)).tolist()) for _ in range(4 * distinct)})[:distinct]
    strings = [words[i] for i in rng.integers(0, len(words), ROWS)]
    nulls = rng.random(ROWS) < null_fraction
    return strings, nulls


def widened(segments, width):
    """The same segments with attribute vectors of `width` bytes (a wider one than the narrowest is legal), or bit-packed ("bits")."""
    if width is None:
        return segments
    if width == "bits":
        return [storage.bit_pack_segment(s) for s in segments]
    return [HostSegment(s.encoding, s.data_type, s.size, width, s.data.astype(UINT[width]), aux=None, aux_size=s.aux_size) for s in segments]


class Case:
    def __init__(self, strings, nulls, width=None):
        self.strings, self.nulls = strings, nulls
        segments, self.dictionaries = encode_string_column(strings, nulls, CHUNK)
        self.string_host = HostColumn(widened(segments, width), abi.TYPE_STRING)
        self.string_dev = DeviceColumn(self.string_host)
        self.dev_dict = DeviceStringDictionary(self.dictionaries)
        self.stand_in = column_string_ranks(self.string_dev, self.dev_dict)
        self.ranks_host, _ = string_rank_column(segments, self.dictionaries)          # the host path: int64 ranks over the same vectors
        self.ranks_dev = DeviceColumn(self.ranks_host)
        rank_of = {}
        for dictionary, ranks in zip(self.dictionaries, oracle.column_order(self.dictionaries)[0]):
            rank_of.update(zip(dictionary, ranks))
        self.row_ranks = np.array([0 if is_null else rank_of[s] for s, is_null in zip(strings, nulls)], dtype=np.int32)


def export(column):
    import torch
    lib = abi.load_library()
    values = torch.full((max(1, column.rows),), -7, dtype=torch.int32, device="cuda")
    nulls = torch.full((max(1, column.rows),), 9, dtype=torch.uint8, device="cuda")
    abi.check(lib.hy_column_export(column.handle, values.data_ptr(), nulls.data_ptr()))
    abi.check(lib.hy_synchronize())
    return values.cpu().numpy()[:column.rows], nulls.cpu().numpy()[:column.rows].astype(bool)


def assert_same_sorts(stand_in_keys, host_keys, rows, context):
    """hy_sort and hy_sort_limit (both forced paths; limits 1, 10 and rows + 1) over the two key lists give the same bytes."""
    for modes in ([ASC] * len(host_keys), [DESC] * len(host_keys), [ASC, DESC][:len(host_keys)]):
        want = sort(host_keys, modes).numpy()
        assert sort(stand_in_keys, modes).numpy().tobytes() == want.tobytes(), f"{context} modes {modes}"
        for limit in (1, 10, rows + 1):
            for flags in (abi.SORT_LIMIT_FORCE_FULL_SORT, abi.SORT_LIMIT_FORCE_SELECT):
                got = sort(stand_in_keys, modes, limit=limit, flags=flags).numpy()
                assert got.tobytes() == sort(host_keys, modes, limit=limit, flags=flags).numpy().tobytes(), f"{context} modes {modes} limit {limit} flags {flags}"
                assert got.tobytes() == want[:limit].tobytes(), f"{context} modes {modes} limit {limit} flags {flags}"


@pytest.mark.parametrize("width", [None, 1, 2, 4, "bits"], ids=lambda w: f"width_{w}")
def test_data_column_export_and_sort(device, width):
    strings, nulls = string_table(1, distinct=200 if width in (None, 1) else 300)
    case = Case(strings, nulls, width)
    assert case.stand_in.rows == ROWS and case.stand_in.n_chunks == 4
    values, null_flags = export(case.stand_in)
    assert np.array_equal(null_flags, nulls) and np.array_equal(values[~nulls], case.row_ranks[~nulls])
    assert_same_sorts([case.stand_in], [case.ranks_dev], ROWS, f"width {width}")
    # the sorted order is the strings' own: NULLs first, then byte order, ties in input order
    got = sort([case.stand_in], [ASC]).numpy()
    order = (got[:, 0].astype(np.int64) * CHUNK + got[:, 1]).tolist()
    present = [i for i in range(ROWS) if not nulls[i]]
    assert order == [i for i in range(ROWS) if nulls[i]] + sorted(present, key=lambda i: strings[i])


def test_two_keys_in_both_orders(device):
    strings, nulls = string_table(2, distinct=40)
    case = Case(strings, nulls)
    ints = DeviceColumn(storage.make_column(np.random.default_rng(2).integers(0, 5, ROWS).astype(np.int32), None, abi.ENC_DICTIONARY, chunk_size=CHUNK))
    assert_same_sorts([case.stand_in, ints], [case.ranks_dev, ints], ROWS, "(string, int)")
    assert_same_sorts([ints, case.stand_in], [ints, case.ranks_dev], ROWS, "(int, string)")


def test_one_distinct_string_keeps_the_input_order(device):
    case = Case([b"same"] * ROWS, np.zeros(ROWS, dtype=bool))
    assert_same_sorts([case.stand_in], [case.ranks_dev], ROWS, "one string")
    for mode in (ASC, DESC):
        got = sort([case.stand_in], [mode]).numpy()
        assert (got[:, 0].astype(np.int64) * CHUNK + got[:, 1]).tolist() == list(range(ROWS))


@pytest.mark.parametrize("lists", ["host", "device"])
def test_reference_columns(device, lists):
    """The stand-in of a reference column reads the same PosLists: a scan's output (one referenced chunk per list, one list an entire chunk,
    one empty) and lists that span the chunks, with NULL RowIDs -- in host memory (uploaded) and in the caller's device memory."""
    strings, nulls = string_table(3)
    case = Case(strings, nulls)
    rng = np.random.default_rng(4)
    keep = [np.flatnonzero(rng.random(CHUNK) < 0.5) for _ in range(4)]
    scan_lists = [np.stack([np.full(len(k), c), k], axis=1).astype(np.uint32) for c, k in enumerate(keep)]
    scan_lists[1], scan_lists[3] = 1, scan_lists[3][:0]
    spanning = []
    for size in (1, 65, 2_049):
        rows = rng.integers(0, ROWS, size)
        pos = np.stack([rows // CHUNK, rows % CHUNK], axis=1).astype(np.uint32)
        pos[rng.random(size) < 0.05] = 0xFFFFFFFF
        spanning.append(pos)
    for pos_lists, common in ((scan_lists, [0, 1, 2, 3]), (spanning, None)):
        string_ref = storage.make_reference_column(case.string_host, pos_lists, common)
        ranks_ref = storage.make_reference_column(case.ranks_host, pos_lists, common)
        if lists == "device":
            string_ref_dev = PlacedColumn(string_ref, "aligned", 0x00, refs={id(case.string_host): case.string_dev})
        else:
            string_ref_dev = DeviceColumn(string_ref, refs={id(case.string_host): case.string_dev})
        ranks_ref_dev = DeviceColumn(ranks_ref, refs={id(case.ranks_host): case.ranks_dev})
        stand_in = column_string_ranks(string_ref_dev, case.dev_dict)
        assert stand_in.rows == string_ref.rows and stand_in.n_chunks == string_ref.n_chunks
        # row by row: the rank of the referenced row, NULL for a NULL row or a NULL RowID
        flat = []
        for pos in pos_lists:
            flat += [c * CHUNK + o if c != 0xFFFFFFFF else -1 for c, o in ([(pos, o) for o in range(CHUNK)] if isinstance(pos, int) else pos.tolist())]
        flat = np.array(flat, dtype=np.int64)
        want_nulls = (flat < 0) | nulls[np.maximum(flat, 0)]
        values, null_flags = export(stand_in)
        assert np.array_equal(null_flags, want_nulls) and np.array_equal(values[~want_nulls], case.row_ranks[flat[~want_nulls]])
        assert_same_sorts([stand_in], [ranks_ref_dev], string_ref.rows, f"{lists} lists, common {common}")
        stand_in.close()
        if lists == "device":
            string_ref_dev.assert_untouched()


def test_the_dictionary_may_die_before_the_sort_and_the_stand_in_before_the_column(device):
    strings, nulls = string_table(5)
    case = Case(strings, nulls)
    want = sort([case.ranks_dev], [DESC]).numpy()
    case.dev_dict.close()
    assert sort([case.stand_in], [DESC]).numpy().tobytes() == want.tobytes()
    case.stand_in.close()
    # the string column is as it was: a second stand-in over a fresh dictionary sorts the same
    again = column_string_ranks(case.string_dev, DeviceStringDictionary(case.dictionaries))
    assert sort([again], [DESC]).numpy().tobytes() == want.tobytes()
    again.close()
    case.string_dev.close()

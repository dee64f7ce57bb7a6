"""The join keys of two string columns made in HBM (csrc/string_join_keys.hip): hy_string_dictionary_order_pair and
hy_string_dictionary_join_ids against tests/string_join_keys_oracle.py bit for bit, with HY_MEM_HOST and HY_MEM_DEVICE results;
hy_column_string_join_keys' stand-ins row for row; and hy_join_hash / hy_join_sort_merge over the stand-ins against the joins over
host-made keys and over the strings themselves."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.join_keys import StringJoinKeys, std_hash_bytes
from hyrise_amd.operators import (column_string_join_keys, join_hash, join_sort_merge, string_dictionary_join_ids, string_dictionary_order_pair,
                                  table_scan_like)
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn, HostSegment
from hyrise_amd.string_keys import encode_string_column
from placed_columns import PlacedArray
from support import oracle_join
from test_join_gpu import assert_join_equal
from test_string_join_keys_oracle import key_column, words_table
import string_join_keys_oracle as oracle

pytestmark = pytest.mark.gpu

UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
NULL_ROW = 0xFFFFFFFF


def flat(per_chunk, dtype):
    return np.array([x for chunk in per_chunk for x in chunk], dtype=dtype)


class PlacedDictionary:
    """An HY_MEM_DEVICE hy_string_dictionary whose chars begin `residue` bytes behind a 16-byte boundary inside a larger tensor (offsets
    layout, offsets on 4 bytes only; or slots of `fixed_length` bytes), with filler around every buffer."""

    def __init__(self, dictionaries, residue, fill, fixed_length=None):
        self.lib = abi.load_library()
        self.n_chunks, self.n_entries = len(dictionaries), [len(d) for d in dictionaries]
        self.arrays = []
        chunks = (abi.StringDictionaryChunk * max(1, self.n_chunks))()
        for c, dictionary in enumerate(dictionaries):
            chars, offsets = storage.pack_string_dictionary(dictionary, fixed_length)
            placed_chars = PlacedArray(len(chars), residue, fill, contents=chars)
            self.arrays.append(placed_chars)
            chunks[c].n_entries, chunks[c].string_length, chunks[c].chars, chunks[c].offsets = len(dictionary), fixed_length or 0, placed_chars.pointer, None
            if offsets is not None:
                placed_offsets = PlacedArray(offsets.nbytes, 4, fill, contents=offsets)
                self.arrays.append(placed_offsets)
                chunks[c].offsets = placed_offsets.pointer
        self.handle = C.c_void_p()
        abi.check(self.lib.hy_string_dictionary_create(chunks, self.n_chunks, abi.MEM_DEVICE, C.byref(self.handle)))

    def assert_untouched(self):
        for array in self.arrays:
            array.assert_untouched()

    def __del__(self):
        if self.handle:
            self.lib.hy_string_dictionary_destroy(self.handle)


def assert_keys(left_dicts, right_dicts, left_dev, right_dev, context, fill=0x00):
    """Ranks, n_distinct and ids of the pair, with host results and into caller-owned device buffers between guards."""
    lib = abi.load_library()
    want_left, want_right, want_distinct = oracle.joint_order(left_dicts, right_dicts)
    want_left_ids, want_right_ids = oracle.join_ids(left_dicts, right_dicts)
    got_left, got_right, n_distinct = string_dictionary_order_pair(left_dev, right_dev)
    assert n_distinct == want_distinct, context
    for got, want in ((got_left, want_left), (got_right, want_right)):
        assert len(got) == len(want) and all(g.dtype == np.int32 and g.tolist() == w for g, w in zip(got, want)), f"{context}: host ranks"
    got_left, got_right = string_dictionary_join_ids(left_dev, right_dev)
    for got, want in ((got_left, want_left_ids), (got_right, want_right_ids)):
        assert len(got) == len(want) and all(g.dtype == np.int64 and g.tolist() == w for g, w in zip(got, want)), f"{context}: host ids"
    n_left, n_right = sum(map(len, left_dicts)), sum(map(len, right_dicts))
    for width, dtype, want_l, want_r in ((4, np.int32, want_left, want_right), (8, np.int64, want_left_ids, want_right_ids)):
        left_out, right_out = PlacedArray(width * n_left, width, fill, guard=64), PlacedArray(width * n_right, 16 - width, fill, guard=64)
        n = C.c_uint32(0xFFFFFFFF)
        if width == 4:
            abi.check(lib.hy_string_dictionary_order_pair(left_dev.handle, right_dev.handle, abi.MEM_DEVICE, left_out.pointer, right_out.pointer, C.byref(n)))
            assert n.value == want_distinct
        else:
            abi.check(lib.hy_string_dictionary_join_ids(left_dev.handle, right_dev.handle, abi.MEM_DEVICE, left_out.pointer, right_out.pointer))
            abi.check(lib.hy_synchronize())   # (no host round trip: stream order)
        for out, want in ((left_out, want_l), (right_out, want_r)):
            inside, guards_intact = out.read(dtype)
            assert guards_intact and np.array_equal(inside, flat(want, dtype)), f"{context}: device {'ranks' if width == 4 else 'ids'}"


# ---- the hash -------------------------------------------------------------------------------------------------------------------------------
def hash_entries():
    """Every length 0 .. 17 plus 23, 24, 25 and 78: no word, the 8- and 16-byte word boundaries, every tail length; \\0 inside, 0x7F, 0x80, 0xFF."""
    special = [0x00, 0x7F, 0x80, 0xFF]
    entries = set()
    for length in list(range(18)) + [23, 24, 25, 78]:
        for variant in range(2):
            entries.add(bytes((0x61 + (i + variant) % 7) if (i + variant) % 3 else special[(i + length + variant) % 4] for i in range(length)))
    return sorted(entries)


@pytest.mark.parametrize("residue", range(8))
def test_hash_of_every_length_at_every_byte_address(device, residue):
    entries = hash_entries()
    assert {len(e) for e in entries} == set(range(18)) | {23, 24, 25, 78} and any(0 in e[:-1] for e in entries) and any(0xFF in e for e in entries)
    other = [e for e in entries if len(e) % 3 == 0] + [b"right only " * 7]
    fill = 0xFF if residue % 2 else 0x00
    left, right = PlacedDictionary([entries[:20], entries[20:]], residue, fill), PlacedDictionary([sorted(other)], (residue + 5) % 16, fill)
    got_left, _ = string_dictionary_join_ids(left, right)
    assert [int(i) & 0xFFFFF for i in np.concatenate(got_left)] == [std_hash_bytes(e) & 0xFFFFF for e in entries]
    assert_keys([entries[:20], entries[20:]], [sorted(other)], left, right, f"offsets layout at {residue}", fill)
    left.assert_untouched()
    right.assert_untouched()


@pytest.mark.parametrize("residue", range(8))
@pytest.mark.parametrize("string_length", [5, 16])
def test_hash_of_fixed_length_slots(device, residue, string_length):
    """Entries shorter than the slot, one byte short of it, and filling it (no terminator: the next slot's bytes must not be hashed)."""
    L = string_length
    lengths = sorted({0, 1, 2, L // 2, L - 1, L} | ({8, 9} if L > 9 else set()))
    entries = sorted({bytes((0x80 + 0x7F * (i % 2) + n) % 255 + 1 for i in range(n)) for n in lengths} | {b"\xff" * L, b"\x7f" * (L - 1), b"a" * L, b"a" * (L - 1)})
    fill = 0xFF if residue % 2 else 0x00
    left = PlacedDictionary([entries[::2], entries[1::2], entries], residue, fill, fixed_length=L)
    right_dicts = [[b"a" * L, b"b"], entries[:3]]
    right = PlacedDictionary(right_dicts, residue + 8, fill)   # (the offsets layout on the other side)
    assert_keys([entries[::2], entries[1::2], entries], right_dicts, left, right, f"slots of {L} at {residue}", fill)
    left.assert_untouched()


# ---- the joint order ------------------------------------------------------------------------------------------------------------------------
def five_runs():
    big = [b"k%05d" % i for i in range(257)]                                         # crosses the 256-entry block
    left = [[b"", b"ab", b"abc", b"left only", b"shared"], [], [b"ab", b"left too", b"shared", b"zz\x00", b"zz\x00a"]]
    right = [sorted(big + [b"", b"abc", b"shared"]), [b"ab", b"right only", b"zz\x00a", b"\xff"]]
    return left, right


def test_joint_order_of_three_and_two_chunks(device):
    left, right = five_runs()
    assert_keys(left, right, DeviceStringDictionary(left), DeviceStringDictionary(right), "3 + 2 chunks")
    assert_keys(right, left, DeviceStringDictionary(right), DeviceStringDictionary(left), "2 + 3 chunks")
    left[1] = [b"k%05d" % i for i in range(100, 357)]                                 # 257 entries on the left too, half of them shared
    assert_keys(left, right, DeviceStringDictionary(left), DeviceStringDictionary(right), "3 + 2 chunks, two of 257")


@pytest.mark.parametrize("empty", [[], [[]], [[], []]], ids=["no_chunks", "one_empty_chunk", "two_empty_chunks"])
def test_one_side_without_entries(device, empty):
    left, _ = five_runs()
    assert_keys(left, empty, DeviceStringDictionary(left), DeviceStringDictionary(empty), "right empty")
    assert_keys(empty, left, DeviceStringDictionary(empty), DeviceStringDictionary(left), "left empty")


def test_a_self_join_passes_one_object_twice(device):
    _, right = five_runs()
    dev = DeviceStringDictionary(right)
    assert_keys(right, right, dev, dev, "self join")
    got_left, got_right, n_distinct = string_dictionary_order_pair(dev, dev)
    assert all(np.array_equal(a, b) for a, b in zip(got_left, got_right)) and n_distinct == len({e for d in right for e in d})


# ---- the stand-in columns -------------------------------------------------------------------------------------------------------------------
def widened(segments, width):
    if width == "bits":
        return [storage.bit_pack_segment(s) for s in segments]
    return [HostSegment(s.encoding, s.data_type, s.size, width, s.data.astype(UINT[width]), aux=None, aux_size=s.aux_size) for s in segments]


def export(column, dtype):
    import torch
    lib = abi.load_library()
    values = torch.full((max(1, column.rows),), -7, dtype=torch.int64 if dtype == np.int64 else torch.int32, device="cuda")
    nulls = torch.full((max(1, column.rows),), 9, dtype=torch.uint8, device="cuda")
    abi.check(lib.hy_column_export(column.handle, values.data_ptr(), nulls.data_ptr()))
    abi.check(lib.hy_synchronize())
    return values.cpu().numpy()[:column.rows], nulls.cpu().numpy()[:column.rows].astype(bool)


def key_of_string(left_dicts, right_dicts, kind):
    if kind == abi.STRING_KEYS_RANKS:
        left_keys, right_keys, _ = oracle.joint_order(left_dicts, right_dicts)
    else:
        left_keys, right_keys = oracle.join_ids(left_dicts, right_dicts)
    return {e: k for d, keys in zip(left_dicts + right_dicts, left_keys + right_keys) for e, k in zip(d, keys)}


@pytest.mark.parametrize("kind", [abi.STRING_KEYS_RANKS, abi.STRING_KEYS_HASH_IDS], ids=["ranks", "ids"])
@pytest.mark.parametrize("width", [1, 2, 4, "bits"], ids=lambda w: f"width_{w}")
def test_stand_ins_of_a_data_and_a_reference_column(device, kind, width):
    """Left: a data column of the given attribute vector width.  Right: a reference column behind a LIKE scan's PosLists over a data column
    of that width.  Row for row the stand-ins hold the oracle's key of the row's string, NULL where the row is NULL."""
    dtype = np.int64 if kind == abi.STRING_KEYS_HASH_IDS else np.int32
    left_strings, left_nulls, left_segments, left_dicts = words_table(3, 400, 90, 128)
    right_strings, right_nulls, right_segments, right_dicts = words_table(4, 600, 120, 150)
    left_host, right_host = HostColumn(widened(left_segments, width), abi.TYPE_STRING), HostColumn(widened(right_segments, width), abi.TYPE_STRING)
    left_dev, right_dev = DeviceColumn(left_host), DeviceColumn(right_host)
    left_dict, right_dict = DeviceStringDictionary(left_dicts), DeviceStringDictionary(right_dicts)
    scan = table_scan_like(right_dev, right_dict, b"w1%", abi.PRED_LIKE, nullable=True, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    pos_lists = [scan.pos_list(c).copy() for c in range(right_dev.n_chunks)]
    kept = np.concatenate([p[:, 0].astype(np.int64) * 150 + p[:, 1] for p in pos_lists])
    assert 50 < len(kept) < 600
    reference = DeviceColumn(storage.make_reference_column(right_host, pos_lists, list(range(right_dev.n_chunks))), refs={id(right_host): right_dev})
    key = key_of_string(left_dicts, right_dicts, kind)
    left_in, right_in = column_string_join_keys(left_dev, left_dict, reference, right_dict, kind)
    left_dict.close()   # (the dictionaries may die as soon as the call has returned)
    right_dict.close()
    assert (left_in.rows, left_in.n_chunks, right_in.rows, right_in.n_chunks) == (400, left_dev.n_chunks, len(kept), reference.n_chunks)
    values, nulls = export(left_in, dtype)
    assert np.array_equal(nulls, left_nulls) and values[~nulls].tolist() == [key[s] for s, n in zip(left_strings, left_nulls) if not n]
    values, nulls = export(right_in, dtype)
    assert not nulls.any() and values.tolist() == [key[right_strings[i]] for i in kept]
    # and the other way round: the reference column on the left, the data column on the right
    left_in.close()
    right_in.close()
    right_dict, left_dict = DeviceStringDictionary(right_dicts), DeviceStringDictionary(left_dicts)
    left_in, right_in = column_string_join_keys(reference, right_dict, left_dev, left_dict, kind)
    values, nulls = export(left_in, dtype)
    assert not nulls.any() and values.tolist() == [key[right_strings[i]] for i in kept]
    values, nulls = export(right_in, dtype)
    assert np.array_equal(nulls, left_nulls) and values[~nulls].tolist() == [key[s] for s, n in zip(left_strings, left_nulls) if not n]


def test_stand_in_refusals_leave_both_outputs_null(device):
    lib = abi.load_library()
    _, _, segments, dicts = words_table(5, 300, 40, 128)
    column = DeviceColumn(HostColumn(segments, abi.TYPE_STRING))
    good = DeviceStringDictionary(dicts)
    ints = DeviceColumn(storage.make_column(np.arange(9, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    int_dict = DeviceStringDictionary([[b"a", b"b", b"c"]] * 3)

    def status_of(left, left_dict, right, right_dict, kind=abi.STRING_KEYS_HASH_IDS):
        a, b = C.c_void_p(1), C.c_void_p(1)
        status = lib.hy_column_string_join_keys(left.handle, left_dict.handle, right.handle, right_dict.handle, kind, C.byref(a), C.byref(b))
        assert status != abi.OK and not a.value and not b.value
        return status

    short = DeviceStringDictionary(dicts[:2])
    longer = DeviceStringDictionary([dicts[0] + [b"~~~~"]] + dicts[1:])
    for bad in (short, longer):
        assert status_of(column, bad, column, good) == abi.ERR_INVALID
        assert status_of(column, good, column, bad) == abi.ERR_INVALID
    assert status_of(ints, int_dict, column, good) == abi.ERR_INVALID and b"string column" in lib.hy_last_error()
    assert status_of(column, good, ints, int_dict) == abi.ERR_INVALID and b"string column" in lib.hy_last_error()
    assert status_of(column, good, column, good, kind=2) == abi.ERR_INVALID


# ---- the joins over the stand-ins -----------------------------------------------------------------------------------------------------------
class JoinCase:
    """400 x 600 rows over about a hundred words: duplicates and NULL keys on both sides, shared and one-sided words."""

    def __init__(self):
        self.left_strings, self.left_nulls, self.left_segments, self.left_dicts = words_table(6, 400, 90, 128)
        self.right_strings, self.right_nulls, self.right_segments, self.right_dicts = words_table(7, 600, 120, 150)
        self.left_dev = DeviceColumn(HostColumn(self.left_segments, abi.TYPE_STRING))
        self.right_dev = DeviceColumn(HostColumn(self.right_segments, abi.TYPE_STRING))
        self.left_dict, self.right_dict = DeviceStringDictionary(self.left_dicts), DeviceStringDictionary(self.right_dicts)

    def stand_ins(self, kind):
        return column_string_join_keys(self.left_dev, self.left_dict, self.right_dev, self.right_dict, kind)


@pytest.fixture(scope="module")
def join_case(device):
    return JoinCase()


@pytest.mark.parametrize("radix_bits", [0, 3])
@pytest.mark.parametrize("mode", [abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_FALSE])
def test_join_hash_over_the_hash_ids(join_case, mode, radix_bits):
    """Pairs, order and slice offsets: the join over ids made in HBM, the join over StringJoinKeys' ids, the oracle's join over the oracle's ids."""
    case = join_case
    left_in, right_in = case.stand_ins(abi.STRING_KEYS_HASH_IDS)
    got = join_hash(left_in, right_in, mode, radix_bits)
    registry = StringJoinKeys()
    left_host, right_host = registry.column(case.left_segments, case.left_dicts), registry.column(case.right_segments, case.right_dicts)
    assert_join_equal(got, join_hash(DeviceColumn(left_host), DeviceColumn(right_host), mode, radix_bits), mode, "against the device join over registry ids")
    assert_join_equal(got, oracle_join(left_host, right_host, mode, radix_bits), mode, "against the oracle over registry ids")
    left_ids, right_ids = oracle.join_ids(case.left_dicts, case.right_dicts)
    assert_join_equal(got, oracle_join(key_column(case.left_segments, left_ids), key_column(case.right_segments, right_ids), mode, radix_bits), mode, "against the oracle over oracle ids")
    # ... and the strings themselves
    n = got.n_pairs
    left_rows = got.left[:n, 0].astype(np.int64) * 128 + got.left[:n, 1]
    right_present = [s if not null else None for s, null in zip(case.right_strings, case.right_nulls)]
    partners = Counter(s for s in right_present if s is not None)
    if mode in (abi.JOIN_INNER, abi.JOIN_LEFT):
        want = Counter()
        for i, (s, null) in enumerate(zip(case.left_strings, case.left_nulls)):
            matches = 0 if null else partners[s]
            if matches or mode == abi.JOIN_LEFT:
                want[(i, s if matches else None)] += max(matches, 1)
        right_rows = got.right[:n, 0].astype(np.int64) * 150 + got.right[:n, 1]
        seen = Counter((int(l), None if got.right[k, 0] == NULL_ROW else case.right_strings[int(r)]) for k, (l, r) in enumerate(zip(left_rows, right_rows)))
        assert seen == want and n > 400
    else:
        keep = (lambda s, null: not null and partners[s] > 0) if mode == abi.JOIN_SEMI else (lambda s, null: null or partners[s] == 0)
        assert sorted(left_rows.tolist()) == [i for i, (s, null) in enumerate(zip(case.left_strings, case.left_nulls)) if keep(s, null)]


CONDITIONS = {abi.PRED_EQUALS: lambda a, b: a == b, abi.PRED_LESS_THAN: lambda a, b: a < b, abi.PRED_GREATER_THAN_EQUALS: lambda a, b: a >= b,
              abi.PRED_NOT_EQUALS: lambda a, b: a != b}


@pytest.mark.parametrize("mode,condition", [(abi.JOIN_INNER, c) for c in CONDITIONS] + [(abi.JOIN_FULL_OUTER, abi.PRED_EQUALS)])
def test_join_sort_merge_over_the_ranks(join_case, mode, condition):
    """The operator's contract is the multiset of pairs: a nested loop over the strings, NULL keys matching nothing."""
    case = join_case
    left_in, right_in = case.stand_ins(abi.STRING_KEYS_RANKS)
    pairs = join_sort_merge(left_in, right_in, mode, condition)
    left, right = pairs.numpy()
    pairs.close()
    holds = CONDITIONS[condition]
    left_present = [(i, s) for i, (s, null) in enumerate(zip(case.left_strings, case.left_nulls)) if not null]
    right_present = [(j, s) for j, (s, null) in enumerate(zip(case.right_strings, case.right_nulls)) if not null]
    want = Counter((i, j) for i, a in left_present for j, b in right_present if holds(a, b))
    if mode == abi.JOIN_FULL_OUTER:
        matched_left, matched_right = {i for i, _ in want}, {j for _, j in want}
        want.update((i, -1) for i in range(400) if i not in matched_left)
        want.update((-1, j) for j in range(600) if j not in matched_right)
    row = lambda pos, chunk: np.where(pos[:, 0] == NULL_ROW, -1, pos[:, 0].astype(np.int64) * chunk + pos[:, 1])
    assert Counter(zip(row(left, 128).tolist(), row(right, 150).tolist())) == want and len(left) > 400

"""hy_table_scan_in_list on the device: `column IN (list)` / `column NOT IN (list)` over every segment layout, against the union of the
oracle's Equals scans (tests/in_list_oracle.py), cross-checked by a numpy brute force.  Every case asserts byte equality of the PosLists.

Chunk rows sit at the kernel's boundaries -- the eight-row group (1, 7, 8, 9), a wave (63, 64, 65), the FrameOfReference block and a
slice's quarter (2047, 2048, 2049) -- as the chunks of ONE column, so one scan meets them all."""
import ctypes as C
import glob
import os
import zlib

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import HostScanResult, in_list_predicate, make_predicate, string_in_list_predicate, table_scan, table_scan_in_list
from hyrise_amd.storage import DeviceColumn

from in_list_oracle import assert_in_list_result, brute_force_in, expected_matches, union_of_equals
from placed_columns import PlacedColumn
from support import GOLDEN, DeviceArray, assert_scan_equal, result_rows

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049)
N = sum(SIZES)
LIST_SIZES = (1, 2, 4, 19, 20, 255, 256)
TYPES = [np.int32, np.int64, np.float32, np.float64]
KINDS = ["value", "dictionary1", "dictionary2", "dictionary4", "bit_packed3", "bit_packed17", "frame_of_reference", "run_length"]
DOMAIN = {"value": 300, "dictionary1": 200, "dictionary2": 300, "dictionary4": 300, "bit_packed3": 6, "bit_packed17": 300, "frame_of_reference": 300, "run_length": 40}


def to_type(integers, dtype):
    """Integers -> the column's values: quarters for floating types (exact in float32), with -0.0 for 0 in the odd positions."""
    if np.dtype(dtype).kind != "f":
        return np.asarray(integers).astype(dtype)
    out = (np.asarray(integers) * 0.25).astype(dtype)
    zero = np.flatnonzero(out == 0)
    out[zero[1::2]] = -0.0
    return out


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    if kind == "frame_of_reference":
        assert values.dtype == np.int32, "FrameOfReference holds int32 only"
        return storage.encode_segment(values, nulls, abi.ENC_FRAME_OF_REFERENCE)
    if kind == "value":
        return storage.encode_segment(values, nulls, abi.ENC_UNENCODED)
    segment = storage.encode_segment(values, nulls, abi.ENC_DICTIONARY)
    if kind == "bit_packed3":
        packed = storage.bit_pack_segment(segment)
        assert packed.bits <= 3
        return storage.HostSegment(segment.encoding, segment.data_type, segment.size, 0, storage.pack_bits(segment.data, 3), aux=segment.aux, aux_size=segment.aux_size, bits=3)
    if kind == "bit_packed17":   # (wider than the ids need: a valid BitPackingVector all the same)
        return storage.HostSegment(segment.encoding, segment.data_type, segment.size, 0, storage.pack_bits(segment.data, 17), aux=segment.aux, aux_size=segment.aux_size, bits=17)
    want = int(kind[-1])
    if segment.width < want:
        segment = storage.HostSegment(segment.encoding, segment.data_type, segment.size, want, segment.data.astype({2: np.uint16, 4: np.uint32}[want]), aux=segment.aux,
                                      aux_size=segment.aux_size)
    return segment


def column_of(values, nulls, kind, sizes=SIZES, nullable=False):
    segments, begin = [], 0
    for size in sizes:
        chunk_nulls = nulls[begin:begin + size] if nulls is not None else (np.zeros(size, dtype=bool) if nullable and kind == "value" else None)
        segments.append(segment_of(values[begin:begin + size], chunk_nulls, kind))
        begin += size
    return storage.HostColumn(segments, storage.TYPE_OF_NP[np.dtype(values.dtype)])


def make_values(rng, kind, dtype, n=N):
    domain = DOMAIN[kind]
    base = np.repeat(rng.integers(0, domain, n // 5 + 1), 5)[:n] if kind == "run_length" else rng.integers(0, domain, n)
    return to_type(base - domain // 2, dtype)


def make_list(rng, kind, dtype, k):
    """k elements, unsorted: below, inside and above the column's range, with duplicates from four elements on."""
    domain = DOMAIN[kind]
    low, high = -(domain // 2), domain - domain // 2
    pool = np.concatenate([rng.integers(low, high, max(1, k)), rng.integers(low - 500, low, max(1, k // 3)), rng.integers(high, high + 500, max(1, k // 3))])
    picked = rng.permutation(pool)[:k]
    if k >= 4:
        picked[-1] = picked[0]
    elements = to_type(picked, dtype)
    return [v.item() for v in elements]


def run_matrix(host, dev, values, nulls, lists, nullable, context, chunk_starts):
    cache = {}
    for elements in lists:
        for negated in (False, True):
            per_chunk = union_of_equals(host, elements, negated=negated, nullable=nullable, equals_cache=cache)
            mask = brute_force_in(values, nulls, elements, negated)
            rows = np.concatenate([chunk_starts[c] + p.astype(np.int64) for c, p in enumerate(per_chunk)])
            np.testing.assert_array_equal(rows, np.flatnonzero(mask), err_msg=f"oracle union against brute force {context}")
            for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH):
                got = table_scan_in_list(dev, elements, negated=negated, nullable=nullable, flags=flags)
                assert_in_list_result(got, per_chunk, f"{context} k {len(elements)} negated {negated} flags {flags}")


# (FrameOfReference holds int32 only, encoding_supports_data_type(): no case pretends otherwise)
CASES = [(dtype, kind) for dtype in TYPES for kind in KINDS if kind != "frame_of_reference" or dtype == np.int32]


@pytest.mark.parametrize("nullable", [False, True], ids=["not_null", "nullable"])
@pytest.mark.parametrize("dtype,kind", CASES, ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_every_encoding_and_list_size(device, dtype, kind, nullable):
    rng = np.random.default_rng(zlib.crc32(f"{np.dtype(dtype).name} {kind} {nullable}".encode()))
    values = make_values(rng, kind, dtype)
    nulls = (rng.random(N) < 0.15) if nullable else None
    if nullable and kind == "run_length":
        nulls = np.repeat(rng.random(N // 5 + 1) < 0.15, 5)[:N]
    host = column_of(values, nulls, kind, nullable=nullable)
    dev = DeviceColumn(host)
    starts = np.concatenate([[0], np.cumsum(SIZES)])
    run_matrix(host, dev, values, nulls, [make_list(rng, kind, dtype, k) for k in LIST_SIZES], nullable, f"{np.dtype(dtype).name} {kind}", starts)


def test_nan_rows_and_signed_zero(device):
    """Unencoded and RunLength floating-point segments may hold NaN: never IN, always NOT IN; -0.0 and 0.0 are one element."""
    for dtype in (np.float32, np.float64):
        rng = np.random.default_rng(5)
        values = to_type(rng.integers(-8, 8, N), dtype)
        values[rng.random(N) < 0.2] = np.nan
        nulls = rng.random(N) < 0.1
        for kind in ("value", "run_length"):
            host = column_of(values, nulls, kind, nullable=True)
            dev = DeviceColumn(host)
            starts = np.concatenate([[0], np.cumsum(SIZES)])
            run_matrix(host, dev, values, nulls, [[0.0], [-0.0, 1.25], [0.5, -0.0, 100.0, 0.5, -2.0]], True, f"NaN rows {np.dtype(dtype).name} {kind}", starts)


def test_dictionaries_that_differ_between_chunks(device):
    """An element that is present in the first chunk, absent in the second and the only value of the third; chunk states: a dictionary
    chunk without any element is NONE_MATCH under IN, nothing is ever ALL_MATCH."""
    chunks = [np.array([5, 9, 5, 3, 9, 9, 5, 1, 5] * 3, dtype=np.int32), np.array([1, 3, 9, 9, 3, 1, 1] * 5, dtype=np.int32), np.full(70, 5, dtype=np.int32)]
    values = np.concatenate(chunks)
    sizes = [len(c) for c in chunks]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for nullable in (False, True):
        nulls = (np.arange(len(values)) % 11 == 3) if nullable else None
        for kind in ("dictionary1", "dictionary4", "bit_packed3"):
            host = column_of(values, nulls, kind, sizes=sizes, nullable=nullable)
            dev = DeviceColumn(host)
            run_matrix(host, dev, values, nulls, [[5], [5, 7], [7, 8, 2, 2], [5, 1, 3, 9]], nullable, f"three dictionaries {kind}", starts)
            got = table_scan_in_list(dev, [5, 7], nullable=nullable)
            assert got.chunk_state[:3].tolist() == [abi.CHUNK_SCANNED, abi.CHUNK_NONE_MATCH, abi.CHUNK_SCANNED]
            assert got.counts[2] == 70 - (0 if nulls is None else int(nulls[starts[2]:].sum()))
            got = table_scan_in_list(dev, [5, 7], negated=True, nullable=nullable)
            assert got.chunk_state[:3].tolist() == [abi.CHUNK_SCANNED] * 3 and got.counts[2] == 0


def test_refusals_write_nothing(device):
    lib = device
    values = np.arange(100, dtype=np.int32)
    dev = DeviceColumn(storage.make_column(values, None, abi.ENC_DICTIONARY))
    floats = DeviceColumn(storage.make_column(values.astype(np.float32)))

    def status_of(column, predicate):
        result = HostScanResult(column.n_chunks, column.rows)
        result.matches[:] = 0xAB
        result.counts[:] = 0xCD
        status = lib.hy_table_scan_in_list(column.handle, C.byref(predicate), None, 0, C.byref(result.c))
        assert np.all(result.matches == 0xAB) and np.all(result.counts == 0xCD), "a refused call wrote to the result"
        return status

    assert status_of(dev, in_list_predicate(abi.TYPE_INT, list(range(257)))) == abi.ERR_UNSUPPORTED
    assert status_of(dev, in_list_predicate(abi.TYPE_INT, [])) == abi.ERR_INVALID
    assert status_of(dev, in_list_predicate(abi.TYPE_LONG, [1, 2])) == abi.ERR_INVALID
    assert status_of(floats, in_list_predicate(abi.TYPE_FLOAT, [1.0, float("nan")])) == abi.ERR_INVALID
    assert status_of(floats, in_list_predicate(abi.TYPE_INT, [1])) == abi.ERR_INVALID
    assert lib.hy_table_scan_in_list(dev.handle, None, None, 0, None) == abi.ERR_INVALID
    # hy_table_scan itself still refuses the conditions, as before
    result = HostScanResult(dev.n_chunks, dev.rows)
    p = make_predicate(abi.PRED_IN, abi.TYPE_INT, 1)
    assert lib.hy_table_scan(dev.handle, C.byref(p), None, 0, C.byref(result.c)) == abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["value", "dictionary2", "frame_of_reference", "run_length"])
def test_one_element_is_equals_and_not_equals(device, kind):
    """IN (v) selects the rows of `= v` and NOT IN (v) those of `<> v`, PosLists byte for byte under the same flags (hy_table_scan may call a
    chunk ALL_MATCH and elide its RowIDs without HY_SCAN_MATERIALIZE_ALL_MATCH; the list scan never does: those rows are compared expanded)."""
    rng = np.random.default_rng(11)
    for dtype in ([np.int32] if kind == "frame_of_reference" else TYPES):
        values = make_values(rng, kind, dtype)
        values[SIZES[0] + SIZES[1]:SIZES[0] + SIZES[1] + SIZES[2]] = values[0]   # a chunk with one value
        nulls = rng.random(N) < 0.1
        if kind == "run_length":
            nulls = np.repeat(rng.random(N // 5 + 1) < 0.1, 5)[:N]
        host = column_of(values, nulls, kind, nullable=True)
        dev = DeviceColumn(host)
        data_type = host.data_type
        for value in (values[0].item(), values[-1].item(), 10_000):
            for negated, condition in ((False, abi.PRED_EQUALS), (True, abi.PRED_NOT_EQUALS)):
                predicate = make_predicate(condition, data_type, value, nullable=True)
                want = table_scan(dev, predicate, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
                got = table_scan_in_list(dev, [value], negated=negated, nullable=True, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
                np.testing.assert_array_equal(got.counts, want.counts)
                np.testing.assert_array_equal(got.offsets, want.offsets)
                assert got.matches[:want.total].tobytes() == want.matches[:want.total].tobytes(), f"{kind} {value} negated {negated}"
                plain, plain_got = table_scan(dev, predicate), table_scan_in_list(dev, [value], negated=negated, nullable=True)
                np.testing.assert_array_equal(plain_got.counts, plain.counts)
                assert result_rows(plain_got) == result_rows(plain)
                if not np.any(plain.chunk_state[:plain.n_chunks] == abi.CHUNK_ALL_MATCH):   # nothing elided: the bytes are the same without the flag, too
                    np.testing.assert_array_equal(plain_got.offsets, plain.offsets)
                    assert plain_got.matches[:plain.total].tobytes() == plain.matches[:plain.total].tobytes(), f"{kind} {value} negated {negated} flags 0"


def test_string_dictionaries(device):
    """p_container IN (4 strings): elements resolved against every chunk's dictionary on the host, value ids tested on the device."""
    rng = np.random.default_rng(3)
    words = [b"SM CASE", b"SM BOX", b"SM PACK", b"SM PKG", b"MED BAG", b"LG BOX", b"JUMBO JAR", b"WRAP DRUM", b""]
    sizes = (65, 2049, 9, 64)
    picks = [rng.integers(0, len(words), sizes[0]), rng.integers(4, len(words), sizes[1]), np.zeros(sizes[2], dtype=np.int64), rng.integers(0, 3, sizes[3])]
    segments, dictionaries = [], []
    nulls_all = []
    for pick in picks:
        nulls = rng.random(len(pick)) < 0.1
        segment, dictionary = storage.encode_string_dictionary([words[i] for i in pick], nulls)
        segments.append(segment)
        dictionaries.append(dictionary)
        nulls_all.append(nulls)
    host = storage.HostColumn(segments, abi.TYPE_STRING)
    dev = DeviceColumn(host)
    flat = np.concatenate(picks)
    nulls = np.concatenate(nulls_all)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for elements in ([b"SM CASE", b"SM BOX", b"SM PACK", b"SM PKG"], [b"SM CASE"], [b"NO SUCH", b"", b"LG BOX", b"LG BOX"], [b"ZZZ"]):
        for negated in (False, True):
            per_chunk = union_of_equals(host, elements, negated=negated, nullable=True, dictionaries=dictionaries)
            hit = np.isin(flat, [words.index(e) for e in elements if e in words])
            mask = (~hit if negated else hit) & ~nulls
            rows = np.concatenate([starts[c] + p.astype(np.int64) for c, p in enumerate(per_chunk)])
            np.testing.assert_array_equal(rows, np.flatnonzero(mask))
            predicate = string_in_list_predicate(dictionaries, elements, negated=negated, nullable=True)
            for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH):
                got = table_scan_in_list(dev, None, predicate=predicate, flags=flags)
                assert_in_list_result(got, per_chunk, f"strings {elements} negated {negated}")
    no_ids = in_list_predicate(abi.TYPE_STRING, [b"SM BOX"])
    result = HostScanResult(dev.n_chunks, dev.rows)
    assert device.hy_table_scan_in_list(dev.handle, C.byref(no_ids), None, 0, C.byref(result.c)) == abi.ERR_INVALID


def device_in_list_pos_list(lib, host, dev, predicate, layout):
    """hy_table_scan_in_list into device memory (chunk regions, all-match materialised), then hy_poslist_translate."""
    rows, n_chunks = max(1, host.rows), host.n_chunks
    regions, offsets, counts = DeviceArray(lib, (rows, 2), np.uint32), DeviceArray(lib, (n_chunks + 1,), np.int64), DeviceArray(lib, (max(1, n_chunks),), np.int32)
    result = abi.ScanResult()
    result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH
    result.matches, result.capacity, result.offsets, result.counts = regions.pointer, rows, offsets.pointer, counts.pointer
    abi.check(lib.hy_table_scan_in_list(dev.handle, C.byref(predicate), None, 0, C.byref(result)))
    out = DeviceArray(lib, (rows, 2), np.uint32)
    written = C.c_uint64(0)
    abi.check(lib.hy_poslist_translate(dev.handle, C.byref(result), layout, out.pointer, rows, C.byref(written)))
    if layout == abi.POSLIST_CHUNK_REGIONS:
        begin, count, everything = offsets.numpy(), counts.numpy(), out.numpy()
        parts = [everything[int(begin[c]):int(begin[c]) + int(count[c])] for c in range(n_chunks)]
        assert sum(len(part) for part in parts) == written.value
        return np.concatenate(parts) if parts else everything[:0]
    return out.numpy()[:written.value]


def translated(host, per_chunk):
    """What TableScan::_on_execute assembles from the chunks' matches (table_scan.cpp:158-196)."""
    out = []
    for c, segment in enumerate(host.segments):
        offsets = per_chunk[c]
        if segment.encoding != abi.ENC_REFERENCE:
            out.append(np.stack([np.full(len(offsets), c, dtype=np.uint32), offsets], axis=1))
        elif segment.data is None:
            out.append(np.stack([np.full(len(offsets), segment.ref_chunk_id, dtype=np.uint32), offsets], axis=1))
        else:
            out.append(np.asarray(segment.data, dtype=np.uint32).reshape(-1, 2)[offsets])
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.uint32)


@pytest.mark.parametrize("kind", ["value", "dictionary2", "frame_of_reference", "run_length", "bit_packed3"])
def test_reference_columns_and_device_results(device, kind):
    """Single-chunk, entire-chunk and shuffled multi-chunk PosLists with NULL RowIDs over every layout (RunLength / bit-packed: their decoded
    twins), host results and HY_MEM_DEVICE results translated in both layouts."""
    rng = np.random.default_rng(17)
    dtype = np.int32
    sizes = (2049, 65, 9, 2048)
    n = sum(sizes)
    values = make_values(rng, kind, dtype, n)
    nulls = rng.random(n) < 0.1
    if kind == "run_length":
        nulls = np.repeat(rng.random(n // 5 + 1) < 0.1, 5)[:n]
    base = column_of(values, nulls, kind, sizes=sizes, nullable=True)
    base_dev = DeviceColumn(base)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    single = []
    for c, size in enumerate(sizes):
        keep = np.flatnonzero(rng.random(size) < 0.6)
        single.append(np.stack([np.full(len(keep), c), keep], axis=1).astype(np.uint32))
    single_host = storage.make_reference_column(base, single + [1], list(range(len(sizes))) + [1])
    many = []
    for size in (0, 1, 65, 2049):
        rows = rng.integers(0, n, size)
        chunk = np.searchsorted(starts, rows, side="right") - 1
        pos = np.stack([chunk, rows - starts[chunk]], axis=1).astype(np.uint32)
        pos[rng.random(size) < 0.05] = 0xFFFFFFFF
        many.append(pos)
    many_host = storage.make_reference_column(base, many, [None] * len(many))
    lists = [make_list(rng, kind, dtype, k) for k in (1, 4, 19, 256)]
    for name, host, dev in (("data", base, base_dev), ("single", single_host, DeviceColumn(single_host, refs={id(base): base_dev})),
                            ("many", many_host, DeviceColumn(many_host, refs={id(base): base_dev}))):
        cache = {}
        for elements in lists:
            for negated in (False, True):
                per_chunk = union_of_equals(host, elements, negated=negated, nullable=True, equals_cache=cache)
                got = table_scan_in_list(dev, elements, negated=negated, nullable=True, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
                assert_in_list_result(got, per_chunk, f"{kind} {name} k {len(elements)} negated {negated}")
                want = translated(host, per_chunk)
                predicate = in_list_predicate(abi.TYPE_INT, elements, negated=negated, nullable=True)
                for layout in (abi.POSLIST_DENSE, abi.POSLIST_CHUNK_REGIONS):
                    got_list = device_in_list_pos_list(device, host, dev, predicate, layout)
                    assert got_list.tobytes() == want.tobytes(), f"{kind} {name} k {len(elements)} negated {negated} layout {layout}"


def test_excluded_chunks_sorted_flag_and_caller_owned_memory(device):
    rng = np.random.default_rng(29)
    for dtype, kind in ((np.int32, "value"), (np.int32, "dictionary1"), (np.int64, "value"), (np.int32, "frame_of_reference"), (np.float64, "dictionary2")):
        values = make_values(rng, kind, dtype)
        nulls = rng.random(N) < 0.1
        host = column_of(values, nulls, kind, nullable=True)
        elements = make_list(rng, kind, dtype, 8)
        for negated in (False, True):
            per_chunk = union_of_equals(host, elements, negated=negated, nullable=True)
            # excluded chunks: no matches, NONE_MATCH
            excluded = [1, 7, 9]
            dev = DeviceColumn(host)
            got = table_scan_in_list(dev, elements, negated=negated, nullable=True, excluded_chunks=excluded)
            pruned = [p if c not in excluded else p[:0] for c, p in enumerate(per_chunk)]
            assert_in_list_result(got, pruned, f"excluded {kind}")
            assert all(got.chunk_state[c] == abi.CHUNK_NONE_MATCH for c in excluded)
            # caller-owned device memory at the minimum alignment of the header's rules: every buffer on its element size only
            placed = PlacedColumn(host, "natural", 0xFF)
            assert_in_list_result(table_scan_in_list(placed, elements, negated=negated, nullable=True), per_chunk, f"placed natural {kind}")
            placed.assert_untouched()
        # a chunk flagged as sorted (and sorted): no range shortcut is needed, the rows must simply be right
        order = np.argsort(values[-SIZES[-1]:], kind="stable")
        sorted_values = values.copy()
        sorted_values[-SIZES[-1]:] = values[-SIZES[-1]:][order]
        sorted_nulls = nulls.copy()
        sorted_nulls[-SIZES[-1]:] = False
        flagged = column_of(sorted_values, sorted_nulls, kind, nullable=True)
        flagged.segments[-1].sorted_by = abi.SORT_ASCENDING_NULLS_FIRST
        plain = column_of(sorted_values, sorted_nulls, kind, nullable=True)
        for negated in (False, True):
            per_chunk = union_of_equals(plain, elements, negated=negated, nullable=True)
            assert_in_list_result(table_scan_in_list(DeviceColumn(flagged), elements, negated=negated, nullable=True), per_chunk, f"sorted flag {kind}")


def test_lz4_segments(device):
    """LZ4 segments as Hyrise wrote them are decompressed on the device and scanned like their unencoded twins."""
    from hyrise_amd import binary
    root = os.path.join(os.path.dirname(GOLDEN), "bin")
    checked = 0
    for path in sorted(glob.glob(os.path.join(root, "**", "LZ4*.bin"), recursive=True)):
        table = binary.read_table(path, keep_lz4=True)
        for c, data_type in enumerate(table.types):
            column = table.columns[c]
            if data_type == abi.TYPE_STRING or table.chunk_count == 0 or not any(s.encoding == abi.ENC_LZ4 for s in column.segments) or checked >= 6:
                continue
            if not all(s.encoding == abi.ENC_LZ4 for s in column.segments):
                continue
            twins = []
            for chunk, segment in enumerate(column.segments):
                nulls = table.null_masks[c][chunk]
                twins.append(storage.encode_segment(np.where(nulls, 0, segment.decoded).astype(segment.decoded.dtype) if nulls is not None else segment.decoded, nulls, abi.ENC_UNENCODED))
            twin = storage.HostColumn(twins, data_type)
            present = np.concatenate([s.data for s in twins])
            if np.dtype(present.dtype).kind == "f":
                present = present[~np.isnan(present)]
            if len(present) == 0:
                continue
            elements = [v.item() for v in np.unique(present)[:3]] + [present[-1].item(), 123456]
            nullable = any(m is not None for m in table.null_masks[c])
            dev = DeviceColumn(column)
            for negated in (False, True):
                per_chunk = union_of_equals(twin, elements, negated=negated, nullable=nullable)
                assert_in_list_result(table_scan_in_list(dev, elements, negated=negated, nullable=nullable), per_chunk, f"{os.path.basename(path)} column {c}")
            checked += 1
    assert checked >= 2

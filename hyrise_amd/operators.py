"""Thin Python callers of the C ABI (tests / bench plumbing).  Every function here ends in a call into
libhyrise_amd.so; nothing is computed in Python."""
import ctypes as C

import numpy as np

from . import abi


def make_predicate(condition, data_type=abi.TYPE_INT, value=None, value2=None, nullable=False, per_chunk_lower=None,
                   per_chunk_upper=None, per_chunk_found=None, dictionary_matches=None):
    """dictionary_matches (LIKE family): per data chunk a bool array over the chunk's dictionary -- what
    ColumnLikeTableScanImpl::_find_matches_in_dictionary computes."""
    p = abi.Predicate()
    p.condition = condition
    p.value_type = data_type
    for field, v in (("value", value), ("value2", value2)):
        if v is None:
            continue
        u = getattr(p, field)
        if data_type == abi.TYPE_INT:
            u.i32 = int(v)
        elif data_type == abi.TYPE_LONG:
            u.i64 = int(v)
        elif data_type == abi.TYPE_FLOAT:
            u.f32 = float(v)
        elif data_type == abi.TYPE_DOUBLE:
            u.f64 = float(v)
    p.column_is_nullable = 1 if nullable else 0
    keep = []
    for name, arr, dt in (("per_chunk_lower", per_chunk_lower, np.uint32), ("per_chunk_upper", per_chunk_upper, np.uint32),
                          ("per_chunk_found", per_chunk_found, np.uint8)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype=dt)
            keep.append(arr)
            setattr(p, name, arr.ctypes.data)
    if dictionary_matches is not None:
        words, offsets = [], [0]
        for matches in dictionary_matches:
            bits = np.zeros(((len(matches) + 63) // 64) * 64, dtype=np.uint8)
            bits[:len(matches)] = np.asarray(matches, dtype=bool)
            words.append(np.packbits(bits, bitorder="little").view(np.uint64))
            offsets.append(offsets[-1] + len(words[-1]))
        flat = np.ascontiguousarray(np.concatenate(words) if words else np.zeros(0, dtype=np.uint64))
        if len(flat) == 0:
            flat = np.zeros(1, dtype=np.uint64)
        starts = np.array(offsets, dtype=np.uint64)
        keep += [flat, starts]
        p.match_words, p.match_word_offsets = flat.ctypes.data, starts.ctypes.data
    p._keepalive = keep
    return p


def string_predicate(condition, dictionaries, value, value2=None, nullable=False):
    """The predicate of `string_column <condition> 'literal'` over DictionarySegment<pmr_string> chunks: the literal(s) are
    resolved against every chunk's (byte-wise sorted) dictionary on the host -- lower_bound / upper_bound, as
    column_vs_value_table_scan_impl.cpp:211-226 and column_between_table_scan_impl.cpp:112-124 do per segment -- and the device
    compares value ids.  `dictionaries`: per chunk the sorted list of bytes."""
    import bisect

    def encoded(x):
        return x if isinstance(x, bytes) else str(x).encode("utf-8")

    first, second = encoded(value), (encoded(value2) if value2 is not None else None)
    between = abi.PRED_BETWEEN_INCLUSIVE <= condition <= abi.PRED_BETWEEN_EXCLUSIVE
    lower_inclusive = condition in (abi.PRED_BETWEEN_INCLUSIVE, abi.PRED_BETWEEN_UPPER_EXCLUSIVE)
    upper_inclusive = condition in (abi.PRED_BETWEEN_INCLUSIVE, abi.PRED_BETWEEN_LOWER_EXCLUSIVE)
    lower, upper, found = [], [], []
    for dictionary in dictionaries:
        def bound(position):
            return position if position < len(dictionary) else abi.INVALID_VALUE_ID
        if between:
            lower.append(bound(bisect.bisect_left(dictionary, first) if lower_inclusive else bisect.bisect_right(dictionary, first)))
            upper.append(bound(bisect.bisect_right(dictionary, second) if upper_inclusive else bisect.bisect_left(dictionary, second)))
            found.append(0)
        else:
            position = bisect.bisect_left(dictionary, first)
            lower.append(bound(position))
            upper.append(bound(bisect.bisect_right(dictionary, first)))
            found.append(1 if position < len(dictionary) and dictionary[position] == first else 0)
    return make_predicate(condition, abi.TYPE_STRING, nullable=nullable, per_chunk_lower=lower, per_chunk_upper=upper, per_chunk_found=found)


def _literal(data_type, value):
    v = abi.Value()
    C.memset(C.byref(v), 0, C.sizeof(v))
    if data_type == abi.TYPE_INT:
        v.i32 = int(value)
    elif data_type == abi.TYPE_LONG:
        v.i64 = int(value)
    elif data_type == abi.TYPE_FLOAT:
        v.f32 = float(value)
    elif data_type == abi.TYPE_DOUBLE:
        v.f64 = float(value)
    return v


def predicate_for_column(condition, column_type, literal_type, literal, literal2_type=None, literal2=None, nullable=False):
    """The predicate of `column <condition> literal [AND literal2]` as the scan takes it: hy_predicate_cast applies
    TableScan::create_impl's lossless predicate cast (table_scan.cpp:336-366, 406-448).  Returns None where the reference
    falls back to its ExpressionEvaluator scan (HY_ERR_UNSUPPORTED)."""
    lib = abi.load_library()
    out = abi.Predicate()
    first = _literal(literal_type, literal)
    second = _literal(literal2_type, literal2) if literal2 is not None else None
    status = lib.hy_predicate_cast(condition, column_type, literal_type, C.addressof(first), literal2_type if literal2 is not None else abi.TYPE_NULL,
                                   C.addressof(second) if second is not None else None, C.byref(out))
    if status == abi.ERR_UNSUPPORTED:
        return None
    abi.check(status)
    out.column_is_nullable = 1 if nullable else 0
    return out


def join_output_chunks(slice_offsets, n_slices):
    """Pair ranges of the output chunks JoinHash builds from a join result's PosLists (hy_join_output_chunks: write_output_chunks'
    1000 / 4000 merge, join_output_writing.cpp:245-296) -> numpy uint64 array of n_chunks + 1 offsets."""
    lib = abi.load_library()
    offsets = np.ascontiguousarray(slice_offsets[:n_slices + 1], dtype=np.uint64)
    out = np.zeros(n_slices + 1, dtype=np.uint64)
    n = C.c_uint32(0)
    abi.check(lib.hy_join_output_chunks(offsets.ctypes.data, n_slices, out.ctypes.data, C.byref(n)))
    return out[:n.value + 1]


class HostScanResult:
    """Scan result in host memory, numpy views."""

    def __init__(self, n_chunks, capacity, flags=0):
        self.matches = np.zeros((max(1, capacity), 2), dtype=np.uint32)
        self.offsets = np.zeros(n_chunks + 1, dtype=np.uint64)
        self.counts = np.zeros(max(1, n_chunks), dtype=np.uint32)
        self.chunk_state = np.zeros(max(1, n_chunks), dtype=np.uint8)
        self.n_chunks = n_chunks
        r = abi.ScanResult()
        r.mem = abi.MEM_HOST
        r.flags = flags
        r.matches = self.matches.ctypes.data
        r.capacity = capacity
        r.offsets = self.offsets.ctypes.data
        r.counts = self.counts.ctypes.data
        r.chunk_state = self.chunk_state.ctypes.data
        self.c = r

    def pos_list(self, chunk):
        return self.matches[int(self.offsets[chunk]):int(self.offsets[chunk + 1])]

    @property
    def total(self):
        return int(self.offsets[self.n_chunks])


def table_scan(column, predicate, excluded_chunks=None, flags=0, capacity=None):
    """hy_table_scan with a host-memory result."""
    lib = abi.load_library()
    result = HostScanResult(column.n_chunks, column.rows if capacity is None else capacity, flags)
    excluded = None
    n_excluded = 0
    if excluded_chunks is not None and len(excluded_chunks):
        excluded = np.ascontiguousarray(excluded_chunks, dtype=np.uint32)
        n_excluded = len(excluded)
    abi.check(lib.hy_table_scan(column.handle, C.byref(predicate), excluded.ctypes.data if excluded is not None else None,
                                n_excluded, C.byref(result.c)))
    return result


def _pattern_bytes(pattern):
    return pattern if isinstance(pattern, bytes) else str(pattern).encode("utf-8")


def like_match_words(dev_dict, pattern, condition=abi.PRED_LIKE):
    """hy_like_matches with a host result -> the bitmap words of all chunks, chunk c's from dev_dict.word_offsets[c]."""
    lib = abi.load_library()
    pattern = _pattern_bytes(pattern)
    total = int(dev_dict.word_offsets[dev_dict.n_chunks])
    words = np.zeros(max(1, total), dtype=np.uint64)
    abi.check(lib.hy_like_matches(dev_dict.handle, pattern, len(pattern), condition, abi.MEM_HOST, words.ctypes.data))
    return words[:total]


def like_matches(dev_dict, pattern, condition=abi.PRED_LIKE):
    """hy_like_matches over a storage.DeviceStringDictionary -> one bool array per chunk over that chunk's dictionary (what
    like.dictionary_matches computes on the host)."""
    words = like_match_words(dev_dict, pattern, condition)
    out = []
    for c in range(dev_dict.n_chunks):
        chunk_words = words[int(dev_dict.word_offsets[c]):int(dev_dict.word_offsets[c + 1])]
        out.append(np.unpackbits(chunk_words.view(np.uint8), bitorder="little")[:dev_dict.n_entries[c]].astype(bool))
    return out


def table_scan_like(dev_column, dev_dict, pattern, condition, nullable=False, flags=0, excluded=(), device=False):
    """hy_table_scan_like: `column <LIKE condition> pattern` with the dictionary bitmaps made on the device -> HostScanResult like table_scan,
    or with device=True the chunk-region result in device memory as table_scan_expression returns it."""
    lib = abi.load_library()
    pattern = _pattern_bytes(pattern)
    excluded_array = np.ascontiguousarray(excluded, dtype=np.uint32) if len(excluded) else None
    excluded_pointer, n_excluded = (excluded_array.ctypes.data, len(excluded_array)) if excluded_array is not None else (None, 0)
    n_chunks, rows = dev_column.n_chunks, dev_column.rows
    if not device:
        result = HostScanResult(n_chunks, rows, flags)
        abi.check(lib.hy_table_scan_like(dev_column.handle, dev_dict.handle, pattern, len(pattern), condition, 1 if nullable else 0, excluded_pointer, n_excluded,
                                         C.byref(result.c)))
        return result
    import torch
    matches = torch.zeros((max(1, rows) + 2, 2), dtype=torch.int32, device="cuda")   # (16 bytes of slack behind the last RowID)
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(max(1, n_chunks), dtype=torch.int32, device="cuda")
    chunk_state = torch.zeros(max(1, n_chunks), dtype=torch.uint8, device="cuda")
    r = abi.ScanResult()
    r.mem, r.flags = abi.MEM_DEVICE, flags | abi.SCAN_CHUNK_REGIONS
    r.matches, r.capacity = matches.data_ptr(), rows
    r.offsets, r.counts, r.chunk_state = offsets.data_ptr(), counts.data_ptr(), chunk_state.data_ptr()
    abi.check(lib.hy_table_scan_like(dev_column.handle, dev_dict.handle, pattern, len(pattern), condition, 1 if nullable else 0, excluded_pointer, n_excluded, C.byref(r)))
    return matches[:max(1, rows)], offsets, counts[:n_chunks], chunk_state[:n_chunks]


def in_list_predicate(data_type, values, negated=False, nullable=False, per_chunk_value_ids=None):
    """hy_in_list of `column [NOT] IN (values)`: `values` are non-NULL literals of exactly the column's type (in_list_cast makes them
    so).  per_chunk_value_ids: [n_data_chunks][n_values] for dictionaries that are not on the device (string_in_list_predicate)."""
    p = abi.InList()
    p.value_type, p.n_values = data_type, len(values)
    p.negated, p.column_is_nullable = (1 if negated else 0), (1 if nullable else 0)
    keep = []
    if data_type != abi.TYPE_STRING:
        array = (abi.Value * max(1, len(values)))()
        for i, v in enumerate(values):
            array[i] = _literal(data_type, v)
        keep.append(array)
        p.values = C.addressof(array)
    if per_chunk_value_ids is not None:
        ids = np.ascontiguousarray(per_chunk_value_ids, dtype=np.uint32)
        keep.append(ids)
        p.per_chunk_value_ids = ids.ctypes.data
    p._keepalive = keep
    return p


def string_in_list_predicate(dictionaries, values, negated=False, nullable=False):
    """`string_column [NOT] IN ('a', 'b', ...)` over DictionarySegment<pmr_string> chunks: every element is resolved against every
    chunk's (byte-wise sorted) dictionary on the host -- lower_bound plus an equality check, like string_predicate -- and the device
    tests value ids.  `dictionaries`: per data chunk the sorted list of bytes."""
    import bisect
    elements = [v if isinstance(v, bytes) else str(v).encode("utf-8") for v in values]
    ids = np.full((max(1, len(dictionaries)), max(1, len(elements))), abi.INVALID_VALUE_ID, dtype=np.uint32)
    for c, dictionary in enumerate(dictionaries):
        for i, element in enumerate(elements):
            position = bisect.bisect_left(dictionary, element)
            if position < len(dictionary) and dictionary[position] == element:
                ids[c, i] = position
    return in_list_predicate(abi.TYPE_STRING, elements, negated, nullable, per_chunk_value_ids=ids)


def in_list_cast(column_type, literals):
    """hy_in_list_cast: literals = [(HY_TYPE_*, value) | None for NULL, ...] -> (values of the column's type that can equal a row, in
    input order; whether the list held a NULL)."""
    lib = abi.load_library()
    n = len(literals)
    types = (C.c_uint32 * max(1, n))()
    values = (abi.Value * max(1, n))()
    for i, literal in enumerate(literals):
        if literal is None:
            types[i] = abi.TYPE_NULL
        else:
            types[i] = literal[0]
            if literal[0] != abi.TYPE_STRING:
                values[i] = _literal(literal[0], literal[1])
    out = (abi.Value * max(1, n))()
    n_out, has_null = C.c_uint32(0), C.c_uint32(0)
    abi.check(lib.hy_in_list_cast(column_type, C.addressof(types), C.addressof(values), n, C.addressof(out), C.byref(n_out), C.byref(has_null)))
    field = {abi.TYPE_INT: "i32", abi.TYPE_LONG: "i64", abi.TYPE_FLOAT: "f32", abi.TYPE_DOUBLE: "f64"}[column_type]
    return [getattr(out[i], field) for i in range(n_out.value)], bool(has_null.value)


def table_scan_in_list(column, values, negated=False, nullable=False, excluded_chunks=None, flags=0, capacity=None, predicate=None):
    """hy_table_scan_in_list with a host-memory result: `column [NOT] IN (values)`, or a ready hy_in_list as `predicate`."""
    lib = abi.load_library()
    if predicate is None:
        predicate = in_list_predicate(column.data_type, values, negated, nullable)
    result = HostScanResult(column.n_chunks, column.rows if capacity is None else capacity, flags)
    excluded, n_excluded = None, 0
    if excluded_chunks is not None and len(excluded_chunks):
        excluded = np.ascontiguousarray(excluded_chunks, dtype=np.uint32)
        n_excluded = len(excluded)
    abi.check(lib.hy_table_scan_in_list(column.handle, C.byref(predicate), excluded.ctypes.data if excluded is not None else None, n_excluded, C.byref(result.c)))
    return result


def table_scan_columns(left, right, condition, capacity=None):
    lib = abi.load_library()
    result = HostScanResult(left.n_chunks, left.rows if capacity is None else capacity)
    abi.check(lib.hy_table_scan_columns(left.handle, right.handle, condition, C.byref(result.c)))
    return result


def string_dictionary_ranks(left_dict, right_dict):
    """hy_string_dictionary_ranks with a host result over two storage.DeviceStringDictionary -> per chunk the int32 ranks of the left
    chunk's entries against the right chunk's: 2 * lower_bound, minus one where the right dictionary does not hold the entry."""
    lib = abi.load_library()
    total = sum(left_dict.n_entries)
    ranks = np.zeros(max(1, total), dtype=np.int32)
    abi.check(lib.hy_string_dictionary_ranks(left_dict.handle, right_dict.handle, abi.MEM_HOST, ranks.ctypes.data))
    bounds = np.concatenate([[0], np.cumsum(left_dict.n_entries, dtype=np.int64)]).astype(np.int64)
    return [ranks[int(bounds[c]):int(bounds[c + 1])] for c in range(left_dict.n_chunks)]


def string_dictionary_order(dev_dict):
    """hy_string_dictionary_order with a host result over one storage.DeviceStringDictionary -> (per chunk the int32 dense ranks of the
    chunk's entries among the distinct strings of ALL chunks in byte order, the number of distinct strings): what StringRanks computes on
    the host, made in HBM."""
    lib = abi.load_library()
    total = sum(dev_dict.n_entries)
    ranks = np.zeros(max(1, total), dtype=np.int32)
    n_distinct = C.c_uint32(0xFFFFFFFF)
    abi.check(lib.hy_string_dictionary_order(dev_dict.handle, abi.MEM_HOST, ranks.ctypes.data, C.byref(n_distinct)))
    bounds = np.concatenate([[0], np.cumsum(dev_dict.n_entries, dtype=np.int64)]).astype(np.int64)
    return [ranks[int(bounds[c]):int(bounds[c + 1])] for c in range(dev_dict.n_chunks)], int(n_distinct.value)


class StringRankColumn:
    """hy_column_string_ranks' int32 stand-in of a string column: usable wherever a DeviceColumn is (a sort key, hy_column_export, ...).  It
    reads the string column's attribute vectors and PosLists in place, so it keeps that column alive, and is destroyed before it."""

    def __init__(self, handle, parents):
        self.lib = abi.load_library()
        self.handle = handle
        self.parents = parents
        self.rows, self.n_chunks, self.data_type = parents[0].rows, parents[0].n_chunks, abi.TYPE_INT

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None
        self.parents = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def column_string_ranks(dev_column, dev_dict):
    """hy_column_string_ranks: a string DeviceColumn (data or reference column) and the DeviceStringDictionary of its data column -> the
    column of each row's rank among the column's distinct strings (StringRankColumn), ranks made and kept in HBM."""
    lib = abi.load_library()
    handle = C.c_void_p()
    abi.check(lib.hy_column_string_ranks(dev_column.handle, dev_dict.handle, C.byref(handle)))
    return StringRankColumn(handle, (dev_column, dev_dict))


def _split_by_chunk(values, dev_dict):
    bounds = np.concatenate([[0], np.cumsum(dev_dict.n_entries, dtype=np.int64)]).astype(np.int64)
    return [values[int(bounds[c]):int(bounds[c + 1])] for c in range(dev_dict.n_chunks)]


def string_dictionary_order_pair(left_dict, right_dict):
    """hy_string_dictionary_order_pair with a host result over two storage.DeviceStringDictionary -> (per chunk of the left dictionary the
    int32 dense ranks of its entries among the distinct strings of BOTH dictionaries, the same for the right one, the number of distinct
    strings): equal strings on either side have one rank."""
    lib = abi.load_library()
    left = np.zeros(max(1, sum(left_dict.n_entries)), dtype=np.int32)
    right = np.zeros(max(1, sum(right_dict.n_entries)), dtype=np.int32)
    n_distinct = C.c_uint32(0xFFFFFFFF)
    abi.check(lib.hy_string_dictionary_order_pair(left_dict.handle, right_dict.handle, abi.MEM_HOST, left.ctypes.data, right.ctypes.data, C.byref(n_distinct)))
    return _split_by_chunk(left, left_dict), _split_by_chunk(right, right_dict), int(n_distinct.value)


def string_dictionary_join_ids(left_dict, right_dict):
    """hy_string_dictionary_join_ids with a host result -> per chunk of either dictionary the int64 join ids of its entries:
    (joint rank + 1) << 20 | std::hash & 0xFFFFF, what join_keys.StringJoinKeys hands out on the host with another unique number on top."""
    lib = abi.load_library()
    left = np.zeros(max(1, sum(left_dict.n_entries)), dtype=np.int64)
    right = np.zeros(max(1, sum(right_dict.n_entries)), dtype=np.int64)
    abi.check(lib.hy_string_dictionary_join_ids(left_dict.handle, right_dict.handle, abi.MEM_HOST, left.ctypes.data, right.ctypes.data))
    return _split_by_chunk(left, left_dict), _split_by_chunk(right, right_dict)


def column_string_join_keys(left_column, left_dict, right_column, right_dict, kind):
    """hy_column_string_join_keys: two string DeviceColumns (data or reference columns, independently) and the DeviceStringDictionary of
    each one's data column -> their two stand-ins (StringRankColumn) over keys consistent across both: abi.STRING_KEYS_RANKS (int32, for
    join_sort_merge / join_nested_loop) or abi.STRING_KEYS_HASH_IDS (int64, for join_hash), made and kept in HBM."""
    lib = abi.load_library()
    left, right = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_column_string_join_keys(left_column.handle, left_dict.handle, right_column.handle, right_dict.handle, kind, C.byref(left), C.byref(right)))
    data_type = abi.TYPE_LONG if kind == abi.STRING_KEYS_HASH_IDS else abi.TYPE_INT
    stand_ins = StringRankColumn(left, (left_column, left_dict)), StringRankColumn(right, (right_column, right_dict))
    for stand_in in stand_ins:
        stand_in.data_type = data_type
    return stand_ins


class StringResultColumn:
    """A dictionary-encoded string column the library made in HBM (hy_string_column_gather / hy_string_ranks_gather) with the
    DeviceStringDictionary that belongs to it: usable wherever a string DeviceColumn and its dictionary are."""

    def __init__(self, handle, dict_handle):
        from .storage import DeviceStringDictionary
        self.lib = abi.load_library()
        self.handle = handle
        rows, chunks = C.c_uint64(0), C.c_uint32(0)
        abi.check(self.lib.hy_column_row_count(handle, C.byref(rows)))
        abi.check(self.lib.hy_column_chunk_count(handle, C.byref(chunks)))
        self.rows, self.n_chunks, self.data_type = int(rows.value), int(chunks.value), abi.TYPE_STRING
        self.dictionary = DeviceStringDictionary.adopt(dict_handle, self.n_chunks)

    def read_value_ids(self):
        """Per chunk the uint32 attribute vector, copied back."""
        out = []
        for chunk in range(self.n_chunks):
            ids = np.zeros(int(self.lib.hy_column_chunk_rows(self.handle, chunk)), dtype=np.uint32)
            abi.check(self.lib.hy_column_read_chunk(self.handle, chunk, ids.ctypes.data if len(ids) else np.zeros(1, np.uint32).ctypes.data, None))
            out.append(ids)
        return out

    def read(self):
        """The rows as Python bytes, None for NULL: every chunk's dictionary and attribute vector copied back."""
        rows = []
        for chunk, ids in enumerate(self.read_value_ids()):
            entries = self.dictionary.read_chunk(chunk)[0]
            rows += [entries[v] if v < len(entries) else None for v in ids.tolist()]
        return rows

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None
        if getattr(self, "dictionary", None):
            self.dictionary.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def string_column_gather(column, dictionary, positions, chunk_rows):
    """hy_string_column_gather: the rows of a string DeviceColumn (data or reference column; `dictionary`: the DeviceStringDictionary of its
    data column) at `positions` -- an (n, 2) uint32 array of RowIDs, uploaded, or (device pointer, n) -- as a StringResultColumn."""
    lib = abi.load_library()
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    if isinstance(positions, tuple):
        pointer, n = positions
        abi.check(lib.hy_string_column_gather(column.handle, dictionary.handle, pointer, n, chunk_rows, C.byref(handle), C.byref(dict_handle)))
        return StringResultColumn(handle, dict_handle)
    positions = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1, 2)
    n = len(positions)
    pointer = C.c_void_p()
    abi.check(lib.hy_device_malloc(C.byref(pointer), max(16, 8 * n)))
    try:
        if n:
            abi.check(lib.hy_memcpy_h2d(pointer, positions.ctypes.data, 8 * n))
        abi.check(lib.hy_string_column_gather(column.handle, dictionary.handle, pointer, n, chunk_rows, C.byref(handle), C.byref(dict_handle)))
    finally:
        lib.hy_device_free(pointer)
    return StringResultColumn(handle, dict_handle)


def string_ranks_gather(dictionary, ranks):
    """hy_string_ranks_gather: the strings that an int32 column of dense ranks over `dictionary` stands for (MIN / MAX over a stand-in of
    column_string_ranks) as a StringResultColumn with `ranks`' chunk layout."""
    lib = abi.load_library()
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_string_ranks_gather(dictionary.handle, ranks.handle, C.byref(handle), C.byref(dict_handle)))
    return StringResultColumn(handle, dict_handle)


def string_column_substr(column, dictionary, start, length):
    """hy_string_column_substr: SUBSTR(column, start, length) over a string DeviceColumn (data or reference column; `dictionary`: the
    DeviceStringDictionary of its data column) as a StringResultColumn with `column`'s chunk layout.  start / length: int32 literals."""
    lib = abi.load_library()
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_string_column_substr(column.handle, dictionary.handle, start, length, C.byref(handle), C.byref(dict_handle)))
    return StringResultColumn(handle, dict_handle)


def string_column_materialize(column, dictionary):
    """hy_string_column_materialize: the rows of a string DeviceColumn themselves (data or reference column; `dictionary`: the
    DeviceStringDictionary of its data column) as a StringResultColumn with `column`'s chunk layout -- what Projection makes of a forwarded
    string column of a reference table."""
    lib = abi.load_library()
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_string_column_materialize(column.handle, dictionary.handle, C.byref(handle), C.byref(dict_handle)))
    return StringResultColumn(handle, dict_handle)


def table_scan_columns_strings(left, left_dict, right, right_dict, condition, flags=0, device=False):
    """hy_table_scan_columns_strings: `left <condition> right` over two string columns of one table and their dictionaries (for reference
    columns: the referenced data columns') -> HostScanResult like table_scan_columns, or with device=True the chunk-region result in
    device memory as table_scan_like returns it."""
    lib = abi.load_library()
    n_chunks, rows = left.n_chunks, left.rows
    if not device:
        result = HostScanResult(n_chunks, rows, flags)
        abi.check(lib.hy_table_scan_columns_strings(left.handle, left_dict.handle, right.handle, right_dict.handle, condition, C.byref(result.c)))
        return result
    import torch
    matches = torch.zeros((max(1, rows) + 2, 2), dtype=torch.int32, device="cuda")   # (16 bytes of slack behind the last RowID)
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(max(1, n_chunks), dtype=torch.int32, device="cuda")
    chunk_state = torch.zeros(max(1, n_chunks), dtype=torch.uint8, device="cuda")
    r = abi.ScanResult()
    r.mem, r.flags = abi.MEM_DEVICE, flags | abi.SCAN_CHUNK_REGIONS
    r.matches, r.capacity = matches.data_ptr(), rows
    r.offsets, r.counts, r.chunk_state = offsets.data_ptr(), counts.data_ptr(), chunk_state.data_ptr()
    abi.check(lib.hy_table_scan_columns_strings(left.handle, left_dict.handle, right.handle, right_dict.handle, condition, C.byref(r)))
    return matches[:max(1, rows)], offsets, counts[:n_chunks], chunk_state[:n_chunks]


def validate(mvcc, our_tid, snapshot_commit_id, can_use_chunk_shortcut=True, flags=0):
    """Validate (MVCC visibility) over a DeviceColumn of MVCC segments or of reference segments into one."""
    lib = abi.load_library()
    result = HostScanResult(mvcc.n_chunks, mvcc.rows, flags)
    abi.check(lib.hy_validate(mvcc.handle, our_tid, snapshot_commit_id, 1 if can_use_chunk_shortcut else 0, C.byref(result.c)))
    return result


class ResultColumn:
    """A device-resident column produced by an operator (hy_projection_arithmetic): usable wherever a DeviceColumn is."""

    def __init__(self, handle):
        self.lib = abi.load_library()
        self.handle = handle
        rows, chunks = C.c_uint64(0), C.c_uint32(0)
        abi.check(self.lib.hy_column_row_count(handle, C.byref(rows)))
        abi.check(self.lib.hy_column_chunk_count(handle, C.byref(chunks)))
        self.rows, self.n_chunks = int(rows.value), int(chunks.value)
        self.data_type = int(self.lib.hy_column_data_type(handle))

    def read(self):
        """(values, null mask) of the whole column, copied back to the host."""
        from .storage import NP_TYPES
        values, nulls = [], []
        for chunk in range(self.n_chunks):
            rows = int(self.lib.hy_column_chunk_rows(self.handle, chunk))
            v = np.zeros(rows, dtype=NP_TYPES[self.data_type])
            words = np.zeros((rows + 63) // 64, dtype=np.uint64)
            abi.check(self.lib.hy_column_read_chunk(self.handle, chunk, v.ctypes.data, words.ctypes.data))
            values.append(v)
            nulls.append(np.unpackbits(words.view(np.uint8), bitorder="little")[:rows].astype(bool))
        if not values:
            return np.zeros(0, dtype=NP_TYPES[self.data_type]), np.zeros(0, dtype=bool)
        return np.concatenate(values), np.concatenate(nulls)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _operand(x):
    """DeviceColumn / ResultColumn, or a literal: (HY_TYPE_*, value) / None for a NULL literal."""
    o = abi.Operand()
    if hasattr(x, "handle"):
        o.column = x.handle
        return o
    o.column = None
    if x is None:
        o.literal_type = abi.TYPE_NULL
        return o
    o.literal_type, value = x
    if o.literal_type == abi.TYPE_INT:
        o.literal.i32 = int(value)
    elif o.literal_type == abi.TYPE_LONG:
        o.literal.i64 = int(value)
    elif o.literal_type == abi.TYPE_FLOAT:
        o.literal.f32 = float(value)
    else:
        o.literal.f64 = float(value)
    return o


def projection_arithmetic(op, left, right):
    """left <op> right (abi.ARITH_*), operands: columns or literals -> ResultColumn (stays on the device)."""
    lib = abi.load_library()
    handle = C.c_void_p()
    lo, ro = _operand(left), _operand(right)
    abi.check(lib.hy_projection_arithmetic(op, C.byref(lo), C.byref(ro), C.byref(handle)))
    return ResultColumn(handle)


class HostJoinResult:
    """Join result in host memory (numpy views): pairs[k] = (left RowID, right RowID), slice boundaries."""

    def __init__(self, capacity, slice_capacity, radix_bits=None):
        self.left = np.zeros((max(1, capacity), 2), dtype=np.uint32)
        self.right = np.zeros((max(1, capacity), 2), dtype=np.uint32)
        self.slice_offsets = np.zeros(slice_capacity + 2, dtype=np.uint64)
        r = abi.JoinResult()
        r.mem = abi.MEM_HOST
        r.radix_bits = 0xFFFFFFFF if radix_bits is None else radix_bits
        r.left_pos, r.right_pos = self.left.ctypes.data, self.right.ctypes.data
        r.capacity = capacity
        r.slice_offsets = self.slice_offsets.ctypes.data
        r.slice_capacity = slice_capacity
        self.c = r

    @property
    def n_pairs(self):
        return int(self.c.n_pairs)


def join_hash_count(left, right, mode):
    lib = abi.load_library()
    n = C.c_uint64(0)
    abi.check(lib.hy_join_hash_count(left.handle, right.handle, mode, C.byref(n)))
    return int(n.value)


def join_predicates(secondary):
    """[(left DeviceColumn, condition, right DeviceColumn), ...] -> (ctypes array or None, count)"""
    if not secondary:
        return None, 0
    array = (abi.JoinPredicate * len(secondary))()
    for i, (left_column, condition, right_column) in enumerate(secondary):
        array[i].left_column, array[i].right_column, array[i].condition = left_column.handle, right_column.handle, condition
    return array, len(secondary)


def join_hash(left, right, mode, radix_bits=None, secondary=None, capacity=None):
    """hy_join_hash (hy_join_hash_predicates with secondary predicates) with a host-memory result, in ONE call: the result is
    sized for one partner per row of the larger input (every key / foreign-key join fits); a join that multiplies rows answers
    HY_ERR_CAPACITY with what it needs (nothing written) and runs once more with exactly that -- never a counting call first."""
    lib = abi.load_library()
    predicates, n = join_predicates(secondary)
    capacity = max(1, left.rows, right.rows) if capacity is None else capacity
    slice_capacity = max(left.rows, right.rows) // 131070 + max(left.n_chunks, right.n_chunks) + 600
    for attempt in (0, 1):
        result = HostJoinResult(capacity, slice_capacity, radix_bits)
        status = lib.hy_join_hash_predicates(left.handle, right.handle, mode, predicates, n, C.byref(result.c)) if n else \
            lib.hy_join_hash(left.handle, right.handle, mode, C.byref(result.c))
        if status == abi.ERR_CAPACITY and attempt == 0 and (result.n_pairs > capacity or int(result.c.n_slices) > slice_capacity):
            capacity, slice_capacity = max(capacity, result.n_pairs), max(slice_capacity, int(result.c.n_slices))
            continue
        abi.check(status)
        return result


class HostAggregateResult:
    """Aggregate result in host memory.  values of aggregate a: .column(a) (None = NULL)."""
    _NP = {abi.TYPE_INT: np.int32, abi.TYPE_LONG: np.int64, abi.TYPE_FLOAT: np.float32, abi.TYPE_DOUBLE: np.float64}

    def __init__(self, n_aggregates, group_capacity):
        self.row_ids = np.zeros((max(1, group_capacity), 2), dtype=np.uint32)
        self.raw = [np.zeros(max(1, group_capacity), dtype=np.uint64) for _ in range(n_aggregates)]
        self.nulls = [np.zeros(max(1, group_capacity), dtype=np.uint8) for _ in range(n_aggregates)]
        self.columns = (abi.AggregateColumn * max(1, n_aggregates))()
        for a in range(n_aggregates):
            self.columns[a].values = self.raw[a].ctypes.data
            self.columns[a].is_null = self.nulls[a].ctypes.data
        r = abi.AggregateResult()
        r.mem = abi.MEM_HOST
        r.group_capacity = group_capacity
        r.group_row_ids = self.row_ids.ctypes.data
        r.columns = self.columns
        self.c = r

    @property
    def n_groups(self):
        return int(self.c.n_groups)

    def column(self, a):
        t = self._NP[self.columns[a].data_type]
        n = self.n_groups
        values = np.frombuffer(self.raw[a].tobytes(), dtype=t)[:n]
        return [None if self.nulls[a][i] else values[i].item() for i in range(n)]


def aggregate_hash(groupby_columns, aggregates, group_capacity=None, result=None):
    """aggregates: list of (HY_AGG_*, DeviceColumn or None for COUNT(*)).  result: a HostAggregateResult of an earlier call with the same
    aggregates and capacity, written again (a caller that runs the plan repeatedly keeps its buffers; fresh numpy arrays are first touched --
    one page fault per 4 KiB -- while the result is copied into them)."""
    lib = abi.load_library()
    garr = (C.c_void_p * max(1, len(groupby_columns)))(*[c.handle for c in groupby_columns])
    specs = (abi.AggregateSpec * max(1, len(aggregates)))()
    for i, (function, column) in enumerate(aggregates):
        specs[i].function = function
        specs[i].column = column.handle if column is not None else None
    shape = groupby_columns[0] if groupby_columns else next(c for _, c in aggregates if c is not None)
    if result is None:
        result = HostAggregateResult(len(aggregates), (shape.rows + 1) if group_capacity is None else group_capacity)
    abi.check(lib.hy_aggregate_hash(garr, len(groupby_columns), specs, len(aggregates), C.byref(result.c)))
    return result


class GroupRowIds:
    """The representative rows of hy_aggregate_hash_columns' groups: RowIDs in a block of the library's result-buffer pool (device memory),
    owned by this object.  (pointer, rows) is what column_gather and the positions arguments take; numpy() copies them back."""

    def __init__(self, pointer, rows):
        self.lib = abi.load_library()
        self.pointer, self.rows = pointer, int(rows)

    def numpy(self):
        out = np.zeros((self.rows, 2), dtype=np.uint32)
        if self.rows:
            abi.check(self.lib.hy_memcpy_d2h(out.ctypes.data, self.pointer, out.nbytes))
        return out

    def close(self):
        if getattr(self, "pointer", None):
            self.lib.hy_result_pool_release(self.pointer)
            self.pointer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AggregateColumnsResult:
    """hy_aggregate_hash_columns' output table in device memory: .aggregates[a] and .groupby[g] are ResultColumns (groupby[g] is None where
    the library made no column: a string column passed as key names), .row_ids the GroupRowIds."""

    def __init__(self, n_groups, groupby, aggregates, row_ids):
        self.n_groups, self.groupby, self.aggregates, self.row_ids = n_groups, groupby, aggregates, row_ids

    def column(self, a):
        """Aggregate a as a list (None = NULL), like HostAggregateResult.column."""
        values, nulls = self.aggregates[a].read()
        return [None if nulls[i] else values[i].item() for i in range(self.n_groups)]


def aggregate_hash_columns(groupby_columns, aggregates, chunk_rows=abi.CHUNK_DEFAULT_SIZE, key_name_columns=()):
    """hy_aggregate_hash_columns: hy_aggregate_hash's result as device-resident columns of chunk_rows-row chunks.  aggregates as for
    aggregate_hash; key_name_columns: indices of GROUP BY columns that hold stand-ins for strings (no output column is made for them: the
    caller reads the strings through the representative rows)."""
    lib = abi.load_library()
    garr = (C.c_void_p * max(1, len(groupby_columns)))(*[c.handle for c in groupby_columns])
    specs = (abi.AggregateSpec * max(1, len(aggregates)))()
    for i, (function, column) in enumerate(aggregates):
        specs[i].function = function
        specs[i].column = column.handle if column is not None else None
    out_aggregates = (C.c_void_p * max(1, len(aggregates)))()
    out_groupby = (C.c_void_p * max(1, len(groupby_columns)))()
    out = abi.AggregateColumns()
    out.skip_groupby_mask = sum(1 << g for g in key_name_columns)
    out.aggregate_columns, out.groupby_columns = out_aggregates, out_groupby
    abi.check(lib.hy_aggregate_hash_columns(garr, len(groupby_columns), specs, len(aggregates), chunk_rows, C.byref(out)))
    row_ids = GroupRowIds(out.group_row_ids, out.n_groups)
    return AggregateColumnsResult(int(out.n_groups), [ResultColumn(C.c_void_p(out_groupby[g])) if out_groupby[g] else None for g in range(len(groupby_columns))],
                                  [ResultColumn(C.c_void_p(out_aggregates[a])) for a in range(len(aggregates))], row_ids)


def star_join_aggregate(dimensions, groupby, aggregates, group_capacity=4096, result=None):
    """hy_star_join_aggregate: the star join fact x dimensions -> GROUP BY -> aggregates as one call (csrc/plan.hip).
    dimensions: [(key column, filter column or None, predicate or None, fact foreign-key column)]; groupby: [(table, column)] with table 0 =
    the fact table, d + 1 = dimension d; aggregates: [(function, (table, column) or None for COUNT(*), op or None, (table, column) or None)].
    -> (HostAggregateResult, rows of the join result)"""
    lib = abi.load_library()
    dims = (abi.StarDimension * len(dimensions))()
    for d, (key, filter_column, predicate, fact_key) in enumerate(dimensions):
        dims[d].key, dims[d].fact_key = key.handle, fact_key.handle
        dims[d].filter_column = filter_column.handle if filter_column is not None else None
        if predicate is not None:
            dims[d].predicate = predicate
    groups = (abi.StarColumn * max(1, len(groupby)))()
    for g, (table, column) in enumerate(groupby):
        groups[g].table, groups[g].column = table, column.handle
    specs = (abi.StarAggregate * max(1, len(aggregates)))()
    for a, (function, left, op, right) in enumerate(aggregates):
        specs[a].function, specs[a].op = function, abi.STAR_NO_OP if op is None else op
        if left is not None:
            specs[a].left.table, specs[a].left.column = left[0], left[1].handle
        if right is not None:
            specs[a].right.table, specs[a].right.column = right[0], right[1].handle
    if result is None:
        result = HostAggregateResult(len(aggregates), group_capacity)
    joined = C.c_uint64(0)
    abi.check(lib.hy_star_join_aggregate(dims, len(dimensions), groups, len(groupby), specs, len(aggregates), C.byref(result.c), C.byref(joined)))
    return result, int(joined.value)


def _star_filters(filters, keep):
    """[(column, predicate or hy_in_list)] -> an hy_star_filter array (an abi.InList is an IN list, anything else a predicate)."""
    array = (abi.StarFilter * max(1, len(filters)))()
    for k, (column, test) in enumerate(filters):
        array[k].column = column.handle
        if isinstance(test, abi.InList):
            array[k].in_list = C.pointer(test)
        else:
            array[k].predicate = test
        keep.append(test)
    keep.append(array)
    return array


def star_join_aggregate_where(dimensions, fact_filters, groupby, aggregates, group_capacity=4096, result=None):
    """hy_star_join_aggregate_where: star_join_aggregate over filtered tables, as one call (csrc/plan.hip).
    dimensions: [(key column, [(filter column, predicate or in_list_predicate(...)), ...], fact foreign-key column)] -- a dimension's filters are a
    conjunction, an empty list leaves it unfiltered; fact_filters: [(column of the fact table, predicate or in_list_predicate(...)), ...];
    groupby (may be empty: one result row) and aggregates as star_join_aggregate takes them.
    -> (HostAggregateResult, rows left after the fact filters and every join)"""
    lib = abi.load_library()
    keep = []
    dims = (abi.StarDimensionWhere * max(1, len(dimensions)))()
    for d, (key, filters, fact_key) in enumerate(dimensions):
        dims[d].key, dims[d].fact_key = key.handle, fact_key.handle
        dims[d].n_filters = len(filters)
        if filters:
            dims[d].filters = _star_filters(filters, keep)
    fact = _star_filters(fact_filters, keep)
    groups = (abi.StarColumn * max(1, len(groupby)))()
    for g, (table, column) in enumerate(groupby):
        groups[g].table, groups[g].column = table, column.handle
    specs = (abi.StarAggregate * max(1, len(aggregates)))()
    for a, (function, left, op, right) in enumerate(aggregates):
        specs[a].function, specs[a].op = function, abi.STAR_NO_OP if op is None else op
        if left is not None:
            specs[a].left.table, specs[a].left.column = left[0], left[1].handle
        if right is not None:
            specs[a].right.table, specs[a].right.column = right[0], right[1].handle
    if result is None:
        result = HostAggregateResult(len(aggregates), group_capacity)
    joined = C.c_uint64(0)
    abi.check(lib.hy_star_join_aggregate_where(dims, len(dimensions), fact, len(fact_filters), groups, len(groupby), specs, len(aggregates), C.byref(result.c), C.byref(joined)))
    return result, int(joined.value)


def expression(tree):
    """An arithmetic expression as hy_expression (postfix).  tree: a column (DeviceColumn), a literal (HY_TYPE_*, value), None (the
    NULL literal) or (abi.ARITH_*, left tree, right tree)."""
    e = abi.Expression()
    nodes = []

    def walk(t):
        n = abi.ExpressionNode()
        if hasattr(t, "handle"):
            n.kind, n.column = abi.EXPR_COLUMN, t.handle
        elif t is None or len(t) == 2:
            literal = _operand(t)
            n.kind, n.literal_type, n.literal = abi.EXPR_LITERAL, literal.literal_type, literal.literal
        else:
            op, left, right = t
            walk(left)
            walk(right)
            n.kind, n.op = abi.EXPR_ARITHMETIC, op
        nodes.append(n)

    walk(tree)
    if len(nodes) > abi.MAX_EXPRESSION_NODES:
        raise ValueError(f"an expression has at most {abi.MAX_EXPRESSION_NODES} nodes")
    e.n_nodes = len(nodes)
    for i, n in enumerate(nodes):
        e.nodes[i] = n
    return e


class ColumnTest:
    """`column <predicate>` as a node of a projection program: the column and what make_predicate / string_predicate / predicate_for_column
    (an abi.Predicate) or in_list_predicate / string_in_list_predicate (an abi.InList) produce."""

    def __init__(self, column, predicate):
        self.column, self.predicate = column, predicate


def projection_program(tree):
    """A whole expression tree as hy_projection_program (postfix).  tree: a column (DeviceColumn / ResultColumn), a literal (HY_TYPE_*, value),
    None (the NULL literal), a ColumnTest, or a nested tuple whose first element names the node:
      ("arith", abi.ARITH_*, left, right)   ("cmp", abi.PRED_*, left, right)   ("and", left, right)   ("or", left, right)
      ("is_null", x)   ("is_not_null", x)   ("neg", x)   ("case", when, then, otherwise)
    and, to be told HY_ERR_UNSUPPORTED by the library, ("between" | "cast" | "extract" | "function" | "subquery" | "parameter", operand...).
    -> (abi.ProjectionProgram, what it points to: keep it alive)"""
    program = abi.ProjectionProgram()
    nodes, columns, tests, keep = [], [], [], []
    named = {"and": abi.PROJ_AND, "or": abi.PROJ_OR, "is_null": abi.PROJ_IS_NULL, "is_not_null": abi.PROJ_IS_NOT_NULL, "neg": abi.PROJ_UNARY_MINUS, "case": abi.PROJ_CASE,
             "between": abi.PROJ_BETWEEN, "cast": abi.PROJ_CAST, "extract": abi.PROJ_EXTRACT, "function": abi.PROJ_FUNCTION, "subquery": abi.PROJ_SUBQUERY,
             "parameter": abi.PROJ_PARAMETER}

    def walk(t):
        n = abi.ProjectionNode()
        if hasattr(t, "handle"):
            if not any(t is c for c in columns):
                columns.append(t)
            n.kind, n.index = abi.PROJ_COLUMN, next(i for i, c in enumerate(columns) if c is t)
        elif isinstance(t, ColumnTest):
            if not any(t is known for known in tests):
                tests.append(t)
            n.kind, n.index = abi.PROJ_COLUMN_TEST, next(i for i, known in enumerate(tests) if known is t)
        elif t is None or not isinstance(t[0], str):
            literal = _operand(t)
            n.kind, n.literal_type, n.literal = abi.PROJ_LITERAL, literal.literal_type, literal.literal
        elif t[0] in ("arith", "cmp"):
            walk(t[2])
            walk(t[3])
            n.kind, n.op = (abi.PROJ_ARITHMETIC if t[0] == "arith" else abi.PROJ_COMPARISON), t[1]
        else:
            for operand in t[1:]:
                walk(operand)
            n.kind = named[t[0]]
        nodes.append(n)

    walk(tree)
    # over a limit: the true counts go to the library, which refuses them before it reads the arrays (only what fits is filled in)
    program.n_nodes, program.n_columns, program.n_tests = len(nodes), len(columns), len(tests)
    nodes, columns, tests = nodes[:abi.MAX_PROJECTION_NODES], columns[:abi.MAX_PROJECTION_COLUMNS], tests[:abi.MAX_PROJECTION_TESTS]
    for i, n in enumerate(nodes):
        program.nodes[i] = n
    for i, c in enumerate(columns):
        program.columns[i] = c.handle if not isinstance(c.handle, C.c_void_p) else c.handle.value
    for i, t in enumerate(tests):
        handle = t.column.handle
        program.tests[i].column = handle if not isinstance(handle, C.c_void_p) else handle.value
        if isinstance(t.predicate, abi.InList):
            program.tests[i].in_list = C.pointer(t.predicate)
        else:
            program.tests[i].predicate = t.predicate
        keep.append(t.predicate)
    return program, (keep, columns, tests)


def projection_expression(tree):
    """hy_projection_expression: the whole tree (projection_program) evaluated per row in one pass -> ResultColumn (stays on the device)."""
    lib = abi.load_library()
    program, keep = projection_program(tree)
    handle = C.c_void_p()
    abi.check(lib.hy_projection_expression(C.byref(program), C.byref(handle)))
    del keep
    return ResultColumn(handle)


BETWEEN_BOUNDS = {abi.PRED_BETWEEN_INCLUSIVE: (abi.PRED_GREATER_THAN_EQUALS, abi.PRED_LESS_THAN_EQUALS), abi.PRED_BETWEEN_LOWER_EXCLUSIVE: (abi.PRED_GREATER_THAN, abi.PRED_LESS_THAN_EQUALS),
                  abi.PRED_BETWEEN_UPPER_EXCLUSIVE: (abi.PRED_GREATER_THAN_EQUALS, abi.PRED_LESS_THAN), abi.PRED_BETWEEN_EXCLUSIVE: (abi.PRED_GREATER_THAN, abi.PRED_LESS_THAN)}


def lower_between(tree, on_spine=True):
    """A scan's predicate tree with every ("between", abi.PRED_BETWEEN_*, operand, lower, upper) replaced by `operand >= lower AND operand <=
    upper` (> / < for the exclusive conditions): rewrite_between_expression.  Only on the spine -- the root and the nodes all of whose ancestors
    are AND / OR -- where a row is dropped for FALSE and for NULL alike; anywhere else _evaluate_between_expression's FALSE for a NULL operand
    (expression_evaluator.cpp:590-656) could be told from the rewrite's NULL: ValueError."""
    if not isinstance(tree, tuple) or not tree or not isinstance(tree[0], str):
        return tree
    if tree[0] == "between" and len(tree) == 5:
        if not on_spine:
            raise ValueError("BETWEEN below the AND / OR spine of a scan's predicate is not lowered: its FALSE for a NULL operand would become NULL")
        lower_condition, upper_condition = BETWEEN_BOUNDS[tree[1]]
        operand, lower, upper = (lower_between(t, False) for t in tree[2:])
        return ("and", ("cmp", lower_condition, operand, lower), ("cmp", upper_condition, operand, upper))
    if tree[0] in ("and", "or"):
        return (tree[0],) + tuple(lower_between(t, on_spine) for t in tree[1:])
    first = 2 if tree[0] in ("arith", "cmp") else 1
    return tree[:first] + tuple(lower_between(t, False) for t in tree[first:])


def table_scan_expression(tree, excluded_chunks=None, flags=0, capacity=None, device=False):
    """hy_table_scan_expression: TableScan over a predicate expression -- the tuple trees of projection_program plus ("between", condition,
    operand, lower, upper) on the spine (lower_between) -- evaluated and compacted in one pass.  -> HostScanResult like table_scan, or with
    device=True the chunk-region result in device memory: (matches [rows, 2] int32, offsets [n_chunks + 1] int64, counts [n_chunks] int32,
    chunk_state [n_chunks] uint8) torch tensors, flags | HY_SCAN_CHUNK_REGIONS."""
    lib = abi.load_library()
    program, keep = projection_program(lower_between(tree))
    shape = (keep[1] + [t.column for t in keep[2]])
    n_chunks, rows = (shape[0].n_chunks, shape[0].rows) if shape else (0, 0)
    excluded, n_excluded = None, 0
    if excluded_chunks is not None and len(excluded_chunks):
        excluded = np.ascontiguousarray(excluded_chunks, dtype=np.uint32)
        n_excluded = len(excluded)
    excluded_pointer = excluded.ctypes.data if excluded is not None else None
    if not device:
        result = HostScanResult(n_chunks, rows if capacity is None else capacity, flags)
        abi.check(lib.hy_table_scan_expression(C.byref(program), excluded_pointer, n_excluded, C.byref(result.c)))
        del keep
        return result
    import torch
    capacity = rows if capacity is None else capacity
    matches = torch.zeros((max(1, capacity) + 2, 2), dtype=torch.int32, device="cuda")   # (16 bytes of slack behind the last RowID)
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(max(1, n_chunks), dtype=torch.int32, device="cuda")
    chunk_state = torch.zeros(max(1, n_chunks), dtype=torch.uint8, device="cuda")
    r = abi.ScanResult()
    r.mem, r.flags = abi.MEM_DEVICE, flags | abi.SCAN_CHUNK_REGIONS
    r.matches, r.capacity = matches.data_ptr(), capacity
    r.offsets, r.counts, r.chunk_state = offsets.data_ptr(), counts.data_ptr(), chunk_state.data_ptr()
    abi.check(lib.hy_table_scan_expression(C.byref(program), excluded_pointer, n_excluded, C.byref(r)))
    del keep
    return matches[:max(1, capacity)], offsets, counts[:n_chunks], chunk_state[:n_chunks]


PAIR_LIST_PERIOD = 2 << 20          # the two output PosLists of a join are written at the same pair index at the same time: when their
PAIR_LIST_OFFSET = 5 << 18          # addresses are congruent modulo 2 MiB the two streams meet in the same memory channels -- pk_emit takes
                                    # 306 - 315 us; 1.25 MiB apart (mod 2 MiB) 274 - 283 us (tools/join_placement.py, profiles/r03_join_placement.txt)


def pair_lists(torch, device, capacity):
    """Device buffers for a join's two output PosLists ([capacity, 2] int32 each), carved out of ONE allocation so that the second starts
    1.25 MiB past a 2 MiB boundary when the first starts on one (callers that hold torch tensors; the C++ adapter and bench.py take
    their lists from the library's pool, hy_result_pool_acquire_pair, which applies the same rule).
    -> (left, right, the allocation: keep it alive)"""
    list_bytes = 8 * max(1, int(capacity))
    arena = torch.empty(2 * list_bytes + 3 * PAIR_LIST_PERIOD, dtype=torch.uint8, device=device)
    first = -arena.data_ptr() % PAIR_LIST_PERIOD
    second = (first + list_bytes + PAIR_LIST_PERIOD - 1) // PAIR_LIST_PERIOD * PAIR_LIST_PERIOD + PAIR_LIST_OFFSET
    rows = max(1, int(capacity))
    left = arena[first:first + list_bytes].view(torch.int32).view(rows, 2)
    right = arena[second:second + list_bytes].view(torch.int32).view(rows, 2)
    return left, right, arena


def validate_filter(mvcc_column, our_tid, snapshot_commit_id, can_use_chunk_shortcut=True):
    """Validate as a filter of hy_scan_project_aggregate: (the table's MvccData as a DeviceColumn, its predicate)."""
    predicate = abi.Predicate()
    predicate.condition = abi.FILTER_VALIDATE
    predicate.value.value_id, predicate.value2.value_id = int(our_tid), int(snapshot_commit_id)
    predicate.column_is_nullable = 1 if can_use_chunk_shortcut else 0
    return mvcc_column, predicate


def scan_project_aggregate(filters, groupby_columns, aggregates, group_capacity=None):
    """hy_scan_project_aggregate: TableScan(s) -> Projection -> AggregateHash of one data table in one pass.
    filters: [(DeviceColumn, predicate)], ANDed in order; aggregates: [(HY_AGG_*, expression tree or None for COUNT(*))]."""
    lib = abi.load_library()
    farr = (abi.Filter * max(1, len(filters)))()
    for i, (column, predicate) in enumerate(filters):
        farr[i].column = column.handle
        farr[i].predicate = predicate          # (a copy of the struct; `filters` keeps the arrays it points to alive)
    garr = (C.c_void_p * max(1, len(groupby_columns)))(*[c.handle for c in groupby_columns])
    expressions = [expression(tree) if tree is not None or function != abi.AGG_COUNT else None for function, tree in aggregates]
    specs = (abi.FusedAggregate * max(1, len(aggregates)))()
    for i, (function, _) in enumerate(aggregates):
        specs[i].function = function
        if expressions[i] is not None:
            specs[i].input = C.pointer(expressions[i])

    def columns_of(tree):
        if hasattr(tree, "handle"):
            yield tree
        elif tree is not None and len(tree) == 3:
            yield from columns_of(tree[1])
            yield from columns_of(tree[2])

    table = [c for c, _ in filters] + list(groupby_columns) + [c for _, tree in aggregates for c in columns_of(tree)]
    if not table:
        raise ValueError("hy_scan_project_aggregate needs at least one column")
    result = HostAggregateResult(len(aggregates), (table[0].rows + 1) if group_capacity is None else group_capacity)
    abi.check(lib.hy_scan_project_aggregate(farr, len(filters), garr, len(groupby_columns), specs, len(aggregates), C.byref(result.c)))
    return result


class SortedPositions:
    """hy_sort's output: the input table's positions (chunk, offset) in sorted order, in a block of the library's result-buffer pool (device
    memory; the next operator reads it in place).  numpy() copies it back."""

    def __init__(self, rows):
        self.lib = abi.load_library()
        self.rows = int(rows)
        pointer = C.c_void_p()
        abi.check(self.lib.hy_result_pool_acquire(8 * max(1, self.rows), C.byref(pointer)))
        self.pointer = pointer.value

    def numpy(self):
        out = np.zeros((self.rows, 2), dtype=np.uint32)
        if self.rows:
            abi.check(self.lib.hy_memcpy_d2h(out.ctypes.data, self.pointer, out.nbytes))
        return out

    def close(self):
        if getattr(self, "pointer", None):
            self.lib.hy_result_pool_release(self.pointer)
            self.pointer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sort(keys, modes, limit=None, flags=0):
    """hy_sort: ORDER BY keys[0], keys[1], ... (DeviceColumn / ResultColumn of one table; abi.SORT_ASCENDING_NULLS_FIRST or
    abi.SORT_DESCENDING_NULLS_FIRST each) -> SortedPositions.  A string column takes part as ranks (string_rank_column).
    limit: ORDER BY ... LIMIT limit through hy_sort_limit (flags: 0 or abi.SORT_LIMIT_FORCE_*) -> SortedPositions of min(limit, rows) rows
    whose .path says whether every row was sorted (0) or the selection ran first (1)."""
    if len(keys) != len(modes) or not keys:
        raise ValueError("one mode per sort key, at least one key")
    lib = abi.load_library()
    array = (abi.SortKey * len(keys))()
    for i, (column, mode) in enumerate(zip(keys, modes)):
        array[i].column, array[i].mode = column.handle, mode
    n_out = C.c_uint64(0)
    if limit is None:
        out = SortedPositions(keys[0].rows)
        abi.check(lib.hy_sort(array, len(keys), out.pointer, max(1, out.rows), C.byref(n_out)))
        assert n_out.value == out.rows
        return out
    out = SortedPositions(min(int(limit), keys[0].rows))
    path = C.c_uint32(0)
    try:
        abi.check(lib.hy_sort_limit(array, len(keys), int(limit), flags, out.pointer, out.rows, C.byref(n_out), C.byref(path)))
    except Exception:
        out.close()
        raise
    assert n_out.value == out.rows
    out.path = path.value
    return out


def column_gather(column, positions, chunk_rows=abi.CHUNK_DEFAULT_SIZE):
    """hy_column_gather: the rows of `column` at `positions` (SortedPositions, or (device pointer, n)) as a ResultColumn of chunk_rows-row
    unencoded chunks -- Sort's materialised output of a numeric column."""
    pointer, n = (positions.pointer, positions.rows) if isinstance(positions, SortedPositions) else positions
    lib = abi.load_library()
    handle = C.c_void_p()
    abi.check(lib.hy_column_gather(column.handle, pointer, n, chunk_rows, C.byref(handle)))
    return ResultColumn(handle)


class UnionedPositions:
    """hy_union_positions' output: one PosList per column cluster, each in a block of the library's result-buffer pool (device memory; the
    next operator reads them in place).  numpy(c) copies cluster c's list back; path: bit 0 / 1 = the left / right side was sorted."""

    def __init__(self, n_clusters, capacity):
        self.lib = abi.load_library()
        self.capacity = max(1, int(capacity))
        self.rows, self.path, self.pointers = 0, 0, []
        for _ in range(n_clusters):
            pointer = C.c_void_p()
            abi.check(self.lib.hy_result_pool_acquire(8 * self.capacity, C.byref(pointer)))
            self.pointers.append(pointer.value)

    def numpy(self, cluster=0):
        out = np.zeros((self.rows, 2), dtype=np.uint32)
        if self.rows:
            abi.check(self.lib.hy_memcpy_d2h(out.ctypes.data, self.pointers[cluster], out.nbytes))
        return out

    def close(self):
        pointers, self.pointers = getattr(self, "pointers", []), []
        for pointer in pointers:
            self.lib.hy_result_pool_release(pointer)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def union_positions(left, right, force_sort=False, capacity=None):
    """hy_union_positions: the set union (UnionPositions, max(m, n) copies of a row) of two reference tables, each given as one reference
    DeviceColumn per column cluster -> UnionedPositions.  capacity: rows per output list (default: rows(left) + rows(right), which always fits)."""
    if len(left) != len(right) or not left:
        raise ValueError("one column per cluster on both sides, at least one cluster")
    lib = abi.load_library()
    handles = [(C.c_void_p * len(side))(*[column.handle for column in side]) for side in (left, right)]
    out = UnionedPositions(len(left), left[0].rows + right[0].rows if capacity is None else capacity)
    lists = (C.c_void_p * len(left))(*out.pointers)
    n_out, path = C.c_uint64(0), C.c_uint32(0)
    try:
        abi.check(lib.hy_union_positions(handles[0], handles[1], len(left), abi.UNION_FORCE_SORT if force_sort else 0, lists, 0 if capacity == 0 else out.capacity,
                                         C.byref(n_out), C.byref(path)))
    except Exception:
        out.close()
        raise
    out.rows, out.path = n_out.value, path.value
    return out


class SortMergePairs:
    """hy_join_sort_merge's output: the two PosLists in blocks of the library's result-buffer pool (device memory; the next operator reads
    them in place) -- n_matched pairs, then n_left_outer unmatched left rows, then the unmatched right rows.  numpy() copies both back."""

    def __init__(self, capacity):
        self.lib = abi.load_library()
        self.capacity = int(capacity)
        self.n_pairs = self.n_matched = self.n_left_outer = 0
        left, right = C.c_void_p(), C.c_void_p()
        abi.check(self.lib.hy_result_pool_acquire_pair(max(1, self.capacity), C.byref(left), C.byref(right)))
        self.left_pointer, self.right_pointer = left.value, right.value

    def numpy(self):
        left, right = np.zeros((self.n_pairs, 2), dtype=np.uint32), np.zeros((self.n_pairs, 2), dtype=np.uint32)
        if self.n_pairs:
            abi.check(self.lib.hy_memcpy_d2h(left.ctypes.data, self.left_pointer, left.nbytes))
            abi.check(self.lib.hy_memcpy_d2h(right.ctypes.data, self.right_pointer, right.nbytes))
        return left, right

    def close(self):
        for name in ("left_pointer", "right_pointer"):
            pointer = getattr(self, name, None)
            if pointer:
                self.lib.hy_result_pool_release(pointer)
                setattr(self, name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def join_sort_merge_count(left, right, mode, condition):
    lib = abi.load_library()
    n = C.c_uint64(0)
    abi.check(lib.hy_join_sort_merge_count(left.handle, right.handle, mode, condition, C.byref(n)))
    return int(n.value)


def join_sort_merge(left, right, mode, condition):
    """hy_join_sort_merge: left <condition> right (abi.PRED_EQUALS .. PRED_GREATER_THAN_EQUALS) under abi.JOIN_INNER / LEFT / RIGHT /
    FULL_OUTER -> SortMergePairs.  The lists are sized for one partner per row of the larger input; a join that needs more answers
    HY_ERR_CAPACITY with what it needs (nothing written) and runs once more with exactly that."""
    lib = abi.load_library()
    capacity = max(1, left.rows, right.rows)
    for attempt in (0, 1):
        out = SortMergePairs(capacity)
        result = abi.SortMergeResult()
        result.mem, result.left_pos, result.right_pos, result.capacity = abi.MEM_DEVICE, out.left_pointer, out.right_pointer, out.capacity
        status = lib.hy_join_sort_merge(left.handle, right.handle, mode, condition, C.byref(result))
        if status == abi.ERR_CAPACITY and attempt == 0:
            out.close()
            capacity = int(result.n_pairs)
            continue
        if status != abi.OK:
            out.close()
        abi.check(status)
        out.n_pairs, out.n_matched, out.n_left_outer = int(result.n_pairs), int(result.n_matched), int(result.n_left_outer)
        return out


class NestedLoopPairs(SortMergePairs):
    """hy_join_nested_loop's output in blocks of the result-buffer pool, in the reference's order; Semi / Anti fill the left list only."""

    def __init__(self, capacity, semi_anti=False):
        super().__init__(capacity)
        self.semi_anti = semi_anti

    def numpy(self):
        left, right = super().numpy() if not self.semi_anti else (np.zeros((self.n_pairs, 2), dtype=np.uint32), None)
        if self.semi_anti and self.n_pairs:
            abi.check(self.lib.hy_memcpy_d2h(left.ctypes.data, self.left_pointer, left.nbytes))
        return left, right


def join_nested_loop_count(left, right, mode, condition, secondary=None):
    lib = abi.load_library()
    predicates, n_secondary = join_predicates(secondary)
    n = C.c_uint64(0)
    abi.check(lib.hy_join_nested_loop_count(left.handle, right.handle, mode, condition, predicates, n_secondary, C.byref(n)))
    return int(n.value)


def join_nested_loop(left, right, mode, condition, secondary=None):
    """hy_join_nested_loop: left <condition> right AND the secondary predicates [(left column, condition, right column), ...] under any join
    mode but Cross -> NestedLoopPairs.  Sized for one partner per row of the larger input; a join that needs more answers HY_ERR_CAPACITY with
    what it needs (nothing written) and runs once more with exactly that."""
    lib = abi.load_library()
    predicates, n_secondary = join_predicates(secondary)
    semi_anti = mode in (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE)
    capacity = max(1, left.rows, right.rows)
    for attempt in (0, 1):
        out = NestedLoopPairs(capacity, semi_anti)
        result = abi.NestedLoopResult()
        result.mem, result.left_pos, result.right_pos, result.capacity = abi.MEM_DEVICE, out.left_pointer, None if semi_anti else out.right_pointer, out.capacity
        status = lib.hy_join_nested_loop(left.handle, right.handle, mode, condition, predicates, n_secondary, C.byref(result))
        if status == abi.ERR_CAPACITY and attempt == 0:
            out.close()
            capacity = int(result.n_pairs)
            continue
        if status != abi.OK:
            out.close()
        abi.check(status)
        out.n_pairs = int(result.n_pairs)
        return out


class ProductLists(SortMergePairs):
    """hy_product's output in blocks of the result-buffer pool: n_rows RowIDs per wanted side, pair (cl, cr) owning the rows
    [pair_offsets[cl * n_right_chunks + cr], pair_offsets[cl * n_right_chunks + cr + 1]).  numpy() copies the wanted lists back (None for the other)."""

    def __init__(self, capacity, want_left=True, want_right=True):
        super().__init__(capacity)
        self.want_left, self.want_right = want_left, want_right
        self.n_rows, self.pair_offsets = 0, None

    def numpy(self):
        lists = []
        for wanted, pointer in ((self.want_left, self.left_pointer), (self.want_right, self.right_pointer)):
            rows = np.zeros((self.n_rows, 2), dtype=np.uint32) if wanted else None
            if wanted and self.n_rows:
                abi.check(self.lib.hy_memcpy_d2h(rows.ctypes.data, pointer, rows.nbytes))
            lists.append(rows)
        return tuple(lists)


def product_count(left, right):
    lib = abi.load_library()
    n = C.c_uint64(0)
    abi.check(lib.hy_product_count(left.handle, right.handle, C.byref(n)))
    return int(n.value)


def product(left, right, want_left=True, want_right=True):
    """hy_product: the two PosLists of the cross join left x right (any column of each input table: only its chunk layout and, for a
    reference column, its PosLists are read) in the reference's order -> ProductLists in device memory, sized by hy_product_count."""
    lib = abi.load_library()
    out = ProductLists(product_count(left, right), want_left, want_right)
    offsets = np.zeros(left.n_chunks * right.n_chunks + 1, dtype=np.uint64)
    result = abi.ProductResult()
    result.mem, result.capacity, result.pair_offsets = abi.MEM_DEVICE, out.capacity, offsets.ctypes.data
    result.left_pos, result.right_pos = out.left_pointer if want_left else None, out.right_pointer if want_right else None
    status = lib.hy_product(left.handle, right.handle, C.byref(result))
    if status != abi.OK:
        out.close()
    abi.check(status)
    out.n_rows = out.n_pairs = int(result.n_rows)
    out.pair_offsets = offsets
    return out


def string_rank_column(segments, dictionaries):
    """A DictionarySegment<pmr_string> column (string_keys.encode_string_column) as a sort key: the same attribute vectors over dictionaries
    of the strings' ranks among all of the column's distinct strings in byte order (StringRanks) -> (HostColumn of int64, StringRanks)."""
    from .string_keys import StringRanks
    ranks = StringRanks([entry for dictionary in dictionaries for entry in dictionary])
    return ranks.dictionary_column(segments, dictionaries), ranks

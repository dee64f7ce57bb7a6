"""Row-by-row oracle of ColumnVsColumn on two string columns (column_vs_column_table_scan_impl.cpp:145-187 over pmr_string), and the rank
definition hy_string_dictionary_ranks implements.

A column is a list of chunks, a chunk a triple (dictionary, value_ids, null_id): the dictionary a sorted, duplicate-free list of bytes,
value_ids a sequence of ints, null_id == len(dictionary) the id that stands for NULL.  Python orders bytes as std::string orders its chars
taken as unsigned: byte by byte, the shorter first when it is the other's prefix."""
import bisect
import operator

from hyrise_amd import abi

COMPARISONS = {abi.PRED_EQUALS: operator.eq, abi.PRED_NOT_EQUALS: operator.ne, abi.PRED_LESS_THAN: operator.lt, abi.PRED_LESS_THAN_EQUALS: operator.le,
               abi.PRED_GREATER_THAN: operator.gt, abi.PRED_GREATER_THAN_EQUALS: operator.ge}
CONDITIONS = tuple(COMPARISONS)


def ranks(left_dictionary, right_dictionary):
    """rank(v) = 2 * lo(v) - (0 if right_dictionary[lo(v)] == left_dictionary[v] else 1), lo = lower_bound; the rank of right entry r is 2 * r."""
    out = []
    for entry in left_dictionary:
        lo = bisect.bisect_left(right_dictionary, entry)
        equal = lo < len(right_dictionary) and right_dictionary[lo] == entry
        out.append(2 * lo - (0 if equal else 1))
    return out


def column_ranks(left_dictionaries, right_dictionaries):
    return [ranks(l, r) for l, r in zip(left_dictionaries, right_dictionaries)]


def scan_chunk(left, right, condition):
    """Offsets of the rows of one chunk pair with left <condition> right; a NULL on either side matches nothing."""
    compare = COMPARISONS[condition]
    (left_dictionary, left_ids, left_null), (right_dictionary, right_ids, right_null) = left, right
    assert len(left_ids) == len(right_ids)
    return [row for row, (l, r) in enumerate(zip(left_ids, right_ids))
            if l != left_null and r != right_null and compare(left_dictionary[l], right_dictionary[r])]


def scan(left_chunks, right_chunks, condition):
    """Per chunk the list of matching chunk offsets."""
    assert len(left_chunks) == len(right_chunks)
    return [scan_chunk(l, r, condition) for l, r in zip(left_chunks, right_chunks)]


def scan_by_ranks(left_chunks, right_chunks, condition):
    """The same through the integer stand-ins: rank(v) <condition> 2 * r."""
    compare = COMPARISONS[condition]
    out = []
    for (left_dictionary, left_ids, left_null), (right_dictionary, right_ids, right_null) in zip(left_chunks, right_chunks):
        rank = ranks(left_dictionary, right_dictionary)
        out.append([row for row, (l, r) in enumerate(zip(left_ids, right_ids)) if l != left_null and r != right_null and compare(rank[l], 2 * r)])
    return out


def chunks_of(host_column, dictionaries):
    """The oracle's view of a storage.HostColumn of string dictionary segments and encode_string_dictionary's dictionaries."""
    return [(dictionary, [int(v) for v in segment.data], len(dictionary)) for segment, dictionary in zip(host_column.segments, dictionaries)]

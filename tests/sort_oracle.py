"""The order Sort::_on_execute produces (operators/sort.cpp:287-516), restated with numpy: one stable sort per definition from the last to
the first (std::stable_sort with std::less / std::greater), the NULL rows of each step moved to the front in the order they had (:435-443)."""
import numpy as np

from hyrise_amd import abi


def sorted_order(keys, modes):
    """keys: [(values, nulls or None)] of equal length (row order = chunk order, then offset); modes: abi.SORT_*_NULLS_FIRST.
    -> the row indices in sorted order."""
    n = len(keys[0][0]) if keys else 0
    order = np.arange(n, dtype=np.int64)
    for (values, nulls), mode in reversed(list(zip(keys, modes))):
        values = np.asarray(values)[order]
        is_null = np.zeros(n, dtype=bool) if nulls is None else np.asarray(nulls, dtype=bool)[order]
        present = np.flatnonzero(~is_null)
        v = values[present]
        if mode == abi.SORT_DESCENDING_NULLS_FIRST:
            v = -v if v.dtype.kind == "f" else ~v   # (order-reversing without overflow; -(-0.0) == 0.0 still ties)
        else:
            assert mode == abi.SORT_ASCENDING_NULLS_FIRST
        order = np.concatenate([order[is_null], order[present][np.argsort(v, kind="stable")]])
    return order


def positions_of(rows, chunk_sizes):
    """Flat row indices -> (chunk_id, chunk_offset) RowIDs of a table with the given chunk sizes."""
    base = np.concatenate([[0], np.cumsum(np.asarray(chunk_sizes, dtype=np.int64))])
    rows = np.asarray(rows, dtype=np.int64)
    chunk = np.searchsorted(base, rows, side="right") - 1
    return np.stack([chunk, rows - base[chunk]], axis=1).astype(np.uint32)

"""UnionPositions restated in numpy (union_positions.cpp:71-233): both inputs are matrices of RowIDs, one row per table row and one RowID per
column cluster; each is sorted lexicographically -- a RowID by (chunk_id, chunk_offset) as unsigned numbers, NULL_ROW_ID an ordinary largest
value -- and merged with std::set_union: a row that the left side holds m times and the right side n times appears max(m, n) times, in
ascending order.  Equal rows are indistinguishable, so the result is fully determined."""
import numpy as np

NULL_ROW_ID = (0xFFFFFFFF, 0xFFFFFFFF)


def as_matrix(clusters):
    """clusters: per column cluster an (n, 2) array of (chunk_id, chunk_offset) -> (n, n_clusters) uint64 keys, chunk_id in the high half."""
    columns = []
    for pos in clusters:
        pos = np.asarray(pos, dtype=np.uint64).reshape(-1, 2)
        columns.append((pos[:, 0] << np.uint64(32)) | pos[:, 1])
    return np.stack(columns, axis=1) if columns else np.zeros((0, 0), np.uint64)


def sorted_runs(matrix):
    """-> (the distinct rows in ascending order, how often each occurs)."""
    if len(matrix) == 0:
        return matrix, np.zeros(0, np.int64)
    order = np.lexsort(matrix.T[::-1])   # (lexsort's LAST key is the primary one)
    rows = matrix[order]
    first = np.ones(len(rows), dtype=bool)
    first[1:] = np.any(rows[1:] != rows[:-1], axis=1)
    starts = np.flatnonzero(first)
    return rows[starts], np.diff(np.append(starts, len(rows)))


def union_positions(left, right):
    """left / right: per cluster an (n, 2) array of RowIDs -> per cluster the (n_out, 2) uint32 PosList of the union."""
    n_clusters = len(left)
    assert n_clusters == len(right) and n_clusters >= 1
    a, m = sorted_runs(as_matrix(left))
    b, n = sorted_runs(as_matrix(right))
    both = np.concatenate([a.reshape(-1, n_clusters), b.reshape(-1, n_clusters)])
    counts = np.concatenate([m, n])
    from_right = np.concatenate([np.zeros(len(a), np.int64), np.ones(len(b), np.int64)])
    order = np.lexsort((from_right,) + tuple(both.T[::-1]))   # ascending, a left run before the equal right run
    both, counts, from_right = both[order], counts[order], from_right[order]
    paired = np.zeros(len(both), dtype=bool)   # a left run that is followed by the equal right run
    if len(both) > 1:
        paired[:-1] = np.all(both[:-1] == both[1:], axis=1) & (from_right[:-1] == 0) & (from_right[1:] == 1)
    repeat = counts.copy()
    after_left = np.flatnonzero(paired) + 1
    repeat[after_left] = np.maximum(counts[after_left], counts[after_left - 1])   # the pair yields max(m, n) rows ...
    repeat[paired] = 0                                                            # ... once
    rows = np.repeat(both, repeat, axis=0)
    out = []
    for c in range(n_clusters):
        keys = rows[:, c] if len(rows) else np.zeros(0, np.uint64)
        out.append(np.stack([(keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1))
    return out

"""Product (operators/product.cpp:51-61, 114-128) restated: chunk sizes and optional input PosLists -> both output lists and pair_offsets.

The chunk pairs run (cl, cr) with cl outermost; row p of a pair pairs left offset p // rows(cr) with right offset p % rows(cr); a data
input's RowID is (chunk, offset), a reference input's is its PosList's entry at that offset."""
import numpy as np

NULL_ROW_ID = (0xFFFFFFFF, 0xFFFFFFFF)


def entire_chunk(chunk_id, size):
    """An EntireChunkPosList as the RowIDs it stands for."""
    return np.stack([np.full(size, chunk_id, dtype=np.uint32), np.arange(size, dtype=np.uint32)], axis=1)


def product(left_sizes, right_sizes, left_lists=None, right_lists=None):
    """left_lists / right_lists: None for a data input, else one (n, 2) uint32 PosList per chunk.
    -> (left list, right list, pair_offsets): (n, 2) uint32 each, uint64 [len(left_sizes) * len(right_sizes) + 1]."""
    left, right, offsets = [], [], [0]
    for cl, rows_left in enumerate(left_sizes):
        for cr, rows_right in enumerate(right_sizes):
            for p in range(rows_left * rows_right):
                l, r = p // rows_right, p % rows_right
                left.append((cl, l) if left_lists is None else tuple(left_lists[cl][l]))
                right.append((cr, r) if right_lists is None else tuple(right_lists[cr][r]))
            offsets.append(len(left))
    as_list = lambda rows: np.array(rows, dtype=np.uint32).reshape(-1, 2)
    return as_list(left), as_list(right), np.array(offsets, dtype=np.uint64)


def product_numpy(left_sizes, right_sizes, left_lists=None, right_lists=None):
    """The same lists pair by pair with numpy's repeat / tile (the tests' large shapes); checked against product() in test_product_oracle.py."""
    left, right, offsets = [np.zeros((0, 2), dtype=np.uint32)], [np.zeros((0, 2), dtype=np.uint32)], [0]
    for cl, rows_left in enumerate(left_sizes):
        for cr, rows_right in enumerate(right_sizes):
            l = entire_chunk(cl, rows_left) if left_lists is None else np.asarray(left_lists[cl], dtype=np.uint32).reshape(-1, 2)
            r = entire_chunk(cr, rows_right) if right_lists is None else np.asarray(right_lists[cr], dtype=np.uint32).reshape(-1, 2)
            left.append(np.repeat(l, rows_right, axis=0))
            right.append(np.tile(r, (rows_left, 1)))
            offsets.append(offsets[-1] + rows_left * rows_right)
    return np.concatenate(left), np.concatenate(right), np.array(offsets, dtype=np.uint64)

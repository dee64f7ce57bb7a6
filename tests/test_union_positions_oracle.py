"""tests/union_positions_oracle.py against brute force (collections.Counter: max(m, n) copies of every row, ascending) on small random
multisets, and against the matrices of the reference's MultipleShuffledPosList case (union_positions_test.cpp:228-316), whose expected table
(tests/golden/tbl/union_positions/union_positions_multiple_shuffled_pos_list.tbl) holds the row ((2, 0), (1, 0)) three times: m = 1, n = 3."""
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest

from union_positions_oracle import NULL_ROW_ID, union_positions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tbl", "union_positions")


def brute_force(left, right):
    rows = lambda side: [tuple((int(pos[i][0]), int(pos[i][1])) for pos in side) for i in range(len(side[0]))]
    m, n = Counter(rows(left)), Counter(rows(right))
    out = []
    for row in sorted(set(m) | set(n)):
        out += [row] * max(m[row], n[row])
    return out


def as_rows(lists):
    return [tuple((int(pos[i][0]), int(pos[i][1])) for pos in lists) for i in range(len(lists[0]))]


@pytest.mark.parametrize("n_clusters", [1, 2, 3, 8])
@pytest.mark.parametrize("seed", range(6))
def test_oracle_matches_counter_arithmetic(n_clusters, seed):
    rng = np.random.default_rng(100 * n_clusters + seed)
    pool = [(0, 0), (0, 1), (1, 0), (2, 7), (0xFFFFFFFE, 3), NULL_ROW_ID, (3, 0xFFFFFFFF), (0x80000000, 0)]

    def side(n):
        return [np.array([pool[k] for k in rng.integers(0, 3 if c + 1 < n_clusters else len(pool), n)], dtype=np.uint32).reshape(-1, 2) for c in range(n_clusters)]

    left, right = side(int(rng.integers(0, 40))), side(int(rng.integers(0, 40)))
    assert as_rows(union_positions(left, right)) == brute_force(left, right)


def test_a_row_m_times_left_and_n_times_right_comes_max_m_n_times():
    row = np.array([[5, 9]], dtype=np.uint32)
    for m in range(4):
        for n in range(4):
            got = union_positions([np.repeat(row, m, axis=0)], [np.repeat(row, n, axis=0)])
            assert len(got[0]) == max(m, n), (m, n)


# The reference matrices of MultipleShuffledPosList, chunks concatenated: cluster 0 = columns a, b over int_float4.tbl, cluster 1 = column c
# over 10_ints.tbl, both tables in chunks of 3 rows.
LEFT = [[(1, 2), (0, 1), (1, 2), (2, 0), (0, 1)], [(2, 0), (1, 1), (1, 1), (1, 0), (2, 0)]]
RIGHT = [[(2, 0), (2, 0), (1, 2), (1, 0), (0, 0), (2, 0)], [(1, 0), (1, 0), (2, 0), (0, 0), (1, 0), (1, 0)]]


def load_tbl(path):
    with open(path) as f:
        lines = [line for line in f.read().splitlines() if line.strip()]
    return [tuple(line.split("|")) for line in lines[2:]]


def test_multiple_shuffled_pos_list_matrices():
    left, right = [np.array(c, np.uint32) for c in LEFT], [np.array(c, np.uint32) for c in RIGHT]
    got = as_rows(union_positions(left, right))
    assert got == brute_force(left, right)
    assert len(got) == 9
    assert got.count(((2, 0), (1, 0))) == 3   # m = 1, n = 3: max(m, n), not the "exactly once" of the operator's header comment
    int_float4 = load_tbl(os.path.join(os.path.dirname(GOLDEN), "int_float4.tbl"))
    ten_ints = load_tbl(os.path.join(GOLDEN, "10_ints.tbl"))
    values = sorted(int_float4[3 * ab[0] + ab[1]] + ten_ints[3 * c[0] + c[1]] for ab, c in got)
    assert values == sorted(load_tbl(os.path.join(GOLDEN, "union_positions_multiple_shuffled_pos_list.tbl")))


def test_golden_tables_match_their_manifest():
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        manifest = json.load(f)
    names = {"10_ints.tbl", "10_ints_exclusive_ranges.tbl", "int_float4_overlapping_ranges.tbl", "int_float4_int_int_union_positions.tbl",
             "union_positions_multiple_shuffled_pos_list.tbl", "int_int.tbl"}
    assert set(manifest) == names
    for name, entry in manifest.items():
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = f.read()
        assert len(data) < 200, name
        assert hashlib.sha256(data).hexdigest() == entry["sha256"], name

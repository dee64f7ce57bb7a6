"""Expected results of `column IN (list)` / `column NOT IN (list)` from what is already pinned to the reference: IN is the union of the
oracle's Equals scans over the elements (rewrite_in_list_expression ORs exactly those terms), NOT IN is the oracle's IS NOT NULL rows
without that union; a numpy brute force restates the same independently."""
import numpy as np

from hyrise_amd import abi
from hyrise_amd.operators import make_predicate, string_predicate

from support import oracle_scan

FLAGS = abi.SCAN_MATERIALIZE_ALL_MATCH


def brute_force_in(values, nulls, elements, negated=False):
    """Row mask: not NULL and == some element (IN) / no element (NOT IN).  NaN == x is False, -0.0 == 0.0 is True: numpy's == is C++'s."""
    values = np.asarray(values)
    valid = ~np.asarray(nulls, dtype=bool) if nulls is not None else np.ones(len(values), dtype=bool)
    listed = np.asarray(elements, dtype=values.dtype)
    hit = (values[:, None] == listed[None, :]).any(1)
    return (~hit if negated else hit) & valid


def _referenced_chunk(segment, positions):
    """Sort key of a chunk's matches: a PosList over several chunks is scanned sub-list by sub-list (by referenced chunk id)."""
    if segment.encoding != abi.ENC_REFERENCE or segment.data is None or segment.ref_chunk_id != abi.INVALID_CHUNK_ID:
        return np.zeros(len(positions), dtype=np.int64)
    return np.asarray(segment.data, dtype=np.uint32).reshape(-1, 2)[positions, 0].astype(np.int64)


def union_of_equals(host_column, elements, negated=False, nullable=False, dictionaries=None, equals_cache=None):
    """Per chunk the matching chunk offsets (uint32, in the order the scan emits them).  dictionaries: a string column's per-chunk
    dictionaries (elements are then strings).  equals_cache: {element: oracle result} shared between calls over one column."""
    equals_cache = {} if equals_cache is None else equals_cache
    n_chunks = host_column.n_chunks
    union = [np.zeros(0, dtype=np.uint32) for _ in range(n_chunks)]
    for element in elements:
        key = element if dictionaries is not None else (float(element) if isinstance(element, (float, np.floating)) else int(element))
        if key not in equals_cache:
            if dictionaries is not None:
                predicate = string_predicate(abi.PRED_EQUALS, dictionaries, element, nullable=nullable)
            else:
                predicate = make_predicate(abi.PRED_EQUALS, host_column.data_type, element, nullable=nullable)
            result = oracle_scan(host_column, predicate, flags=FLAGS)
            equals_cache[key] = [result.pos_list(c)[:, 1].copy() for c in range(n_chunks)]
        union = [np.union1d(union[c], equals_cache[key][c]).astype(np.uint32) for c in range(n_chunks)]
    if negated:
        data_type = abi.TYPE_INT if dictionaries is not None else host_column.data_type
        not_null = oracle_scan(host_column, make_predicate(abi.PRED_IS_NOT_NULL, data_type, nullable=nullable), flags=FLAGS)
        union = [np.setdiff1d(not_null.pos_list(c)[:, 1], union[c]).astype(np.uint32) for c in range(n_chunks)]
    out = []
    for c, positions in enumerate(union):   # ascending; by referenced chunk first where the PosList spans several
        order = np.lexsort((positions, _referenced_chunk(host_column.segments[c], positions)))
        out.append(positions[order])
    return out


def expected_matches(per_chunk):
    """(matches [n, 2] uint32, offsets [n_chunks + 1] uint64, counts [n_chunks] uint32) of a host scan result."""
    counts = np.array([len(p) for p in per_chunk], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)
    rows = [np.stack([np.full(len(p), c, dtype=np.uint32), p], axis=1) for c, p in enumerate(per_chunk)]
    return (np.concatenate(rows) if rows else np.zeros((0, 2), dtype=np.uint32)), offsets, counts


def assert_in_list_result(result, per_chunk, context=""):
    """Byte equality of a host scan result with the expected PosLists; chunk states: never ALL_MATCH, NONE_MATCH only without matches."""
    matches, offsets, counts = expected_matches(per_chunk)
    n = len(per_chunk)
    np.testing.assert_array_equal(result.counts[:n], counts, err_msg=f"counts {context}")
    np.testing.assert_array_equal(result.offsets, offsets, err_msg=f"offsets {context}")
    assert result.matches[:len(matches)].tobytes() == matches.tobytes(), f"PosLists differ {context}"
    for c in range(n):
        assert result.chunk_state[c] != abi.CHUNK_ALL_MATCH, f"chunk {c} reported ALL_MATCH {context}"
        assert result.chunk_state[c] != abi.CHUNK_NONE_MATCH or counts[c] == 0, f"chunk {c} reported NONE_MATCH with matches {context}"

"""hy_table_scan_expression against tests/expression_scan_oracle.py: PosLists byte-equal to the oracle's -- chunk sizes at the lane, wave,
round (1024 rows) and slice (8192 rows) edges, tables of several chunks, more chunks than 64 workgroups, selectivities 0 .. 1, host and
device results, every tree shape of the issue, every encoding, reference columns, excluded chunks, and the routes that already exist."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import (ColumnTest, make_predicate, predicate_for_column, projection_expression, string_in_list_predicate, string_predicate, table_scan,
                                  table_scan_expression)
from hyrise_amd.storage import DeviceColumn
import expression_scan_oracle as scan_oracle
import projection_expression_oracle as oracle
from support import build_column
from test_projection_expression_gpu import segment_of, string_table

pytestmark = pytest.mark.gpu
INT, LONG, FLOAT, DOUBLE = abi.TYPE_INT, abi.TYPE_LONG, abi.TYPE_FLOAT, abi.TYPE_DOUBLE
EQ, NE, LT, LE, GT, GE = abi.PRED_EQUALS, abi.PRED_NOT_EQUALS, abi.PRED_LESS_THAN, abi.PRED_LESS_THAN_EQUALS, abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS


def expected(rows, sizes):
    """The oracle's row numbers of the whole table as per-chunk RowIDs: ([total, 2] uint32, counts)."""
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    chunk = np.searchsorted(starts, rows, side="right") - 1
    matches = np.stack([chunk, rows - starts[chunk]], axis=1).astype(np.uint32) if len(rows) else np.zeros((0, 2), dtype=np.uint32)
    return matches, np.bincount(chunk, minlength=len(sizes)).astype(np.uint32)


def check(tree, resolve, sizes, context, want_rows=None, excluded=None, **kwargs):
    n = int(sum(sizes))
    if want_rows is None:
        want_rows = scan_oracle.pos_list(tree, resolve, n)
    matches, counts = expected(want_rows, sizes)
    got = table_scan_expression(tree, excluded_chunks=excluded, **kwargs)
    assert got.total == len(matches), f"{context}: total"
    np.testing.assert_array_equal(got.counts[:len(sizes)], counts, err_msg=f"{context}: counts")
    np.testing.assert_array_equal(got.offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), err_msg=f"{context}: offsets")
    assert got.matches[:got.total].tobytes() == matches.tobytes(), f"{context}: PosLists"
    want_state = [abi.CHUNK_NONE_MATCH if excluded is not None and c in excluded else abi.CHUNK_SCANNED for c in range(len(sizes))]
    assert got.chunk_state[:len(sizes)].tolist() == want_state, f"{context}: chunk_state is never ALL_MATCH"
    return want_rows


def int_table(values, nulls, chunk):
    column = DeviceColumn(build_column(values, nulls, chunk, abi.ENC_UNENCODED))
    sizes = [min(chunk, len(values) - b) for b in range(0, len(values), chunk)]
    return column, {id(column): oracle.Column.of(values, nulls)}, sizes


@pytest.mark.parametrize("chunk", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 65535])
def test_chunk_sizes_at_the_lane_wave_round_and_slice_edges(device, chunk):
    """`a < b + 1`, Int against Long, about half the rows, NULLs on both sides; two chunks: one of the size, one of three rows."""
    rng = np.random.default_rng(chunk)
    n = chunk + min(chunk, 3) if chunk > 1 else 4
    a_values, b_values = rng.integers(-20, 20, n).astype(np.int32), rng.integers(-20, 20, n).astype(np.int64)
    a_nulls, b_nulls = rng.random(n) < 0.1, rng.random(n) < 0.1
    a_values[-1], b_values[-1], a_nulls[-1], b_nulls[-1] = 0, 5, False, False   # the table's last row matches
    a = DeviceColumn(build_column(a_values, a_nulls, chunk, abi.ENC_UNENCODED))
    b = DeviceColumn(build_column(b_values, b_nulls, chunk, abi.ENC_UNENCODED))
    resolve = {id(a): oracle.Column.of(a_values, a_nulls), id(b): oracle.Column.of(b_values, b_nulls)}
    sizes = [min(chunk, n - begin) for begin in range(0, n, chunk)]
    rows = check(("cmp", LT, a, ("arith", abi.ARITH_ADD, b, (INT, 1))), resolve, sizes, f"chunk {chunk}")
    assert rows[-1] == n - 1 and (n < 8 or 0 < len(rows) < n)


def test_mixed_chunk_sizes_and_more_chunks_than_workgroups_of_a_wave_of_slices(device):
    rng = np.random.default_rng(3)
    for sizes in ([1, 1025, 64, 8193, 2, 300], list(rng.integers(1, 101, 65))):
        n = int(sum(sizes))
        values, nulls = rng.integers(0, 4, n).astype(np.int32), rng.random(n) < 0.2
        starts = np.concatenate([[0], np.cumsum(sizes)])
        column = DeviceColumn(storage.HostColumn([storage.encode_segment(values[b:e], nulls[b:e], abi.ENC_UNENCODED) for b, e in zip(starts[:-1], starts[1:])], INT))
        resolve = {id(column): oracle.Column.of(values, nulls)}
        rows = check(("or", ("cmp", EQ, column, (INT, 1)), ("is_null", column)), resolve, sizes, f"{len(sizes)} chunks")
        assert 0 < len(rows) < n


@pytest.mark.parametrize("name", ["none", "all", "last row of the last slice", "alternating", "random half"])
def test_selectivities(device, name):
    rng = np.random.default_rng(5)
    chunk, n = 8192 + 1024, 2 * (8192 + 1024)   # two slices per chunk, the second one round long
    values = {"none": np.zeros(n), "all": np.ones(n), "last row of the last slice": np.arange(n) == n - 1, "alternating": np.arange(n) % 2,
              "random half": rng.integers(0, 2, n)}[name].astype(np.int32)
    column, resolve, sizes = int_table(values, None, chunk)
    rows = check(("cmp", EQ, ("arith", abi.ARITH_MUL, column, (INT, 3)), (INT, 3)), resolve, sizes, name, want_rows=np.flatnonzero(values == 1))
    assert len(rows) == {"none": 0, "all": n, "last row of the last slice": 1, "alternating": n // 2}.get(name, len(rows))
    if name == "random half":
        assert 0 < len(rows) < n


def device_result(torch, n_chunks, rows, flags, misalign=0):
    matches = torch.zeros((rows + 4, 2), dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(n_chunks, dtype=torch.int32, device="cuda")
    state = torch.full((n_chunks,), 77, dtype=torch.uint8, device="cuda")
    r = abi.ScanResult()
    r.mem, r.flags = abi.MEM_DEVICE, flags
    r.matches, r.capacity = matches.data_ptr() + misalign, rows
    r.offsets, r.counts, r.chunk_state = offsets.data_ptr(), counts.data_ptr(), state.data_ptr()
    return r, (matches, offsets, counts, state)


def test_device_results_alignment_and_poslist_translate(device):
    import torch
    from hyrise_amd.operators import projection_program
    rng = np.random.default_rng(7)
    sizes = [300, 1025, 70]
    n = sum(sizes)
    values, nulls = rng.integers(0, 3, n).astype(np.int32), rng.random(n) < 0.2
    starts = np.concatenate([[0], np.cumsum(sizes)])
    column = DeviceColumn(storage.HostColumn([storage.encode_segment(values[b:e], nulls[b:e], abi.ENC_UNENCODED) for b, e in zip(starts[:-1], starts[1:])], INT))
    resolve = {id(column): oracle.Column.of(values, nulls)}
    tree = ("cmp", GT, ("arith", abi.ARITH_ADD, column, (INT, 1)), (INT, 1))
    rows = check(tree, resolve, sizes, "host")
    check(tree, resolve, sizes, "host, materialize flag", flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    want, want_counts = expected(rows, sizes)
    assert 0 < len(rows) < n
    for flags in (0, abi.SCAN_MATERIALIZE_ALL_MATCH):
        matches, offsets, counts, state = table_scan_expression(tree, flags=flags, device=True)
        assert matches.data_ptr() % 16 == 0
        np.testing.assert_array_equal(offsets.cpu().numpy(), starts)
        np.testing.assert_array_equal(counts.cpu().numpy().astype(np.uint32), want_counts)
        assert state.cpu().numpy().tolist() == [abi.CHUNK_SCANNED] * 3
        regions = matches.cpu().numpy().view(np.uint32)
        got = np.concatenate([regions[starts[c]:starts[c] + want_counts[c]] for c in range(3)])
        assert got.tobytes() == want.tobytes()
    program, keep = projection_program(tree)
    r, buffers = device_result(torch, 3, n, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH, misalign=8)
    assert device.hy_table_scan_expression(C.byref(program), None, 0, C.byref(r)) == abi.ERR_INVALID, "matches on 8 bytes only: refused"
    assert int(buffers[3].cpu()[0]) == 77 and not buffers[0].any(), "before any launch"
    r, buffers = device_result(torch, 3, n, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH)
    abi.check(device.hy_table_scan_expression(C.byref(program), None, 0, C.byref(r)))
    for layout in (abi.POSLIST_DENSE, abi.POSLIST_CHUNK_REGIONS):
        out = torch.zeros((n + 2, 2), dtype=torch.int32, device="cuda")
        total = C.c_uint64(0)
        abi.check(device.hy_poslist_translate(column.handle, C.byref(r), layout, out.data_ptr(), n, C.byref(total)))
        assert total.value == len(want)
        translated = out.cpu().numpy().view(np.uint32)
        if layout == abi.POSLIST_DENSE:
            assert translated[:len(want)].tobytes() == want.tobytes()
        else:
            assert np.concatenate([translated[starts[c]:starts[c] + want_counts[c]] for c in range(3)]).tobytes() == want.tobytes()
    del keep


def numeric_table(rng, n, chunk, encodings=abi.ENC_UNENCODED):
    raw = {INT: rng.integers(-3, 4, n).astype(np.int32), LONG: rng.integers(-3, 4, n).astype(np.int64), FLOAT: (rng.integers(-8, 9, n) / 4.0).astype(np.float32),
           DOUBLE: rng.integers(-8, 9, n) / 4.0}
    nulls = {t: rng.random(n) < 0.2 for t in raw}
    devs = {t: DeviceColumn(build_column(raw[t], nulls[t], chunk, encodings)) for t in raw}
    resolve = {id(devs[t]): oracle.Column.of(raw[t], nulls[t]) for t in raw}
    sizes = [min(chunk, n - b) for b in range(0, n, chunk)]
    return devs, resolve, sizes, raw, nulls


def test_the_trees_of_the_fallback(device):
    rng = np.random.default_rng(11)
    n, chunk = 700, 257
    devs, resolve, sizes, raw, nulls = numeric_table(rng, n, chunk)
    i, l, f, d = devs[INT], devs[LONG], devs[FLOAT], devs[DOUBLE]
    one_minus = lambda x: ("arith", abi.ARITH_SUB, (INT, 1), x)
    trees = {
        "a * (1 - b) > c in Float": ("cmp", GT, ("arith", abi.ARITH_MUL, f, one_minus(f)), (FLOAT, -0.5)),
        "a * (1 - b) > c in Double": ("cmp", GT, ("arith", abi.ARITH_MUL, d, one_minus(f)), d),
        "a < b + 1, Int against Long": ("cmp", LT, i, ("arith", abi.ARITH_ADD, l, (INT, 1))),
        "Int column = 3.1": ("cmp", EQ, i, (DOUBLE, 3.1)),
        "Int column < 2.5": ("cmp", LT, i, (DOUBLE, 2.5)),
        "x = 1 OR y IS NULL": ("or", ("cmp", EQ, i, (INT, 1)), ("is_null", l)),
        "CASE WHEN a > 0 THEN b ELSE c END = 1": ("cmp", EQ, ("case", ("cmp", GT, i, (INT, 0)), l, f), (INT, 1)),
        "IS NOT NULL of a quotient": ("is_not_null", ("arith", abi.ARITH_DIV, d, i)),
        "between on the spine": ("and", ("between", abi.PRED_BETWEEN_UPPER_EXCLUSIVE, d, (DOUBLE, -1.0), (INT, 1)), ("is_not_null", i)),
    }
    for name, tree in trees.items():
        rows = check(tree, resolve, sizes, name)
        assert name == "Int column = 3.1" or 0 < len(rows) < n, name
    assert predicate_for_column(EQ, INT, DOUBLE, 3.1) is None, "the literal hy_predicate_cast refuses"
    # a numeric BETWEEN as a column test on the spine: the range job, FALSE and NULL both dropped
    between = ColumnTest(i, make_predicate(abi.PRED_BETWEEN_INCLUSIVE, INT, -1, 2, nullable=True))
    resolve[id(between)] = oracle.Test(resolve[id(i)].cells, lambda cell: -1 <= cell <= 2)
    rows = check(("or", between, ("cmp", GT, f, (INT, 1))), resolve, sizes, "BETWEEN column test under OR")
    assert rows == scan_oracle.pos_list(("or", ("between", abi.PRED_BETWEEN_INCLUSIVE, i, (INT, -1), (INT, 2)), ("cmp", GT, f, (INT, 1))), resolve, n)
    for tree in (("is_null", between), ("cmp", EQ, ("case", between, i, l), (INT, 1))):   # below the spine: refused, nothing written
        with pytest.raises(abi.HyriseAmdError) as error:
            table_scan_expression(tree)
        assert error.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(abi.HyriseAmdError) as error:
        table_scan_expression(("arith", abi.ARITH_ADD, i, l))
    assert error.value.status == abi.ERR_INVALID


def test_p_and_q_or_r_with_nulls_in_every_position(device):
    cells = [0, 1, None]
    triples = [(p, q, r) for p in cells for q in cells for r in cells] * 3
    columns, resolve = [], {}
    for k in range(3):
        values = np.array([0 if t[k] is None else t[k] for t in triples], dtype=np.int32)
        nulls = np.array([t[k] is None for t in triples])
        columns.append(DeviceColumn(build_column(values, nulls, 40, abi.ENC_UNENCODED)))
        resolve[id(columns[-1])] = oracle.Column.of(values, nulls)
    p, q, r = (("cmp", NE, c, (INT, 0)) for c in columns)
    sizes = [40, 40, 1]
    rows = check(("or", ("and", p, q), r), resolve, sizes, "(p AND q) OR r")
    assert rows == [k for k, (a, b, c) in enumerate(triples) if (a == 1 and b == 1) or c == 1]
    check(("and", ("or", p, q), ("or", r, ("is_null", columns[0]))), resolve, sizes, "(p OR q) AND (r OR p IS NULL)")


def test_string_column_tests_anded_with_a_numeric_comparison(device):
    rng = np.random.default_rng(13)
    sizes = (65, 300, 9, 64)
    n = sum(sizes)
    host, dictionaries, cells = string_table(rng, sizes)
    column = DeviceColumn(host)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    amounts = rng.integers(0, 100, n).astype(np.int32)
    amount = DeviceColumn(storage.HostColumn([storage.encode_segment(amounts[b:e], None, abi.ENC_UNENCODED) for b, e in zip(starts[:-1], starts[1:])], INT))
    elements = [b"1-URGENT", b"2-HIGH", b"NO SUCH WORD"]
    tests = {"=": (string_predicate(EQ, dictionaries, b"1-URGENT", nullable=True), lambda s: s == b"1-URGENT"),
             "like": (make_predicate(abi.PRED_LIKE, abi.TYPE_STRING, nullable=True, dictionary_matches=[[w.startswith(b"PROMO") for w in dictionary] for dictionary in dictionaries]),
                      lambda s: s.startswith(b"PROMO")),
             "in": (string_in_list_predicate(dictionaries, elements, nullable=True), lambda s: s in elements),
             "between": (string_predicate(abi.PRED_BETWEEN_INCLUSIVE, dictionaries, b"1", b"3", nullable=True), lambda s: b"1" <= s <= b"3")}
    for name, (predicate, holds) in tests.items():
        test = ColumnTest(column, predicate)
        resolve = {id(test): oracle.Test(cells, holds), id(amount): oracle.Column.of(amounts)}
        rows = check(("and", test, ("cmp", LT, ("arith", abi.ARITH_MUL, amount, (INT, 2)), (INT, 120))), resolve, sizes, f"string {name}")
        assert 0 < len(rows) < n, name
        if name != "in":   # the column test alone is hy_table_scan's predicate
            alone = table_scan_expression(test)
            scanned = table_scan(column, predicate, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
            assert alone.total == scanned.total and alone.matches[:alone.total].tobytes() == scanned.matches[:scanned.total].tobytes(), name


def test_q6_as_one_program_and_the_routes_that_exist(device):
    """l_shipdate >= a AND l_shipdate < b AND l_discount BETWEEN 0.05 AND 0.07 AND l_quantity < 24 as one program; the same rows as
    hy_projection_expression followed by hy_table_scan(<> 0); and `column < literal` equals hy_table_scan itself."""
    rng = np.random.default_rng(17)
    n, chunk = 20_000, 8_193
    shipdate = rng.integers(0, 2500, n).astype(np.int32)
    discount = (rng.integers(0, 11, n) / 100.0).astype(np.float32)
    quantity = rng.integers(1, 51, n).astype(np.float32)
    s, d, q = (DeviceColumn(build_column(v, None, chunk, e)) for v, e in ((shipdate, abi.ENC_DICTIONARY), (discount, abi.ENC_DICTIONARY), (quantity, abi.ENC_UNENCODED)))
    sizes = [min(chunk, n - b) for b in range(0, n, chunk)]
    dates = ColumnTest(s, make_predicate(abi.PRED_BETWEEN_UPPER_EXCLUSIVE, INT, 731, 1096))
    discounts = ColumnTest(d, make_predicate(abi.PRED_BETWEEN_INCLUSIVE, FLOAT, 0.05, 0.07001))
    q6 = ("and", ("and", dates, discounts), ("cmp", LT, q, (INT, 24)))
    want = np.flatnonzero((shipdate >= 731) & (shipdate < 1096) & (discount >= np.float32(0.05)) & (discount <= np.float32(0.07001)) & (quantity < 24))
    assert 0 < len(want) < n
    check(q6, {}, sizes, "Q6", want_rows=want)
    # a tree both routes can express
    tree = ("and", ("cmp", GT, ("arith", abi.ARITH_MUL, q, ("arith", abi.ARITH_SUB, (INT, 1), d)), (INT, 20)), ("cmp", GE, s, (INT, 731)))
    one_pass = table_scan_expression(tree)
    column = projection_expression(tree)
    two_calls = table_scan(column, make_predicate(NE, INT, 0, nullable=True), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    assert 0 < one_pass.total < n and one_pass.total == two_calls.total
    assert one_pass.matches[:one_pass.total].tobytes() == two_calls.matches[:two_calls.total].tobytes()
    np.testing.assert_array_equal(one_pass.counts, two_calls.counts)
    alone = table_scan_expression(("cmp", LT, s, (INT, 1000)))
    scanned = table_scan(s, make_predicate(LT, INT, 1000), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    assert alone.total == scanned.total and alone.matches[:alone.total].tobytes() == scanned.matches[:scanned.total].tobytes()


def test_every_encoding_reference_columns_and_excluded_chunks(device):
    rng = np.random.default_rng(19)
    kinds = ["value", "dictionary", "frame_of_reference", "run_length", "bit_packed"]
    chunk, n = 257, 257 * 5
    ints = np.repeat(rng.integers(-100, 100, n // 4 + 1), 4)[:n].astype(np.int32)
    int_nulls = np.repeat(rng.random(n // 4 + 1) < 0.1, 4)[:n]
    doubles, double_nulls = rng.integers(-40, 40, n) / 8.0, rng.random(n) < 0.1
    host_i = storage.HostColumn([segment_of(ints[c * chunk:(c + 1) * chunk], int_nulls[c * chunk:(c + 1) * chunk], kind) for c, kind in enumerate(kinds)], INT)
    host_d = storage.HostColumn([segment_of(doubles[c * chunk:(c + 1) * chunk], double_nulls[c * chunk:(c + 1) * chunk], kind if kind != "frame_of_reference" else "dictionary")
                                 for c, kind in enumerate(kinds)], DOUBLE)
    i, d = DeviceColumn(host_i), DeviceColumn(host_d)
    resolve = {id(i): oracle.Column.of(ints, int_nulls), id(d): oracle.Column.of(doubles, double_nulls)}
    tree = lambda x, y: ("or", ("cmp", GT, ("arith", abi.ARITH_MUL, x, y), (INT, 50)), ("and", ("is_null", y), ("cmp", LT, x, (INT, 0))))
    sizes = [chunk] * 5
    rows = check(tree(i, d), resolve, sizes, "data segments of every encoding")
    assert 0 < len(rows) < n
    excluded = [1, 3]
    kept = [r for r in rows if r // chunk not in excluded]
    check(tree(i, d), resolve, sizes, "excluded chunks", want_rows=kept, excluded=excluded)
    test = ColumnTest(i, make_predicate(abi.PRED_BETWEEN_INCLUSIVE, INT, -10, 60, nullable=True))
    resolve[id(test)] = oracle.Test(resolve[id(i)].cells, lambda cell: -10 <= cell <= 60)
    check(("and", test, ("is_not_null", d)), resolve, sizes, "a numeric BETWEEN test over every encoding")
    # reference columns: one host PosList over all chunks with NULL RowIDs; one PosList per chunk, each of one chunk; entire-chunk lists
    picks = rng.integers(0, n, 700)
    pos = np.stack([picks // chunk, picks % chunk], axis=1).astype(np.uint32)
    null_rows = rng.random(len(picks)) < 0.1
    pos[null_rows] = 0xFFFFFFFF
    every_second = [np.stack([np.full((chunk + 1) // 2, c), np.arange(0, chunk, 2)], axis=1).astype(np.uint32) for c in range(5)]
    for name, lists, single, flat, null_ids in (("multi-chunk PosList with NULL RowIDs", [pos], [None], picks, null_rows),
                                                ("single-chunk PosLists", every_second, list(range(5)), np.concatenate([c * chunk + np.arange(0, chunk, 2) for c in range(5)]), None),
                                                ("entire-chunk PosLists", list(range(5)), list(range(5)), np.arange(n), None)):
        null_ids = np.zeros(len(flat), dtype=bool) if null_ids is None else null_ids
        ri = DeviceColumn(storage.make_reference_column(host_i, lists, single), refs={id(host_i): i})
        rd = DeviceColumn(storage.make_reference_column(host_d, lists, single), refs={id(host_d): d})
        through = {id(ri): oracle.Column.of(ints[flat], int_nulls[flat] | null_ids), id(rd): oracle.Column.of(doubles[flat], double_nulls[flat] | null_ids)}
        through_sizes = [chunk if isinstance(l, int) else len(l) for l in lists]
        rows = check(tree(ri, rd), through, through_sizes, name)
        assert 0 < len(rows) < len(flat), name
        with pytest.raises(abi.HyriseAmdError) as error:
            table_scan_expression(tree(ri, rd), excluded_chunks=[0])
        assert error.value.status == abi.ERR_INVALID


def test_dictionary_and_frame_of_reference_vectors_of_one_two_and_four_bytes(device):
    """Attribute vectors of u8, u16 and u32 (a dictionary of more than 65 535 entries) and FrameOfReference offsets of 1, 2 and 4 bytes, read
    as a column of the program (decode_rows) and through a BETWEEN column test (test_cell)."""
    rng = np.random.default_rng(23)
    sizes = [80_000, 1_000, 300, 3_000, 3_000, 3_000]
    n = sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    parts = [rng.permutation(3 * 80_000)[:80_000] - 80_000,          # 80 000 distinct values, a tenth of them NULL: u32 value ids
             rng.permutation(5_000)[:1_000] - 2_000,                 # 1 000 distinct: u16
             rng.integers(-100, 100, 300),                           # u8
             rng.integers(-1_000_000, 1_000_000, 3_000),             # FrameOfReference, 4-byte offsets
             rng.integers(-20_000, 20_000, 3_000),                   # 2-byte offsets
             rng.integers(1_000, 1_200, 3_000)]                      # 1-byte offsets
    ints = np.concatenate(parts).astype(np.int32)
    nulls = rng.random(n) < 0.1
    encodings = [abi.ENC_DICTIONARY] * 3 + [abi.ENC_FRAME_OF_REFERENCE] * 3
    segments = [storage.encode_segment(ints[b:e], nulls[b:e], encoding) for b, e, encoding in zip(starts[:-1], starts[1:], encodings)]
    assert [s.width for s in segments] == [4, 2, 1, 4, 2, 1]
    i = DeviceColumn(storage.HostColumn(segments, INT))
    doubles = rng.integers(-8, 9, n) / 4.0
    d = DeviceColumn(storage.HostColumn([storage.encode_segment(doubles[b:e], None, abi.ENC_UNENCODED) for b, e in zip(starts[:-1], starts[1:])], DOUBLE))
    want = np.flatnonzero(~nulls & (ints * doubles > 1000.0))
    assert 0 < len(want) < n
    check(("cmp", GT, ("arith", abi.ARITH_MUL, i, d), (INT, 1000)), {}, sizes, "vectors of every width as a program column", want_rows=want)
    test = ColumnTest(i, make_predicate(abi.PRED_BETWEEN_INCLUSIVE, INT, -1_500, 1_100, nullable=True))
    want = np.flatnonzero((~nulls & (ints >= -1_500) & (ints <= 1_100)) | (doubles > 1.5))
    assert 0 < len(want) < n
    check(("or", test, ("cmp", GT, d, (DOUBLE, 1.5))), {}, sizes, "vectors of every width under a BETWEEN column test", want_rows=want)

"""hy_projection_expression against tests/projection_expression_oracle.py, bit for bit (floats by their bits too: every operation is a
single IEEE operation in a stated type, nothing is reassociated) -- every node kind, operand type pairing and NULL position, chunk sizes
around the null-word boundaries, every encoding, reference columns, column tests over dictionary string columns, and the result column
handed to the next operator.  NaN is kept out of the inputs: the evaluator's swapped > / >= differ from the direct forms only there."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import (ColumnTest, aggregate_hash, column_gather, make_predicate, projection_arithmetic, projection_expression, projection_program, sort,
                                  string_in_list_predicate, string_predicate, table_scan)
from hyrise_amd.storage import DeviceColumn
import projection_expression_oracle as oracle
from placed_columns import PlacedColumn
from support import build_column

pytestmark = pytest.mark.gpu
TYPES = (abi.TYPE_INT, abi.TYPE_LONG, abi.TYPE_FLOAT, abi.TYPE_DOUBLE)
ARITH = (abi.ARITH_ADD, abi.ARITH_SUB, abi.ARITH_MUL, abi.ARITH_DIV, abi.ARITH_MOD)
CMP = (abi.PRED_EQUALS, abi.PRED_NOT_EQUALS, abi.PRED_LESS_THAN, abi.PRED_LESS_THAN_EQUALS, abi.PRED_GREATER_THAN, abi.PRED_GREATER_THAN_EQUALS)
INT, DOUBLE = abi.TYPE_INT, abi.TYPE_DOUBLE


def check(tree, resolve, rows, context):
    got = projection_expression(tree)
    want_type, cells = oracle.evaluate(tree, resolve, rows)
    want_values, want_nulls = oracle.as_arrays(want_type, cells)
    values, nulls = got.read()
    assert got.data_type == want_type and values.dtype == want_values.dtype, context
    np.testing.assert_array_equal(nulls, want_nulls, err_msg=f"NULLs {context}")
    assert values.tobytes() == want_values.tobytes(), f"values (NULL cells hold T{{}}) {context}"
    return got


def raw_columns(rng, n):
    raw = {abi.TYPE_INT: rng.integers(-50, 50, n).astype(np.int32), abi.TYPE_LONG: (rng.integers(-5, 5, n) * 3_000_000_000).astype(np.int64),
           abi.TYPE_FLOAT: (rng.integers(-400, 400, n) / 7.0).astype(np.float32), abi.TYPE_DOUBLE: rng.normal(0, 1000, n)}
    raw[abi.TYPE_INT][::11] = 0
    raw[abi.TYPE_FLOAT][::13] = 0.0
    raw[abi.TYPE_FLOAT][1::26] = -0.0
    raw[abi.TYPE_DOUBLE][::17] = 0.0
    if n > 6:
        raw[abi.TYPE_INT][5], raw[abi.TYPE_LONG][5], raw[abi.TYPE_FLOAT][5], raw[abi.TYPE_DOUBLE][5] = 16_777_217, 16_777_217, 16_777_216.0, 16_777_216.0
        raw[abi.TYPE_INT][6] = np.iinfo(np.int32).max
    return raw


def table(rng, n, chunk, encodings=abi.ENC_UNENCODED, null_rate=0.15):
    raw = raw_columns(rng, n)
    nulls = {t: rng.random(n) < null_rate for t in raw}
    for t in raw:
        nulls[t][min(5, n - 1)] = False
    devs = {t: DeviceColumn(build_column(raw[t], nulls[t], chunk, encodings)) for t in raw}
    resolve = {id(devs[t]): oracle.Column.of(raw[t], nulls[t]) for t in raw}
    return devs, resolve


@pytest.mark.parametrize("chunk,n", [(1, 5), (63, 200), (64, 200), (65, 200), (257, 600), (65_535, 65_536)])
def test_chunk_sizes_around_the_null_words(device, chunk, n):
    """A null-word tail, a chunk that is one word exactly, a last chunk of one row: CASE WHEN a > b OR c IS NULL THEN a * d ELSE -d END."""
    rng = np.random.default_rng(chunk)
    devs, resolve = table(rng, n, chunk)
    a, b, c, d = (devs[t] for t in TYPES)
    tree = ("case", ("or", ("cmp", abi.PRED_GREATER_THAN, a, b), ("is_null", c)), ("arith", abi.ARITH_MUL, a, d), ("neg", d))
    got = check(tree, resolve, n, f"chunk {chunk}")
    assert got.n_chunks == (n + chunk - 1) // chunk


def test_every_binary_node_over_every_type_pair(device):
    """Arithmetic and comparisons, Int / Long / Float / Double in every pairing, columns and literals, NULLs on both sides.  Row 5 holds Int
    16 777 217 against Float 16 777 216.0f: equal in the common type float; -0.0 meets 0.0."""
    rng = np.random.default_rng(7)
    n = 300
    devs, resolve = table(rng, n, 129)
    literal = {abi.TYPE_INT: 3, abi.TYPE_LONG: 5_000_000_000, abi.TYPE_FLOAT: 2.5, abi.TYPE_DOUBLE: 0.1}
    for lt in TYPES:
        for rt in TYPES:
            for op in ARITH:
                check(("arith", op, devs[lt], devs[rt]), resolve, n, f"arith {op} types {lt},{rt}")
            for condition in CMP:
                check(("cmp", condition, devs[lt], devs[rt]), resolve, n, f"cmp {condition} types {lt},{rt}")
            check(("arith", abi.ARITH_DIV, devs[lt], (rt, literal[rt])), resolve, n, f"{lt} / literal {rt}")
            check(("cmp", abi.PRED_LESS_THAN_EQUALS, (rt, literal[rt]), devs[lt]), resolve, n, f"literal {rt} <= {lt}")
        check(("cmp", abi.PRED_EQUALS, devs[lt], None), resolve, n, f"{lt} = NULL")
        check(("neg", devs[lt]), resolve, n, f"-{lt}")
        check(("is_not_null", ("neg", devs[lt])), resolve, n, f"-{lt} IS NOT NULL")
    equal = projection_expression(("cmp", abi.PRED_EQUALS, devs[abi.TYPE_INT], devs[abi.TYPE_FLOAT])).read()[0]
    assert equal[5] == 1, "Int 16 777 217 = Float 16 777 216.0f in float"
    zero = DeviceColumn(build_column(np.array([0.0, -0.0], dtype=np.float64), None, 2, abi.ENC_UNENCODED))
    values, nulls = projection_expression(("cmp", abi.PRED_EQUALS, zero, (abi.TYPE_FLOAT, -0.0))).read()
    assert values.tolist() == [1, 1] and not nulls.any()


def test_ternary_logic_truth_tables(device):
    """AND / OR over {0, 1 (any non-zero), NULL} x {0, 1, NULL} in both operand positions, and against NULL and Int literals."""
    cells = [0, 7, None]
    left = [x for x in cells for _ in cells] * 3
    right = [y for _ in cells for y in cells] * 3
    as_column = lambda xs: (np.array([0 if x is None else x for x in xs], dtype=np.int32), np.array([x is None for x in xs]))
    a, b = (DeviceColumn(build_column(*as_column(xs), 5, abi.ENC_UNENCODED)) for xs in (left, right))
    resolve = {id(a): oracle.Column.of(*as_column(left)), id(b): oracle.Column.of(*as_column(right))}
    for kind in ("and", "or"):
        got = check((kind, a, b), resolve, len(left), kind)
        values, nulls = got.read()
        table_got = [None if nulls[i] else int(values[i]) for i in range(9)]
        assert table_got == ([0, 0, 0, 0, 1, None, 0, None, None] if kind == "and" else [0, 1, None, 1, 1, 1, None, 1, None])
        for literal in (None, (INT, 0), (INT, 1)):
            check((kind, a, literal), resolve, len(left), f"{kind} literal {literal} right")
            check((kind, literal, b), resolve, len(left), f"{kind} literal {literal} left")
        check((kind, ("is_null", a), ("cmp", abi.PRED_GREATER_THAN, b, (INT, 0))), resolve, len(left), f"{kind} of predicates")


def test_case(device):
    rng = np.random.default_rng(9)
    n = 400
    devs, resolve = table(rng, n, 130)
    i, l, f, d = (devs[t] for t in TYPES)
    when = ("cmp", abi.PRED_GREATER_THAN, i, (INT, 0))   # NULL where i is
    for then, otherwise in ((i, d), (d, i), (None, i), (i, None), (f, l), ((INT, 1), (DOUBLE, 0.5)), (l, (INT, 0)), (("arith", abi.ARITH_DIV, d, i), (INT, 0))):
        check(("case", when, then, otherwise), resolve, n, f"case {then} {otherwise}")
    check(("case", None, i, d), resolve, n, "NULL literal when")
    # a chained CASE (a CASE in the otherwise position) at the stack depth limit: when, then, when, then and the two operands of the last otherwise
    depth = abi.MAX_PROJECTION_DEPTH
    chained = ("case", ("cmp", abi.PRED_LESS_THAN, i, (INT, -20)), l, ("case", ("cmp", abi.PRED_EQUALS, i, (INT, 0)), f, ("arith", abi.ARITH_ADD, d, i)))
    assert depth == 6
    check(chained, resolve, n, "chained case at the depth limit")
    nested = ("case", ("case", when, ("is_null", l), (INT, 0)), ("case", when, i, l), ("neg", f))
    check(nested, resolve, n, "case in when and then")
    over = ("case", when, i, ("case", when, i, ("case", when, i, ("arith", abi.ARITH_ADD, i, i))))   # seven entries
    with pytest.raises(abi.HyriseAmdError) as error:
        projection_expression(over)
    assert error.value.status == abi.ERR_UNSUPPORTED


def segment_of(values, nulls, kind):
    if kind == "run_length":
        return storage.encode_run_length(values, nulls)
    if kind == "bit_packed":
        segment = storage.encode_segment(values, nulls, abi.ENC_DICTIONARY)
        return storage.HostSegment(segment.encoding, segment.data_type, segment.size, 0, storage.pack_bits(segment.data, 9), aux=segment.aux, aux_size=segment.aux_size, bits=9)
    return storage.encode_segment(values, nulls, {"value": abi.ENC_UNENCODED, "dictionary": abi.ENC_DICTIONARY, "frame_of_reference": abi.ENC_FRAME_OF_REFERENCE}[kind])


def test_every_encoding_and_reference_columns(device):
    """Unencoded, Dictionary, FrameOfReference, RunLength and BitPacking chunks in one column; the same column behind a host PosList over
    several chunks with NULL RowIDs, behind one PosList per chunk, and behind a device PosList with NULL RowIDs (an outer join's output)."""
    import torch
    from hyrise_amd.distributed import HipExecutor
    rng = np.random.default_rng(11)
    kinds = ["value", "dictionary", "frame_of_reference", "run_length", "bit_packed"]
    chunk, n = 257, 257 * 5
    ints = np.repeat(rng.integers(-100, 100, n // 4 + 1), 4)[:n].astype(np.int32)
    int_nulls = np.repeat(rng.random(n // 4 + 1) < 0.1, 4)[:n]
    doubles = (rng.integers(-40, 40, n) / 8.0)
    double_nulls = rng.random(n) < 0.1
    host_i = storage.HostColumn([segment_of(ints[c * chunk:(c + 1) * chunk], int_nulls[c * chunk:(c + 1) * chunk], kind) for c, kind in enumerate(kinds)], abi.TYPE_INT)
    host_d = storage.HostColumn([segment_of(doubles[c * chunk:(c + 1) * chunk], double_nulls[c * chunk:(c + 1) * chunk], kind if kind != "frame_of_reference" else "dictionary")
                                 for c, kind in enumerate(kinds)], abi.TYPE_DOUBLE)
    i, d = DeviceColumn(host_i), DeviceColumn(host_d)
    resolve = {id(i): oracle.Column.of(ints, int_nulls), id(d): oracle.Column.of(doubles, double_nulls)}
    tree = lambda x, y: ("case", ("cmp", abi.PRED_GREATER_THAN_EQUALS, x, y), ("arith", abi.ARITH_MUL, x, ("arith", abi.ARITH_SUB, (INT, 1), y)), ("arith", abi.ARITH_MOD, x, (INT, 7)))
    check(tree(i, d), resolve, n, "data segments of every encoding")
    test = ColumnTest(i, make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, 10, nullable=True))
    resolve[id(test)] = oracle.Test(resolve[id(i)].cells, lambda cell: cell < 10)
    check(("case", test, d, (INT, 0)), resolve, n, "a numeric column test over every encoding")
    # host PosLists: one list over all chunks with NULL RowIDs; one list per chunk (every second row)
    picks = rng.integers(0, n, 700)
    pos = np.stack([picks // chunk, picks % chunk], axis=1).astype(np.uint32)
    null_rows = rng.random(len(picks)) < 0.1
    pos[null_rows] = 0xFFFFFFFF
    for lists, single, flat, null_ids in (([pos], [None], picks, null_rows),
                                          ([np.stack([np.full((chunk + 1) // 2, c), np.arange(0, chunk, 2)], axis=1).astype(np.uint32) for c in range(5)], list(range(5)),
                                           np.concatenate([c * chunk + np.arange(0, chunk, 2) for c in range(5)]), None)):
        null_ids = np.zeros(len(flat), dtype=bool) if null_ids is None else null_ids
        ri = DeviceColumn(storage.make_reference_column(host_i, lists, single), refs={id(host_i): i})
        rd = DeviceColumn(storage.make_reference_column(host_d, lists, single), refs={id(host_d): d})
        through = {id(ri): oracle.Column.of(ints[flat], int_nulls[flat] | null_ids), id(rd): oracle.Column.of(doubles[flat], double_nulls[flat] | null_ids)}
        check(tree(ri, rd), through, len(flat), f"host PosLists, single chunk ids {single}")
        referenced_test = ColumnTest(ri, make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, 10, nullable=True))
        through[id(referenced_test)] = oracle.Test(through[id(ri)].cells, lambda cell: cell < 10)
        check(("case", referenced_test, rd, (INT, 0)), through, len(flat), f"column test behind host PosLists {single}")
        null_test = ColumnTest(ri, make_predicate(abi.PRED_IS_NULL, abi.TYPE_INT, nullable=True))
        through[id(null_test)] = oracle.Test(through[id(ri)].cells, null_test="is_null")
        check(null_test, through, len(flat), "IS NULL behind PosLists never yields NULL")
    ex = HipExecutor(torch.device("cuda", 0))
    on_device = torch.from_numpy(pos.view(np.int32)).to("cuda")
    ri, rd = ex.reference_column(i, on_device, 300), ex.reference_column(d, on_device, 300)
    through = {id(ri): oracle.Column.of(ints[picks], int_nulls[picks] | null_rows), id(rd): oracle.Column.of(doubles[picks], double_nulls[picks] | null_rows)}
    check(tree(ri, rd), through, len(picks), "a device PosList with NULL RowIDs")


WORDS = [b"PROMO BRUSHED TIN", b"PROMO PLATED STEEL", b"STANDARD POLISHED TIN", b"ECONOMY ANODIZED BRASS", b"1-URGENT", b"2-HIGH", b"5-LOW", b""]


def string_table(rng, sizes):
    picks = [rng.integers(0, len(WORDS), sizes[0]), rng.integers(2, len(WORDS), sizes[1]), np.full(sizes[2], 3), rng.integers(0, 3, sizes[3])]   # chunk 1 holds no PROMO, chunk 2 one word
    segments, dictionaries, nulls = [], [], []
    for pick in picks:
        chunk_nulls = rng.random(len(pick)) < 0.15
        segment, dictionary = storage.encode_string_dictionary([WORDS[k] for k in pick], chunk_nulls)
        segments.append(segment)
        dictionaries.append(dictionary)
        nulls.append(chunk_nulls)
    flat, flat_nulls = np.concatenate(picks), np.concatenate(nulls)
    cells = [None if flat_nulls[k] else WORDS[flat[k]] for k in range(len(flat))]
    return storage.HostColumn(segments, abi.TYPE_STRING), dictionaries, cells


def string_tests(column, dictionaries, cells):
    """[(name, ColumnTest, oracle.Test)]: =, <>, <, LIKE 'PROMO%', IN, NOT IN, IS NULL over a dictionary string column."""
    out = []
    for name, condition, holds in (("=", abi.PRED_EQUALS, lambda s: s == b"1-URGENT"), ("<>", abi.PRED_NOT_EQUALS, lambda s: s != b"1-URGENT"), ("<", abi.PRED_LESS_THAN, lambda s: s < b"1-URGENT")):
        out.append((name, ColumnTest(column, string_predicate(condition, dictionaries, b"1-URGENT", nullable=True)), oracle.Test(cells, holds)))
    absent = string_predicate(abi.PRED_EQUALS, dictionaries, b"NO SUCH WORD", nullable=True)
    out.append(("= absent", ColumnTest(column, absent), oracle.Test(cells, lambda s: False)))
    like = make_predicate(abi.PRED_LIKE, abi.TYPE_STRING, nullable=True, dictionary_matches=[[w.startswith(b"PROMO") for w in dictionary] for dictionary in dictionaries])
    out.append(("like", ColumnTest(column, like), oracle.Test(cells, lambda s: s.startswith(b"PROMO"))))
    elements = [b"1-URGENT", b"2-HIGH", b"NO SUCH WORD", b""]
    for negated in (False, True):
        predicate = string_in_list_predicate(dictionaries, elements, negated=negated, nullable=True)
        out.append((f"in negated {negated}", ColumnTest(column, predicate), oracle.Test(cells, (lambda s: s not in elements) if negated else (lambda s: s in elements))))
    out.append(("is null", ColumnTest(column, make_predicate(abi.PRED_IS_NULL, abi.TYPE_STRING, nullable=True)), oracle.Test(cells, null_test="is_null")))
    return out


def test_column_tests_on_a_dictionary_string_column(device):
    """NULL cells come out NULL, not 0; a value absent from a chunk's dictionary; and the same predicate through hy_table_scan selects
    exactly the rows where the projection says 1."""
    rng = np.random.default_rng(13)
    sizes = (65, 300, 9, 64)
    host, dictionaries, cells = string_table(rng, sizes)
    column = DeviceColumn(host)
    n = sum(sizes)
    amount = DeviceColumn(storage.HostColumn([storage.encode_segment(np.arange(b, b + size, dtype=np.int32), None, abi.ENC_UNENCODED) for b, size in zip(np.cumsum((0,) + sizes[:-1]), sizes)], abi.TYPE_INT))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for name, test, oracle_test in string_tests(column, dictionaries, cells):
        resolve = {id(test): oracle_test, id(amount): oracle.Column.of(np.arange(n, dtype=np.int32))}
        got = check(test, resolve, n, f"string test {name}")
        values, nulls = got.read()
        if oracle_test.null_test is None:
            assert nulls.tolist() == [cell is None for cell in cells], f"NULL where the cell is NULL: {name}"
        check(("case", test, amount, (INT, 0)), resolve, n, f"CASE WHEN string test {name}")
        if not isinstance(test.predicate, abi.InList):
            scanned = table_scan(column, test.predicate, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
            rows = np.concatenate([starts[c] + scanned.pos_list(c)[:, 1].astype(np.int64) for c in range(len(sizes))])
            np.testing.assert_array_equal(rows, np.flatnonzero((values == 1) & ~nulls), err_msg=f"scan and projection agree: {name}")
    with pytest.raises(abi.HyriseAmdError) as error:
        projection_expression(ColumnTest(column, string_predicate(abi.PRED_BETWEEN_INCLUSIVE, dictionaries, b"1", b"3", nullable=True)))
    assert error.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(abi.HyriseAmdError) as error:
        projection_expression(("cmp", abi.PRED_EQUALS, column, column))
    assert error.value.status == abi.ERR_UNSUPPORTED


def test_q12_and_q14_shapes_into_aggregate_hash(device):
    """Q12: SUM(CASE WHEN o_orderpriority = '1-URGENT' OR o_orderpriority = '2-HIGH' THEN 1 ELSE 0 END); Q14: SUM(CASE WHEN p_type LIKE 'PROMO%'
    THEN l_extendedprice * (1 - l_discount) ELSE 0 END).  program -> hy_aggregate_hash(SUM); the Int sum is exact, the Double sum within
    hy_aggregate_hash's stated 1e-9 relative (its partial sums are added in another order than the oracle's)."""
    rng = np.random.default_rng(17)
    sizes = (1500, 1200, 300, 1000)
    n = sum(sizes)
    host, dictionaries, cells = string_table(rng, sizes)
    column = DeviceColumn(host)
    price = (rng.integers(90_000, 10_000_000, n) / 100.0).astype(np.float32)
    discount = (rng.integers(0, 11, n) / 100.0).astype(np.float32)
    split = lambda values: storage.HostColumn([storage.encode_segment(values[b:b + size], None, abi.ENC_UNENCODED) for b, size in zip(np.cumsum((0,) + sizes[:-1]), sizes)], storage.TYPE_OF_NP[values.dtype])
    p, d = DeviceColumn(split(price)), DeviceColumn(split(discount))
    resolve = {id(p): oracle.Column.of(price), id(d): oracle.Column.of(discount)}
    tests = {name: (test, oracle_test) for name, test, oracle_test in string_tests(column, dictionaries, cells)}
    urgent, like = tests["="], tests["like"]
    high = (ColumnTest(column, string_predicate(abi.PRED_EQUALS, dictionaries, b"2-HIGH", nullable=True)), oracle.Test(cells, lambda s: s == b"2-HIGH"))
    for test, oracle_test in (urgent, like, high):
        resolve[id(test)] = oracle_test
    q12 = ("case", ("or", urgent[0], high[0]), (INT, 1), (INT, 0))
    got = check(q12, resolve, n, "Q12 shape")
    result = aggregate_hash([], [(abi.AGG_SUM, got)])
    assert result.column(0) == [sum(1 for s in cells if s in (b"1-URGENT", b"2-HIGH"))]
    q14 = ("case", like[0], ("arith", abi.ARITH_MUL, p, ("arith", abi.ARITH_SUB, (INT, 1), d)), (INT, 0))
    got = check(q14, resolve, n, "Q14 shape")
    assert got.data_type == abi.TYPE_FLOAT
    _, want_cells = oracle.evaluate(q14, resolve, n)
    want_sum = float(np.sum(np.array([c for c in want_cells if c is not None], dtype=np.float64)))
    result = aggregate_hash([], [(abi.AGG_SUM, got)])
    assert abs(result.column(0)[0] - want_sum) <= 1e-9 * abs(want_sum)


def test_q1_charge_as_one_program_equals_the_chain_of_three_calls(device):
    """l_extendedprice * (1 - l_discount) * (1 + l_tax): one pass, bit-equal to three hy_projection_arithmetic calls; under both settings of
    HY_OPT_LDS_ORDERED_ATOMICS (the kernel uses no LDS atomics); and the result column scanned, sorted and gathered."""
    rng = np.random.default_rng(19)
    n, chunk = 20_001, 8_193
    price = (rng.integers(90_000, 10_000_000, n) / 100.0).astype(np.float32)
    discount, tax = (rng.integers(0, 11, n) / 100.0).astype(np.float32), (rng.integers(0, 9, n) / 100.0).astype(np.float32)
    p, d, t = (DeviceColumn(build_column(values, None, chunk, abi.ENC_UNENCODED)) for values in (price, discount, tax))
    one_minus = projection_arithmetic(abi.ARITH_SUB, (INT, 1), d)
    disc_price = projection_arithmetic(abi.ARITH_MUL, p, one_minus)
    one_plus = projection_arithmetic(abi.ARITH_ADD, (INT, 1), t)
    chain_values, chain_nulls = projection_arithmetic(abi.ARITH_MUL, disc_price, one_plus).read()
    tree = ("arith", abi.ARITH_MUL, ("arith", abi.ARITH_MUL, p, ("arith", abi.ARITH_SUB, (INT, 1), d)), ("arith", abi.ARITH_ADD, (INT, 1), t))
    assert projection_program(tree)[0].n_columns == 3
    for ordered in (1, 0):
        with abi.option(abi.OPT_LDS_ORDERED_ATOMICS, ordered):
            charge = projection_expression(tree)
            values, nulls = charge.read()
            assert values.dtype == np.float32 and values.tobytes() == chain_values.tobytes() and not nulls.any() and not chain_nulls.any(), f"ordered atomics {ordered}"
    want = ((price * (np.float32(1) - discount)) * (np.float32(1) + tax)).astype(np.float32)
    assert values.tobytes() == want.tobytes()
    # the result column like any other: hy_table_scan, hy_sort, hy_column_gather
    threshold = float(np.median(want))
    scanned = table_scan(charge, make_predicate(abi.PRED_GREATER_THAN, abi.TYPE_FLOAT, threshold, nullable=True), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    rows = np.concatenate([c * chunk + scanned.pos_list(c)[:, 1].astype(np.int64) for c in range(charge.n_chunks)])
    np.testing.assert_array_equal(rows, np.flatnonzero(want > np.float32(threshold)))
    positions = sort([charge], [abi.SORT_ASCENDING_NULLS_FIRST])
    order = positions.numpy()
    flat = order[:, 0].astype(np.int64) * chunk + order[:, 1]
    np.testing.assert_array_equal(flat, np.argsort(want, kind="stable"))
    gathered, gathered_nulls = column_gather(charge, positions).read()
    assert gathered.tobytes() == want[flat].tobytes() and not gathered_nulls.any()


@pytest.mark.parametrize("placement", ["natural", "last"])
def test_caller_owned_device_columns_at_odd_alignments(device, placement):
    rng = np.random.default_rng(23)
    n, chunk = 1_000, 333
    raw = raw_columns(rng, n)
    raw[abi.TYPE_FLOAT][raw[abi.TYPE_FLOAT] == 0] = 0.0   # (a dictionary holds one of -0.0 and 0.0: they are equal)
    nulls = {t: rng.random(n) < 0.1 for t in raw}
    hosts = {t: build_column(raw[t], nulls[t], chunk, [abi.ENC_UNENCODED, abi.ENC_DICTIONARY, abi.ENC_FRAME_OF_REFERENCE, abi.ENC_UNENCODED]) for t in raw}
    placed = {t: PlacedColumn(hosts[t], placement, 0xFF) for t in raw}
    resolve = {id(placed[t]): oracle.Column.of(raw[t], nulls[t]) for t in raw}
    i, l, f, d = (placed[t] for t in TYPES)
    test = ColumnTest(i, make_predicate(abi.PRED_GREATER_THAN, abi.TYPE_INT, 0, nullable=True))
    resolve[id(test)] = oracle.Test(resolve[id(i)].cells, lambda cell: cell > 0)
    tree = ("case", ("and", test, ("cmp", abi.PRED_LESS_THAN, f, d)), ("arith", abi.ARITH_ADD, l, i), ("arith", abi.ARITH_MUL, f, d))
    check(tree, resolve, n, f"placement {placement}")


def test_columns_of_two_tables_are_refused(device):
    a = DeviceColumn(build_column(np.arange(10, dtype=np.int32), None, 5, abi.ENC_UNENCODED))
    b = DeviceColumn(build_column(np.arange(10, dtype=np.int32), None, 4, abi.ENC_UNENCODED))
    with pytest.raises(abi.HyriseAmdError) as error:
        projection_expression(("arith", abi.ARITH_ADD, a, b))
    assert error.value.status == abi.ERR_INVALID
    program, keep = projection_program(("arith", abi.ARITH_ADD, a, a))
    assert program.n_columns == 1
    handle = C.c_void_p(1)
    program.nodes[0].index = 5
    assert device.hy_projection_expression(C.byref(program), C.byref(handle)) == abi.ERR_INVALID and not handle.value


def test_string_column_tests_behind_pos_lists(device):
    """The jobs of a column test belong to the DATA chunks: behind a PosList the RowID's chunk picks the job (value-id ranges and the value-id
    sets of LIKE / IN).  A host PosList over several chunks with NULL RowIDs, a device PosList with NULL RowIDs (what an outer join leaves),
    and a scan's own output in HBM (one PosList per chunk); a test that is used twice in a tree is one test of the program."""
    import torch
    from hyrise_amd.distributed import HipExecutor
    rng = np.random.default_rng(29)
    sizes = (65, 300, 9, 64)
    n = sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    host, dictionaries, cells = string_table(rng, sizes)
    column = DeviceColumn(host)
    amounts = np.arange(n, dtype=np.int32)
    amount_host = storage.HostColumn([storage.encode_segment(amounts[b:b + size], None, abi.ENC_UNENCODED) for b, size in zip(starts[:-1], sizes)], abi.TYPE_INT)
    amount = DeviceColumn(amount_host)
    picks = rng.integers(0, n, 500)
    chunk_of = np.searchsorted(starts, picks, side="right") - 1
    pos = np.stack([chunk_of, picks - starts[chunk_of]], axis=1).astype(np.uint32)
    null_rows = rng.random(len(picks)) < 0.1
    pos[null_rows] = 0xFFFFFFFF
    ex = HipExecutor(torch.device("cuda", 0))
    on_device = torch.from_numpy(pos.view(np.int32)).to("cuda")
    scanned = ex.scan_chunked(amount, make_predicate(abi.PRED_GREATER_THAN, abi.TYPE_INT, 30))   # rows 31 .. n - 1: a partial chunk, then whole ones
    kept = np.arange(31, n)
    cases = (("host PosList", DeviceColumn(storage.make_reference_column(host, [pos], [None]), refs={id(host): column}),
              DeviceColumn(storage.make_reference_column(amount_host, [pos], [None]), refs={id(amount_host): amount}), picks, null_rows),
             ("device PosList with NULL RowIDs", ex.reference_column(column, on_device, 200), ex.reference_column(amount, on_device, 200), picks, null_rows),
             ("a scan's output", ex.reference_column_chunked(column, scanned), ex.reference_column_chunked(amount, scanned), kept, np.zeros(len(kept), dtype=bool)))
    for name, through, amount_through, flat, null_ids in cases:
        through_cells = [None if null_ids[k] else cells[flat[k]] for k in range(len(flat))]
        assert through.rows == len(flat), name
        for test_name, test, oracle_test in string_tests(through, dictionaries, through_cells):
            resolve = {id(test): oracle_test, id(amount_through): oracle.Column.of(amounts[flat], null_ids)}
            tree = ("case", test, amount_through, ("case", ("is_null", test), (INT, -1), (INT, 0)))
            program, _ = projection_program(tree)
            assert program.n_tests == 1, "a reused test is one test"
            check(tree, resolve, len(flat), f"{name}: {test_name}")

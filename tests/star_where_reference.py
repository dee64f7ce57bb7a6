"""What hy_star_join_aggregate_where computes, in numpy: a plan as ssb.star_plan(columns, query, where=True) returns it -- built with
`columns = {name: name}`, so that it names its columns instead of holding device handles -- evaluated over plain arrays.  Shared by
test_ssb_queries_cpu.py (against SQLite) and test_star_where_gpu.py (the joined-row counts)."""
import ctypes as C

import numpy as np

from hyrise_amd import abi


def names(all_tables):
    """{name: name} over a {table: column names} schema: the `columns` argument that makes star_plan name its columns."""
    return {name: name for columns in all_tables.values() for name in columns}


def matches(values, test, nulls=None):
    """Rows of `values` that pass one filter (an abi.Predicate or an abi.InList over int32 literals); a NULL cell passes none."""
    if isinstance(test, abi.InList):
        literals = C.cast(test.values, C.POINTER(abi.Value))
        inside = np.isin(values, [literals[i].i32 for i in range(test.n_values)])
        out = ~inside if test.negated else inside
    else:
        low, high = test.value.i32, test.value2.i32
        out = {abi.PRED_EQUALS: lambda: values == low, abi.PRED_NOT_EQUALS: lambda: values != low, abi.PRED_LESS_THAN: lambda: values < low,
               abi.PRED_LESS_THAN_EQUALS: lambda: values <= low, abi.PRED_GREATER_THAN: lambda: values > low,
               abi.PRED_GREATER_THAN_EQUALS: lambda: values >= low, abi.PRED_BETWEEN_INCLUSIVE: lambda: (values >= low) & (values <= high)}[test.condition]()
    return out & ~nulls if nulls is not None else out


def evaluate(arrays, plan, nulls=None):
    """-> (rows left after the fact filters and every join, sorted [(GROUP BY values..., SUM)]) of a plan whose first aggregate is
    SUM(left [op right]) over fact-table columns.  arrays: {name: int array}; nulls: {name: bool array} of NULL cells (filter columns)."""
    nulls = nulls or {}
    dimensions, fact_filters, groupby, aggregates = plan
    n_fact = len(arrays[dimensions[0][2]])
    alive = np.ones(n_fact, dtype=bool)
    for name, test in fact_filters:
        alive &= matches(arrays[name], test, nulls.get(name))
    partner = []
    for key, filters, fact_key in dimensions:
        keys = arrays[key]
        keep = np.ones(len(keys), dtype=bool)
        for name, test in filters:
            keep &= matches(arrays[name], test, nulls.get(name))
        row_of_key = np.full(int(max(keys.max(), arrays[fact_key].max())) + 2, -1, dtype=np.int64)
        row_of_key[keys[keep]] = np.nonzero(keep)[0]
        rows = row_of_key[arrays[fact_key]]
        alive &= rows >= 0
        partner.append(rows)
    fact_rows = np.nonzero(alive)[0]

    def cells(table, name):
        return arrays[name][fact_rows if table == 0 else partner[table - 1][fact_rows]].astype(np.int64)

    function, left, op, right = aggregates[0]
    assert function == abi.AGG_SUM
    inputs = cells(*left)
    if op is not None:
        other = cells(*right)
        inputs = {abi.ARITH_ADD: inputs + other, abi.ARITH_SUB: inputs - other, abi.ARITH_MUL: inputs * other}[op]
    if not groupby:
        return len(fact_rows), [(int(inputs.sum()) if len(fact_rows) else None,)]
    keys = np.stack([cells(table, name) for table, name in groupby], axis=1) if len(fact_rows) else np.zeros((0, len(groupby)), dtype=np.int64)
    totals = {}
    for row, value in zip(map(tuple, keys.tolist()), inputs.tolist()):
        totals[row] = totals.get(row, 0) + value
    return len(fact_rows), sorted(key + (total,) for key, total in totals.items())


def sqlite_rows(data, query):
    """SQLite's rows for ssb.SQL[query] in evaluate()'s shape: sorted [(GROUP BY values in the plan's order..., SUM)]."""
    from hyrise_amd import ssb
    rows = data.sqlite_result(ssb.SQL[query])
    groupby = ssb.STAR_QUERIES[query][2]
    if not groupby:
        return [tuple(rows[0])]
    # which SQL output column holds which GROUP BY column: flights 2 / 3 / 4 put the sum first / last / last
    if query.startswith("2."):
        return sorted(tuple(r[1:]) + (r[0],) for r in rows)
    return sorted(tuple(r) for r in rows)


def bind(plan, columns):
    """A plan that names its columns -> the same plan over `columns` ({name: device column})."""
    dimensions, fact_filters, groupby, aggregates = plan
    column = lambda c: None if c is None else (c[0], columns[c[1]])
    return ([(columns[key], [(columns[name], test) for name, test in filters], columns[fact_key]) for key, filters, fact_key in dimensions],
            [(columns[name], test) for name, test in fact_filters], [(table, columns[name]) for table, name in groupby],
            [(function, column(left), op, column(right)) for function, left, op, right in aggregates])


def tuned_data():
    """SsbData(0.01, seed=7, lineorder_rows=50_001) with the supplier's and the customer's nations drawn from four codes (9 'UNITED STATES',
    19 'UNITED KINGDOM', 10 and 12 in ASIA) and their cities from two per nation (.. 1, .. 5): twenty suppliers of twenty-five nations leave
    Q2.2 and flight 3 without a row, four nations leave every query some."""
    from hyrise_amd import ssb
    data = ssb.SsbData(0.01, seed=7, lineorder_rows=50_001)
    rng = np.random.default_rng(5)
    for prefix, n in (("s", len(data.s_suppkey)), ("c", len(data.c_custkey))):
        nation = rng.choice(np.array([9, 19, 10, 12], dtype=np.int32), n)
        setattr(data, prefix + "_nation", nation)
        setattr(data, prefix + "_region", (nation // 5).astype(np.int32))
        setattr(data, prefix + "_city", (nation * 10 + rng.choice(np.array([1, 5], dtype=np.int32), n)).astype(np.int32))
    return data


def arrays_of(data):
    from hyrise_amd import ssb
    return {name: getattr(data, name) for columns in ssb.SsbData.ALL_TABLES.values() for name in columns}

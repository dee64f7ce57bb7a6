"""hy_star_join_aggregate_where on the device: the thirteen SSB queries as one call each -- fact-table filters inside the probe pass, up to four
filters and IN lists where a dimension's table is built, the aggregate without a GROUP BY column reduced inside the join -- against SQLite and a
numpy evaluation of the same plan, on each of the three paths (grouped inside the join; the fused probe and hy_aggregate_hash; the chain of
scans and joins).  lineorder: 50 001 rows in chunks of 20 000 -- three chunks, the last ragged, several 8192-row slices each."""
import numpy as np
import pytest

from hyrise_amd import abi, ssb, storage
from hyrise_amd.operators import aggregate_hash, in_list_predicate, make_predicate, star_join_aggregate, star_join_aggregate_where
import star_where_reference as reference

pytestmark = pytest.mark.gpu

PATHS = ((2, 1, 1), (1, 1, 0), (0, 0, 1))   # (hy_debug_star_fused(), HY_OPT_STAR_FUSED_PROBE, HY_OPT_STAR_FUSED_FINISH)
NAMES = reference.names(ssb.SsbData.ALL_TABLES)
INT = abi.TYPE_INT


def star_was_fused():
    lib = abi.load_library()
    lib.hy_debug_star_fused.restype = int
    return lib.hy_debug_star_fused()


def options():
    import ctypes as C
    values = []
    for option in (abi.OPT_STAR_FUSED_PROBE, abi.OPT_STAR_FUSED_FINISH):
        value = C.c_int64(-1)
        abi.check(abi.load_library().hy_get_option(option, C.byref(value)))
        values.append(value.value)
    return tuple(values)


def result_bytes(result, n_aggregates):
    """Everything the call wrote: the groups in their order, representative RowIDs, every cell with its type and NULL flag."""
    n = result.n_groups
    return (n, result.row_ids[:n].tobytes(), [(result.columns[a].data_type, result.raw[a][:n].tobytes(), result.nulls[a][:n].tobytes()) for a in range(n_aggregates)])


def rows_of(result, n_groupby):
    """The result in reference.evaluate's shape: sorted [(GROUP BY values..., SUM)]"""
    return sorted(key + (cells[0],) for key, cells in ssb.star_groups(result, n_groupby))


class World:
    def __init__(self):
        self.data = reference.tuned_data()
        self.arrays = reference.arrays_of(self.data)
        self.host = self.data.host_columns(chunk_size=20_000, tables=ssb.SsbData.ALL_TABLES)
        self.columns = {name: storage.DeviceColumn(column) for name, column in self.host.items()}
        self.expected = {}
        for query in ssb.QUERIES:   # computed once, on the host, before anything runs on the device
            joined, rows = reference.evaluate(self.arrays, ssb.star_plan(NAMES, query, where=True))
            assert rows == reference.sqlite_rows(self.data, query)
            assert joined > 0 and (len(rows) >= 2 or not ssb.STAR_QUERIES[query][2]), f"Q{query} is vacuous on this data"
            self.expected[query] = (joined, rows)

    def with_column(self, name, values, encoding, nulls=None):
        """The device columns with `name` made anew (another encoding, NULL cells)."""
        columns = dict(self.columns)
        if encoding == abi.ENC_RUN_LENGTH:
            host = storage.HostColumn([storage.encode_run_length(values[b:b + 20_000], None) for b in range(0, len(values), 20_000)], abi.TYPE_INT)
        else:
            host = storage.make_column(values, nulls, encoding, 20_000)
        columns[name] = storage.DeviceColumn(host)
        return columns

    def run(self, plan, columns=None):
        dimensions, fact_filters, groupby, aggregates = reference.bind(plan, columns or self.columns)
        result, joined = star_join_aggregate_where(dimensions, fact_filters, groupby, aggregates)
        return result, joined, len(groupby), len(aggregates)

    def check_on_every_path(self, plan, nulls=None, columns=None, fused=None):
        """The plan's rows and joined-row count against numpy on the three paths; `fused`: hy_debug_star_fused() per path, where it is known."""
        joined_want, rows_want = reference.evaluate(self.arrays, plan, nulls)
        for p, (want_fused, probe, finish) in enumerate(PATHS):
            with abi.option(abi.OPT_STAR_FUSED_PROBE, probe), abi.option(abi.OPT_STAR_FUSED_FINISH, finish):
                result, joined, n_groupby, _ = self.run(plan, columns)
            if fused is not None:
                assert star_was_fused() == fused[p]
            assert joined == joined_want and rows_of(result, n_groupby) == rows_want, f"path {want_fused}"
        return joined_want, rows_want


@pytest.fixture(scope="module")
def world(device):
    return World()


@pytest.mark.parametrize("query", ssb.QUERIES)
def test_query_on_every_path(world, query):
    joined_want, rows_want = world.expected[query]
    plan = ssb.star_plan(NAMES, query, where=True)
    before = options()
    same = {}
    for want_fused, probe, finish in PATHS:
        with abi.option(abi.OPT_STAR_FUSED_PROBE, probe), abi.option(abi.OPT_STAR_FUSED_FINISH, finish):
            result, joined, n_groupby, n_aggregates = world.run(plan)
        assert star_was_fused() == want_fused, f"Q{query}: path {want_fused}"
        assert joined == joined_want, f"Q{query}: joined rows on path {want_fused}"
        assert rows_of(result, n_groupby) == rows_want, f"Q{query}: groups and cells on path {want_fused}"
        assert not any(result.nulls[a][:result.n_groups].any() for a in range(n_aggregates))
        same[want_fused] = result_bytes(result, n_aggregates)
    # grouped inside the join vs hy_aggregate_hash over the survivors' exported cells: group order, representative rows, types, cells
    assert same[2] == same[1], f"Q{query}"
    assert options() == before == (1, 1)   # (abi.option put back what it found)


def empty_aggregate(n_groupby):
    """hy_aggregate_hash over no rows: SUM(x) [, MIN(g)] [GROUP BY g]"""
    empty = storage.DeviceColumn(storage.make_column(np.zeros(0, dtype=np.int32), None, abi.ENC_UNENCODED, 20_000))
    aggregates = [(abi.AGG_SUM, empty)] + [(abi.AGG_MIN, empty)] * n_groupby
    return aggregate_hash([empty] * n_groupby, aggregates, group_capacity=4096), len(aggregates)


@pytest.mark.parametrize("n_groupby", [0, 1])
def test_fact_filter_that_matches_nothing(world, n_groupby):
    want, n_aggregates = empty_aggregate(n_groupby)
    assert want.n_groups == (1 if n_groupby == 0 else 0)
    groupby = [(2, "d_year")][:n_groupby]
    plan = ([("p_partkey", [], "lo_partkey"), ("d_datekey", [], "lo_orderdate")], [("lo_quantity", make_predicate(abi.PRED_LESS_THAN, INT, 1))], groupby,
            [(abi.AGG_SUM, (0, "lo_revenue"), None, None)] + [(abi.AGG_MIN, g, None, None) for g in groupby])
    for want_fused, probe, finish in PATHS:
        with abi.option(abi.OPT_STAR_FUSED_PROBE, probe), abi.option(abi.OPT_STAR_FUSED_FINISH, finish):
            result, joined, _, _ = world.run(plan)
        assert star_was_fused() == want_fused and joined == 0
        assert result_bytes(result, n_aggregates) == result_bytes(want, n_aggregates), f"path {want_fused}"


def test_null_cells_of_a_fact_filter_column_drop_the_row(world):
    nulls = np.arange(world.data.n_lineorder) % 7 == 3
    columns = world.with_column("lo_quantity", world.data.lo_quantity, abi.ENC_UNENCODED, nulls)
    plan = ssb.star_plan(NAMES, "1.1", where=True)
    joined, _ = world.check_on_every_path(plan, nulls={"lo_quantity": nulls}, columns=columns, fused=(2, 1, 0))
    assert 0 < joined < world.expected["1.1"][0]
    # ... NOT IN as well: a NULL cell is in no list and outside none
    plan = (plan[0], [("lo_quantity", in_list_predicate(INT, [1, 2, 3], negated=True, nullable=True))], plan[2], plan[3])
    world.check_on_every_path(plan, nulls={"lo_quantity": nulls}, columns=columns, fused=(2, 1, 0))


def test_not_in_on_a_dimension(world):
    groupby = [(2, "d_year"), (1, "p_mfgr")]
    plan = ([("p_partkey", [("p_mfgr", in_list_predicate(INT, [3, 5, 4, 3], negated=True))], "lo_partkey"), ("d_datekey", [], "lo_orderdate")], [], groupby,
            [(abi.AGG_SUM, (0, "lo_revenue"), abi.ARITH_SUB, (0, "lo_supplycost"))] + [(abi.AGG_MIN, g, None, None) for g in groupby])
    _, rows = world.check_on_every_path(plan, fused=(2, 1, 0))
    assert {row[1] for row in rows} == {1, 2}


def test_four_filters_on_one_dimension(world):
    filters = [("p_mfgr", make_predicate(abi.PRED_BETWEEN_INCLUSIVE, INT, 2, 3)), ("p_category", make_predicate(abi.PRED_NOT_EQUALS, INT, 22)),
               ("p_brand1", in_list_predicate(INT, list(range(1101, 3541, 10)))), ("p_partkey", make_predicate(abi.PRED_LESS_THAN, INT, 1800))]
    groupby = [(1, "p_category")]
    plan = ([("p_partkey", filters, "lo_partkey"), ("s_suppkey", [("s_region", make_predicate(abi.PRED_GREATER_THAN_EQUALS, INT, 2))], "lo_suppkey")],
            [("lo_discount", make_predicate(abi.PRED_GREATER_THAN, INT, 2))], groupby,
            [(abi.AGG_SUM, (0, "lo_extendedprice"), abi.ARITH_MUL, (0, "lo_discount"))] + [(abi.AGG_MIN, g, None, None) for g in groupby])
    joined, rows = world.check_on_every_path(plan, fused=(2, 1, 0))
    assert joined > 0 and len(rows) >= 2 and 22 not in {row[0] for row in rows}
    # each of the four filters matters: without any one of them more rows survive
    for k in range(4):
        fewer = ([("p_partkey", filters[:k] + filters[k + 1:], "lo_partkey"), plan[0][1]], plan[1], plan[2], plan[3])
        assert reference.evaluate(world.arrays, fewer)[0] > joined


def test_dictionary_encoded_fact_filter_column(world):
    columns = world.with_column("lo_discount", world.data.lo_discount, abi.ENC_DICTIONARY)
    for query in ("1.1", "1.3"):
        world.check_on_every_path(ssb.star_plan(NAMES, query, where=True), columns=columns, fused=(2, 1, 0))
    plan = ssb.star_plan(NAMES, "1.2", where=True)   # ... and as a list of value ids' values
    plan = (plan[0], [("lo_discount", in_list_predicate(INT, [6, 4, 5, 40])), plan[1][1]], plan[2], plan[3])
    joined, rows = world.check_on_every_path(plan, columns=columns, fused=(2, 1, 0))
    assert (joined, rows) == world.expected["1.2"]


def test_run_length_filter_column_takes_the_chain(world):
    """A fact filter column the probe pass does not read: the scans and joins of the chain, the same groups."""
    columns = world.with_column("lo_quantity", world.data.lo_quantity, abi.ENC_RUN_LENGTH)
    for query in ("1.1", "1.2"):
        world.check_on_every_path(ssb.star_plan(NAMES, query, where=True), columns=columns, fused=(0, 0, 0))
    groupby = [(1, "d_year")]
    plan = ([("d_datekey", [("d_year", make_predicate(abi.PRED_BETWEEN_INCLUSIVE, INT, 1993, 1995))], "lo_orderdate")],
            [("lo_quantity", make_predicate(abi.PRED_LESS_THAN, INT, 25)), ("lo_discount", in_list_predicate(INT, [1, 2, 3]))], groupby,
            [(abi.AGG_SUM, (0, "lo_revenue"), None, None)] + [(abi.AGG_MIN, g, None, None) for g in groupby])
    _, rows = world.check_on_every_path(plan, columns=columns, fused=(0, 0, 0))
    assert [row[0] for row in rows] == [1993, 1994, 1995]
    assert world.check_on_every_path(plan, fused=(2, 1, 0))[1] == rows   # (the plain column: inside the probe)


@pytest.mark.parametrize("query", ["2.1", "4.1"])
def test_old_entry_point_and_new_agree(world, query):
    old_dimensions, old_groupby, old_aggregates = ssb.star_plan(world.columns, query)
    plan = ssb.star_plan(NAMES, query, where=True)
    for want_fused, probe, finish in PATHS:
        with abi.option(abi.OPT_STAR_FUSED_PROBE, probe), abi.option(abi.OPT_STAR_FUSED_FINISH, finish):
            old, old_joined = star_join_aggregate(old_dimensions, old_groupby, old_aggregates)
            old_fused = star_was_fused()
            new, new_joined, _, n_aggregates = world.run(plan)
            assert star_was_fused() == old_fused == want_fused
        assert new_joined == old_joined == world.expected[query][0]
        assert result_bytes(new, n_aggregates) == result_bytes(old, len(old_aggregates)), f"Q{query}: path {want_fused}"

"""hy_star_join_aggregate_where's argument checks: they come before anything touches a device -- these calls are made without one -- and leave
a message; nothing is written."""
import ctypes as C

from hyrise_amd import abi


def call(dimensions, n_dimensions, fact_filters, n_fact_filters, groupby=None, n_groupby=0, aggregates=None, n_aggregates=1, result=True):
    lib = abi.load_library()
    out = abi.AggregateResult()
    out.n_groups = 77
    joined = C.c_uint64(77)
    aggregates = (abi.StarAggregate * 1)() if aggregates is None else aggregates
    status = lib.hy_star_join_aggregate_where(dimensions, n_dimensions, fact_filters, n_fact_filters, groupby, n_groupby, aggregates, n_aggregates,
                                              C.byref(out) if result else None, C.byref(joined))
    assert out.n_groups == 77 and joined.value == 77   # nothing is written on error
    return status, (lib.hy_last_error() or b"").decode()


def test_binding_matches_the_header():
    assert "hy_star_join_aggregate_where" in {name for name, _, _ in abi.SYMBOLS} and hasattr(abi.load_library(), "hy_star_join_aggregate_where")
    assert abi.MAX_STAR_FILTERS == 4
    assert C.sizeof(abi.StarFilter) == 8 + C.sizeof(abi.Predicate) + 8 and C.sizeof(abi.StarDimensionWhere) == 32


def test_null_arguments_are_invalid():
    dimensions, filters = (abi.StarDimensionWhere * 1)(), (abi.StarFilter * 1)()
    assert call(None, 1, None, 0)[0] == abi.ERR_INVALID
    assert call(dimensions, 1, None, 1)[0] == abi.ERR_INVALID                        # fact filters announced, none given
    assert call(dimensions, 1, None, 0, None, 1)[0] == abi.ERR_INVALID               # GROUP BY columns announced, none given
    assert call(dimensions, 1, None, 0, result=False)[0] == abi.ERR_INVALID
    assert call(dimensions, 1, filters, 1)[0] == abi.ERR_INVALID                     # a dimension without key columns
    dimensions[0].n_filters = 1
    assert call(dimensions, 1, None, 0)[0] == abi.ERR_INVALID                        # a dimension's filters announced, none given


def test_dimension_count():
    dimensions = (abi.StarDimensionWhere * 9)()
    for n in (0, 9):
        status, message = call(dimensions, n, None, 0)
        assert status == abi.ERR_INVALID and "dimensions" in message


def test_more_filters_than_a_table_takes():
    dimensions, filters = (abi.StarDimensionWhere * 1)(), (abi.StarFilter * 5)()
    status, message = call(dimensions, 1, filters, 5)
    assert status == abi.ERR_UNSUPPORTED and "5 filters on the fact table" in message
    dimensions[0].filters, dimensions[0].n_filters = filters, 5
    status, message = call(dimensions, 1, None, 0)
    assert status == abi.ERR_UNSUPPORTED and "dimension 0" in message and "5 filters" in message


def test_nothing_to_aggregate():
    dimensions = (abi.StarDimensionWhere * 1)()
    assert call(dimensions, 1, None, 0, n_aggregates=0)[0] == abi.ERR_INVALID

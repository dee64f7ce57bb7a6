"""hyrise_amd/ssb.py without a device: the generator still makes the columns it made before it learnt the thirteen queries' columns, and every
query's plan (ssb.star_plan(..., where=True): what hy_star_join_aggregate_where is given) means what its SQL text means -- the plan evaluated in
numpy against SQLite over the same tables."""
import hashlib

import pytest

from hyrise_amd import ssb
import star_where_reference as reference

# sha256 (first sixteen hex digits) of every column of SsbData(0.01, seed=7, lineorder_rows=50_001) as the commit before this file generated it
PARENT_COLUMNS = {
    "c_custkey": (300, "d1c1a7d9abac10c9"), "c_nation": (300, "a0e5ece468bd1fde"), "c_region": (300, "62a76937ee6e2401"),
    "d_datekey": (2557, "cec196013e7c916e"), "d_year": (2557, "4649b2a3afeba22a"),
    "lo_custkey": (50001, "937db4bf171474da"), "lo_orderdate": (50001, "38b5a2bb7180c4bc"), "lo_partkey": (50001, "d25317409ae0e2ff"),
    "lo_revenue": (50001, "bf020fef9d31b66c"), "lo_suppkey": (50001, "b1413b8455ab09aa"), "lo_supplycost": (50001, "ad678e0b4aa2edc3"),
    "p_brand1": (2000, "6e78c3bda0b4ecb4"), "p_category": (2000, "5aab305ca20d0cac"), "p_mfgr": (2000, "695a170a268271bc"), "p_partkey": (2000, "0aa3ebcdbd4feafe"),
    "s_nation": (20, "df552ec7ae0158cc"), "s_region": (20, "3d4e1addb500a81b"), "s_suppkey": (20, "3d499aab79d40fad"),
}


@pytest.fixture(scope="module")
def plain():
    return ssb.SsbData(0.01, seed=7, lineorder_rows=50_001)


@pytest.fixture(scope="module")
def tuned():
    return reference.tuned_data()


def test_earlier_columns_are_byte_identical(plain):
    assert {name for names in ssb.SsbData.TABLES.values() for name in names} == set(PARENT_COLUMNS)
    for name, (rows, digest) in PARENT_COLUMNS.items():
        column = getattr(plain, name)
        assert column.dtype == "int32" and len(column) == rows and hashlib.sha256(column.tobytes()).hexdigest()[:16] == digest, name


def test_new_columns_follow_the_conventions(plain):
    assert (plain.c_city // 10 == plain.c_nation).all() and (plain.s_city // 10 == plain.s_nation).all()
    assert set(plain.c_city % 10) == set(range(10))
    assert (plain.d_yearmonthnum == plain.d_datekey // 100).all()
    assert plain.d_weeknuminyear.min() == 1 and plain.d_weeknuminyear.max() == 53 and (plain.d_weeknuminyear[:7] == 1).all() and plain.d_weeknuminyear[7] == 2
    assert (plain.lo_extendedprice.astype("int64") * (100 - plain.lo_discount) // 100 == plain.lo_revenue).all()
    assert plain.lo_quantity.min() == 1 and plain.lo_quantity.max() == 50 and plain.lo_discount.min() == 0 and plain.lo_discount.max() == 10
    assert set(ssb.SsbData.ALL_TABLES) == set(ssb.SsbData.TABLES) and all(set(ssb.SsbData.TABLES[t]) <= set(ssb.SsbData.ALL_TABLES[t]) for t in ssb.SsbData.TABLES)
    assert set(plain.host_columns()) == set(PARENT_COLUMNS)   # (what the benchmark encodes and uploads stays what it was)


def test_there_are_thirteen_queries():
    assert ssb.QUERIES == ("1.1", "1.2", "1.3", "2.1", "2.2", "2.3", "3.1", "3.2", "3.3", "3.4", "4.1", "4.2", "4.3") and set(ssb.STAR_QUERIES) == set(ssb.SQL)


@pytest.mark.parametrize("query", ssb.QUERIES)
def test_plan_means_what_the_sql_means(plain, tuned, query):
    plan = ssb.star_plan(reference.names(ssb.SsbData.ALL_TABLES), query, where=True)
    for data in (plain, tuned):
        joined, rows = reference.evaluate(reference.arrays_of(data), plan)
        assert rows == reference.sqlite_rows(data, query)
    # the second data set is the device test's: no query may be vacuous on it
    assert joined > 0 and (len(rows) >= 2 or not ssb.STAR_QUERIES[query][2])


def test_old_plans_are_what_they_were(plain):
    names = reference.names(ssb.SsbData.ALL_TABLES)
    for query in ("2.1", "4.1"):
        dimensions, groupby, aggregates = ssb.star_plan(names, query)
        assert len(dimensions) == len(ssb.STAR_QUERIES[query][0]) and [name for _, name in groupby] == ssb.STAR_QUERIES[query][2]
    with pytest.raises(ValueError):
        ssb.star_plan(names, "1.1")

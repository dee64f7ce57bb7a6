"""Every route of AggregateHash's host side (csrc/aggregate.hip, DESIGN.md 4.3 "Routes") taken once, against the CPU oracle, with the route
asserted through the debug accessors: (hy_debug_aggregate_path, hy_debug_aggregate_small_domain, hy_debug_aggregate_finished_on_device).
The expected triples were read off the library before its host side was split into stages and are written as literals: the test passes with
that library and with this one -- which is what it is for.  Small worlds: chunks of 65 535 / 65 535 / remainder, or 300 / 257 / 1 where the row
count does not matter.

Routes not reached from here:
  * `n_groups > out_capacity` (next_step's second way to a larger table): direct groups plus the global table's would have to exceed rows + 1.
  * the give-up at 14 bits into "unlimited" (next_step's third arm): 2^14 partitions whose LDS tables still lose more than
    max(65 536, rows / 16) rows need millions of rows, nearly each its own group.
  * the table-size ladder beyond its second rung (2 Mi slots hold a million groups), its last rung's two errors ("overflowed at two slots per
    row", "more groups than rows"), "the device group table did not settle" after twelve rounds, and "too many rows for the device group
    table" (2^31 slots): internal errors and sizes no test of a few seconds has.
  * sd_wide skipped by SmallDomainPlan::debug: HY_AGG_SMALL_DEBUG is a timing aid of a -DHY_DEBUG_SWITCHES build, not of the library under test.
  * FIXED_AGG_SPLIT, a compile-time constant (the automatic split > 1 IS covered: test_partitions_shared_by_several_workgroups).
  * t_aggregate_next_path (a star plan telling the call where to start): hy_star_join_aggregate's second call needs an SSB-sized world to
    end on the partitioned path; tests/test_star_where_gpu.py and the SSB workload run it.  The column hint, the other way, is covered.
  * sort keys of 2^32 and more on the device finish (download after all): needs more than 2^32 rows or keys spread that far with the
    immediate-key shortcut still on.
  * results beyond 16 MiB on the device finish into a host result (device arrays and one copy each, not the pinned block).
  * of the refusals: "more than %u device accumulators" (the entry points split such a call into passes before run_aggregate sees it) and
    "more than %u aggregates" (the same).
sd_groups alone and sd_groups + sd_wide report the same triple; that sd_wide ran shows in the launch lists (profiles/aggregate_host_stages.txt)
and in the result: only sd_wide reads the 2-byte column."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.operators import HostAggregateResult, aggregate_hash
from hyrise_amd.storage import DeviceColumn
from support import build_column, oracle_aggregate, oracle_chain
from test_aggregate_gpu import assert_aggregate_equal, ragged_column, run_both
from test_fused_gpu import assert_matches_chain

pytestmark = pytest.mark.gpu
CHUNK = 65_535
SMALL_SIZES = [300, 257, 1]
SMALL_CHUNKS = sum(SMALL_SIZES)


def route(lib):
    for name in ("hy_debug_aggregate_path", "hy_debug_aggregate_small_domain", "hy_debug_aggregate_finished_on_device"):
        getattr(lib, name).restype = int
    return lib.hy_debug_aggregate_path(), lib.hy_debug_aggregate_small_domain(), lib.hy_debug_aggregate_finished_on_device()


def column(values, nulls=None, chunk=CHUNK, encoding=abi.ENC_UNENCODED):
    return build_column(values, nulls, chunk, encoding)


def small(values, nulls=None):
    return ragged_column(values, nulls, SMALL_SIZES, abi.ENC_UNENCODED)


def small_world(seed=1):
    """558 rows in chunks of 300 / 257 / 1"""
    rng = np.random.default_rng(seed)
    n = SMALL_CHUNKS
    return {"key": small(rng.integers(0, 5, n).astype(np.int32) * 1000, rng.random(n) < 0.05),
            "ints": small(rng.integers(-50, 50, n).astype(np.int32), rng.random(n) < 0.1),
            "doubles": small(rng.normal(100.0, 5.0, n))}


def q1_world(n=2 * CHUNK + 1000, prices=200, seed=3):
    """Dictionary columns: two 1-byte keys (four groups), a 1-byte and a 2-byte numeric input."""
    rng = np.random.default_rng(seed)
    return {"flag": column(rng.integers(0, 2, n).astype(np.int64), None, CHUNK, abi.ENC_DICTIONARY),
            "status": column(rng.integers(0, 2, n).astype(np.int64), None, CHUNK, abi.ENC_DICTIONARY),
            "quantity": column(rng.integers(1, 51, n).astype(np.float32), None, CHUNK, abi.ENC_DICTIONARY),
            "price": column((rng.integers(0, prices, n) / 4.0).astype(np.float32), None, CHUNK, abi.ENC_DICTIONARY)}


def many_groups_world(n=140_000, distinct=None, seed=9, dense=False):
    """About 140 000 rows, nearly each its own group: more than 65 536 rows leave aggregate_rows' LDS tables (its spill limit's floor)."""
    rng = np.random.default_rng(seed)
    keys = rng.permutation(n).astype(np.int32) if distinct is None else rng.integers(0, distinct, n).astype(np.int32)
    if not dense:
        keys = keys * 13 - 70_000
    return {"key": column(keys), "ints": column(rng.integers(-1000, 1000, n).astype(np.int32), rng.random(n) < 0.1),
            "longs": column(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)), "doubles": column(rng.random(n) * 1e3)}


PLAIN = [(abi.AGG_SUM, "ints"), (abi.AGG_AVG, "doubles"), (abi.AGG_MIN, "ints"), (abi.AGG_MAX, "doubles"), (abi.AGG_COUNT, None)]


def specs(world, aggregates):
    return [(f, world[name] if name else None) for f, name in aggregates]


# ---- aggregate_rows ----------------------------------------------------------------------------------------------------------------------
def test_rows_few_groups_host_finish(device):
    w = small_world()
    run_both([w["key"]], specs(w, PLAIN), "five groups")
    assert route(device) == (0, 0, 0)
    got = run_both([], [(abi.AGG_COUNT, None), (abi.AGG_SUM, w["ints"])], "lone COUNT(*) first: the shape is the SUM's column")
    assert route(device) == (0, 0, 0) and got.n_groups == 1 and got.column(0) == [SMALL_CHUNKS]


def test_no_group_by_over_an_empty_input(device):
    empty = column(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=bool), 300)
    got = run_both([], [(abi.AGG_SUM, empty), (abi.AGG_COUNT, empty), (abi.AGG_COUNT, None), (abi.AGG_MIN, empty)], "empty input")
    assert got.n_groups == 1 and got.column(0) == [None] and got.column(1) == [0] and got.column(2) == [0] and got.column(3) == [None]
    assert route(device) == (0, 0, 0)


def test_rows_over_a_reference_table(device):
    """reference columns with PosLists in HBM: aggregate_rows caches the slice's PosList offsets (AggArgs::pos_cache)"""
    import torch
    from hyrise_amd import storage
    from hyrise_amd.distributed import HipExecutor
    from hyrise_amd.operators import make_predicate, table_scan
    rng = np.random.default_rng(21)
    n, chunk = 20_000, 6_000
    host = {"key": storage.make_column(rng.integers(0, 300, n).astype(np.int32) * 3, None, abi.ENC_DICTIONARY, chunk),
            "value": storage.make_column(rng.integers(-1000, 1000, n).astype(np.int32), rng.random(n) < 0.1, abi.ENC_UNENCODED, chunk),
            "pick": storage.make_column((rng.random(n) < 0.7).astype(np.int32), None, abi.ENC_UNENCODED, chunk)}
    data = {name: DeviceColumn(c) for name, c in host.items()}
    predicate = make_predicate(abi.PRED_EQUALS, abi.TYPE_INT, 1)
    lists = HipExecutor(torch.device("cuda:0")).scan_chunked(data["pick"], predicate)
    ref = {name: HipExecutor(torch.device("cuda:0")).reference_column_chunked(c, lists) for name, c in data.items()}
    on_host = table_scan(data["pick"], predicate)
    host_lists = [on_host.pos_list(c).copy() for c in range(data["pick"].n_chunks)]
    host_ref = {name: storage.make_reference_column(c, host_lists, list(range(c.n_chunks))) for name, c in host.items()}
    aggregates = [(abi.AGG_SUM, "value"), (abi.AGG_COUNT, None), (abi.AGG_MIN, "value")]
    got = aggregate_hash([ref["key"]], specs(ref, aggregates))
    assert_aggregate_equal(got, oracle_aggregate([host_ref["key"]], specs(host_ref, aggregates)), 3, "reference table")
    assert route(device) == (0, 0, 0) and got.n_groups == 300


# ---- the small-domain kernels ------------------------------------------------------------------------------------------------------------
def test_small_domain_narrow_and_wide(device):
    w = q1_world()
    run_both([w["flag"], w["status"]], specs(w, [(abi.AGG_SUM, "quantity"), (abi.AGG_AVG, "quantity"), (abi.AGG_COUNT, None)]), "sd_groups alone")
    assert route(device) == (0, 1, 0)
    wide = q1_world(prices=20_000)   # (more than 255 prices per chunk: 2-byte value ids)
    run_both([wide["flag"], wide["status"]], specs(wide, [(abi.AGG_SUM, "quantity"), (abi.AGG_SUM, "price"), (abi.AGG_MIN, "price"), (abi.AGG_COUNT, None)]), "sd_groups + sd_wide")
    assert route(device) == (0, 1, 0)


def test_small_domain_refused_at_run_time(device):
    """a 2-byte column's value that forty rows of one group share inside one chunk overflows sd_wide's 4-bit counter: FLAG_SMALL_REFUSED,
    the same round again with aggregate_rows -- the accessor reports 0, the result is the oracle's"""
    n = 60_000
    price = (np.arange(n) % 50_000 * 1.37 + 900.0).astype(np.float32)
    price[np.random.default_rng(5).choice(n, 40, replace=False)] = 123.5
    key = column(np.zeros(n, np.int32), None, CHUNK, abi.ENC_DICTIONARY)
    repeated = column(price, None, CHUNK, abi.ENC_DICTIONARY)
    assert repeated.segments[0].width == 2
    got = run_both([key], [(abi.AGG_SUM, repeated), (abi.AGG_COUNT, None)], "a value forty times in one group of one chunk")
    assert route(device) == (0, 0, 0) and got.n_groups == 1


def fused_q1(lib, **table_arguments):
    from test_fused_small_gpu import plans, run, table
    hosts, plan = table(**table_arguments), plans()[0]
    got, _ = run(lib, hosts, plan)
    assert_matches_chain(got, oracle_chain(*plan.on(hosts)), len(plan.aggregates), f"fused q1 {table_arguments}")
    return got


def test_fused_routes(device, options):
    fused_q1(device, n=25_000, chunk=10_000)
    assert route(device) == (0, 2, 0)   # fused_small_domain
    fused_q1(device, n=25_000, chunk=10_000, flags=3)
    assert route(device) == (0, 0, 0)   # a fifth group in a chunk: refused at run time, fused_rows
    fused_q1(device, n=25_000, chunk=10_000, null_share=0.05)
    assert route(device) == (0, 0, 0)   # a NULL input: the same
    options.set(abi.OPT_FUSED_SMALL_DOMAIN, 0)
    fused_q1(device, n=25_000, chunk=10_000)
    assert route(device) == (0, 0, 0)   # fused_rows from the start


# ---- retries -----------------------------------------------------------------------------------------------------------------------------
def test_table_overflow_ladder_where_nothing_partitions(device):
    """nine GROUP BY columns (the seventeen-word build keeps to aggregate_rows) and 70 000 groups: the 64 Ki-slot table overflows, 2 Mi slots hold"""
    w = many_groups_world(distinct=70_000)
    n = w["key"].rows
    constants = [column(np.full(n, i, dtype=np.int32)) for i in range(8)]
    got = run_both([w["key"]] + constants, specs(w, [(abi.AGG_SUM, "ints"), (abi.AGG_COUNT, None)]), "nine GROUP BY columns")
    assert got.n_groups > 60_000
    assert route(device) == (0, 0, 1)


def test_give_up_into_the_partitioned_path_and_the_remembered_start(device, options):
    w = many_groups_world()
    groupby, aggregates = [DeviceColumn(w["key"])], [(f, DeviceColumn(c) if c is not None else None) for f, c in specs(w, PLAIN[:2] + PLAIN[4:])]
    want = oracle_aggregate([w["key"]], specs(w, PLAIN[:2] + PLAIN[4:]))
    routes = []
    for call in range(2):   # the second call over the same device columns starts where the first ended (the column hint): the same route, the same result
        got = aggregate_hash(groupby, aggregates)
        assert_aggregate_equal(got, want, 3, f"give-up, call {call}")
        routes.append(route(device))
    assert routes == [(14, 0, 1), (14, 0, 1)]
    options.set(abi.OPT_AGG_PARTITION_BITS, 3)   # forced start: 2^3 partitions of 17 500 groups each give up to 14 bits
    run_both([w["key"]], specs(w, PLAIN[:2] + PLAIN[4:]), "forced 3 bits")
    assert route(device) == (14, 0, 1)
    options.set(abi.OPT_AGG_PARTITION_BITS, 9)
    fewer = many_groups_world(distinct=20_000, seed=10)
    run_both([fewer["key"]], specs(fewer, PLAIN), "forced 9 bits, narrow records")
    assert route(device) == (9, 0, 1)
    run_both([fewer["key"]], specs(fewer, [(abi.AGG_SUM, "longs"), (abi.AGG_COUNT, None)]), "forced 9 bits, wide records")
    assert route(device) == (9, 0, 1)


def test_partitions_shared_by_several_workgroups(device, options):
    """A few hundred groups over 140 000 rows at one and two forced bits: 70 000 / 35 000 rows per partition are shared by eight / four
    workgroups (PartitionArgs::split > 1), whose groups meet in the global table -- no direct groups.  Narrow and wide records."""
    w = many_groups_world(distinct=500, seed=14)
    for bits in (1, 2):
        options.set(abi.OPT_AGG_PARTITION_BITS, bits)
        got = run_both([w["key"]], specs(w, [(abi.AGG_SUM, "ints"), (abi.AGG_MIN, "ints"), (abi.AGG_COUNT, None)]), f"forced {bits} bits, narrow records")
        assert route(device) == (bits, 0, 0) and got.n_groups == 500
        run_both([w["key"]], specs(w, [(abi.AGG_SUM, "longs"), (abi.AGG_AVG, "doubles"), (abi.AGG_COUNT, None)]), f"forced {bits} bits, wide records")
        assert route(device) == (bits, 0, 0)


def test_the_start_path_is_remembered_by_the_columns(device):
    """300 groups over 60 000 rows: aggregate_rows runs to the end (path 0) with more groups than its LDS tables have slots, so the first
    GROUP BY column remembers 4 bits; the second call over the same device columns starts there (path 4); the same data in fresh device
    columns has another signature and no hint: path 0 again.  The same result every time."""
    rng = np.random.default_rng(15)
    n = 60_000
    w = {"key": column(rng.integers(0, 300, n).astype(np.int32) * 17 - 999), "ints": column(rng.integers(-1000, 1000, n).astype(np.int32), rng.random(n) < 0.1)}
    aggregates = [(abi.AGG_SUM, "ints"), (abi.AGG_COUNT, None)]
    want = oracle_aggregate([w["key"]], specs(w, aggregates))
    routes = []
    for columns in ({name: DeviceColumn(c) for name, c in w.items()}, None, {name: DeviceColumn(c) for name, c in w.items()}):
        kept = columns or kept
        assert_aggregate_equal(aggregate_hash([kept["key"]], specs(kept, aggregates)), want, 2, f"call {len(routes)}")
        routes.append(route(device))
    assert routes == [(0, 0, 0), (4, 0, 0), (0, 0, 0)]


# ---- the finishes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["first_row", "immediate"])
def test_device_finish_into_a_host_result(device, order):
    w = many_groups_world(distinct=20_000, seed=12, dense=order == "immediate")
    got = run_both([w["key"]], specs(w, PLAIN), order)
    assert got.n_groups > 19_000 and route(device)[2] == 1


def test_column_sink_device_finish_and_host_finish(device):
    from test_aggregate_columns_gpu import Col, check
    rng = np.random.default_rng(31)
    n = 60_000
    large = Col(rng.integers(0, 6_000, n).astype(np.int32) * 7)
    few = Col(rng.integers(0, 40, n).astype(np.int32) * 7)
    # (quarters: their sums are exact in any order, so the two entry points' separate device passes agree byte for byte)
    ints, doubles = Col(rng.integers(-100, 100, n).astype(np.int32), rng.random(n) < 0.1), Col(rng.integers(-4000, 4000, n) / 4.0)
    plain = [(abi.AGG_SUM, ints), (abi.AGG_AVG, doubles), (abi.AGG_COUNT, None)]
    check(device, [large], plain, 1000, "sink, device finish")
    assert route(device)[2] == 1
    check(device, [few], plain, 1000, "sink, at most 4 096 groups: host finish uploaded")
    assert route(device)[2] == 0
    check(device, [large], plain + [(abi.AGG_STDDEV_SAMP, doubles)], 1000, "sink, STDDEV_SAMP: host finish uploaded")
    assert route(device)[2] == 0
    nine = plain + [(abi.AGG_MIN, ints), (abi.AGG_MAX, ints), (abi.AGG_MIN, doubles), (abi.AGG_MAX, doubles), (abi.AGG_SUM, doubles), (abi.AGG_AVG, ints), (abi.AGG_COUNT, ints)]
    check(device, [few], nine, 1000, "sink, ten aggregates in passes")


def test_host_finish_functions_and_passes(device):
    w = small_world(seed=4)
    everything = specs(w, [(abi.AGG_COUNT_DISTINCT, "ints"), (abi.AGG_ANY, "key"), (abi.AGG_STDDEV_SAMP, "doubles"), (abi.AGG_STDDEV_SAMP, "ints")] + PLAIN)
    run_both([w["key"]], everything, "COUNT(DISTINCT), ANY, STDDEV_SAMP")
    assert route(device) == (0, 0, 0)
    run_both([w["key"]], everything + specs(w, PLAIN), "fourteen aggregates, sixteen accumulators: passes")
    others = [small(np.full(SMALL_CHUNKS, i, dtype=np.int64)) for i in range(3)]
    run_both([w["key"]] + others, everything[:2], "COUNT(DISTINCT) with four GROUP BY columns: the nine-word build")


def test_device_memory_result(device):
    import torch
    w = small_world(seed=6)
    keys, ints = DeviceColumn(w["key"]), DeviceColumn(w["ints"])
    want = oracle_aggregate([w["key"]], [(abi.AGG_SUM, w["ints"]), (abi.AGG_COUNT, None)])
    capacity = 16
    rows = torch.zeros((capacity, 2), dtype=torch.int32, device="cuda")
    values = [torch.zeros(capacity, dtype=torch.int64, device="cuda") for _ in range(2)]
    nulls = [torch.ones(capacity, dtype=torch.uint8, device="cuda") for _ in range(2)]
    shadow = HostAggregateResult(2, capacity)
    for a in range(2):
        shadow.columns[a].values, shadow.columns[a].is_null = values[a].data_ptr(), nulls[a].data_ptr()
    shadow.c.mem, shadow.c.group_row_ids = abi.MEM_DEVICE, rows.data_ptr()
    aggregate_hash([keys], [(abi.AGG_SUM, ints), (abi.AGG_COUNT, None)], result=shadow)
    n = want.n_groups
    assert shadow.n_groups == n
    np.testing.assert_array_equal(rows.cpu().numpy().astype(np.uint32)[:n], want.row_ids[:n])
    for a in range(2):
        got = [None if null else value for value, null in zip(values[a].cpu().tolist()[:n], nulls[a].cpu().tolist()[:n])]
        assert got == want.column(a)


# ---- refusals: every one before any device work, the result untouched --------------------------------------------------------------------
def test_refusals(device):
    w = small_world(seed=8)
    key, ints = DeviceColumn(w["key"]), DeviceColumn(w["ints"])
    other_layout = DeviceColumn(column(np.arange(SMALL_CHUNKS, dtype=np.int32), None, 200))
    cases = [([key], [(9, ints)], abi.ERR_INVALID),                                   # unknown function
             ([key], [(abi.AGG_SUM, None)], abi.ERR_INVALID),                         # only COUNT may omit its column
             ([key], [(abi.AGG_SUM, other_layout)], abi.ERR_INVALID),                 # another chunk layout
             ([key, other_layout], [(abi.AGG_COUNT, None)], abi.ERR_INVALID),
             ([], [(abi.AGG_COUNT, None)], abi.ERR_INVALID),                          # nothing to take the shape from
             ([key], [(abi.AGG_STDDEV_SAMP, ints), (abi.AGG_SUM, other_layout)], abi.ERR_INVALID)]   # a later aggregate's refusal, behind a STDDEV_SAMP
    lib = abi.load_library()
    for groupby, aggregates, status in cases:
        result = HostAggregateResult(len(aggregates), 64)
        for raw in result.raw:
            raw[:] = 0xABABABABABABABAB
        garr = (C.c_void_p * max(1, len(groupby)))(*[c.handle for c in groupby])
        array = (abi.AggregateSpec * len(aggregates))()
        for i, (function, c) in enumerate(aggregates):
            array[i].function, array[i].column = function, c.handle if c is not None else None
        assert lib.hy_aggregate_hash(garr, len(groupby), array, len(aggregates), C.byref(result.c)) == status, f"{aggregates}"
        assert all((raw == 0xABABABABABABABAB).all() for raw in result.raw), "a refused call wrote into the result's columns"
    # ... and the ones with a status of their own
    from hyrise_amd import storage
    from hyrise_amd.operators import aggregate_hash_columns, scan_project_aggregate
    names = np.array([b"a", b"b", b"c"], dtype=object)[np.arange(SMALL_CHUNKS) % 3]
    strings = DeviceColumn(storage.HostColumn([storage.encode_string_dictionary(names[b:e])[0] for b, e in ((0, 300), (300, 557), (557, 558))], abi.TYPE_STRING))
    unsupported = [([strings], [(abi.AGG_COUNT, None)]),                              # a string GROUP BY column
                   ([key], [(abi.AGG_MIN, strings)]),                                  # a string aggregate other than COUNT
                   ([key] * 16, [(abi.AGG_COUNT_DISTINCT, ints)]),                     # COUNT(DISTINCT): a seventeenth key word in the widest build
                   ([key] * 17, [(abi.AGG_COUNT, None)])]                              # more GROUP BY columns than the widest build takes
    for groupby, aggregates in unsupported:
        for call in (aggregate_hash, aggregate_hash_columns):
            with pytest.raises(abi.HyriseAmdError) as error:
                call(groupby, aggregates)
            assert error.value.status == abi.ERR_UNSUPPORTED, f"{call.__name__} {aggregates}"
    with pytest.raises(abi.HyriseAmdError) as error:   # hy_scan_project_aggregate: MIN / MAX / SUM / AVG / COUNT only
        scan_project_aggregate([], [key], [(abi.AGG_STDDEV_SAMP, ints)])
    assert error.value.status == abi.ERR_UNSUPPORTED
    missing = HostAggregateResult(2, 64)   # "aggregate 1: values buffer missing": where it was, behind the device pass and the first column
    missing.columns[1].values = None
    with pytest.raises(abi.HyriseAmdError) as error:
        aggregate_hash([key], [(abi.AGG_COUNT, None), (abi.AGG_SUM, ints)], result=missing)
    assert error.value.status == abi.ERR_INVALID and "aggregate 1: values buffer missing" in str(error.value)
    few = HostAggregateResult(1, 2)   # five groups into room for two: HY_ERR_CAPACITY, behind the device pass, with the group count
    garr = (C.c_void_p * 1)(key.handle)
    array = (abi.AggregateSpec * 1)()
    array[0].function, array[0].column = abi.AGG_COUNT, None
    assert lib.hy_aggregate_hash(garr, 1, array, 1, C.byref(few.c)) == abi.ERR_CAPACITY and few.n_groups == 6

"""Every sort and join path under both answers of lds_atomics_are_lane_ordered (csrc/join.hip).  The device's answer picks between two
implementations in five places -- sort_pairs_u32 (staged 8192-element tiles | sort_histogram / sort_scatter on 2048-element tiles),
prepare_build's directory sort, prepare_build's unsorted unique 32-bit keys (sort + rank_table_fill_sorted | rank_table_mark .. rank_table_
scatter_rows), hy_join_hash's probe_takes_pk (PK-FK kernels | general rank-table kernels) and rt_probe_emit's ranking (one returning LDS
atomic per pair | match-any groups) -- and one device gives one answer.  HY_OPT_LDS_ORDERED_ATOMICS = 0 forces "no": every case here runs
under 1 (the device decides) and 0, is compared byte for byte with its oracle, and proves through hy_debug_lds_order_in_effect which column
of that table ran.  On a device whose own verdict is "no" both runs take the fallback; that is printed, not skipped."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import aggregate_hash
from hyrise_amd.storage import DeviceColumn
from sort_oracle import positions_of, sorted_order
from support import build_column, oracle_aggregate, oracle_join
from test_join_gpu import MODES, SEMI, assert_join_equal, used_pkfk, used_rank_table
from test_sort_gpu import check_sort, chunk_sizes_of, host_column, tied_values

import test_aggregate_columns_gpu as aggregate_columns
import test_join_sort_merge_gpu as sort_merge
import test_sort_limit_gpu as sort_limit
import test_union_positions_gpu as union

pytestmark = pytest.mark.gpu

ASC, DESC = abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST
SORT_TILE, SORT_BIG_TILE = 2048, 8192   # join.hip: the fallback's tile and the staged path's
ORDERED = pytest.mark.parametrize("ordered", [1, 0], ids=["device_decides", "forced_unordered"])


def bound(lib):
    lib.hy_debug_lds_order_in_effect.restype = C.c_int
    lib.hy_debug_join_lane_ordered_atomics.restype = C.c_int
    return lib


class Setting:
    """HY_OPT_LDS_ORDERED_ATOMICS = `ordered` for one test.  arm() lets a two-row sort run under the OTHER setting, so that the in-effect
    word holds the other answer (where the device has two); ran() then shows that the call in between asked under this one."""

    def __init__(self, lib, options, ordered):
        self.lib, self.options, self.ordered = bound(lib), options, ordered
        self.tiny = DeviceColumn(host_column(np.array([1, 0], dtype=np.int32), None, 2, "value"))
        options.set(abi.OPT_LDS_ORDERED_ATOMICS, ordered)

    def _tiny_sort(self):
        got = check_sort([self.tiny], [(np.array([1, 0], dtype=np.int32), None)], [ASC], [2], "two rows")
        got.close()

    def arm(self):
        self.options.set(abi.OPT_LDS_ORDERED_ATOMICS, 1 - self.ordered)
        self._tiny_sort()
        self.options.set(abi.OPT_LDS_ORDERED_ATOMICS, self.ordered)

    def ran(self, context=""):
        effect, verdict = self.lib.hy_debug_lds_order_in_effect(), self.lib.hy_debug_join_lane_ordered_atomics()
        assert verdict in (1, 2), f"{context}: the device was never probed"
        if self.ordered == 0:
            assert effect == 2, f"{context}: in effect {effect} under HY_OPT_LDS_ORDERED_ATOMICS = 0"
        else:
            assert effect == verdict, f"{context}: in effect {effect}, the probe said {verdict}"
        note = "" if verdict == 1 else " (the device's own verdict is 'not ordered': both settings take the fallback)"
        print(f"{context}: ordered={self.ordered} hy_debug_lds_order_in_effect() = {effect}, probe verdict {verdict}{note}")


def test_the_option_forces_no_and_the_probe_s_verdict_comes_back(device, options):
    """0 answers "not ordered" without touching the cached verdict; after the options fixture's reset the option is 1 again and the next
    hy_sort reports what the probe said."""
    lib = bound(device)
    setting = Setting(lib, options, 1)
    setting._tiny_sort()
    verdict = lib.hy_debug_join_lane_ordered_atomics()
    assert verdict in (1, 2) and lib.hy_debug_lds_order_in_effect() == verdict
    options.set(abi.OPT_LDS_ORDERED_ATOMICS, 0)
    setting._tiny_sort()
    assert lib.hy_debug_lds_order_in_effect() == 2
    assert lib.hy_debug_join_lane_ordered_atomics() == verdict   # (the verdict is the probe's, not the option's)
    options.reset()
    value = C.c_int64(-1)
    abi.check(lib.hy_get_option(abi.OPT_LDS_ORDERED_ATOMICS, C.byref(value)))
    assert value.value == 1
    setting._tiny_sort()
    assert lib.hy_debug_lds_order_in_effect() == verdict == lib.hy_debug_join_lane_ordered_atomics()
    print(f"probe verdict: {verdict} ({'lane-ordered' if verdict == 1 else 'not lane-ordered'})")


# ---- a. the sort primitive through hy_sort: one NULL-free int32 value column = one word of `bits` bits ------------------------------------

BITS = [1, 7, 8, 9, 16, 17, 24, 25, 32]   # 1 .. 4 passes of 8 bits: the result ends in the caller's arrays (even) or the temporaries (odd)
ROWS = [2, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1, SORT_BIG_TILE - 1, SORT_BIG_TILE, SORT_BIG_TILE + 1, 3 * SORT_BIG_TILE + 17]
CHUNK = 3_000


def values_of_range(rng, n, bits):
    """n int32 values, about min(n, 40) distinct ones spread evenly over a range that needs exactly `bits` bits (both ends present), around
    zero: long runs of ties in every pass."""
    span = (1 << bits) - 1
    if bits == 32:
        span -= 2_000   # (INT32_MIN + 1000 .. INT32_MAX - 1000: the limits themselves are the case below)
    low = -(span // 2) - 1 if bits > 1 else 0
    distinct = min(n, 40, span + 1)
    pool = low + np.round(np.linspace(0, span, distinct)).astype(np.int64)
    values = pool[rng.integers(0, distinct, n)]
    ends = rng.choice(n, 2, replace=False)
    values[ends[0]], values[ends[1]] = pool[0], pool[-1]
    assert int(values.max() - values.min()).bit_length() == bits and np.iinfo(np.int32).min <= values.min() and values.max() <= np.iinfo(np.int32).max
    return values.astype(np.int32)


@ORDERED
@pytest.mark.parametrize("n", ROWS)
def test_sort_primitive_rows_and_key_bits(device, options, ordered, n):
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(n)
    limits = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min + 1, np.iinfo(np.int32).max - 1, 0, -1], dtype=np.int32)
    cases = [(f"{bits} bits", values_of_range(rng, n, bits)) for bits in BITS]
    with_limits = values_of_range(rng, n, 25)
    with_limits[rng.choice(n, min(n, len(limits)), replace=False)] = limits[:min(n, len(limits))]
    assert (int(with_limits.min()), int(with_limits.max())) == (np.iinfo(np.int32).min, np.iinfo(np.int32).max)
    cases.append(("INT32_MIN and INT32_MAX", with_limits))
    for name, values in cases:
        column = DeviceColumn(host_column(values, None, CHUNK, "value"))
        for mode in (ASC, DESC):
            context = f"n={n} {name} mode={mode}"
            setting.arm()
            check_sort([column], [(values, None)], [mode], chunk_sizes_of(n, CHUNK), context)
            setting.ran(context)


# ---- b. chains of words: (int64 with NULLs, float64 with ties) ---------------------------------------------------------------------------

@ORDERED
@pytest.mark.parametrize("n", [SORT_TILE + 1, SORT_BIG_TILE + 1, 20_000])
def test_sort_two_wide_keys(device, options, ordered, n):
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(n + 1)
    longs, long_nulls = tied_values(rng, n, np.int64), rng.random(n) < 0.05
    doubles = tied_values(rng, n, np.float64, 10)
    columns = [DeviceColumn(host_column(longs, long_nulls, CHUNK, "value")), DeviceColumn(host_column(doubles, None, CHUNK, "value"))]
    for modes in ([ASC, ASC], [DESC, DESC], [ASC, DESC], [DESC, ASC]):
        setting.arm()
        check_sort(columns, [(longs, long_nulls), (doubles, None)], modes, chunk_sizes_of(n, CHUNK), f"n={n} modes={modes}")
        setting.ran(f"two keys n={n} modes={modes}")


# ---- c. the operators on the primitive ---------------------------------------------------------------------------------------------------

@ORDERED
@pytest.mark.parametrize("dtype", [np.int32, np.float64], ids=lambda t: np.dtype(t).name)
def test_sort_limit_selection(device, options, ordered, dtype):
    """hy_sort_limit, k = 100 of 40 003 rows: check_limits runs it under FORCE_SELECT (the candidates' word sorts), FORCE_FULL_SORT and flags 0."""
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    n, chunk, k = 40_003, 7_000, 100
    for name, values in sort_limit.distributions(rng, n, dtype):
        if name not in ("about 40 distinct values", "cluster with outliers"):
            continue
        column = DeviceColumn(host_column(values, None, chunk, "value"))
        for mode in (ASC, DESC):
            setting.arm()
            sort_limit.check_limits([column], [(values, None)], [mode], chunk_sizes_of(n, chunk), [k], f"{np.dtype(dtype).name} {name} mode={mode}")
            setting.ran(f"sort limit {np.dtype(dtype).name} {name} mode={mode}")


@ORDERED
@pytest.mark.parametrize("n", [SORT_TILE + 1, 20_000])
def test_union_positions_forced_sort(device, options, ordered, n):
    """Two shuffled sides of n RowIDs each, drawn from n / 2 rows of the table: duplicates within a side and across the sides."""
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(n + 2)
    table = union.Table(60_000, 7_000)
    sides = [table.positions(rng.integers(0, n // 2, n) * 5 % 60_000) for _ in range(2)]
    columns = [union.host_lists(table, union.split(side, union.chunks_of(n, 1_500))) for side in sides]
    setting.arm()
    want = union.check_union([columns[0]], [columns[1]], [sides[0]], [sides[1]], path=3, force_sort=True, context=f"n {n}")
    setting.ran(f"union positions n={n}")
    assert len(want[0]) < 2 * n   # (rows both sides hold were merged)


@ORDERED
def test_join_sort_merge_both_sides(device, options, ordered):
    """3 000 x 2 000 uniform keys in [0, 64) under (FULL, =) and (INNER, <), and the 20 000-row run of one int64 key of
    test_duplicate_run_longer_than_the_lds_window: both sides are sorted by sort_pairs_u32."""
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(42)
    left_values, right_values = rng.integers(0, 64, 3000).astype(np.int32), rng.integers(0, 64, 2000).astype(np.int32)
    left, right = sort_merge.Side(left_values, chunk=1000), sort_merge.Side(right_values, chunk=[1999, 1])
    for mode, condition in ((sort_merge.FULL, sort_merge.EQ), (sort_merge.INNER, sort_merge.LT)):
        setting.arm()
        sort_merge.check(device, left, right, mode, condition, "general")
        setting.ran(f"sort merge mode={mode} condition={condition}")
    rng = np.random.default_rng(3)
    short = rng.integers(9, 12, 40).astype(np.int64) << 33
    long_run = np.concatenate([np.full(20_000, 10), rng.integers(0, 20, 500)]).astype(np.int64) << 33
    setting.arm()
    sort_merge.check(device, sort_merge.Side(short), sort_merge.Side(long_run, chunk=4_096), sort_merge.FULL, sort_merge.EQ, "long run, int64")
    setting.ran("sort merge long run, int64")


# aggregate.hip: a result of more than STAGED_GROUPS groups of plain aggregates stays on the device, where sort_pairs_u32 orders the groups
FIRST_DEVICE_ORDERED_GROUPS = aggregate_columns.STAGED_GROUPS + 1


@ORDERED
@pytest.mark.parametrize("dense", [True, False], ids=["key_order", "first_row_order"])
def test_aggregate_group_order(device, options, ordered, dense):
    """4 097 groups, the smallest result whose group order comes from sort_pairs_u32 (by key for dense int keys, by first row otherwise): the
    representative RowIDs and the COUNT / SUM cells against the oracle's bytes."""
    setting = Setting(device, options, ordered)
    rng = np.random.default_rng(7 + dense)
    group = rng.permutation(np.repeat(np.arange(FIRST_DEVICE_ORDERED_GROUPS, dtype=np.int64), 2))
    keys = build_column(group.astype(np.int32) if dense else (group * 7919 - 1_000_000).astype(np.int32), None, 3_000, abi.ENC_UNENCODED)
    ints = build_column(rng.integers(-1000, 1000, len(group)).astype(np.int32), None, 3_000, abi.ENC_UNENCODED)
    aggregates = [(abi.AGG_COUNT, None), (abi.AGG_SUM, ints)]
    want = oracle_aggregate([keys], aggregates)
    device_keys, device_ints = DeviceColumn(keys), DeviceColumn(ints)
    setting.arm()
    got = aggregate_hash([device_keys], [(abi.AGG_COUNT, None), (abi.AGG_SUM, device_ints)])
    setting.ran(f"aggregate dense={dense}")
    assert aggregate_columns.finished_on_device(device) == 1
    groups = want.n_groups
    assert got.n_groups == groups == FIRST_DEVICE_ORDERED_GROUPS
    assert got.row_ids[:groups].tobytes() == want.row_ids[:groups].tobytes()
    for a in range(len(aggregates)):
        assert got.nulls[a][:groups].tobytes() == want.nulls[a][:groups].tobytes(), a
        assert got.raw[a][:groups].tobytes() == want.raw[a][:groups].tobytes(), a


# ---- d. JoinHash -------------------------------------------------------------------------------------------------------------------------

_shared = {}   # host columns and oracle results, computed once and read by both settings


def shared(key, make):
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def join_columns():
    def make():
        rng = np.random.default_rng(11)
        keys = (np.arange(70_000, dtype=np.int64) * 3).astype(np.int32)
        probe_values = np.where(rng.random(150_000) < 0.5, rng.choice(keys, 150_000), rng.integers(-300, 210_300, 150_000)).astype(np.int32)
        return {"unique": build_column(rng.permutation(keys), None, 20_000, abi.ENC_UNENCODED),
                "twice": build_column(rng.permutation(np.concatenate([keys, keys])), None, 20_000, abi.ENC_UNENCODED),
                "probe": build_column(probe_values[:100_000], rng.random(100_000) < 0.1, 65_535, abi.ENC_UNENCODED),
                "long probe": build_column(probe_values, rng.random(150_000) < 0.1, 65_535, abi.ENC_UNENCODED),
                "probe without NULLs": build_column(probe_values[:100_000], None, 65_535, abi.ENC_UNENCODED)}
    return shared("join columns", make)


def check_join(setting, case, left, right, mode):
    """Fresh DeviceColumns (a build column remembers join hints), the oracle's result shared between the settings."""
    from hyrise_amd.operators import join_hash
    want = shared((case, mode), lambda: oracle_join(left, right, mode))
    setting.arm()
    got = join_hash(DeviceColumn(left), DeviceColumn(right), mode)
    setting.ran(f"{case} mode={mode}")
    assert_join_equal(got, want, mode, f"{case} mode={mode} ordered={setting.ordered}")
    return got


@ORDERED
@pytest.mark.parametrize("mode", [abi.JOIN_INNER, abi.JOIN_LEFT])
def test_join_shuffled_unique_build(device, options, ordered, mode):
    """70 000 shuffled unique int32 build keys with packed ids: the sort and rank_table_fill_sorted where the atomics are ordered,
    rank_table_mark .. rank_table_scatter_rows<uint32_t, uint32_t> where not.  A rank table either way."""
    setting = Setting(device, options, ordered)
    columns = join_columns()
    build, probe = columns["unique"], columns["probe"]
    check_join(setting, "shuffled unique build", *((probe, build) if mode == abi.JOIN_LEFT else (build, probe)), mode)
    assert used_rank_table() != 0


@ORDERED
@pytest.mark.parametrize("mode", [abi.JOIN_INNER, abi.JOIN_SEMI])
def test_join_shuffled_duplicate_build(device, options, ordered, mode):
    """The same keys twice, shuffled (140 000 rows): the build side's directory sort.  Inner: 32-bit keys and packed ids -- the staged sort |
    sort_scatter<uint32_t, uint32_t>; its probe side has 150 000 rows, since an Inner join builds on the smaller input.  Semi joins keep whole
    RowIDs on the build side (sort_scatter<uint32_t, hy_row_id> under both settings); their probe column has no NULLs, so that the join asks
    for the setting where it decides about the PK-FK kernels."""
    setting = Setting(device, options, ordered)
    columns = join_columns()
    if mode == abi.JOIN_INNER:
        check_join(setting, "duplicate shuffled build", columns["twice"], columns["long probe"], mode)
        assert used_rank_table() == 0
    else:
        check_join(setting, "duplicate shuffled build", columns["probe without NULLs"], columns["twice"], mode)


_pkfk_results = {}   # mode -> (ordered, left bytes, right bytes): the two settings' outputs are the same bytes


@ORDERED
def test_join_pkfk_shape_takes_match_any_ranking(device, options, ordered):
    """test_primary_key_foreign_key_probe's shape at 40 000 x 120 000 rows: a sorted dense build side and a NULL-free FrameOfReference probe
    column.  Forced unordered, the PK-FK kernels must not run: the general rank-table kernels do, rt_probe_emit ranking with match-any groups."""
    setting = Setting(device, options, ordered)
    lib = bound(device)

    def make():
        rng = np.random.default_rng(300)
        keys = np.arange(40_000, dtype=np.int32) - 11_000
        values = rng.choice(keys, 120_000).astype(np.int32)
        outside = rng.random(120_000) < 0.04
        values[outside] = rng.integers(int(keys.min()) - 300, int(keys.max()) + 300, int(outside.sum())).astype(np.int32)
        alias = rng.random(120_000) < 0.02   # a build key's Bloom filter bit, no build key
        values[alias] = (rng.choice(keys, int(alias.sum())).astype(np.int64) + (1 << 20) * rng.integers(1, 3, int(alias.sum()))).astype(np.int32)
        return build_column(keys, None, 4_096, abi.ENC_UNENCODED), build_column(np.sort(values), None, 65_535, abi.ENC_FRAME_OF_REFERENCE)

    build, probe = shared("pkfk columns", make)
    for mode in MODES:
        args = (probe, build) if mode in SEMI or mode == abi.JOIN_LEFT else (build, probe)
        got = check_join(setting, "pk-fk shape", *args, mode)
        assert used_rank_table() != 0, mode
        if ordered == 0:
            assert used_pkfk() == 0, mode
        else:
            assert used_pkfk() == (1 if lib.hy_debug_join_lane_ordered_atomics() == 1 else 0), mode
        n = got.n_pairs
        mine = (ordered, got.left[:n].tobytes(), b"" if mode in SEMI else got.right[:n].tobytes())
        other = _pkfk_results.setdefault(mode, mine)
        if other[0] != ordered:
            assert other[1:] == mine[1:], f"mode {mode}: the two settings wrote different pairs"

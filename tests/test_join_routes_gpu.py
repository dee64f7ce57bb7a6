"""Every route of JoinHash's host side ("Routes") over one small world: each build step, each family of probe kernels,
each place a result can go, the modes that change the route, the first joins of a new thread and the refusals of a result without its
buffers.  Expected results: support.oracle_join, byte for byte (pairs and PosList cuts); the three debug counters say which route ran.
Build columns have chunks of 300 / 257 / 1 rows (the identity table wants equally sized chunks: 300 / 300 / 1; the sort-then-fill
route starts at 65 536 rows: 65 535 / 2), probe columns 700 / 257 / 1 (behind the large build: 65 535 / 4 466)."""
import ctypes as C
import threading
import types

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import join_hash, join_hash_count, join_predicates
from hyrise_amd.storage import DeviceColumn, HostColumn
from support import oracle_join
from test_join_gpu import _device_buffer, _read_back, assert_join_equal, used_pkfk, used_rank_table

pytestmark = pytest.mark.gpu

SIZES = (300, 257, 1)
UNIFORM = (300, 300, 1)
PROBE_SIZES = (700, 257, 1)
LARGE = (65535, 2)
LARGE_PROBE = (65535, 4466)
BUILD_ON_THE_RIGHT = (abi.JOIN_LEFT, abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE)


def column(values, sizes, encoding, nulls_in_chunk_1=None):
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    assert bounds[-1] == len(values)
    segments = [storage.encode_segment(values[b:e], nulls_in_chunk_1[b:e] if nulls_in_chunk_1 is not None and c == 1 else None, encoding)
                for c, (b, e) in enumerate(zip(bounds, bounds[1:]))]
    return HostColumn(segments, storage.TYPE_OF_NP[values.dtype])


def was_hinted():
    lib = abi.load_library()
    lib.hy_debug_join_build_was_hinted.restype = C.c_int
    return int(lib.hy_debug_join_build_was_hinted())


class World:
    """builds[name] = (host column, the probes it is joined with, hy_debug_join_used_rank_table of an Inner join over it);
    probes[name] = host column.  Device columns are made per test: a build column remembers what earlier joins learned about it."""

    def __init__(self):
        rng = np.random.default_rng(4242)
        n = sum(SIZES)
        keys = (np.arange(sum(UNIFORM), dtype=np.int64) * 997 - 50_000).astype(np.int32)   # sparse enough that 64 probe rows span > 2^16 key values
        large = (np.arange(sum(LARGE), dtype=np.int64) * 7 - 100_000).astype(np.int32)
        nulls = rng.random(n) < 0.2
        shuffled_large = rng.permutation(large)
        with_duplicate = shuffled_large.copy()
        with_duplicate[70] = with_duplicate[65_000]
        self.builds = {
            "identity": (column(keys, UNIFORM, abi.ENC_UNENCODED), "plain", 2),
            "sorted_dictionary": (column(keys[:n], SIZES, abi.ENC_DICTIONARY), "plain", 1),
            "mark_and_scatter": (column(rng.permutation(keys[:n]), SIZES, abi.ENC_UNENCODED), "plain", 1),
            "sort_then_fill": (column(shuffled_large, LARGE, abi.ENC_UNENCODED), "large", 1),
            "sort_then_fill_duplicate": (column(with_duplicate, LARGE, abi.ENC_UNENCODED), "large", 0),
            "lsd_sort": (column(rng.choice(keys[:200], n), SIZES, abi.ENC_UNENCODED), "plain", 0),
            "int64": (column(rng.permutation(keys[:n]).astype(np.int64) + 10_000_000_000, SIZES, abi.ENC_UNENCODED), "int64", 1),
            "float": (column(rng.integers(0, 300, n).astype(np.float32) / 4, SIZES, abi.ENC_UNENCODED), "float", 0),
            "nulls": (column(keys[:n], SIZES, abi.ENC_UNENCODED, nulls), "plain", 1),
            "empty": (HostColumn([], abi.TYPE_INT), "plain", 0),
        }
        m = sum(PROBE_SIZES)
        drawn = rng.choice(keys, m).astype(np.int32)
        outside = rng.random(m) < 0.05
        drawn[outside] = rng.integers(int(keys.min()) - 500, int(keys.max()) + 500, int(outside.sum())).astype(np.int32)
        probe_nulls = rng.random(m) < 0.1
        self.probes = {
            "plain": column(drawn, PROBE_SIZES, abi.ENC_UNENCODED),
            "dictionary": column(drawn, PROBE_SIZES, abi.ENC_DICTIONARY),
            "nulls": column(drawn, PROBE_SIZES, abi.ENC_UNENCODED, probe_nulls),
            "large": column(rng.choice(large, sum(LARGE_PROBE)).astype(np.int32), LARGE_PROBE, abi.ENC_UNENCODED),
            "int64": column(drawn.astype(np.int64) + 10_000_000_000, PROBE_SIZES, abi.ENC_UNENCODED),
            "float": column(rng.integers(0, 320, m).astype(np.float32) / 4, PROBE_SIZES, abi.ENC_UNENCODED),
        }
        # the second column of each table, for a secondary predicate
        self.build_other = column(rng.integers(0, 100, n).astype(np.int32), SIZES, abi.ENC_UNENCODED)
        self.probe_other = column(rng.integers(0, 100, m).astype(np.int32), PROBE_SIZES, abi.ENC_DICTIONARY)
        self.wanted = {}

    def sides(self, build, probe, mode):
        """(left, right) for the mode: JoinHash builds over the right input of a Left / Semi / Anti join, over the smaller one of an Inner join."""
        return (probe, build) if mode in BUILD_ON_THE_RIGHT else (build, probe)

    def want(self, build_name, probe_name, mode, secondary=False):
        key = (build_name, probe_name, mode, secondary)
        if key not in self.wanted:
            left, right = self.sides(self.builds[build_name][0], self.probes[probe_name], mode)
            other_left, other_right = self.sides(self.build_other, self.probe_other, mode)
            self.wanted[key] = oracle_join(left, right, mode, secondary=[(other_left, abi.PRED_LESS_THAN, other_right)] if secondary else None)
        return self.wanted[key]


@pytest.fixture(scope="module")
def world(device):
    return World()


class Pair:
    """A build and a probe column on the device (new ones: no hint from an earlier test), and a secondary predicate's columns if wanted."""

    def __init__(self, world, build_name, probe_name=None, secondary=False):
        self.world, self.build_name = world, build_name
        self.probe_name = probe_name or world.builds[build_name][1]
        self.build, self.probe = DeviceColumn(world.builds[build_name][0]), DeviceColumn(world.probes[self.probe_name])
        self.others = (DeviceColumn(world.build_other), DeviceColumn(world.probe_other)) if secondary else None

    def want(self, mode):
        return self.world.want(self.build_name, self.probe_name, mode, self.others is not None)

    def arguments(self, mode):
        left, right = self.world.sides(self.build, self.probe, mode)
        secondary = None
        if self.others:
            other_left, other_right = self.world.sides(*self.others, mode)
            secondary = [(other_left, abi.PRED_LESS_THAN, other_right)]
        return left, right, secondary


def call(lib, left, right, mode, secondary, result):
    predicates, n = join_predicates(secondary)
    if n:
        return lib.hy_join_hash_predicates(left.handle, right.handle, mode, predicates, n, C.byref(result))
    return lib.hy_join_hash(left.handle, right.handle, mode, C.byref(result))


def run(pair, mode, placement):
    """The join's result as assert_join_equal reads it.  placement: host | device | async (device, HY_JOIN_ASYNC and hy_join_hash_finish)."""
    lib = abi.load_library()
    left, right, secondary = pair.arguments(mode)
    if placement == "host":
        return join_hash(left, right, mode, secondary=secondary)
    want = pair.want(mode)
    n, slices = want.n_pairs, int(want.c.n_slices)
    p_left, like = _device_buffer(lib, (n + 8, 2), np.uint32, 0xABABABAB)
    p_right, _ = _device_buffer(lib, (n + 8, 2), np.uint32, 0xABABABAB)
    p_offsets, like_offsets = _device_buffer(lib, (slices + 8,), np.uint64, 0xCDCDCDCDCDCDCDCD)
    p_status, like_status = _device_buffer(lib, (4,), np.uint64, 0xEEEEEEEEEEEEEEEE)
    r = abi.JoinResult()
    r.mem, r.radix_bits = abi.MEM_DEVICE, 0xFFFFFFFF
    r.left_pos, r.right_pos, r.capacity = p_left, p_right, n
    r.slice_offsets, r.slice_capacity = p_offsets, slices
    if placement == "async":
        r.flags, r.status = abi.JOIN_ASYNC, p_status
    try:
        abi.check(call(lib, left, right, mode, secondary, r))
        counters = (used_rank_table(), used_pkfk(), was_hinted())
        if placement == "async":
            abi.check(lib.hy_join_hash_finish(left.handle, right.handle, mode, C.byref(r)))
            words = _read_back(lib, p_status, like_status)
            assert (int(words[0]), int(words[1] & 0xFFFFFFFF), int(words[1] >> 32), int(words[2] & 0xFFFFFFFF), int(words[2] >> 32)) == (n, slices, 1, 1, 0)
        got = types.SimpleNamespace(c=r, n_pairs=int(r.n_pairs), left=_read_back(lib, p_left, like), right=_read_back(lib, p_right, like),
                                    slice_offsets=_read_back(lib, p_offsets, like_offsets), counters=counters)
        assert (got.left[n:] == 0xABABABAB).all() and (got.right[n:] == 0xABABABAB).all(), "nothing behind the pairs"
        return got
    finally:
        for p in (p_left, p_right, p_offsets, p_status):
            lib.hy_device_free(p)


def check(pair, mode, placement, counters, context):
    """counters: (used_rank_table, used_pkfk, build_was_hinted) expected of the call; None: not asserted."""
    got = run(pair, mode, placement)
    seen = getattr(got, "counters", None) or (used_rank_table(), used_pkfk(), was_hinted())
    assert_join_equal(got, pair.want(mode), mode, f"{context} ({placement} result)")
    for name, value, expected in zip(("used_rank_table", "used_pkfk", "build_was_hinted"), seen, counters):
        assert expected is None or value == expected, f"{context} ({placement} result): {name} is {value}, expected {expected}"
    return got


def takes_pk(world, build_name):
    """A rank table over int32 keys, probed by this world's plain int32 column: the kernels of join_pkfk.hpp."""
    return 1 if world.builds[build_name][2] and build_name != "int64" else 0


# ---- build routes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_name", ["sorted_dictionary", "mark_and_scatter", "sort_then_fill", "sort_then_fill_duplicate", "lsd_sort", "int64", "float", "nulls", "empty"])
def test_build_route(world, build_name):
    pair = Pair(world, build_name)
    rank = world.builds[build_name][2]
    for placement in ("host", "device"):
        check(pair, abi.JOIN_INNER, placement, (rank, takes_pk(world, build_name), 0), build_name)
    left, right, _ = pair.arguments(abi.JOIN_INNER)
    assert join_hash_count(left, right, abi.JOIN_INNER) == pair.want(abi.JOIN_INNER).n_pairs
    assert used_rank_table() == rank      # (used_pkfk speaks of pass 2, which a count does not have)
    if build_name == "sort_then_fill_duplicate":      # the column remembers its duplicate: no second attempt at a rank table
        check(pair, abi.JOIN_INNER, "host", (0, 0, 0), build_name + ", again")


def identity_then_hinted(world, options_set, options_reset):
    """The dense, sorted, unique column: the identity table on the first join, the hinted one-pass fill from the second on -- wave by wave,
    per slice (HY_OPT_JOIN_FILL_WGS_PER_CU = 0), and with a hint that does not hold (HY_OPT_JOIN_BREAK_HINT = 1: the join runs again)."""
    pair = Pair(world, "identity")
    check(pair, abi.JOIN_INNER, "host", (2, 1, 0), "identity table")
    check(pair, abi.JOIN_INNER, "host", (2, 1, 1), "hinted wave fill")
    check(pair, abi.JOIN_INNER, "device", (2, 1, 1), "hinted wave fill")
    check(pair, abi.JOIN_INNER, "async", (2, 1, 1), "hinted wave fill")
    check(pair, abi.JOIN_INNER, "host", (2, 1, 1), "hinted wave fill, the block the join before left to clear")
    left, right, _ = pair.arguments(abi.JOIN_INNER)
    assert join_hash_count(left, right, abi.JOIN_INNER) == pair.want(abi.JOIN_INNER).n_pairs and was_hinted() == 1
    options_set(abi.OPT_JOIN_FILL_WGS_PER_CU, 0)
    check(pair, abi.JOIN_INNER, "host", (2, 1, 1), "hinted per-slice fill")
    check(pair, abi.JOIN_INNER, "async", (2, 1, 1), "hinted per-slice fill")
    options_reset(abi.OPT_JOIN_FILL_WGS_PER_CU)
    options_set(abi.OPT_JOIN_BREAK_HINT, 1)
    check(pair, abi.JOIN_INNER, "host", (2, 1, 2), "broken hint")
    options_reset(abi.OPT_JOIN_BREAK_HINT)
    check(pair, abi.JOIN_INNER, "host", (2, 1, 0), "a dropped hint stays dropped")


def test_identity_table_then_hinted_fills(world, options):
    identity_then_hinted(world, options.set, options.reset)


def test_broken_hint_is_found_by_finish(world, options):
    """HY_JOIN_ASYNC over a hint that does not hold: nothing is written, hy_join_hash_finish drops the hint and runs the join again."""
    pair = Pair(world, "identity")
    check(pair, abi.JOIN_INNER, "host", (2, 1, 0), "identity table")
    options.set(abi.OPT_JOIN_BREAK_HINT, 1)
    got = check(pair, abi.JOIN_INNER, "async", (2, 1, 1), "broken hint, queued")
    assert was_hinted() == 2, "finish ran the join again"
    assert got.n_pairs == pair.want(abi.JOIN_INNER).n_pairs


def test_first_joins_of_a_new_thread(world, device):
    """A new thread has a new mailbox and no zeroed blocks: the identity table, then the hinted fills that allocate both blocks."""
    outcome = {}

    def set_option(option_id, value):
        abi.check(device.hy_set_option(option_id, value))

    defaults = {}
    for option_id in (abi.OPT_JOIN_FILL_WGS_PER_CU, abi.OPT_JOIN_BREAK_HINT):
        before = C.c_int64(0)
        abi.check(device.hy_get_option(option_id, C.byref(before)))
        defaults[option_id] = before.value

    def body():
        try:
            identity_then_hinted(world, set_option, lambda option_id: set_option(option_id, defaults[option_id]))
            check(Pair(world, "lsd_sort"), abi.JOIN_INNER, "host", (0, 0, 0), "directory on the new thread")
        except BaseException as error:   # noqa: BLE001 (handed to the asserting thread)
            outcome["error"] = error
        finally:
            for option_id, value in defaults.items():
                device.hy_set_option(option_id, value)
            device.hy_shutdown()

    thread = threading.Thread(target=body)
    thread.start()
    thread.join()
    assert "error" not in outcome, repr(outcome.get("error"))


# ---- probe routes ---------------------------------------------------------------------------------------------------------------------------
PROBE_ROUTES = {   # name: (options, probe column, used_pkfk)
    "pk": ({}, "plain", 1),
    "pk_build_in_lds": ({abi.OPT_JOIN_LDS_BUILD_TILES: 1}, "plain", 2),
    "pk_hand_over_ranks": ({abi.OPT_JOIN_HAND_OVER_RANKS: 1, abi.OPT_JOIN_LDS_BUILD: 0}, "plain", 1),
    "rt_stream_count": ({abi.OPT_JOIN_PKFK: 0}, "plain", 0),
    "rt_probe_count_dictionary": ({}, "dictionary", 0),
    "rt_probe_count_nulls": ({}, "nulls", 0),
}


@pytest.mark.parametrize("route", list(PROBE_ROUTES))
@pytest.mark.parametrize("build_name", ["identity", "sorted_dictionary", "mark_and_scatter"])
def test_probe_route_over_a_rank_table(world, options, build_name, route):
    settings, probe_name, pkfk = PROBE_ROUTES[route]
    for option_id, value in settings.items():
        options.set(option_id, value)
    options.set(abi.OPT_JOIN_HINT, 0)      # (every join of this test builds its table the same way)
    pair = Pair(world, build_name, probe_name)
    rank = world.builds[build_name][2]
    for mode in (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_SEMI):
        for placement in ("host", "device"):
            check(pair, mode, placement, (rank, pkfk, 0), f"{build_name} {route} mode {mode}")
    left, right, _ = pair.arguments(abi.JOIN_INNER)
    assert join_hash_count(left, right, abi.JOIN_INNER) == pair.want(abi.JOIN_INNER).n_pairs and used_rank_table() == rank


@pytest.mark.parametrize("secondary", [False, True], ids=["plain", "secondary_predicate"])
@pytest.mark.parametrize("probe_name", ["plain", "nulls"])
def test_probe_route_over_a_directory(world, probe_name, secondary):
    pair = Pair(world, "lsd_sort", probe_name, secondary)
    for mode in (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_SEMI):
        for placement in ("host", "device", "async"):      # (async: a directory needs host decisions -- the call is synchronous, the status filled all the same)
            check(pair, mode, placement, (0, 0, 0), f"directory, probe {probe_name}, secondary {secondary}, mode {mode}")


def test_secondary_predicate_over_unique_keys_takes_the_directory(world):
    pair = Pair(world, "mark_and_scatter", "plain", True)
    for placement in ("host", "device"):
        check(pair, abi.JOIN_INNER, placement, (0, 0, 0), "unique keys, secondary predicate")


# ---- modes ----------------------------------------------------------------------------------------------------------------------------------
def test_anti_null_as_true_over_a_build_side_with_nulls_is_empty(world):
    pair = Pair(world, "nulls")
    for placement in ("host", "device"):
        got = check(pair, abi.JOIN_ANTI_NULL_AS_TRUE, placement, (None, 0, 0), "AntiNullAsTrue, NULL on the build side")
        assert got.n_pairs == 0 and int(got.c.n_slices) == 0 and int(got.slice_offsets[0]) == 0
    left, right, _ = pair.arguments(abi.JOIN_ANTI_NULL_AS_TRUE)
    assert join_hash_count(left, right, abi.JOIN_ANTI_NULL_AS_TRUE) == 0
    check(Pair(world, "mark_and_scatter"), abi.JOIN_ANTI_NULL_AS_TRUE, "host", (1, 1, 0), "AntiNullAsTrue, no NULL on the build side")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_name", ["mark_and_scatter", "lsd_sort"])
def test_result_without_its_buffers_is_refused(world, device, build_name):
    """A result without the probe side's list, and one without slice_offsets: HY_ERR_INVALID, nothing written; the same join with its
    buffers, on the same thread, gives the oracle's result afterwards."""
    pair = Pair(world, build_name)
    left, right, _ = pair.arguments(abi.JOIN_INNER)
    n = max(left.rows, right.rows)
    for missing, message in (("right_pos", b"PosList buffer for the probe side missing"), ("left_pos", b"PosList buffer for the build side missing"),
                             ("slice_offsets", b"slice_offsets missing")):
        left_pos, right_pos = np.full((n, 2), 0xABABABAB, dtype=np.uint32), np.full((n, 2), 0xABABABAB, dtype=np.uint32)
        offsets = np.full(700, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
        r = abi.JoinResult()
        r.mem, r.radix_bits, r.capacity, r.slice_capacity = abi.MEM_HOST, 0xFFFFFFFF, n, 600
        r.left_pos, r.right_pos, r.slice_offsets = left_pos.ctypes.data, right_pos.ctypes.data, offsets.ctypes.data
        setattr(r, missing, None)
        assert device.hy_join_hash(left.handle, right.handle, abi.JOIN_INNER, C.byref(r)) == abi.ERR_INVALID, missing
        assert message in device.hy_last_error(), missing
        assert (left_pos == 0xABABABAB).all() and (right_pos == 0xABABABAB).all() and (offsets == 0xCDCDCDCDCDCDCDCD).all(), missing
        rank = world.builds[build_name][2]
        check(pair, abi.JOIN_INNER, "host", (rank, takes_pk(world, build_name), 0), f"{build_name} after the refusal of a result without {missing}")

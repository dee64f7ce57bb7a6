"""Every job source of the scan's host side over one small table, in the combinations whose scratch layouts compose: a data column and a
reference column whose PosLists span chunks, a host result and a device chunk-region result, excluded chunks, and the first call of a
new thread (a new scratch arena, sized by the layout's dry run alone).  Expected results: the oracles of tests/support.py,
tests/in_list_oracle.py and tests/string_columns_oracle.py, and the host LIKE matcher that tests/like_cases.py pins to the reference."""
import ctypes as C
import threading

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.like import dictionary_matches
from hyrise_amd.operators import HostScanResult, in_list_predicate, make_predicate, string_in_list_predicate
from hyrise_amd.storage import DeviceColumn, HostColumn
from in_list_oracle import union_of_equals
from support import oracle_scan, oracle_scan_columns, oracle_validate
from test_string_columns_gpu import Pair, random_chunk

pytestmark = pytest.mark.gpu

SIZES = (300, 257, 1)      # the second chunk holds NULLs
BOUNDS = (0, 300, 557, 558)
EXCLUDED = [1]


class World:
    """The table's columns on the host and the device, as data columns and behind PosLists that span the chunks."""

    def __init__(self):
        rng = np.random.default_rng(558)
        rows = BOUNDS[-1]
        nulls = rng.random(rows) < 0.2

        def int_column(values, encoding):
            return HostColumn([storage.encode_segment(values[b:e], nulls[b:e] if c == 1 else None, encoding) for c, (b, e) in enumerate(zip(BOUNDS, BOUNDS[1:]))], abi.TYPE_INT)

        self.host = {"dictionary": int_column(rng.integers(0, 40, rows).astype(np.int32), abi.ENC_DICTIONARY),
                     "unencoded": int_column(rng.integers(0, 40, rows).astype(np.int32), abi.ENC_UNENCODED)}
        self.pair = Pair([random_chunk(rng, n, 30, 0.2 if c == 1 else 0.0, alphabet=b"abA") for c, n in enumerate(SIZES)],
                         [random_chunk(rng, n, 25, 0.2 if c == 1 else 0.0, alphabet=b"abA") for c, n in enumerate(SIZES)])
        self.dictionaries = [chunk[0] for chunk in self.pair.left_chunks]
        self.host["strings"], self.host["strings_right"] = self.pair.left_host, self.pair.right_host
        tids = rng.integers(0, 4, rows).astype(np.uint32)
        begins = rng.integers(1, 30, rows).astype(np.uint32)
        ends = np.where(rng.random(rows) < 0.3, rng.integers(1, 40, rows), storage.MAX_COMMIT_ID).astype(np.uint32)
        begins[BOUNDS[2]:], ends[BOUNDS[2]:] = 3, storage.MAX_COMMIT_ID      # the last chunk: entirely visible
        self.host["mvcc"] = HostColumn([storage.make_mvcc_column(tids[b:e], begins[b:e], ends[b:e], chunk_size=e - b).segments[0] for b, e in zip(BOUNDS, BOUNDS[1:])], abi.TYPE_INT)
        self.host["twin_left"], self.host["twin_right"] = self.pair.twins
        self.dev = {name: DeviceColumn(host) for name, host in self.host.items() if not name.startswith("twin")}
        self.dev["strings"], self.dev["strings_right"] = self.pair.left_dev, self.pair.right_dev
        self.left_dict, self.right_dict = self.pair.left_dict, self.pair.right_dict
        # PosLists of 70, 1 and 200 rows drawn from all three chunks, some NULL RowIDs among them (none for Validate)
        starts = np.asarray(BOUNDS)
        pos_lists = []
        for size in (70, 1, 200):
            drawn = rng.integers(0, rows, size)
            chunk = np.searchsorted(starts, drawn, side="right") - 1
            pos_lists.append(np.stack([chunk, drawn - starts[chunk]], axis=1).astype(np.uint32))
        with_nulls = [p.copy() for p in pos_lists]
        for p in with_nulls:
            p[rng.random(len(p)) < 0.05] = 0xFFFFFFFF
        self.ref_host, self.ref_dev = {}, {}
        for name, host in self.host.items():
            self.ref_host[name] = storage.make_reference_column(host, pos_lists if name == "mvcc" else with_nulls, [None] * len(pos_lists))
            if name in self.dev:
                self.ref_dev[name] = DeviceColumn(self.ref_host[name], refs={id(host): self.dev[name]})

    def column(self, name, reference):
        return (self.ref_host if reference else self.host)[name], (self.ref_dev if reference else self.dev).get(name)   # (the twins: host only)


@pytest.fixture(scope="module")
def world(device):
    return World()


# ---- expected results: per chunk (chunk state or None where the oracle does not say, count, RowIDs) -----------------------------------------
def from_oracle(result):
    return [(int(result.chunk_state[c]), int(result.counts[c]), result.pos_list(c).copy()) for c in range(result.n_chunks)]


def from_offsets(per_chunk):
    return [(None, len(p), np.stack([np.full(len(p), c, dtype=np.uint32), p.astype(np.uint32)], axis=1).reshape(-1, 2)) for c, p in enumerate(per_chunk)]


class Route:
    """name, the columns it reads, call(world, reference, excluded pointer, n_excluded, result pointer) -> status, want(world, reference)."""
    def __init__(self, name, column, call, want, excludes=True):
        self.name, self.column, self.call, self.want, self.excludes = name, column, call, want, excludes


def literal_route():
    predicate = make_predicate(abi.PRED_BETWEEN_INCLUSIVE, abi.TYPE_INT, 5, 20, nullable=True)
    return Route("literal", "dictionary",
                 lambda w, ref, ex, n_ex, out: abi.load_library().hy_table_scan(w.column("dictionary", ref)[1].handle, C.byref(predicate), ex, n_ex, out),
                 lambda w, ref: from_oracle(oracle_scan(w.column("dictionary", ref)[0], predicate)))


def like_routes(pattern, condition=abi.PRED_LIKE):
    def predicate(w):
        return make_predicate(condition, abi.TYPE_STRING, nullable=True, dictionary_matches=dictionary_matches(w.dictionaries, pattern, condition))

    def want(w, ref):
        return from_oracle(oracle_scan(w.column("strings", ref)[0], predicate(w)))

    def host_bitmaps(w, ref, ex, n_ex, out):
        return abi.load_library().hy_table_scan(w.column("strings", ref)[1].handle, C.byref(predicate(w)), ex, n_ex, out)

    def on_device(w, ref, ex, n_ex, out):
        return abi.load_library().hy_table_scan_like(w.column("strings", ref)[1].handle, w.left_dict.handle, pattern, len(pattern), condition, 1, ex, n_ex, out)

    return Route("like_host_bitmaps", "strings", host_bitmaps, want), Route("like_device", "strings", on_device, want)


def in_list_route(column, elements, negated):
    def list_of(w):
        if column == "strings":
            return string_in_list_predicate(w.dictionaries, elements, negated=negated, nullable=True)
        return in_list_predicate(abi.TYPE_INT, elements, negated=negated, nullable=True)

    def call(w, ref, ex, n_ex, out):
        return abi.load_library().hy_table_scan_in_list(w.column(column, ref)[1].handle, C.byref(list_of(w)), ex, n_ex, out)

    def want(w, ref):
        return from_offsets(union_of_equals(w.column(column, ref)[0], elements, negated=negated, nullable=True, dictionaries=w.dictionaries if column == "strings" else None))

    return Route(f"{'not_in' if negated else 'in'}_{column}", column, call, want)


ROUTES = {}
FRESH = {}


def register(route, fresh=None):
    ROUTES[route.name] = route
    FRESH[route.name] = fresh or route


register(literal_route())
for _route, _fresh in zip(like_routes(b"%a_b%"), like_routes(b"%")):
    register(_route, _fresh)
for _negated in (False, True):
    register(in_list_route("dictionary", [3, 17, 17, 39, 1000, -4], _negated), in_list_route("dictionary", [17], _negated))
    register(in_list_route("unencoded", [3, 17, 17, 39, 1000, -4], _negated), in_list_route("unencoded", [17], _negated))
register(Route("validate", "mvcc",
               lambda w, ref, ex, n_ex, out: abi.load_library().hy_validate(w.column("mvcc", ref)[1].handle, 2, 15, 1, out),
               lambda w, ref: from_oracle(oracle_validate(w.column("mvcc", ref)[0], 2, 15, True)), excludes=False))
register(Route("columns_ints", "dictionary",
               lambda w, ref, ex, n_ex, out: abi.load_library().hy_table_scan_columns(w.column("dictionary", ref)[1].handle, w.column("unencoded", ref)[1].handle, abi.PRED_LESS_THAN, out),
               lambda w, ref: from_oracle(oracle_scan_columns(w.column("dictionary", ref)[0], w.column("unencoded", ref)[0], abi.PRED_LESS_THAN)), excludes=False))
register(Route("columns_strings", "strings",
               lambda w, ref, ex, n_ex, out: abi.load_library().hy_table_scan_columns_strings(w.column("strings", ref)[1].handle, w.left_dict.handle, w.column("strings_right", ref)[1].handle,
                                                                                            w.right_dict.handle, abi.PRED_LESS_THAN_EQUALS, out),
               lambda w, ref: from_oracle(oracle_scan_columns(w.column("twin_left", ref)[0], w.column("twin_right", ref)[0], abi.PRED_LESS_THAN_EQUALS)), excludes=False))


def string_list_routes(world):
    """The string lists hold entries of the column's own dictionaries (and one that no chunk holds): made once the column exists."""
    entries = [world.dictionaries[0][3], world.dictionaries[1][7], world.dictionaries[0][3], b"no such entry"]
    return {(negated, fresh): in_list_route("strings", entries[:1] if fresh else entries, negated) for negated in (False, True) for fresh in (False, True)}


STRING_LISTS = ("in_strings", "not_in_strings")
ALL_ROUTES = list(ROUTES) + list(STRING_LISTS)


def route_of(world, name, fresh=False):
    if name in STRING_LISTS:
        return string_list_routes(world)[(name == "not_in_strings", fresh)]
    return (FRESH if fresh else ROUTES)[name]


# ---- running a route -----------------------------------------------------------------------------------------------------------------------
def run(world, route, reference, device_result, excluded=()):
    """The route's result per chunk: (chunk state, count, the chunk's RowIDs as written)."""
    _, dev = world.column(route.column, reference)
    excluded_array = np.ascontiguousarray(excluded, dtype=np.uint32)
    ex, n_ex = (excluded_array.ctypes.data if len(excluded) else None), len(excluded)
    n_chunks, rows = dev.n_chunks, dev.rows
    if not device_result:
        result = HostScanResult(n_chunks, rows)
        abi.check(route.call(world, reference, ex, n_ex, C.byref(result.c)))
        return [(int(result.chunk_state[c]), int(result.counts[c]), result.pos_list(c).copy()) for c in range(n_chunks)]
    import torch
    matches = torch.zeros((rows + 2, 2), dtype=torch.int32, device="cuda")   # (16 bytes of slack behind the last RowID)
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(n_chunks, dtype=torch.int32, device="cuda")
    chunk_state = torch.zeros(n_chunks, dtype=torch.uint8, device="cuda")
    r = abi.ScanResult()
    r.mem, r.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS
    r.matches, r.capacity = matches.data_ptr(), rows
    r.offsets, r.counts, r.chunk_state = offsets.data_ptr(), counts.data_ptr(), chunk_state.data_ptr()
    abi.check(route.call(world, reference, ex, n_ex, C.byref(r)))
    abi.check(abi.load_library().hy_synchronize())
    matches, offsets, counts, chunk_state = matches.cpu().numpy().view(np.uint32), offsets.cpu().numpy(), counts.cpu().numpy().view(np.uint32), chunk_state.cpu().numpy()
    sizes = [s.size for s in world.column(route.column, reference)[0].segments]
    assert offsets[:n_chunks].tolist() == np.concatenate([[0], np.cumsum(sizes)])[:n_chunks].tolist(), "a chunk's region begins at the chunk's first row"
    out = []
    for c in range(n_chunks):
        elided = chunk_state[c] == abi.CHUNK_ALL_MATCH
        out.append((int(chunk_state[c]), int(counts[c]), None if elided else matches[int(offsets[c]):int(offsets[c]) + int(counts[c])].copy()))
    return out


def assert_route(got, want, excluded, context):
    assert len(got) == len(want), context
    for c, ((state, count, rows), (want_state, want_count, want_rows)) in enumerate(zip(got, want)):
        where = f"{context} chunk {c}"
        if c in excluded:
            assert state == abi.CHUNK_NONE_MATCH and count == 0 and (rows is None or len(rows) == 0), where
            continue
        if want_state == abi.CHUNK_ALL_MATCH:      # (no RowIDs are written: the count says how many rows the chunk has)
            assert state == abi.CHUNK_ALL_MATCH and count == want_count, where
            continue
        assert count == want_count == len(want_rows), where
        assert rows is not None and rows.tobytes() == want_rows.tobytes(), where
        if want_state is None:
            assert state != abi.CHUNK_ALL_MATCH and (state != abi.CHUNK_NONE_MATCH or count == 0), where
        else:
            assert state == want_state, where


WANTED = {}


def wanted(world, name, reference, fresh=False):
    key = (name, reference, fresh)
    if key not in WANTED:
        WANTED[key] = route_of(world, name, fresh).want(world, reference)
    return WANTED[key]


@pytest.mark.parametrize("name", ALL_ROUTES)
def test_route_over_data_and_reference_columns(world, name):
    route = route_of(world, name)
    for reference in (False, True):
        for device_result in (False, True):
            got = run(world, route, reference, device_result)
            assert_route(got, wanted(world, name, reference), (), f"{name} reference {reference} device result {device_result}")


@pytest.mark.parametrize("name", [n for n in ALL_ROUTES if n in STRING_LISTS or ROUTES[n].excludes])
def test_route_with_excluded_chunks(world, name):
    route = route_of(world, name)
    for device_result in (False, True):
        got = run(world, route, False, device_result, EXCLUDED)
        assert_route(got, wanted(world, name, False), EXCLUDED, f"{name} excluded {EXCLUDED} device result {device_result}")


@pytest.mark.parametrize("name", ALL_ROUTES)
def test_route_as_the_first_call_of_a_new_thread(world, name):
    """A new thread has a new scratch arena: its first reservation is this call's sizing and nothing else."""
    route = route_of(world, name, fresh=True)
    want = wanted(world, name, False, fresh=True)
    for device_result in (False, True):
        outcome = {}

        def body():
            try:
                outcome["got"] = run(world, route, False, device_result)
            except BaseException as error:   # noqa: BLE001 (handed to the asserting thread)
                outcome["error"] = error
            finally:
                abi.load_library().hy_shutdown()

        thread = threading.Thread(target=body)
        thread.start()
        thread.join()
        assert "error" not in outcome, f"{name} device result {device_result}: {outcome.get('error')!r}"
        assert_route(outcome["got"], want, (), f"{name} on a new thread, device result {device_result}")


def test_excluded_chunks_on_a_reference_column_are_refused(world):
    lib = abi.load_library()
    excluded = np.array(EXCLUDED, dtype=np.uint32)
    for name in ("literal", "in_dictionary", "like_device"):
        route = ROUTES[name]
        _, dev = world.column(route.column, True)
        result = HostScanResult(dev.n_chunks, dev.rows)
        assert route.call(world, True, excluded.ctypes.data, len(excluded), C.byref(result.c)) == abi.ERR_INVALID, name
        assert b"excluded chunks" in lib.hy_last_error(), name
        assert not result.matches.any() and not result.counts.any() and not result.offsets.any(), name

"""pk_emit's compact flavour (csrc/join_pk_stage.hpp, csrc/join_pkfk.hpp): where every segment of the probe column is FrameOfReference
with offsets of 1 or 2 bytes, a staged pair is ONE word -- row | null partner << 13 | (rank - the wave's rank base) << 16 -- and three
workgroups share a CU.  The shapes are the smallest that can break a 16-bit delta or a 4-byte slot, not the workload's:

  probe layout   chunks of 10 245, 65 535 and 1 rows: a tile boundary inside a chunk, a partial FrameOfReference block, a partial last
                 wave, a one-row tile, a 65 535-row chunk whose last slice is short.  An Inner join builds its smaller side, so its probe
                 column repeats the three chunks until it has more rows than the build side; the other modes take them once.
  extreme span   the first 2048-row block holds keys M .. M + 65 535 with both ends in the build side: against every key of
                 [0, 200 000) the delta reaches 65 535 exactly; against every third key the block's rows have partners, null partners and
                 no pair, mixed inside one wave.  The two extreme keys lie in one wave, or in the two waves of the block.
  must stay wide a column whose second chunk needs 4-byte offsets, and a plain int32 value column: the accessor says 0.

Every case compares the device result with the CPU oracle pair for pair, order included, asserts the route through
hy_debug_join_compact_stage, runs a second time over the resident build column (the hinted fill) and once more with
HY_OPT_JOIN_COMPACT_STAGE = 0, which must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import join_hash
from hyrise_amd.storage import DeviceColumn
from support import oracle_join
from test_join_gpu import _device_buffer, _read_back, assert_join_equal, used_pkfk

pytestmark = pytest.mark.gpu

SEMI = (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE)
MODES = (abi.JOIN_INNER, abi.JOIN_LEFT) + SEMI
CHUNKS = (10_245, 65_535, 1)
FOR_BLOCK = 2048
KEY_END = 200_000                    # build keys: every key, or every third key, of [0, KEY_END)
M = 30_000                           # the extreme block's minimum: M and M + 65 535 are multiples of 3, inside [0, KEY_END)
EXTREME_ROWS = {"same_wave": (5, 1000), "different_waves": (5, 1500)}   # rows of the first block that hold M and M + 65 535 (a wave: 1024 rows)


def compact_stage():
    lib = abi.load_library()
    lib.hy_debug_join_compact_stage.restype = C.c_int
    return int(lib.hy_debug_join_compact_stage())


def ragged_column(values, sizes, encodings):
    segments, begin = [], 0
    for size, encoding in zip(sizes, encodings):
        segments.append(storage.encode_segment(values[begin:begin + size], None, encoding))
        begin += size
    assert begin == len(values)
    return storage.HostColumn(segments, abi.TYPE_INT)


def narrow_keys(width, sizes, extreme, seed):
    """Keys whose every 2048-row block of every chunk spans at most 65 536 (width 2) or 256 (width 1) values: block bases from below the
    build range to above it, offsets over the whole span.  Width 2: the first block is the extreme one."""
    rng = np.random.default_rng(seed)
    span = 65_536 if width == 2 else 256
    chunks = []
    for size in sizes:
        blocks = (size + FOR_BLOCK - 1) // FOR_BLOCK
        bases = rng.integers(-20_000, KEY_END - span // 2, blocks)
        keys = np.repeat(bases, FOR_BLOCK)[:size] + rng.integers(0, span, size)
        if size >= FOR_BLOCK:   # the first and the last offset of the span, so that the chunk is stored `width` bytes wide and not narrower
            keys[FOR_BLOCK:2 * FOR_BLOCK][:2] = bases[1], bases[1] + span - 1
        chunks.append(keys)
    if width == 2:
        first = M + rng.integers(0, 65_536, FOR_BLOCK)
        low, high = EXTREME_ROWS[extreme]
        first[low], first[high] = M, M + 65_535
        chunks[0][:FOR_BLOCK] = first
    return np.concatenate(chunks).astype(np.int32)


def probe_column(width, repeats=1, extreme="same_wave", seed=1):
    sizes = CHUNKS * repeats
    column = ragged_column(narrow_keys(width, sizes, extreme, seed), sizes, [abi.ENC_FRAME_OF_REFERENCE] * len(sizes))
    assert all(segment.width == width for segment in column.segments if segment.size >= FOR_BLOCK), [segment.width for segment in column.segments]
    assert all(segment.width in (1, 2) for segment in column.segments)
    return column


def build_side(name):
    """dense: every key of [0, 200 000) in 65 535-row chunks -- the identity build, a rank is a row number.  sparse: every third key,
    dictionary-encoded in 20 000-row chunks -- sorted but no identity: the rank table is filled with RowIDs behind it.
    gappy: every key of [0, 100 000), then every 37th -- the rank table has words without a key (and without an entry) between ranks
    above 65 536: a wave's rank base can only come from keys that are present."""
    if name == "gappy":
        keys = np.concatenate([np.arange(100_000), np.arange(100_000, KEY_END, 37)]).astype(np.int32)
        return ragged_column(keys, (65_535, len(keys) - 65_535), [abi.ENC_UNENCODED] * 2)
    if name == "dense":
        return ragged_column(np.arange(KEY_END, dtype=np.int32), (65_535, 65_535, 65_535, KEY_END - 3 * 65_535), [abi.ENC_UNENCODED] * 4)
    keys = np.arange(0, KEY_END, 3, dtype=np.int32)
    sizes = [20_000] * (len(keys) // 20_000) + [len(keys) % 20_000]
    return ragged_column(keys, sizes, [abi.ENC_DICTIONARY] * len(sizes))


@pytest.fixture(scope="module")
def builds():
    return {name: build_side(name) for name in ("dense", "sparse", "gappy")}


@pytest.fixture(scope="module")
def oracle_results():
    return {}


def run(options, oracle_results, build_host, probe_host, mode, radix_bits, context, key, expect_compact=1):
    """The join twice over one resident build column (the second fill is hinted), then with the switch off: the route, the oracle's
    pairs in the oracle's order, and the same bytes from both routes."""
    args_host = (probe_host, build_host) if mode in SEMI or mode == abi.JOIN_LEFT else (build_host, probe_host)
    if not (mode in SEMI or mode == abi.JOIN_LEFT):
        assert probe_host.rows > build_host.rows, "an Inner join builds its smaller side"
    if key not in oracle_results:
        oracle_results[key] = oracle_join(*args_host, mode, radix_bits)
    want = oracle_results[key]
    args = tuple(DeviceColumn(column) for column in args_host)
    results = []
    for attempt in ("first", "second", "switch off"):
        if attempt == "switch off":
            options.set(abi.OPT_JOIN_COMPACT_STAGE, 0)
        got = join_hash(*args, mode, radix_bits)
        assert used_pkfk() == 1, f"{context} {attempt}"
        assert compact_stage() == (0 if attempt == "switch off" else expect_compact), f"{context} {attempt}"
        assert_join_equal(got, want, mode, f"{context} {attempt}")
        results.append(got)
    options.reset(abi.OPT_JOIN_COMPACT_STAGE)
    n = want.n_pairs
    for got in results[:2]:
        assert got.left[:n].tobytes() == results[2].left[:n].tobytes() and got.right[:n].tobytes() == results[2].right[:n].tobytes(), context
    return want


@pytest.mark.parametrize("build_name", ("dense", "sparse", "gappy"))
@pytest.mark.parametrize("width", (2, 1))
def test_compact_stage_every_mode(device, options, builds, oracle_results, width, build_name):
    """Inner, Left (the null-partner bit beside a delta of up to 65 535), Semi and both Anti joins (no build side is written: one PosList),
    without radix partitioning and with 128 partitions, over the identity build, the build with RowIDs behind the ranks and the build
    whose table has empty words."""
    build = builds[build_name]
    once, repeated = probe_column(width), probe_column(width, repeats=3)
    for mode in MODES:
        probe = repeated if mode == abi.JOIN_INNER else once
        for radix_bits in (0, 7):
            run(options, oracle_results, build, probe, mode, radix_bits, f"width {width} {build_name} mode {mode} radix {radix_bits}", (width, build_name, mode, radix_bits))


@pytest.mark.parametrize("extreme", sorted(EXTREME_ROWS))
def test_compact_stage_extreme_span(device, options, builds, oracle_results, extreme):
    """The block whose keys run from M to M + 65 535, both present in the build side.  Dense build: the two partners' ranks are 65 535
    apart -- the largest delta a record can hold.  Sparse build: partners, null partners (Left) and rows without a pair inside one wave."""
    dense = builds["dense"].segments
    assert dense[0].size == 65_535   # (ranks are row numbers: M and M + 65 535 are 65 535 ranks apart)
    once, repeated = probe_column(2, extreme=extreme, seed=2), probe_column(2, repeats=3, extreme=extreme, seed=2)
    for build_name in ("dense", "sparse"):
        for mode in (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_ANTI_NULL_AS_FALSE):
            probe = repeated if mode == abi.JOIN_INNER else once
            for radix_bits in (0, 7):
                want = run(options, oracle_results, builds[build_name], probe, mode, radix_bits, f"extreme {extreme} {build_name} mode {mode} radix {radix_bits}",
                           ("extreme", extreme, build_name, mode, radix_bits))
                if build_name == "dense" and mode == abi.JOIN_INNER and radix_bits == 0:   # both extreme rows found their partners
                    low, high = EXTREME_ROWS[extreme]
                    pairs = {(int(p[0]), int(p[1])): (int(b[0]), int(b[1])) for b, p in zip(want.left[:FOR_BLOCK], want.right[:FOR_BLOCK])}
                    assert pairs[(0, low)] == (M // 65_535, M % 65_535) and pairs[(0, high)] == ((M + 65_535) // 65_535, (M + 65_535) % 65_535)


def test_compact_stage_256_partitions(device, options, builds, oracle_results):
    """radix_bits 8: the largest LDS footprint of the compact flavour.  Once into host memory against the oracle, once into device
    memory of exactly the result's size: the launch succeeds and writes nothing behind the pairs."""
    build_host, probe_host = builds["dense"], probe_column(2, repeats=3, seed=3)
    want = run(options, oracle_results, build_host, probe_host, abi.JOIN_INNER, 8, "radix 8", ("radix 8",))
    build, probe = DeviceColumn(build_host), DeviceColumn(probe_host)
    n, slices = want.n_pairs, int(want.c.n_slices)
    p_left, like_pairs = _device_buffer(device, (n + 8, 2), np.uint32, 0xABABABAB)
    p_right, _ = _device_buffer(device, (n + 8, 2), np.uint32, 0xABABABAB)
    p_offsets, like_offsets = _device_buffer(device, (slices + 8,), np.uint64, 0xCDCDCDCDCDCDCDCD)
    r = abi.JoinResult()
    r.mem, r.radix_bits = abi.MEM_DEVICE, 8
    r.left_pos, r.right_pos, r.capacity = p_left, p_right, n
    r.slice_offsets, r.slice_capacity = p_offsets, slices
    abi.check(device.hy_join_hash(build.handle, probe.handle, abi.JOIN_INNER, C.byref(r)))
    assert compact_stage() == 1 and int(r.n_pairs) == n and int(r.n_slices) == slices
    got_left, got_right = _read_back(device, p_left, like_pairs), _read_back(device, p_right, like_pairs)
    assert got_left[:n].tobytes() == want.left[:n].tobytes() and got_right[:n].tobytes() == want.right[:n].tobytes()
    assert (got_left[n:] == 0xABABABAB).all() and (got_right[n:] == 0xABABABAB).all()
    assert _read_back(device, p_offsets, like_offsets)[:slices + 1].tobytes() == want.slice_offsets[:slices + 1].tobytes()
    for p in (p_left, p_right, p_offsets):
        device.hy_device_free(p)


@pytest.mark.parametrize("case", ("four_byte_chunk", "int32_values"))
def test_wide_columns_keep_the_eight_byte_records(device, options, builds, oracle_results, case):
    """One chunk with 4-byte offsets among 2-byte ones, or unencoded int32 values: the whole launch stays on today's kernels."""
    sizes = CHUNKS * 3
    keys = narrow_keys(2, sizes, "same_wave", 4)
    if case == "four_byte_chunk":
        keys[CHUNKS[0]:CHUNKS[0] + CHUNKS[1]] = np.random.default_rng(5).integers(-20_000, KEY_END + 20_000, CHUNKS[1])
        probe = ragged_column(keys, sizes, [abi.ENC_FRAME_OF_REFERENCE] * len(sizes))
        assert [segment.width for segment in probe.segments[:3]] == [2, 4, 1]
    else:
        probe = ragged_column(keys, sizes, [abi.ENC_UNENCODED] * len(sizes))
    for mode in (abi.JOIN_INNER, abi.JOIN_LEFT):
        for radix_bits in (0, 7):
            run(options, oracle_results, builds["dense"], probe, mode, radix_bits, f"{case} mode {mode} radix {radix_bits}", (case, mode, radix_bits), expect_compact=0)

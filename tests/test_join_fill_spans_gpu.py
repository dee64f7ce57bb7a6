"""The hinted wave fill (csrc/join.hip rank_table_fill_waves): every word of the rank table is stored once, by the wave
that owns it, into a block nobody zeroed.  Every case joins twice over one resident build column -- the first join leaves the key hint, the
second fills the table from it (hy_debug_join_build_was_hinted, hy_debug_join_used_rank_table) -- and both results equal the oracle's byte
for byte.  The shapes are the small ones at which the spans can go wrong: a step is 512 rows, a batch 4 steps; with so few rows a wave
takes one batch (2048 rows) and a workgroup four (8192 rows, a slice); a piece of a wave's window is 2048 table words.
What these shapes cannot reach: the device keeps thousands of waves resident, so below about 2 M rows no wave gets a second batch, and
what a wave carries from batch to batch (the pending word merged into the next batch's first word, or stored alone where the next batch
starts a later word, a wave that has not started after its first batch) runs only at full size: test_full_size_gpu.py's orders column
gives every wave two batches that share a word; the lone store of a pending word is not run by any test.
The hinted route has a second kernel (rank_table_fill_checked, for tables of more than two words per key and key ranges near 2^32) that
sets the same debug counters: wave_fill_shape asserts that a case's keys stay on the wave fill's side of those limits."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.operators import join_hash
from hyrise_amd.storage import DeviceColumn
from support import oracle_join
from test_join_gpu import _device_buffer, assert_join_equal, build_column, used_rank_table

pytestmark = pytest.mark.gpu

BUILD_ON_THE_RIGHT = (abi.JOIN_LEFT, abi.JOIN_SEMI)


def was_hinted():
    lib = abi.load_library()
    lib.hy_debug_join_build_was_hinted.restype = C.c_int
    return int(lib.hy_debug_join_build_was_hinted())


def probe_column(keys, seed, rows=None):
    """More rows than the build side (JoinHash builds over the smaller input of an Inner join), one in twenty without a partner: keys in
    the build side's gaps and around its range -- the Bloom filter has something to reject."""
    rng = np.random.default_rng(seed)
    rows = rows or len(keys) + 2000
    drawn = rng.choice(keys, rows).astype(np.int32)
    lonely = rng.random(rows) < 0.05
    lonely[:3] = True
    drawn[lonely] = rng.integers(int(keys.min()) - 200, int(keys.max()) + 200, int(lonely.sum())).astype(np.int32)
    return build_column(drawn, None, 65535, abi.ENC_UNENCODED)


def sides(build, probe, mode):
    return (probe, build) if mode in BUILD_ON_THE_RIGHT else (build, probe)


def wave_fill_shape(keys):
    """fill_hinted's limits for rank_table_fill_waves (csrc/join.hip: FW_SPARSE_WORDS_PER_KEY, FW_RANGE_LIMIT), with the hint's origin."""
    origin = int(keys.min()) & ~31
    words = ((int(keys.max()) - origin) >> 5) + 1
    return words <= 2 * len(keys) and int(keys.max()) - origin < (1 << 32) - 2048 * 32


def join_twice(build_host, probe_host, context, modes=(abi.JOIN_INNER,), columns=None, keys=None):
    """An Inner join that leaves the hint (or finds it, where `columns` have joined before), then one hinted join per mode."""
    assert keys is not None and wave_fill_shape(keys), f"{context}: these keys would take the per-slice fill"
    build, probe = columns or (DeviceColumn(build_host), DeviceColumn(probe_host))
    wanted = {mode: oracle_join(*sides(build_host, probe_host, mode), mode) for mode in set(modes) | {abi.JOIN_INNER}}
    if columns is None:
        got = join_hash(build, probe, abi.JOIN_INNER)
        assert (was_hinted(), used_rank_table()) == (0, 2), f"{context}: the first join fills the identity table"
        assert_join_equal(got, wanted[abi.JOIN_INNER], abi.JOIN_INNER, f"{context}, first join")
    for mode in modes:
        got = join_hash(*sides(build, probe, mode), mode)
        assert (was_hinted(), used_rank_table()) == (1, 2), f"{context}, mode {mode}: the hinted fill"
        assert_join_equal(got, wanted[mode], mode, f"{context}, hinted join, mode {mode}")
    return build, probe


def dbgen_keys(rows, first=1):
    i = np.arange(first, first + rows, dtype=np.int64)
    return (((i >> 3) << 5) | (i & 7)).astype(np.int32)   # 8 of every 32 integers


@pytest.mark.parametrize("width", [4, 2, 1])
def test_stored_widths(device, width):
    """int32 values, FrameOfReference offsets of 2 bytes and of 1 byte (chunks of 200 rows: a slice and a workgroup each); the last chunk is
    shorter than the others."""
    if width == 4:
        keys, chunk, encoding = dbgen_keys(50_000), 20_000, abi.ENC_UNENCODED
    elif width == 2:
        keys, chunk, encoding = (np.arange(50_000, dtype=np.int32) * 3 - 40_000), 20_000, abi.ENC_FRAME_OF_REFERENCE
    else:
        i = np.arange(6_100, dtype=np.int32)
        keys, chunk, encoding = i + i // 8 + 1000, 200, abi.ENC_FRAME_OF_REFERENCE
    build = build_column(keys, None, chunk, encoding)
    assert all(segment.width == width for segment in build.segments)
    join_twice(build, probe_column(keys, 10 + width), f"width {width}", keys=keys)


@pytest.mark.parametrize("first_key", [0, 16, -4099])
def test_word_edges(device, first_key):
    """Consecutive keys.  From 0: every step's last key has key % 32 == 31 and the next step's first key % 32 == 0 -- no word is shared.
    From 16 (and from -4099, origin -4128): a table word's keys straddle every step, wave (2048 rows), workgroup (8192 rows) and chunk
    (20 000 rows: slices of 8192, 8192 and 3616 rows) boundary."""
    keys = np.arange(45_000, dtype=np.int32) + first_key
    if first_key == 0:
        assert keys[511] % 32 == 31 and keys[512] % 32 == 0
    else:
        assert all((keys[r - 1] - first_key // 32 * 32) // 32 == (keys[r] - first_key // 32 * 32) // 32 for r in (512, 2048, 8192, 20_000))
    join_twice(build_column(keys, None, 20_000, abi.ENC_UNENCODED), probe_column(keys, 20), f"consecutive keys from {first_key}", keys=keys)


@pytest.mark.parametrize("row", [1000, 4096, 4097, 20_000], ids=["inside_a_wave", "at_a_wave_boundary", "behind_a_wave_boundary", "at_a_chunk_boundary"])
def test_one_long_gap(device, row):
    """70 000 empty table words between two consecutive keys: inside a wave's rows (in the middle of a step), exactly at a wave boundary
    (the wave in front owns the gap), one row behind it, at a chunk boundary.  40 000 rows: 71 251 words <= 2 x rows + 4096."""
    keys = np.arange(40_000, dtype=np.int64) + 5
    keys[row:] += 70_000 * 32
    keys = keys.astype(np.int32)
    assert (int(keys[-1]) >> 5) + 1 <= 2 * len(keys) + 4096
    join_twice(build_column(keys, None, 20_000, abi.ENC_UNENCODED), probe_column(keys, 30 + row), f"gap in front of row {row}", keys=keys)


def test_sparse_batches(device):
    """Keys 40 apart: a batch of 2048 rows spans 2560 table words, more than a window -- every batch leaves in two pieces; then a stretch
    320 apart (the table stays under 65 536 words)."""
    keys = np.concatenate([np.arange(30_000, dtype=np.int64) * 40, 30_000 * 40 + np.arange(2_000, dtype=np.int64) * 320]).astype(np.int32)
    assert (int(keys[-1]) >> 5) + 1 <= 65_536
    join_twice(build_column(keys, None, 20_000, abi.ENC_UNENCODED), probe_column(keys, 40), "sparse batches", keys=keys)


@pytest.mark.parametrize("rows", [1, 511, 513])
def test_small_columns(device, rows):
    keys = dbgen_keys(rows, first=77)
    join_twice(build_column(keys, None, 65_535, abi.ENC_UNENCODED), probe_column(keys, 50 + rows, rows=rows + 300), f"{rows} rows", keys=keys)


def test_ragged_chunks(device):
    """Chunks of 8195 rows (a slice of 8192 rows and one of 3), the last chunk shorter; the words straddle the three-row slices."""
    keys = np.arange(30_000, dtype=np.int32) * 2 + 7
    join_twice(build_column(keys, None, 8195, abi.ENC_UNENCODED), probe_column(keys, 60), "ragged chunks", keys=keys)


def test_stale_memory(device):
    """Dense A, sparse B with a smaller range, A again, on one thread: no table is zeroed between the joins, whatever block a fill gets holds
    what an earlier join left there."""
    a_keys = np.arange(60_000, dtype=np.int32) + 3
    b_keys = (np.arange(3_000, dtype=np.int32) * 16 + 11)
    a_build, a_probe = build_column(a_keys, None, 20_000, abi.ENC_UNENCODED), probe_column(a_keys, 70)
    b_build, b_probe = build_column(b_keys, None, 20_000, abi.ENC_UNENCODED), probe_column(b_keys, 71)
    a = join_twice(a_build, a_probe, "A", keys=a_keys)
    b = join_twice(b_build, b_probe, "B behind A", keys=b_keys)
    join_twice(a_build, a_probe, "A behind B", columns=a, keys=a_keys)
    join_twice(b_build, b_probe, "B behind A behind B", columns=b, keys=b_keys)
    join_twice(a_build, a_probe, "A, all three modes", modes=(abi.JOIN_SEMI, abi.JOIN_LEFT, abi.JOIN_INNER), columns=a, keys=a_keys)


@pytest.mark.parametrize("mode", [abi.JOIN_INNER, abi.JOIN_SEMI, abi.JOIN_LEFT])
def test_modes(device, mode):
    """Inner, Semi and Left over one hinted build side; the probe side has rows without a partner (the Bloom filter folded from the table's
    words rejects them, or lets them through to the table)."""
    keys = dbgen_keys(30_000)
    join_twice(build_column(keys, None, 20_000, abi.ENC_UNENCODED), probe_column(keys, 80 + mode), f"mode {mode}", modes=(mode, mode), keys=keys)


@pytest.mark.parametrize("shape", ["four_per_key", "a_word_of_300_rows", "a_word_of_5000_rows"])
def test_repeated_keys(device, shape):
    """Semi joins only ask whether a key exists: a sorted build column whose keys repeat keeps its hint (duplicates allowed), and the wave
    that owns a table word looks as far behind its rows as the word's keys reach -- 64 rows at a time, 4096 at the most.  Up to seven rows
    per key, lineitem's shape (a word's keys straddle every boundary); one word whose keys fill 300 rows across a wave boundary; one whose
    keys fill 5000 rows -- the fill reports keys that do not fit the hint and the join runs again without it."""
    rng = np.random.default_rng(7)
    distinct = dbgen_keys(12_000)
    counts = rng.integers(1, 8, len(distinct))
    if shape != "four_per_key":
        inside = np.flatnonzero((distinct >> 5) == (distinct[1000] >> 5))    # the eight keys of one table word, from row ~ 4000 on
        counts[inside] = (300 if shape == "a_word_of_300_rows" else 5000) // len(inside) + 1
    keys = np.repeat(distinct, counts)
    assert wave_fill_shape(keys)
    if shape != "four_per_key":
        first_row = int(counts[:inside[0]].sum())
        assert first_row < 4096 < first_row + int(counts[inside].sum()), "the word's rows lie across the boundary of two waves"
    build_host = build_column(keys, None, 20_000, abi.ENC_FRAME_OF_REFERENCE)
    probe_keys = np.concatenate([distinct, distinct + 9]).astype(np.int32)      # (distinct + 9: never a key -- bits 8.. of a word are empty)
    probe_host = build_column(np.repeat(probe_keys, 3), None, 65535, abi.ENC_UNENCODED)
    build, probe = DeviceColumn(build_host), DeviceColumn(probe_host)
    want = oracle_join(probe_host, build_host, abi.JOIN_SEMI)
    for attempt in range(3):
        got = join_hash(probe, build, abi.JOIN_SEMI)
        if shape == "a_word_of_5000_rows":
            assert was_hinted() == (0, 2, 0)[attempt], "the hinted attempt is discarded, the hint dropped"
        else:
            assert (was_hinted(), used_rank_table()) == (min(attempt, 1), 2), f"{shape}, attempt {attempt}"
        assert_join_equal(got, want, abi.JOIN_SEMI, f"{shape}, attempt {attempt}")


class CallerOwnedColumn:
    """An int32 column over caller-owned device memory (HY_MEM_DEVICE): what lies in that memory can change behind a hint."""

    def __init__(self, lib, pointer, rows, chunk):
        self.lib, self.rows = lib, rows
        self.n_chunks = (rows + chunk - 1) // chunk
        self.segments = (abi.Segment * self.n_chunks)()
        for c in range(self.n_chunks):
            s = self.segments[c]
            s.encoding, s.data_type, s.size, s.width = abi.ENC_UNENCODED, abi.TYPE_INT, min(chunk, rows - c * chunk), 4
            s.data = pointer + 4 * c * chunk
        self.handle = C.c_void_p()
        abi.check(lib.hy_column_create(self.segments, self.n_chunks, abi.MEM_DEVICE, C.byref(self.handle)))

    def close(self):
        abi.check(self.lib.hy_column_destroy(self.handle))


BROKEN = {
    "two_keys_swapped": lambda keys: keys.__setitem__([12_345, 30_000], keys[[30_000, 12_345]]),
    "neighbours_swapped_across_a_wave": lambda keys: keys.__setitem__([2047, 2048], keys[[2048, 2047]]),
    "one_key_duplicated": lambda keys: keys.__setitem__(20_001, keys[20_000]),
    "last_key_outside": lambda keys: keys.__setitem__(len(keys) - 1, keys[-1] + 6400),
    "first_key_outside": lambda keys: keys.__setitem__(0, keys[0] - 6400),
    "a_key_far_outside": lambda keys: keys.__setitem__(9_000, np.int32(2_000_000_000)),
}


@pytest.mark.parametrize("how", list(BROKEN) + ["option"])
def test_broken_hint(device, options, how):
    """The first join leaves the hint, then the column's memory changes (or HY_OPT_JOIN_BREAK_HINT shortens the hinted range): the fill's
    records contradict the hint, the join's output is discarded and the two-pass build answers -- the oracle's result over the keys as
    they are now."""
    lib = device
    rows, chunk = 40_000, 16_384
    keys = np.arange(rows, dtype=np.int32) * 2 + 64
    probe_host = probe_column(keys, 90)
    probe = DeviceColumn(probe_host)
    pointer, _ = _device_buffer(lib, keys.shape, np.int32, 0)
    abi.check(lib.hy_memcpy_h2d(pointer, keys.ctypes.data, keys.nbytes))
    build = CallerOwnedColumn(lib, pointer, rows, chunk)
    try:
        first = join_hash(build, probe, abi.JOIN_INNER)
        assert (was_hinted(), used_rank_table()) == (0, 2)
        assert_join_equal(first, oracle_join(build_column(keys, None, chunk, abi.ENC_UNENCODED), probe_host, abi.JOIN_INNER), abi.JOIN_INNER, "before")
        now = keys.copy()
        if how == "option":
            options.set(abi.OPT_JOIN_BREAK_HINT, 1)
        else:
            BROKEN[how](now)
            abi.check(lib.hy_memcpy_h2d(pointer, now.ctypes.data, now.nbytes))
        got = join_hash(build, probe, abi.JOIN_INNER)
        assert was_hinted() == 2, "the hinted attempt was discarded"
        assert_join_equal(got, oracle_join(build_column(now, None, chunk, abi.ENC_UNENCODED), probe_host, abi.JOIN_INNER), abi.JOIN_INNER, how)
    finally:
        build.close()
        lib.hy_device_free(pointer)

"""pk_emit / pk_cuts per stored width (csrc/join_pkfk.hpp pk_tile_rows): the evaluation of a tile's rows is one specialisation per width
of the probe column's stored words -- FrameOfReference offsets of 1, 2 and 4 bytes, unencoded int32 values -- picked once per tile.
Probe columns of every kind, and one whose chunks mix the kinds (neighbouring tiles of one launch take different specialisations), with row
counts that end inside a 16-row piece, a 64-row round, a 1024-row wave and a tile; every join mode over a unique int32 build column that
about half the probe keys miss (in range without a partner, below the range, above it: the Bloom re-test, the null partners of the
non-Inner staging); radix_bits 0 and 7 (the 131 070-element cuts evaluate the rows once more); the build side's bits in LDS
(pk_emit<., true>) and ranks handed over by pass 1 (pk_emit<true, false, true>, at the probe size at which the host chooses it unasked).
PosLists and cuts byte-equal to the oracle.

An Inner join builds its smaller side, so an Inner join's probe column has more rows than the build side (N_BUILD); the row counts below
that run in the modes whose build side is fixed (Left: the kernels' non-Inner form, Semi)."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi
from hyrise_amd.operators import join_hash
from hyrise_amd.storage import DeviceColumn
from support import build_column, oracle_join

pytestmark = pytest.mark.gpu

MODES = [abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_RIGHT, abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE]
SEMI = (abi.JOIN_SEMI, abi.JOIN_ANTI_NULL_AS_TRUE, abi.JOIN_ANTI_NULL_AS_FALSE)
TILE = 8192
FOR_BLOCK = 2048
ROW_COUNTS = (1, 15, 17, 63, 65, 1023, 1025, 8191, 8193)
N_BUILD = 100_000
KEY_MIN = 1000                       # build keys: KEY_MIN + 2 i -- unique, sorted; every odd key of the range has no partner
KEY_END = KEY_MIN + 2 * N_BUILD
KINDS = ("for8", "for16", "for32", "int32")
WIDTH = {"for8": 1, "for16": 2, "for32": 4}


def used_pkfk():
    lib = abi.load_library()
    lib.hy_debug_join_used_pkfk.restype = C.c_int
    return int(lib.hy_debug_join_used_pkfk())


@pytest.fixture(scope="module")
def build():
    return build_column((KEY_MIN + 2 * np.arange(N_BUILD)).astype(np.int32), None, 65535, abi.ENC_UNENCODED)


def chunk_keys(kind, rows, rng):
    """One chunk's probe keys, about half of them without a partner.  for8: every 2048-row block spreads over fewer than 256 key values
    somewhere in the build range; for16: over fewer than 65 536, reaching below the build range or above it; for32 / int32: over the
    build range and 50 000 keys to either side (more than 65 536 key values as soon as the chunk has a few rows)."""
    if kind == "for8":
        bases = rng.integers(KEY_MIN - 100, KEY_END - 100, (rows + FOR_BLOCK - 1) // FOR_BLOCK)
        return (np.repeat(bases, FOR_BLOCK)[:rows] + rng.integers(0, 250, rows)).astype(np.int32)
    if kind == "for16":
        base = (KEY_MIN - 30_000, KEY_END - 30_000, 60_000)[int(rng.integers(0, 3))]
        return (base + rng.integers(0, 60_000, rows)).astype(np.int32)
    return rng.integers(KEY_MIN - 50_000, KEY_END + 50_000, rows).astype(np.int32)


def probe_column(kinds, chunk, n_chunks, seed):
    """n_chunks chunks of `chunk` rows, chunk c of kind kinds[c % len(kinds)]."""
    rng = np.random.default_rng(seed)
    kinds = [kinds[c % len(kinds)] for c in range(n_chunks)]
    values = np.concatenate([chunk_keys(kind, chunk, rng) for kind in kinds])
    column = build_column(values, None, chunk, [abi.ENC_UNENCODED if kind == "int32" else abi.ENC_FRAME_OF_REFERENCE for kind in kinds])
    if chunk >= 1023:   # (a chunk of a few rows spreads over less than its kind allows: it is stored narrower, and that is fine)
        for kind, segment in zip(kinds, column.segments):
            assert kind == "int32" or segment.width == WIDTH[kind], f"{kind} chunk of {chunk} rows stored in {segment.width} bytes"
    return column


def run(build, probe, mode, radix_bits, context, expect=1):
    args = (probe, build) if mode in SEMI or mode == abi.JOIN_LEFT else (build, probe)
    capacity = probe.rows + build.rows + 1
    want = oracle_join(*args, mode, radix_bits)
    assert want.n_pairs < capacity, context
    got = join_hash(DeviceColumn(args[0]), DeviceColumn(args[1]), mode, radix_bits, capacity=capacity)
    assert used_pkfk() == expect, context
    assert got.n_pairs == want.n_pairs, f"pair count {context}"
    assert got.c.n_slices == want.c.n_slices, f"slice count {context}"
    n, s = want.n_pairs, want.c.n_slices
    np.testing.assert_array_equal(got.slice_offsets[:s + 1], want.slice_offsets[:s + 1], err_msg=f"slices {context}")
    assert got.left[:n].tobytes() == want.left[:n].tobytes(), f"left PosList differs {context}"
    if mode not in SEMI:
        assert got.right[:n].tobytes() == want.right[:n].tobytes(), f"right PosList differs {context}"


def kinds_of(case):
    return KINDS if case == "mixed" else (case,)


@pytest.mark.parametrize("case", KINDS + ("mixed",))
def test_widths_every_mode(device, build, case):
    """Seven chunks of two tiles and 77 rows (the last tile of every chunk is partial), more rows than the build side: every mode,
    without radix partitioning and with 128 partitions."""
    probe = probe_column(kinds_of(case), 2 * TILE + 77, 7, 100 + len(case))
    assert probe.rows > N_BUILD
    for mode in MODES:
        for radix_bits in (0, 7):
            run(build, probe, mode, radix_bits, f"{case} mode {mode} radix {radix_bits}")


@pytest.mark.parametrize("case", KINDS + ("mixed",))
def test_widths_row_counts(device, build, case):
    """Chunks that end inside a 16-row piece, a 64-row round, a 1024-row wave and a tile.  Four chunks each in the modes whose build side
    is fixed; the counts from 1023 on also in as many chunks as make the probe side the larger one, in an Inner join."""
    for i, rows in enumerate(ROW_COUNTS):
        probe = probe_column(kinds_of(case), rows, 4, 200 + rows)
        for j, mode in enumerate((abi.JOIN_LEFT, abi.JOIN_SEMI)):
            radix_bits = (0, 7)[(i + j) % 2]
            run(build, probe, mode, radix_bits, f"{case} rows {rows} mode {mode} radix {radix_bits}")
        if rows >= 1023:
            probe = probe_column(kinds_of(case), rows, N_BUILD // rows + 4, 300 + rows)
            assert probe.rows > N_BUILD
            radix_bits = (7, 0)[i % 2]
            run(build, probe, abi.JOIN_INNER, radix_bits, f"{case} rows {rows} x {N_BUILD // rows + 4} inner radix {radix_bits}")


@pytest.mark.parametrize("mode", (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_ANTI_NULL_AS_FALSE))
def test_widths_bits_in_lds(device, build, options, mode):
    """pk_count_lds / pk_emit<., true>: a build key range below 2^20 and a selective build (one probe key in two has a partner); the mixed
    column, so that every width reads its rows' bits from pass 1's masks.  (The bar of 2048 tiles is lowered: the kernels are the same.)"""
    options.set(abi.OPT_JOIN_LDS_BUILD_TILES, 1)
    assert KEY_END - KEY_MIN < 1 << 20
    probe = probe_column(KINDS, 2 * TILE + 77, 8, 400)
    for radix_bits in (0, 7):
        run(build, probe, mode, radix_bits, f"lds mode {mode} radix {radix_bits}", expect=2)


def test_widths_handed_over_ranks(device):
    """pk_emit<true, false, true> where run_join chooses it unasked: an Inner join, a probe side of 2^20 rows (HY_OPT_JOIN_HAND_OVER_RANKS'
    default) whose neighbouring rows do not hold neighbouring keys, a rank table of a megabyte (2^22 key values) or more.  4-byte words only:
    1- and 2-byte offsets are local by construction and never take this path.  One chunk stays unencoded, the others are FrameOfReference
    with 4-byte offsets; the last tile is partial (the probe side is 2^20 + 77 rows)."""
    rng = np.random.default_rng(500)
    keys = np.sort(rng.choice(1 << 23, 300_000, replace=False)).astype(np.int32)
    assert int(keys[-1]) - int(keys[0]) >= 1 << 22
    big_build = build_column(keys, None, 65535, abi.ENC_UNENCODED)
    rows = (1 << 20) + 77
    values = np.where(rng.random(rows) < 0.5, keys[rng.integers(0, len(keys), rows)], rng.integers(0, 1 << 23, rows)).astype(np.int32)
    chunk = 65535
    n_chunks = (rows + chunk - 1) // chunk
    probe = build_column(values, None, chunk, [abi.ENC_UNENCODED if c == 1 else abi.ENC_FRAME_OF_REFERENCE for c in range(n_chunks)])
    assert all(segment.width == 4 for c, segment in enumerate(probe.segments) if c != 1)
    for radix_bits in (0, 7):
        run(big_build, probe, abi.JOIN_INNER, radix_bits, f"ranks radix {radix_bits}")

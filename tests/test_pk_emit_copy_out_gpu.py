"""pk_emit's copy-out (csrc/join_pkfk.hpp pk_copy_out): a tile's pairs leave by whole 128-byte output lines -- the lines wholly inside a
run with 16-byte nontemporal stores, a run's edge pairs (the lines it shares with the neighbouring tile's run) with 8-byte write-back
stores.  Probe columns built tile by tile so that the runs (pairs of one radix partition in one 8192-row tile) take the lengths around a
line's 16 pairs, start at every position in a line, fill a whole tile (radix 0) or split it 256 ways, in every join mode, with the
build-side bits in LDS (pk_emit<., true>), with ranks handed over by pass 1 and for each way of turning a rank into a RowID: pairs and
131 070-element cuts byte-equal to the oracle and to the general kernels (HY_OPT_JOIN_PKFK = 0)."""
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
RUN_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33)
N_BUILD = 100_000   # keys 0 .. N_BUILD - 1: a range of more than 65 536 keys (random probe keys count as scattered), fewer rows than every probe side
# (sorted keys in chunks of 65 535 rows: rank -> RowID by the 65 535 identity; in chunks of 4 096: the general identity; shuffled keys
#  in chunks of 4 096: packed 32-bit RowIDs; shuffled keys in chunks of more than 65 536 rows: 64-bit RowIDs)
BUILDS = (("identity_65535", False, 65535), ("identity", False, 4096), ("packed", True, 4096), ("row_ids", True, 100_000))


def used_pkfk():
    lib = abi.load_library()
    lib.hy_debug_join_used_pkfk.restype = C.c_int
    return int(lib.hy_debug_join_used_pkfk())


def assert_join_equal(got, want, mode, context):
    assert got.n_pairs == want.n_pairs, f"pair count {context}"
    assert got.c.n_slices == want.c.n_slices, f"slice count {context}"
    n, s = want.n_pairs, want.c.n_slices
    np.testing.assert_array_equal(got.slice_offsets[:s + 1], want.slice_offsets[:s + 1], err_msg=f"slices {context}")
    assert got.left[:n].tobytes() == want.left[:n].tobytes(), f"left PosList differs {context}"
    if mode not in SEMI:
        assert got.right[:n].tobytes() == want.right[:n].tobytes(), f"right PosList differs {context}"


def build_side(shuffled, chunk):
    keys = np.arange(N_BUILD, dtype=np.int32)
    if shuffled:
        keys = np.random.default_rng(5).permutation(keys)
    return build_column(keys, None, chunk, abi.ENC_UNENCODED)


def probe_keys(rng, radix_bits, tiles, all_match=False):
    """Tile by tile (the sizes in `tiles`): partition p of a full tile gets RUN_LENGTHS[(offset + p) % 9] rows whose key hits the build
    side (key & mask == p: the partition), the other rows miss it (keys above the build range); a tile too small for that gets matching
    keys of random partitions.  Returns the keys and the matching rows per (tile, partition)."""
    partitions = 1 << radix_bits
    out, counts = [], np.zeros((len(tiles), partitions), dtype=np.int64)
    for t, size in enumerate(tiles):
        want = np.array([RUN_LENGTHS[(t * 5 + p) % len(RUN_LENGTHS)] for p in range(partitions)], dtype=np.int64)
        if all_match or want.sum() > size:
            part = rng.integers(0, partitions, size)
        else:
            part = np.concatenate([np.repeat(np.arange(partitions), want), np.full(size - want.sum(), -1)])
        keys = np.where(part >= 0, (rng.integers(0, N_BUILD >> radix_bits, size) << radix_bits) | np.maximum(part, 0),
                        N_BUILD + rng.integers(0, 1 << 20, size))
        order = rng.permutation(size)
        keys, part = keys[order], part[order]
        counts[t] = np.bincount(part[part >= 0], minlength=partitions)
        out.append(keys)
    return np.concatenate(out).astype(np.int32), counts


def chunk_tiles(n_chunks, chunk):
    return [min(TILE, chunk - b) for _ in range(n_chunks) for b in range(0, chunk, TILE)]


def run(build, probe, mode, radix_bits, context, general=False, expect=1):
    args = (probe, build) if mode in SEMI or mode == abi.JOIN_LEFT else (build, probe)
    want = oracle_join(*args, mode, radix_bits)
    got = join_hash(DeviceColumn(args[0]), DeviceColumn(args[1]), mode, radix_bits)
    assert used_pkfk() == expect, context
    assert_join_equal(got, want, mode, context)
    if general:
        with abi.option(abi.OPT_JOIN_PKFK, 0):
            other = join_hash(DeviceColumn(args[0]), DeviceColumn(args[1]), mode, radix_bits)
            assert used_pkfk() == 0
        assert_join_equal(other, want, mode, context + " general kernels")


@pytest.mark.parametrize("mode", MODES)
def test_copy_out_run_lengths(device, mode):
    """Runs of 0, 1, 2, 15, 16, 17, 31, 32 and 33 pairs at every first pair index mod 16, 32 and 256 partitions, partial tiles (chunks
    of four tiles and 5 rows), every build flavour.  (The probe side has more rows than the build side: an Inner join builds the smaller one.)"""
    chunk = 4 * TILE + 5
    tiles = chunk_tiles(4, chunk)
    for radix_bits in (5, 8):
        probe_values, counts = probe_keys(np.random.default_rng(40 + radix_bits), radix_bits, tiles)
        lengths = set(counts[:-1].ravel().tolist())   # (the last tile's 5 rows aside)
        assert set(RUN_LENGTHS) <= lengths
        # an Inner join's pairs: partition by partition, tile by tile -- the first global pair index of every run
        first = (np.cumsum(counts.T.ravel()) - counts.T.ravel())[counts.T.ravel() > 0]
        assert set((first % 16).tolist()) == set(range(16))
        probe = build_column(probe_values, None, chunk, abi.ENC_FRAME_OF_REFERENCE)
        for name, shuffled, build_chunk in BUILDS:
            run(build_side(shuffled, build_chunk), probe, mode, radix_bits, f"mode {mode} radix {radix_bits} build {name}", general=radix_bits == 5)


@pytest.mark.parametrize("mode", MODES)
def test_copy_out_whole_tile(device, mode):
    """Radix 0: one run fills the tile (512 lines), behind a 7-row tile that shifts it off the line grid; an unencoded probe column."""
    chunk = 2 * TILE + 7
    probe_values, _ = probe_keys(np.random.default_rng(50), 0, chunk_tiles(8, chunk), all_match=True)
    probe = build_column(probe_values, None, chunk, abi.ENC_UNENCODED)
    for name, shuffled, build_chunk in BUILDS[:3]:
        run(build_side(shuffled, build_chunk), probe, mode, 0, f"mode {mode} radix 0 build {name}", general=name == "identity_65535")


@pytest.mark.parametrize("mode", MODES)
def test_copy_out_bits_in_lds(device, mode, options):
    """pk_emit<., true>: the found / materialised masks of pk_count_lds (forced for small probes)."""
    options.set(abi.OPT_JOIN_LDS_BUILD_TILES, 1)
    chunk = 4 * TILE + 5
    for radix_bits in (0, 5):
        probe_values, _ = probe_keys(np.random.default_rng(60 + radix_bits), radix_bits, chunk_tiles(4, chunk), all_match=radix_bits == 0)
        probe = build_column(probe_values, None, chunk, abi.ENC_FRAME_OF_REFERENCE)
        for name, shuffled, build_chunk in (BUILDS[0], BUILDS[2]):
            run(build_side(shuffled, build_chunk), probe, mode, radix_bits, f"lds mode {mode} radix {radix_bits} build {name}", expect=2)


def test_copy_out_handed_over_ranks(device, options):
    """pk_emit<true, false, true>: an Inner join whose probe keys have no locality hands every row's rank from pass 1 to pass 2
    (forced for small probes)."""
    options.set(abi.OPT_JOIN_HAND_OVER_RANKS, 1)
    chunk = 4 * TILE + 5
    for radix_bits in (0, 5, 8):
        probe_values, _ = probe_keys(np.random.default_rng(70 + radix_bits), radix_bits, chunk_tiles(4, chunk), all_match=radix_bits == 0)
        spans = [np.ptp(probe_values[b:b + 64]) for b in range(0, len(probe_values) - 64, 997)]
        assert np.mean(np.array(spans) < 65536) < 0.5   # scattered (probe_keys_lack_locality: three samples in four local means clustered)
        probe = build_column(probe_values, None, chunk, abi.ENC_FRAME_OF_REFERENCE)
        for name, shuffled, build_chunk in BUILDS:
            run(build_side(shuffled, build_chunk), probe, abi.JOIN_INNER, radix_bits, f"ranks radix {radix_bits} build {name}", general=radix_bits == 5)

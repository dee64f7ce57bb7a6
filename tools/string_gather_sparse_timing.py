#!/usr/bin/env python3
"""hy_string_column_gather on its dense route (HY_OPT_STRING_SPARSE_GATHER = 0: every source row exported, every dictionary entry ranked)
against its sparse route (= 2: the column read at the RowIDs, the entries they reference ranked), alternated in one process.
Usage: python tools/string_gather_sparse_timing.py [--small] > profiles/string_gather_sparse.txt     (needs the library built and an MI355X)

Shapes:
  c_name      1 500 000 rows of distinct 18-byte strings in 23 chunks of 65 535 rows (E = rows)
  l_shipdate  916 chunks of 65 535 rows (60 030 060 rows), 2 526 dates per chunk (E = 2 313 816), 2-byte value ids
n = 2^4, 2^8, 2^12, 2^16, 2^20 RowIDs drawn uniformly from the column (with repetitions), gathered into chunks of 65 535 rows.
Per n: 2 warm calls of either route, then 7 rounds; a round is one call of each route, dense first in even rounds and sparse first in odd
ones; wall clock around the call (it returns when the result is complete) and the HIP events of its HY_KERNEL_STRING_RANK brackets; medians.
The last column is n / (rows + E): STRING_SPARSE_DIVISOR (csrc/hy_options.hpp) is read from the largest n at which sparse / dense stays
below 0.9 in BOTH shapes -- 10 % is the process-to-process spread of this machine's timings."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyrise_amd import abi, storage  # noqa: E402

CHUNK = 65_535
DENSE, SPARSE = 0, 2


def c_name(rows):
    rng = np.random.default_rng(7)
    order = rng.permutation(rows)
    segments, dictionaries = [], []
    for begin in range(0, rows, CHUNK):
        values = [b"Customer#%09d" % i for i in order[begin:begin + CHUNK].tolist()]
        segment, dictionary = storage.encode_string_dictionary(values)
        segments.append(segment)
        dictionaries.append(dictionary)
    return storage.DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING)), storage.DeviceStringDictionary(dictionaries), rows, rows


def l_shipdate(n_chunks):
    """Every chunk: the same 2 526 sorted dates, 65 535 value ids drawn from them (no NULL rows)."""
    rng = np.random.default_rng(8)
    days = np.arange(np.datetime64("1992-01-02"), np.datetime64("1992-01-02") + 2_526)
    dictionary = [str(day).encode() for day in days]
    segments = [storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, CHUNK, 2, rng.integers(0, len(dictionary), CHUNK).astype(np.uint16), aux=None, aux_size=len(dictionary))
                for _ in range(n_chunks)]
    return (storage.DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING)), storage.DeviceStringDictionary([dictionary] * n_chunks), n_chunks * CHUNK,
            n_chunks * len(dictionary))


def timed_call(lib, column, dictionary, pointer, n, route):
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_set_option(abi.OPT_STRING_SPARSE_GATHER, route))
    abi.check(lib.hy_set_profiling(1))
    begin = time.perf_counter()
    abi.check(lib.hy_string_column_gather(column.handle, dictionary.handle, pointer, n, CHUNK, C.byref(handle), C.byref(dict_handle)))
    wall = (time.perf_counter() - begin) * 1e3
    ms, launches = C.c_float(0), C.c_uint32(0)
    abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(ms), C.byref(launches)))
    abi.check(lib.hy_set_profiling(0))
    abi.check(lib.hy_column_destroy(handle))
    abi.check(lib.hy_string_dictionary_destroy(dict_handle))
    return wall, ms.value, launches.value


def main():
    small = "--small" in sys.argv
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    before = C.c_int64(0)
    abi.check(lib.hy_get_option(abi.OPT_STRING_SPARSE_GATHER, C.byref(before)))
    print("hy_string_column_gather, dense route (HY_OPT_STRING_SPARSE_GATHER = 0) against sparse route (= 2), alternated in one process; ms")
    print("wall: clock around the call, median of 7 after 2 warm calls of either route; events: its HY_KERNEL_STRING_RANK brackets (median), launches inside them")
    for name, make in (("c_name", lambda: c_name(150_000 if small else 1_500_000)), ("l_shipdate", lambda: l_shipdate(92 if small else 916))):
        column, dictionary, rows, entries = make()
        print(f"\n{name}: {rows} rows, E = {entries} entries, {(rows + CHUNK - 1) // CHUNK} chunks")
        print(f"  {'n':>8} {'dense wall':>11} {'sparse wall':>11} {'sparse/dense':>12} {'dense events':>12} {'sparse events':>13} {'launches d/s':>12} {'n/(rows+E)':>11}")
        rng = np.random.default_rng(9)
        for exponent in (4, 8, 12, 16, 20):
            n = 1 << exponent
            flat = rng.integers(0, rows, n)
            positions = np.stack([flat // CHUNK, flat % CHUNK], axis=1).astype(np.uint32)
            pointer = C.c_void_p()
            abi.check(lib.hy_device_malloc(C.byref(pointer), 8 * n + 16))
            abi.check(lib.hy_memcpy_h2d(pointer, positions.ctypes.data, 8 * n))
            for _ in range(2):
                for route in (DENSE, SPARSE):
                    timed_call(lib, column, dictionary, pointer, n, route)
            walls, events, launches = {DENSE: [], SPARSE: []}, {DENSE: [], SPARSE: []}, {}
            for r in range(7):
                for route in ((DENSE, SPARSE) if r % 2 == 0 else (SPARSE, DENSE)):
                    wall, ms, launches[route] = timed_call(lib, column, dictionary, pointer, n, route)
                    walls[route].append(wall)
                    events[route].append(ms)
            dense, sparse = statistics.median(walls[DENSE]), statistics.median(walls[SPARSE])
            print(f"  {n:8d} {dense:11.3f} {sparse:11.3f} {sparse / dense:12.3f} {statistics.median(events[DENSE]):12.3f} {statistics.median(events[SPARSE]):13.3f} "
                  f"{launches[DENSE]:5d}/{launches[SPARSE]:<6d} {n / (rows + entries):11.2e}")
            sys.stdout.flush()
            abi.check(lib.hy_device_free(pointer))
        column.close()
        dictionary.close()
    abi.check(lib.hy_set_option(abi.OPT_STRING_SPARSE_GATHER, before.value))
    abi.check(lib.hy_shutdown())
    return 0


if __name__ == "__main__":
    sys.exit(main())

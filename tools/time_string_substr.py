#!/usr/bin/env python3
"""hy_string_column_substr(column, 1, 4) against hy_string_column_gather over the same column at the identity positions -- the same row pass
and copy plus a positions read that SUBSTR does not do -- and against the host loop that the device path replaces.
Usage: python tools/time_string_substr.py [--rows N ...] > profiles/string_substr.txt        (needs the library built and an MI355X)

Shapes: date columns as TPC-H SF10 has them, dictionary-encoded in chunks of 65 535 rows with 2-byte value ids: o_orderdate (15 000 000 rows
over 2 406 days) and l_shipdate (59 986 052 rows over 2 526 days), the days drawn uniformly.
  device   the two calls alternated, three pairs after one warm pair, one session: wall clock around each call (it returns when the result is
           complete) and the HIP events of its HY_KERNEL_STRING_RANK brackets (windows, ranking, front end, back end; launches = brackets)
  host     the formula over the rows' strings, dictionary lookup per row, as the mirror's host path does per cell (numpy fancy indexing over
           the per-chunk substrings: a lower bound of that loop), once"""
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
SHAPES = (("o_orderdate", 15_000_000, 2_406), ("l_shipdate", 59_986_052, 2_526))


def date_column(rows, n_days, seed):
    days = np.array([str(day).encode() for day in np.datetime64("1992-01-01") + np.arange(n_days)], dtype=object)
    rng = np.random.default_rng(seed)
    segments, dictionaries = [], []
    for begin in range(0, rows, CHUNK):
        size = min(CHUNK, rows - begin)
        present, value_ids = np.unique(rng.integers(0, n_days, size), return_inverse=True)
        segments.append(storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, size, 2, value_ids.astype(np.uint16), aux=None, aux_size=len(present)))
        dictionaries.append(days[present].tolist())
    return storage.HostColumn(segments, abi.TYPE_STRING), dictionaries


def timed(lib, call):
    handle, dict_handle = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_set_profiling(1))
    begin = time.perf_counter()
    abi.check(call(C.byref(handle), C.byref(dict_handle)))
    wall = (time.perf_counter() - begin) * 1e3
    ms, launches = C.c_float(0), C.c_uint32(0)
    abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(ms), C.byref(launches)))
    abi.check(lib.hy_set_profiling(0))
    abi.check(lib.hy_column_destroy(handle))
    abi.check(lib.hy_string_dictionary_destroy(dict_handle))
    return wall, ms.value, launches.value


def main():
    shapes = SHAPES
    if "--rows" in sys.argv:
        shapes = tuple((f"{int(r)} rows", int(r), 2_406) for r in sys.argv[sys.argv.index("--rows") + 1:])
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    print("hy_string_column_substr(column, 1, 4) and hy_string_column_gather at the identity positions (chunk_rows 65 535), alternated; ms")
    for name, rows, n_days in shapes:
        host, dictionaries = date_column(rows, n_days, rows)
        column, dictionary = storage.DeviceColumn(host), storage.DeviceStringDictionary(dictionaries)
        flat = np.arange(rows, dtype=np.int64)
        positions = np.stack([flat // CHUNK, flat % CHUNK], axis=1).astype(np.uint32)
        pointer = C.c_void_p()
        abi.check(lib.hy_device_malloc(C.byref(pointer), 8 * rows + 16))
        abi.check(lib.hy_memcpy_h2d(pointer, positions.ctypes.data, 8 * rows))
        substr = lambda result, result_dict: lib.hy_string_column_substr(column.handle, dictionary.handle, 1, 4, result, result_dict)   # noqa: E731
        gather = lambda result, result_dict: lib.hy_string_column_gather(column.handle, dictionary.handle, pointer, rows, CHUNK, result, result_dict)   # noqa: E731
        timed(lib, substr), timed(lib, gather)
        pairs = [(timed(lib, substr), timed(lib, gather)) for _ in range(3)]
        print(f"\n{name}: {rows} rows, {sum(map(len, dictionaries))} source entries in {len(dictionaries)} chunks")
        for label, runs in (("substr (1, 4)", [p[0] for p in pairs]), ("gather, identity", [p[1] for p in pairs])):
            print(f"  {label:18s} call " + " ".join(f"{wall:9.3f}" for wall, _, _ in runs) + "   events " + " ".join(f"{ms:9.3f}" for _, ms, _ in runs) + f"   brackets {runs[0][2]}")
        ratio = statistics.median(w for w, _, _ in [p[0] for p in pairs]) / statistics.median(w for w, _, _ in [p[1] for p in pairs])
        print(f"  substr / gather (median call) = {ratio:.3f}")
        begin = time.perf_counter()
        for segment, entries in zip(host.segments, dictionaries):
            years = np.array([entry[:4] for entry in entries] + [None], dtype=object)
            years[segment.data]
        print(f"  host loop          {(time.perf_counter() - begin) * 1e3:9.3f}")
        sys.stdout.flush()
        abi.check(lib.hy_device_free(pointer))
        column.close()
        dictionary.close()
    abi.check(lib.hy_shutdown())
    return 0


if __name__ == "__main__":
    sys.exit(main())

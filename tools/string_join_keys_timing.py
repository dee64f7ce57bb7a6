#!/usr/bin/env python3
"""hy_column_string_join_keys against the C++ mirror's host route for JoinHash's string keys (tools/string_join_keys_host_time.cpp:
string_join_id over every dictionary entry of both key columns, cold registry).
Usage: python tools/string_join_keys_timing.py > profiles/string_join_keys.txt        (needs the library built and an MI355X)

Shapes, each side of the join one such column:
  small   916 chunks x 7 entries (the ship modes, the same seven in every chunk of either side): 12 824 entries, launch-bound
  large   64 chunks x 65 535 entries of 27 bytes, distinct within a side, a third shared between the sides: 8 388 480 entries
Protocol: the device call is warmed twice; then REPS rounds, each one host measurement (a process of its own: the registry is
process-wide and must be cold) and one device measurement, in alternating order; medians, with the fastest and the slowest.
  host     the milliseconds of the string_join_id calls alone
  device   wall clock around hy_column_string_join_keys with HY_STRING_KEYS_HASH_IDS (it returns when both stand-ins are complete; it
           includes two hipMalloc and the upload of the joint tables), and the HIP events of its HY_KERNEL_STRING_RANK brackets"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyrise_amd import abi, storage  # noqa: E402

MODES = [b"AIR", b"FOB", b"MAIL", b"RAIL", b"REG AIR", b"SHIP", b"TRUCK"]
SHAPES = {"small": (916, 7, 7), "large": (64, 65_535, 5)}   # chunks, entries per chunk, rounds


def chunk_chars(shape, side, chunk):
    """(chars as uint8, offsets as uint32) of one chunk's dictionary: the generator of tools/string_join_keys_host_time.cpp"""
    if shape == "small":
        return storage.pack_string_dictionary(MODES)
    numbers = (2 if side == 0 else 3) * (np.arange(65_535, dtype=np.int64) * 64 + chunk)
    chars = np.full((65_535, 27), ord("K"), dtype=np.uint8)
    for digit in range(10):
        chars[:, 17 + digit] = (numbers // 10 ** (9 - digit)) % 10 + ord("0")
    return chars.reshape(-1), (np.arange(65_536, dtype=np.uint64) * 27).astype(np.uint32)


class Side:
    """One key column (every row its own value id: the keys are per dictionary entry, the rows do not matter) and its dictionaries."""

    def __init__(self, lib, shape, side):
        n_chunks, n_entries, _ = SHAPES[shape]
        self.keep = [chunk_chars(shape, side, c) for c in range(n_chunks)]
        chunks = (abi.StringDictionaryChunk * n_chunks)()
        for c, (chars, offsets) in enumerate(self.keep):
            chunks[c].n_entries, chunks[c].string_length, chunks[c].chars, chunks[c].offsets = n_entries, 0, chars.ctypes.data, offsets.ctypes.data
        self.dictionary = C.c_void_p()
        abi.check(lib.hy_string_dictionary_create(chunks, n_chunks, abi.MEM_HOST, C.byref(self.dictionary)))
        ids = np.arange(n_entries, dtype=np.uint32)
        segments = [storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, n_entries, 4, ids, aux=None, aux_size=n_entries) for _ in range(n_chunks)]
        self.column = storage.DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))


def device_call(lib, left, right):
    """-> (wall clock ms, ms between the HY_KERNEL_STRING_RANK events)"""
    a, b = C.c_void_p(), C.c_void_p()
    abi.check(lib.hy_set_profiling(1))
    begin = time.perf_counter()
    abi.check(lib.hy_column_string_join_keys(left.column.handle, left.dictionary, right.column.handle, right.dictionary, abi.STRING_KEYS_HASH_IDS, C.byref(a), C.byref(b)))
    wall = (time.perf_counter() - begin) * 1e3
    ms, launches = C.c_float(0), C.c_uint32(0)
    abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(ms), C.byref(launches)))
    abi.check(lib.hy_set_profiling(0))
    abi.check(lib.hy_column_destroy(a))
    abi.check(lib.hy_column_destroy(b))
    return wall, ms.value


def summary(values):
    return f"median {statistics.median(values):10.3f}   fastest {min(values):10.3f}   slowest {max(values):10.3f}"


def main():
    source = os.path.join(ROOT, "tools", "string_join_keys_host_time.cpp")
    binary = os.path.join(ROOT, "tools", "string_join_keys_host_time_bin")
    deps = [source, os.path.join(ROOT, "hyrise_amd", "host", "hyrise_host.hpp"), os.path.join(ROOT, "hyrise_amd", "libhyrise_amd.so")]
    if not os.path.exists(binary) or any(os.path.getmtime(d) > os.path.getmtime(binary) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-o", binary, source, "-L" + os.path.join(ROOT, "hyrise_amd"), "-lhyrise_amd",
                               "-Wl,-rpath,$ORIGIN/../hyrise_amd"], cwd=ROOT)
    if "--build-only" in sys.argv:
        return 0
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    print("JoinHash's string keys for a pair of columns: string_join_id on the host (cold registry, a process per measurement) against")
    print("hy_column_string_join_keys (HY_STRING_KEYS_HASH_IDS) on one MI355X; ms; 2 warm device calls, then rounds in alternating order")
    for shape, (n_chunks, n_entries, rounds) in SHAPES.items():
        left, right = Side(lib, shape, 0), Side(lib, shape, 1)
        for _ in range(2):
            device_call(lib, left, right)
        host, wall, events = [], [], []
        for r in range(rounds):
            for what in (("host", "device") if r % 2 == 0 else ("device", "host")):
                if what == "host":
                    host.append(float(subprocess.run([binary, shape], stdout=subprocess.PIPE, text=True, check=True).stdout.split()[0]))
                else:
                    w, e = device_call(lib, left, right)
                    wall.append(w)
                    events.append(e)
        print(f"\n{shape}: {n_chunks} chunks x {n_entries} entries per side, {2 * n_chunks * n_entries} entries in all, {rounds} rounds")
        print(f"  host    string_join_id                 {summary(host)}")
        print(f"  device  hy_column_string_join_keys     {summary(wall)}")
        print(f"  device  HY_KERNEL_STRING_RANK events   {summary(events)}")
        print(f"  host median / device median: {statistics.median(host) / statistics.median(wall):.2f}")
        sys.stdout.flush()
        abi.check(lib.hy_string_dictionary_destroy(left.dictionary))
        abi.check(lib.hy_string_dictionary_destroy(right.dictionary))
        left.column.close()
        right.column.close()
    abi.check(lib.hy_shutdown())
    return 0


if __name__ == "__main__":
    sys.exit(main())

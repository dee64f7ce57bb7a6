#!/usr/bin/env python3
"""hy_string_column_gather against the C++ mirror's host materialisation of the same column (tools/string_gather_host_time.cpp) and against
a plain device copy of the bytes it writes; the split of the call by kernel.  One process per part, warm runs, medians.
Usage: python tools/string_gather_timing.py [rows] > profiles/string_gather.txt        (needs the library built and an MI355X)

Shapes: `rows` (default 1 500 000) distinct strings of 18 bytes (TPC-H c_name, the Q18 GROUP BY) and of 70 bytes, in chunks of 65 535 rows,
gathered at every row once in a shuffled order into chunks of 65 535 rows -- one group per customer.
  device   wall clock around hy_string_column_gather (it returns when the result is complete), after 2 warm calls, median of 7; and the HIP
           events of its HY_KERNEL_STRING_RANK brackets (the ranking; the sort, value ids, lengths, offsets and byte copy)
  copy     torch's device-to-device copy of as many bytes as the result holds (chars + offsets + value ids), synchronised, median of 7
  host     the mirror's loop: operator[] per RowID, make_value_segment<std::string> per output chunk, median of 3
  split    a second process under `rocprofv3 --kernel-trace --stats` (counters in a run of their own): the kernels of 3 calls by group"""
import csv
import ctypes as C
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyrise_amd import abi, storage  # noqa: E402
from hyrise_amd.operators import string_column_gather  # noqa: E402

CHUNK = 65_535
GROUPS = (("ranking (order_*)", ("order_",)), ("front end (iota_table, export_*, entries_at_positions)", ("iota_table", "export_", "entries_at_positions", "expand_")),
          ("sort (rank_words, chunk_words, sort_*, scan_block*)", ("rank_words", "chunk_words", "sort_", "scan_block", "lds_atomic_order_probe")),
          ("value ids and lengths (key_heads .. chunk_totals)", ("key_heads", "scan_tiles", "chunk_firsts", "value_ids", "unique_lengths", "chunk_totals")),
          ("offsets and byte copy (dictionary_offsets, copy_entry_bytes)", ("dictionary_offsets", "copy_entry_bytes")))


def shape(rows, nbytes):
    """(DeviceColumn, DeviceStringDictionary, positions as an (n, 2) uint32 array): the generator of tools/string_gather_host_time.cpp in spirit
    (distinct strings of nbytes bytes, shuffled over the chunks; the RowIDs every row once, shuffled)."""
    rng = np.random.default_rng(7)
    order = rng.permutation(rows)
    segments, dictionaries = [], []
    for begin in range(0, rows, CHUNK):
        values = [b"C" * (nbytes - 10) + b"#%09d" % i for i in order[begin:begin + CHUNK].tolist()]
        segment, dictionary = storage.encode_string_dictionary(values)
        segments.append(segment)
        dictionaries.append(dictionary)
    column = storage.DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))
    flat = rng.permutation(rows)
    positions = np.stack([flat // CHUNK, flat % CHUNK], axis=1).astype(np.uint32)
    return column, storage.DeviceStringDictionary(dictionaries), positions


def device_positions(lib, positions):
    pointer = C.c_void_p()
    abi.check(lib.hy_device_malloc(C.byref(pointer), 8 * len(positions) + 16))
    abi.check(lib.hy_memcpy_h2d(pointer, positions.ctypes.data, 8 * len(positions)))
    return pointer


def gather_only(rows, nbytes):
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    column, dictionary, positions = shape(rows, nbytes)
    pointer = device_positions(lib, positions)
    for _ in range(3):
        string_column_gather(column, dictionary, (pointer, len(positions)), CHUNK).close()
    abi.check(lib.hy_shutdown())


def kernel_split(rows, nbytes):
    """[(group, ms per call)] from rocprofv3's kernel statistics of a process that makes 3 calls, or None where the profiler is not there."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    with tempfile.TemporaryDirectory() as directory:
        run = subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "--", sys.executable, os.path.abspath(__file__), "--gather-only",
                              str(rows), str(nbytes)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return None
        totals = {label: 0.0 for label, _ in GROUPS}
        other = 0.0
        with open(files[0]) as fh:
            for row in csv.DictReader(fh):
                name, nanoseconds = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
                for label, prefixes in GROUPS:
                    if any(p in name for p in prefixes):
                        totals[label] += nanoseconds
                        break
                else:
                    other += nanoseconds
        return [(label, totals[label] / 3e6) for label, _ in GROUPS] + [("other kernels of the process (uploads' blits, fills)", other / 3e6)]


def main():
    if "--gather-only" in sys.argv:
        at = sys.argv.index("--gather-only")
        return gather_only(int(sys.argv[at + 1]), int(sys.argv[at + 2]))
    import torch
    arguments = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = int(arguments[0]) if arguments else 1_500_000
    source = os.path.join(ROOT, "tools", "string_gather_host_time.cpp")
    binary = os.path.join(ROOT, "tools", "string_gather_host_time_bin")
    deps = [source, os.path.join(ROOT, "hyrise_amd", "host", "hyrise_host.hpp"), os.path.join(ROOT, "hyrise_amd", "libhyrise_amd.so")]
    if not os.path.exists(binary) or any(os.path.getmtime(d) > os.path.getmtime(binary) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-o", binary, source, "-L" + os.path.join(ROOT, "hyrise_amd"), "-lhyrise_amd",
                               "-Wl,-rpath,$ORIGIN/../hyrise_amd"], cwd=ROOT)
    if "--build-only" in sys.argv:
        return 0
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    print(f"hy_string_column_gather, {rows} rows of distinct strings in chunks of {CHUNK}, gathered at every row once (shuffled) into chunks of {CHUNK}; ms")
    print("device call: wall clock, median of 7 after 2 warm calls; events: its HY_KERNEL_STRING_RANK brackets; copy: torch copy_ of the result's bytes, median of 7;")
    print("host: the mirror's materialisation loop (tools/string_gather_host_time.cpp), median of 3; its shuffles come from another generator: the same shape, not the same column")
    host = {}
    for line in subprocess.run([binary, str(rows)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines():
        nbytes, ms = line.split()
        host[int(nbytes)] = float(ms)
    for nbytes in (18, 70):
        column, dictionary, positions = shape(rows, nbytes)
        pointer = device_positions(lib, positions)
        result_bytes = 0
        for _ in range(2):
            result = string_column_gather(column, dictionary, (pointer, rows), CHUNK)
            result_bytes = sum(len(result.dictionary.read_chunk(c)[1]) + 4 * (n + 1) for c, n in enumerate(result.dictionary.n_entries)) + 4 * rows
            result.close()
        calls, events = [], []
        handle, dict_handle = C.c_void_p(), C.c_void_p()
        for _ in range(7):
            abi.check(lib.hy_set_profiling(1))
            begin = time.perf_counter()
            abi.check(lib.hy_string_column_gather(column.handle, dictionary.handle, pointer, rows, CHUNK, C.byref(handle), C.byref(dict_handle)))
            calls.append((time.perf_counter() - begin) * 1e3)
            ms, launches = C.c_float(0), C.c_uint32(0)
            abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(ms), C.byref(launches)))
            abi.check(lib.hy_set_profiling(0))
            events.append(ms.value)
            abi.check(lib.hy_column_destroy(handle))
            abi.check(lib.hy_string_dictionary_destroy(dict_handle))
        src = torch.zeros(result_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copies = []
        for r in range(9):
            torch.cuda.synchronize()
            begin = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            if r >= 2:
                copies.append((time.perf_counter() - begin) * 1e3)
        call, copy = statistics.median(calls), statistics.median(copies)
        print(f"\n{nbytes}-byte strings: result {result_bytes / 1e6:.1f} MB")
        print(f"  device call {call:9.3f}   (min {min(calls):.3f}, max {max(calls):.3f}; events {statistics.median(events):.3f})")
        print(f"  plain copy  {copy:9.3f}   device call / copy = {call / copy:.1f}")
        print(f"  host        {host[nbytes]:9.3f}   host / device call = {host[nbytes] / call:.1f}")
        sys.stdout.flush()
        del src, dst
        abi.check(lib.hy_device_free(pointer))
        column.close()
        dictionary.close()
    abi.check(lib.hy_shutdown())
    for nbytes in (18, 70):
        split = kernel_split(rows, nbytes)
        print(f"\n{nbytes}-byte strings, kernels per call (rocprofv3 --kernel-trace --stats over 3 calls, a process of its own; includes the one-time uploads' kernels under `other`):")
        if split is None:
            print("  not available: rocprofv3 did not run or wrote no kernel statistics")
            continue
        for label, ms in split:
            print(f"  {label:62s} {ms:9.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

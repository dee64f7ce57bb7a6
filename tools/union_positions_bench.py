#!/usr/bin/env python3
"""UnionPositions (hy_union_positions) over SF10 lineitem (59 986 052 rows), one process; HIP-event time of every call (hy_set_profiling: one
event pair around the call's kernels), warm-up, then the median over `steps` calls:
  A. l_shipdate < 1995-01-01 OR l_discount BETWEEN 0.05 AND 0.07: the two scans' PosLists (one cluster, in order, device lists), default path
  B. the same with HY_UNION_FORCE_SORT, alternating with A call by call
  C. both sides shuffled, two clusters (lineitem row, orders row): the two sides of an orders JOIN lineitem output
For each: rows in / out, the algorithmic bytes 8 * n_clusters * (rows_left + rows_right + rows_out), the time, and those bytes over 8 TB/s;
beside them the kernel time of the two TableScans that feed A, and the host route A replaces (D2H of both lists, sort + set union on the
host, H2D of the result).  The host set union here is numpy's (np.union1d of the 64-bit keys, ONE thread), a stand-in: the reference's
std::sort + std::set_union on 16 threads was not measured.
Usage: python tools/union_positions_bench.py [steps]   (not part of the product; DESIGN.md section 4.8 quotes its output)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_SECOND = 8e12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import make_predicate, table_scan, union_positions
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    data = tpch.TpchData(10.0, 42)
    hosts = {"l_shipdate": storage.make_column(data.l_shipdate, None, abi.ENC_DICTIONARY), "l_discount": storage.make_column(data.l_discount, None, abi.ENC_DICTIONARY)}
    devs = {name: DeviceColumn(h) for name, h in hosts.items()}
    discount = np.sort(np.unique(data.l_discount))
    predicates = [("l_shipdate", make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, tpch.DAY_1995_01_01)),
                  ("l_discount", make_predicate(abi.PRED_BETWEEN_INCLUSIVE, storage.TYPE_OF_NP[data.l_discount.dtype], discount[5], discount[7]))]

    def profiled(call):
        abi.check(lib.hy_set_profiling(1))
        result = call()
        ms, launches = C.c_float(0), C.c_uint32(0)
        abi.check(lib.hy_profile_read(C.byref(ms), C.byref(launches)))
        abi.check(lib.hy_set_profiling(0))
        return result, float(ms.value)

    def device_lists(pos_lists, referenced):
        """The lists back to back in one device buffer, as an operator's pooled block holds them."""
        flat = np.ascontiguousarray(np.concatenate(pos_lists))
        pointer = C.c_void_p()
        abi.check(lib.hy_device_malloc(C.byref(pointer), max(256, flat.nbytes)))
        abi.check(lib.hy_memcpy_h2d(pointer, flat.ctypes.data, flat.nbytes))
        segments = (abi.Segment * len(pos_lists))()
        at = 0
        for i, p in enumerate(pos_lists):
            d = segments[i]
            d.encoding, d.data_type, d.size, d.width = abi.ENC_REFERENCE, referenced.data_type, len(p), 8
            d.data, d.ref_chunk_id, d.ref = pointer.value + 8 * at, abi.INVALID_CHUNK_ID, referenced.handle
            at += len(p)
        handle = C.c_void_p()
        abi.check(lib.hy_column_create(segments, len(pos_lists), abi.MEM_DEVICE, C.byref(handle)))
        column = type("Lists", (), {})()
        column.handle, column.rows, column.keep, column.flat, column.pointer = handle, at, segments, flat, pointer.value
        return column

    sides, scan_ms = [], []
    for name, predicate in predicates:
        for _ in range(3):
            scan, ms = profiled(lambda: table_scan(devs[name], predicate))
        scan_ms.append(ms)
        sides.append(device_lists([scan.pos_list(c).copy() for c in range(devs[name].n_chunks)], devs[name]))
    print(f"TableScan kernels feeding A: l_shipdate {scan_ms[0] * 1e3:.0f} us, l_discount {scan_ms[1] * 1e3:.0f} us", flush=True)

    def report(label, n_clusters, rows_left, rows_right, rows_out, times, path):
        algorithmic = 8 * n_clusters * (rows_left + rows_right + rows_out)
        ms = float(np.median(times))
        print(f"{label:44s} rows {rows_left:>9d} + {rows_right:>9d} -> {rows_out:>9d}  path {path}  {ms * 1e3:8.0f} us (median of {len(times)}, min {min(times) * 1e3:.0f})  "
              f"algorithmic {algorithmic / 1e6:7.1f} MB = {algorithmic / HBM_BYTES_PER_SECOND * 1e6:5.0f} us at 8 TB/s -> {ms * 1e-3 / (algorithmic / HBM_BYTES_PER_SECOND):5.1f} x", flush=True)
        return ms

    left, right = [sides[0]], [sides[1]]
    for _ in range(3):
        for force in (False, True):
            union_positions(left, right, force_sort=force).close()
    times = {False: [], True: []}
    pairs_won = 0
    for _ in range(steps):
        pair = {}
        for force in (False, True):
            out, ms = profiled(lambda: union_positions(left, right, force_sort=force))
            rows_out, paths = out.rows, times.setdefault(("path", force), out.path)
            out.close()
            times[force].append(ms)
            pair[force] = ms
        pairs_won += pair[False] < pair[True]
    a_ms = report("A. two scans, in order (default)", 1, sides[0].rows, sides[1].rows, rows_out, times[False], times[("path", False)])
    report("B. the same, HY_UNION_FORCE_SORT", 1, sides[0].rows, sides[1].rows, rows_out, times[True], times[("path", True)])
    print(f"A faster than B in {pairs_won} of {steps} alternating pairs", flush=True)

    # C: (lineitem row, orders row) pairs of the two scans' rows, each side in its own random order
    rng = np.random.default_rng(3)
    order_of_lineitem = np.searchsorted(np.unique(data.l_orderkey), data.l_orderkey)
    shuffled = []
    for side in sides:
        flat = side.flat[rng.permutation(side.rows)]
        rows = flat[:, 0].astype(np.int64) * abi.CHUNK_DEFAULT_SIZE + flat[:, 1]
        orders = order_of_lineitem[rows]
        order_positions = np.stack([orders // abi.CHUNK_DEFAULT_SIZE, orders % abi.CHUNK_DEFAULT_SIZE], axis=1).astype(np.uint32)
        cut = list(range(0, side.rows, abi.CHUNK_DEFAULT_SIZE))
        shuffled.append([device_lists([c[b:b + abi.CHUNK_DEFAULT_SIZE] for b in cut], devs["l_shipdate"]) for c in (flat, order_positions)])
    for _ in range(2):
        union_positions(shuffled[0], shuffled[1]).close()
    c_times = []
    for _ in range(max(5, steps // 5)):
        out, ms = profiled(lambda: union_positions(shuffled[0], shuffled[1]))
        c_rows, c_path = out.rows, out.path
        out.close()
        c_times.append(ms)
    report("C. both sides shuffled, 2 clusters", 2, sides[0].rows, sides[1].rows, c_rows, c_times, c_path)

    # the host route A replaces: D2H of both lists, sort + set union, H2D of the result
    host_times = []
    for _ in range(3):
        t0 = time.perf_counter()
        keys = []
        for side in sides:
            staged = np.empty((side.rows, 2), dtype=np.uint32)
            abi.check(lib.hy_memcpy_d2h(staged.ctypes.data, side.pointer, staged.nbytes))
            keys.append((staged[:, 0].astype(np.uint64) << np.uint64(32)) | staged[:, 1])
        t1 = time.perf_counter()
        merged = np.union1d(keys[0], keys[1])   # (the scans' rows are distinct: the set union IS UnionPositions' result here)
        result = np.stack([(merged >> np.uint64(32)).astype(np.uint32), merged.astype(np.uint32)], axis=1)
        t2 = time.perf_counter()
        pointer = C.c_void_p()
        abi.check(lib.hy_result_pool_acquire(result.nbytes, C.byref(pointer)))
        abi.check(lib.hy_memcpy_h2d(pointer, result.ctypes.data, result.nbytes))
        abi.check(lib.hy_synchronize())
        t3 = time.perf_counter()
        lib.hy_result_pool_release(pointer)
        assert len(result) == rows_out
        host_times.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    total, d2h, merge, h2d = min(host_times)
    print(f"host route for A (numpy, one thread; best of 3): {total * 1e3:.0f} ms = D2H {d2h * 1e3:.0f} + sort / set union {merge * 1e3:.0f} + H2D {h2d * 1e3:.0f} ms"
          f"  -> {total * 1e3 / a_ms:.0f} x the device path; the transfers alone {(d2h + h2d) * 1e3 / a_ms:.0f} x", flush=True)


if __name__ == "__main__":
    main()

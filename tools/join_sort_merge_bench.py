#!/usr/bin/env python3
"""JoinSortMerge (hy_join_sort_merge) at full size, one process; HIP-event time of every call (hy_set_profiling: one event pair around the
call's kernels), median of `steps` calls after a warm-up, results in device memory acquired before the clock starts.
  (a) o_orderkey = l_orderkey, Inner, SF10 (59 986 052 pairs), next to hy_join_hash in alternating order
  (b) the same columns, FullOuter, lineitem behind a 15 % scan (l_shipdate below its 15 % quantile)
  (c) <, two columns of 20 000 rows, about 2 * 10^8 pairs
Every case checks n_pairs / n_matched / n_left_outer against numpy.  Usage: python tools/join_sort_merge_bench.py [steps]
(not part of the product; DESIGN.md section 4.9 quotes its output.  Per-kernel times: rocprofv3 --kernel-trace --stats -- python
tools/join_sort_merge_bench.py 3)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import make_predicate, table_scan
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))

    def timed(call):
        abi.check(lib.hy_set_profiling(1))
        abi.check(call())
        ms, launches = C.c_float(0), C.c_uint32(0)
        abi.check(lib.hy_profile_read(C.byref(ms), C.byref(launches)))
        abi.check(lib.hy_set_profiling(0))
        return ms.value

    def lists(capacity):
        left, right = C.c_void_p(), C.c_void_p()
        abi.check(lib.hy_result_pool_acquire_pair(max(1, capacity), C.byref(left), C.byref(right)))
        return left, right

    def merge_call(left, right, mode, condition, capacity, blocks, result):
        result.mem, result.left_pos, result.right_pos, result.capacity = abi.MEM_DEVICE, blocks[0].value, blocks[1].value, capacity
        return lambda: lib.hy_join_sort_merge(left.handle, right.handle, mode, condition, C.byref(result))

    def report(name, times, pairs):
        t = np.array(times)
        print(f"    {name:22s} {np.median(t):9.3f} ms (median of {len(t)}, min {t.min():.3f}, max {t.max():.3f})  {16 * pairs / np.median(t) / 1e9:7.3f} TB/s of 16 B per pair", flush=True)

    data = tpch.TpchData(10.0, 42)
    orders = DeviceColumn(storage.make_column(data.o_orderkey, None, abi.ENC_FRAME_OF_REFERENCE))
    lineitem_host = storage.make_column(data.l_orderkey, None, abi.ENC_FRAME_OF_REFERENCE)
    lineitem = DeviceColumn(lineitem_host)
    n = data.n_lineitems

    # (a)
    blocks, hash_blocks = lists(n), lists(n)
    result = abi.SortMergeResult()
    merge = merge_call(orders, lineitem, abi.JOIN_INNER, abi.PRED_EQUALS, n, blocks, result)
    slice_capacity = n // 131070 + lineitem.n_chunks + 600
    offsets = C.c_void_p()
    abi.check(lib.hy_device_malloc(C.byref(offsets), 8 * (slice_capacity + 2)))
    hashed = abi.JoinResult()
    hashed.mem, hashed.radix_bits, hashed.left_pos, hashed.right_pos, hashed.capacity = abi.MEM_DEVICE, 0xFFFFFFFF, hash_blocks[0].value, hash_blocks[1].value, n
    hashed.slice_offsets, hashed.slice_capacity = offsets.value, slice_capacity
    hash_call = lambda: lib.hy_join_hash(orders.handle, lineitem.handle, abi.JOIN_INNER, C.byref(hashed))   # noqa: E731
    for call in (merge, hash_call, merge, hash_call):
        timed(call)
    assert result.n_pairs == result.n_matched == hashed.n_pairs == n, (result.n_pairs, hashed.n_pairs)
    times = {"hy_join_sort_merge": [], "hy_join_hash": []}
    for step in range(steps):
        for name, call in (("hy_join_sort_merge", merge), ("hy_join_hash", hash_call))[::1 if step % 2 == 0 else -1]:
            times[name].append(timed(call))
    print(f"(a) o_orderkey = l_orderkey, Inner, SF10: {n} pairs", flush=True)
    report("hy_join_sort_merge", times["hy_join_sort_merge"], n)
    report("hy_join_hash", times["hy_join_hash"], n)
    print(f"    ratio of the medians: {np.median(times['hy_join_sort_merge']) / np.median(times['hy_join_hash']):.2f} x hy_join_hash", flush=True)

    # (b)
    shipdate = DeviceColumn(storage.make_column(data.l_shipdate, None, abi.ENC_DICTIONARY))
    cut = int(np.quantile(data.l_shipdate, 0.15))
    scan = table_scan(shipdate, make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, cut), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    pos_lists = [scan.pos_list(c).copy() for c in range(shipdate.n_chunks)]
    kept = data.l_shipdate < cut
    reference = DeviceColumn(storage.make_reference_column(lineitem_host, pos_lists, list(range(len(pos_lists)))), refs={id(lineitem_host): lineitem})
    matched = int(kept.sum())
    unmatched_orders = len(data.o_orderkey) - len(np.intersect1d(data.o_orderkey, data.l_orderkey[kept]))
    merge = merge_call(orders, reference, abi.JOIN_FULL_OUTER, abi.PRED_EQUALS, n, blocks, result)
    timed(merge)
    assert (result.n_matched, result.n_left_outer, result.n_pairs) == (matched, unmatched_orders, matched + unmatched_orders), (result.n_matched, result.n_left_outer, result.n_pairs)
    print(f"(b) the same, FullOuter, lineitem behind a {100.0 * matched / n:.1f} % scan: {result.n_pairs} rows ({matched} pairs + {unmatched_orders} orders without partner)", flush=True)
    report("hy_join_sort_merge", [timed(merge) for _ in range(steps)], result.n_pairs)

    # (c)
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 1 << 30, 20_000).astype(np.int32), rng.integers(0, 1 << 30, 20_000).astype(np.int32)
    expected = int((20_000 - np.searchsorted(np.sort(b), a, side="right")).sum())
    for block in blocks + hash_blocks:
        lib.hy_result_pool_release(block.value)
    blocks = lists(expected)
    left, right = DeviceColumn(storage.make_column(a, None, abi.ENC_UNENCODED)), DeviceColumn(storage.make_column(b, None, abi.ENC_UNENCODED))
    merge = merge_call(left, right, abi.JOIN_INNER, abi.PRED_LESS_THAN, expected, blocks, result)
    timed(merge)
    assert result.n_pairs == expected, (result.n_pairs, expected)
    print(f"(c) <, 20 000 x 20 000 rows: {expected} pairs", flush=True)
    report("hy_join_sort_merge", [timed(merge) for _ in range(steps)], expected)
    for block in blocks:
        lib.hy_result_pool_release(block.value)


if __name__ == "__main__":
    main()

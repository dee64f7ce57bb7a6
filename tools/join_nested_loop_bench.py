#!/usr/bin/env python3
"""JoinNestedLoop (hy_join_nested_loop), one process; HIP-event time of every call (hy_set_profiling: one event pair around the call's
kernels), median of `steps` calls after a warm-up, results in device memory acquired before the clock starts.
  (a) Inner, 100 000 x 100 000 int, < with a secondary = over a 1 000-value column; the figure is comparisons per second
  (b) Semi, 100 000 x 100 000, int < long
  (c) Inner <=, 20 000 x 20 000, about 2 * 10^8 pairs, next to hy_join_sort_merge on the same inputs in alternating order
Every case checks n_pairs against numpy.  Writes profiles/join_nested_loop_bench.txt, then runs case (c) once more in a child process under
`rocprofv3 --kernel-trace --stats` and keeps its kernel statistics as profiles/join_nested_loop_kernel_stats.csv: nlj_emit's and smj_emit's
bytes per second against the copy ceiling come from there.
Usage: python tools/join_nested_loop_bench.py [steps]     (not part of the product; DESIGN.md section 4.10 quotes its output)"""
import csv
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12   # bytes per second: the measured copy ceiling DESIGN.md section 6 quotes


def main():
    traced = "--traced" in sys.argv
    numbers = [a for a in sys.argv[1:] if a.isdigit()]
    steps = int(numbers[0]) if numbers else 12
    from hyrise_amd import abi, storage
    from hyrise_amd.operators import join_predicates
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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

    def column(values):
        return DeviceColumn(storage.make_column(values, None, abi.ENC_UNENCODED))

    def nested_call(left, right, mode, condition, secondary, capacity, blocks, result):
        predicates, n_secondary = join_predicates(secondary)
        result.mem, result.left_pos, result.right_pos, result.capacity = abi.MEM_DEVICE, blocks[0].value, blocks[1].value, capacity
        return lambda: lib.hy_join_nested_loop(left.handle, right.handle, mode, condition, predicates, n_secondary, C.byref(result))

    def report(name, times, comparisons, pairs):
        t = np.array(times)
        say(f"    {name:22s} {np.median(t):9.3f} ms (median of {len(t)}, min {t.min():.3f}, max {t.max():.3f})  {comparisons / np.median(t) / 1e6:8.2f} G comparisons/s"
            f"  {16 * pairs / np.median(t) / 1e9:7.3f} TB/s of 16 B per pair")
        return float(np.median(t))

    rng = np.random.default_rng(7)
    result = abi.NestedLoopResult()
    if not traced:
        # (a)
        n = 100_000
        a, b = rng.integers(0, 1 << 30, n).astype(np.int32), rng.integers(0, 1 << 30, n).astype(np.int32)
        a2, b2 = rng.integers(0, 1000, n).astype(np.int32), rng.integers(0, 1000, n).astype(np.int32)
        expected = 0
        for value in range(1000):   # pairs with a < b among the rows that share the secondary value
            expected += int((np.count_nonzero(b2 == value) - np.searchsorted(np.sort(b[b2 == value]), a[a2 == value], side="right")).sum())
        left, right, left2, right2 = column(a), column(b), column(a2), column(b2)
        blocks = lists(expected)
        call = nested_call(left, right, abi.JOIN_INNER, abi.PRED_LESS_THAN, [(left2, abi.PRED_EQUALS, right2)], expected, blocks, result)
        timed(call)
        assert result.n_pairs == expected, (result.n_pairs, expected)
        say(f"(a) Inner, {n} x {n} int, < and a secondary = over 1 000 values: {expected} pairs")
        median_a = report("hy_join_nested_loop", [timed(call) for _ in range(steps)], n * n, expected)
        say(f"    at this rate HY_NLJ_MAX_COMPARISONS = {abi.NLJ_MAX_COMPARISONS:.3g} is {abi.NLJ_MAX_COMPARISONS / (n * n / median_a) / 1e3:.2f} s per call; 2 s per call are {2e3 * n * n / median_a:.3g} comparisons")
        # (b)
        b_long = b.astype(np.int64)
        expected = int(np.count_nonzero(a < b.max()))
        call = nested_call(left, column(b_long), abi.JOIN_SEMI, abi.PRED_LESS_THAN, None, n, blocks, result)
        timed(call)
        assert result.n_pairs == expected, (result.n_pairs, expected)
        say(f"(b) Semi, {n} x {n}, int < long: {expected} rows")
        report("hy_join_nested_loop", [timed(call) for _ in range(steps)], n * n, expected)
        for block in blocks:
            lib.hy_result_pool_release(block.value)

    # (c)
    n = 20_000
    a, b = rng.integers(0, 1 << 30, n).astype(np.int32), rng.integers(0, 1 << 30, n).astype(np.int32)
    expected = int((n - np.searchsorted(np.sort(b), a, side="left")).sum())
    left, right = column(a), column(b)
    blocks, merge_blocks = lists(expected), lists(expected)
    nested = nested_call(left, right, abi.JOIN_INNER, abi.PRED_LESS_THAN_EQUALS, None, expected, blocks, result)
    merged = abi.SortMergeResult()
    merged.mem, merged.left_pos, merged.right_pos, merged.capacity = abi.MEM_DEVICE, merge_blocks[0].value, merge_blocks[1].value, expected
    merge = lambda: lib.hy_join_sort_merge(left.handle, right.handle, abi.JOIN_INNER, abi.PRED_LESS_THAN_EQUALS, C.byref(merged))   # noqa: E731
    for call in (nested, merge):
        timed(call)
    assert result.n_pairs == merged.n_pairs == expected, (result.n_pairs, merged.n_pairs, expected)
    times = {"hy_join_nested_loop": [], "hy_join_sort_merge": []}
    for step in range(3 if traced else steps):
        for name, call in (("hy_join_nested_loop", nested), ("hy_join_sort_merge", merge))[::1 if step % 2 == 0 else -1]:
            times[name].append(timed(call))
    say(f"(c) Inner <=, {n} x {n} rows: {expected} pairs")
    for name in times:
        report(name, times[name], n * n, expected)
    say(f"    ratio of the medians: {np.median(times['hy_join_nested_loop']) / np.median(times['hy_join_sort_merge']):.2f} x hy_join_sort_merge")
    for block in blocks + merge_blocks:
        lib.hy_result_pool_release(block.value)
    lib.hy_shutdown()
    if traced:
        return

    # case (c) once more under the kernel trace, in a process of its own
    profiles = os.path.join(ROOT, "profiles")
    with tempfile.TemporaryDirectory() as directory:
        command = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "-o", "nlj", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        child = subprocess.run(command, capture_output=True, text=True, timeout=600)
        found = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
        if child.returncode != 0 or not found:
            say(f"kernel trace: rocprofv3 exit {child.returncode}, no kernel statistics\n{child.stdout[-1500:]}\n{child.stderr[-1500:]}")
        else:
            shutil.copyfile(found[0], os.path.join(profiles, "join_nested_loop_kernel_stats.csv"))
            with open(found[0], newline="") as fh:
                rows = list(csv.DictReader(fh))
            say("kernel trace of case (c) (profiles/join_nested_loop_kernel_stats.csv; 16 B written per pair):")
            rates = {}
            for kernel in ("nlj_emit", "smj_emit", "nlj_count"):
                for row in rows:
                    if kernel + "<" in row["Name"] or kernel + "(" in row["Name"]:
                        average = float(row["AverageNs"])
                        rates[kernel] = 16 * expected / (average * 1e-9)
                        say(f"    {kernel:10s} {average / 1e3:10.1f} us average of {row['Calls']} calls" +
                            (f"  {rates[kernel] / 1e12:6.3f} TB/s = {rates[kernel] / COPY_CEILING:.2f} of the {COPY_CEILING / 1e12:.2f} TB/s copy ceiling" if kernel != "nlj_count" else
                             f"  {n * n / (average * 1e-9) / 1e9:8.2f} G comparisons/s"))
                        break
            if "nlj_emit" in rates and "smj_emit" in rates:
                say(f"    nlj_emit writes at {rates['nlj_emit'] / rates['smj_emit']:.2f} of smj_emit's rate")
    with open(os.path.join(profiles, "join_nested_loop_bench.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

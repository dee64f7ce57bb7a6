"""Times hy_table_scan_expression over lineitem at SF10 against the only device route there was before it -- hy_projection_expression
followed by hy_table_scan(result <> 0) -- for three predicates, both routes alternated in one process, results in device memory
(preallocated once, HY_SCAN_CHUNK_REGIONS):
    l_extendedprice * (1 - l_discount) > 30000
    the Q6 conjunction as one program -- also against the plan's own route: three hy_table_scan calls chained through hy_poslist_translate and
    reference columns (HipExecutor.scan_chunked), PosLists in HBM
    l_quantity < 24 OR l_discount IS NULL
Per route: wall time of the call(s) (each ends with a stream synchronise; the two-call route's result column is freed outside the timed region)
and the HIP-event time of its scan and projection kernels (the chain's translate kernels are in its wall time only); per predicate the bytes the
one-pass scan moves by DESIGN 4.12's model (sum of the columns' stored widths + 8 x selectivity per row) over its kernel time.
Usage: python tools/expression_scan_timing.py [--rows N] [--rounds R]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyrise_amd import abi, storage, tpch   # noqa: E402
from hyrise_amd.operators import ColumnTest, lower_between, make_predicate, projection_expression, projection_program   # noqa: E402


def kernel_us(lib, kind):
    ms, launches = C.c_float(0), C.c_uint32(0)
    abi.check(lib.hy_profile_read_kernel(kind, C.byref(ms), C.byref(launches)))
    return ms.value * 1e3


def timed(lib, call):
    abi.check(lib.hy_set_profiling(1))
    abi.check(lib.hy_synchronize())
    begin = time.perf_counter()
    leftover = call()
    abi.check(lib.hy_synchronize())
    wall = (time.perf_counter() - begin) * 1e6
    if leftover is not None:
        leftover.close()
    kernels = kernel_us(lib, abi.KERNEL_SCAN) + kernel_us(lib, abi.KERNEL_PROJECTION)
    abi.check(lib.hy_profile_read(C.byref(C.c_float(0)), C.byref(C.c_uint32(0))))
    abi.check(lib.hy_set_profiling(0))
    return wall, kernels


def main():
    import torch
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=tpch.LINEITEM_ROWS_SF10)
    parser.add_argument("--rounds", type=int, default=11)
    args = parser.parse_args()
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    from hyrise_amd.distributed import HipExecutor
    ex = HipExecutor(torch.device("cuda", 0))
    rng = np.random.default_rng(1)
    n, chunk = args.rows, abi.CHUNK_DEFAULT_SIZE
    raw = {"l_extendedprice": (rng.integers(90_000, 10_500_000, n) / 100.0).astype(np.float32), "l_discount": (rng.integers(0, 11, n) / 100.0).astype(np.float32),
           "l_quantity": rng.integers(1, 51, n).astype(np.float32), "l_shipdate": rng.integers(0, 2526, n).astype(np.int32)}
    discount_nulls = rng.random(n) < 0.02
    columns = {key: storage.DeviceColumn(storage.make_column(values, discount_nulls if key == "l_discount" else None, abi.ENC_DICTIONARY, chunk)) for key, values in raw.items()}
    n_chunks = columns["l_shipdate"].n_chunks
    widths = {key: columns[key].host.segments[0].width for key in columns}
    price, discount, quantity, shipdate = (columns[k] for k in ("l_extendedprice", "l_discount", "l_quantity", "l_shipdate"))
    one = (abi.TYPE_INT, 1)
    predicates = {
        "l_extendedprice * (1 - l_discount) > 30000": (("cmp", abi.PRED_GREATER_THAN, ("arith", abi.ARITH_MUL, price, ("arith", abi.ARITH_SUB, one, discount)), (abi.TYPE_INT, 30000)),
                                                       ("l_extendedprice", "l_discount")),
        "Q6 as one program": (("and", ("and", ColumnTest(shipdate, make_predicate(abi.PRED_BETWEEN_UPPER_EXCLUSIVE, abi.TYPE_INT, 731, 1096)),
                                       ("between", abi.PRED_BETWEEN_INCLUSIVE, discount, (abi.TYPE_FLOAT, 0.05), (abi.TYPE_FLOAT, 0.07001))),
                               ("cmp", abi.PRED_LESS_THAN, quantity, (abi.TYPE_INT, 24))), ("l_shipdate", "l_discount", "l_quantity"),
                              # (a projection takes no Between column test: the two-call route compares twice)
                              ("and", ("and", ("and", ("cmp", abi.PRED_GREATER_THAN_EQUALS, shipdate, (abi.TYPE_INT, 731)), ("cmp", abi.PRED_LESS_THAN, shipdate, (abi.TYPE_INT, 1096))),
                                       ("between", abi.PRED_BETWEEN_INCLUSIVE, discount, (abi.TYPE_FLOAT, 0.05), (abi.TYPE_FLOAT, 0.07001))),
                               ("cmp", abi.PRED_LESS_THAN, quantity, (abi.TYPE_INT, 24)))),
        "l_quantity < 24 OR l_discount IS NULL": (("or", ("cmp", abi.PRED_LESS_THAN, quantity, (abi.TYPE_INT, 24)), ("is_null", discount)), ("l_quantity", "l_discount")),
    }
    matches = torch.zeros((n + 2, 2), dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n_chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(n_chunks, dtype=torch.int32, device="cuda")
    state = torch.zeros(n_chunks, dtype=torch.uint8, device="cuda")
    result = abi.ScanResult()
    result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH
    result.matches, result.capacity = matches.data_ptr(), n
    result.offsets, result.counts, result.chunk_state = offsets.data_ptr(), counts.data_ptr(), state.data_ptr()
    not_zero = make_predicate(abi.PRED_NOT_EQUALS, abi.TYPE_INT, 0, nullable=True)
    print(f"rows {n}, chunks {n_chunks}, rounds {args.rounds}, dictionary segments, stored widths {widths}")
    for name, (tree, read, *other) in predicates.items():
        lowered = lower_between(tree)
        projected = lower_between(other[0]) if other else lowered
        program, keep = projection_program(lowered)

        def one_pass():
            abi.check(lib.hy_table_scan_expression(C.byref(program), None, 0, C.byref(result)))

        def two_calls():
            column = projection_expression(projected)
            abi.check(lib.hy_table_scan(column.handle, C.byref(not_zero), None, 0, C.byref(result)))
            return column

        routes = {"one pass": one_pass, "two calls": two_calls}
        totals = {}
        for key, call in routes.items():
            leftover = call()
            abi.check(lib.hy_synchronize())
            if leftover is not None:
                leftover.close()
            totals[key] = (int(counts.sum().item()), counts.cpu().numpy().copy())
        assert totals["one pass"][0] == totals["two calls"][0] and (totals["one pass"][1] == totals["two calls"][1]).all(), "the routes differ"
        selectivity = totals["one pass"][0] / n
        if name.startswith("Q6"):
            def three_scans():
                lists = ex.scan_chunked(shipdate, make_predicate(abi.PRED_BETWEEN_UPPER_EXCLUSIVE, abi.TYPE_INT, 731, 1096))
                lists = ex.scan_chunked(ex.reference_column_chunked(discount, lists), make_predicate(abi.PRED_BETWEEN_INCLUSIVE, abi.TYPE_FLOAT, np.float32(0.05), np.float32(0.07001), nullable=True))
                lists = ex.scan_chunked(ex.reference_column_chunked(quantity, lists), make_predicate(abi.PRED_LESS_THAN, abi.TYPE_FLOAT, 24.0))
                three_scans.total = lists.total

            three_scans()
            assert three_scans.total == totals["one pass"][0], "the three-scan chain differs"
            routes["three scans"] = three_scans
        samples = {key: [] for key in routes}
        for _ in range(args.rounds + 2):   # alternated: one pass, two calls, (three scans,) one pass, ...
            for key, call in routes.items():
                samples[key].append(timed(lib, call))
        print(f"-- {name}: {totals['one pass'][0]} matches, selectivity {selectivity:.4f}")
        medians = {}
        for key, rows in samples.items():
            wall, kernel = [r[0] for r in rows[2:]], [r[1] for r in rows[2:]]
            medians[key] = (statistics.median(wall), max(wall) - min(wall), statistics.median(kernel))
            label = "scan kernels only, us" if key == "three scans" else "kernels us"   # (the chain's translate / gather kernels are in its wall time only)
            print(f"{key:10s} {label} median {statistics.median(kernel):8.1f} min {min(kernel):8.1f} max {max(kernel):8.1f}   "
                  f"wall us median {statistics.median(wall):8.1f} min {min(wall):8.1f} max {max(wall):8.1f}")
        spread = max(medians["one pass"][1], medians["two calls"][1])
        gain = medians["two calls"][0] - medians["one pass"][0]
        model_bytes = n * (sum(widths[key] for key in read) + 8 * selectivity)
        if "three scans" in medians:
            print(f"three-scan chain: wall median {medians['three scans'][0]:.1f} us against {medians['one pass'][0]:.1f} us in one pass (reported, decides nothing: the fused operator is Q6's path)")
        print(f"one pass is {gain:.1f} us faster (wall medians); largest spread of either side {spread:.1f} us: {'beyond' if gain > spread else 'WITHIN'} the spread")
        print(f"byte model {model_bytes / 1e6:.1f} MB -> {model_bytes / medians['one pass'][2] / 1e6:.2f} TB/s over the one-pass kernel time")
        del keep


if __name__ == "__main__":
    main()

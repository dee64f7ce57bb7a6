#!/usr/bin/env python3
"""AggregateHash's result in host arrays (hy_aggregate_hash, HY_MEM_HOST) against the output table left in HBM (hy_aggregate_hash_columns), one
process.  Case A of DESIGN.md section 4.3: SF10 lineitem (59 986 052 rows), GROUP BY l_orderkey with SUM(l_quantity), COUNT(*) -- 15 M groups.
The two calls alternate (the order swaps from step to step); host time of the call and HIP-event time on the library's stream, median and
minimum per call, the host call's own spread (max / min over the steps), and in how many pairs the columns call was not slower.  Both results
are compared once, byte for byte -- the full-size parity check.
Usage: python tools/aggregate_columns_bench.py [steps] [scale factor]   (not part of the product.  Per-kernel times:
rocprofv3 --kernel-trace --stats -- python tools/aggregate_columns_bench.py 3)
Case A' is the same pair over four groups (GROUP BY l_orderkey & 3): what the columns call costs where the result is finished on the host.
Case B -- the C++ mirror's AggregateHash -> TableScan (HAVING SUM > 300) -> Sort with a row limit of 100 at the same size, device-resident
results against device_resident_results(false) -- is tests/cpp/aggregate_columns_tests --chain-bench, which this script runs last.

Bytes written per group by the finish (a model): per aggregate the cell (8 B here) and 1/8 B of null bitmap, 8 B of RowID, and 4 B of gathered key;
hy_aggregate_hash writes 8 + 1 B per aggregate and 8 B of RowID into staging memory and copies them to the host once more."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    import torch
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import HostAggregateResult, aggregate_hash, aggregate_hash_columns
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    data = tpch.TpchData(scale, 42)
    quantity = DeviceColumn(storage.make_column(data.l_quantity, None, abi.ENC_DICTIONARY))
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    abi.check(lib.hy_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def timed(call):
        begin.record()
        t0 = time.perf_counter()
        result = call()
        elapsed = time.perf_counter() - t0
        end.record()
        end.synchronize()
        return result, elapsed * 1e3, begin.elapsed_time(end)

    def close(result):
        for column in result.aggregates + result.groupby:
            column.close()
        result.row_ids.close()

    def case(title, key):
        aggregates = [(abi.AGG_SUM, quantity), (abi.AGG_COUNT, None)]
        host = HostAggregateResult(len(aggregates), key.rows + 1)

        def host_call():
            return aggregate_hash([key], aggregates, result=host)

        def columns_call():
            return aggregate_hash_columns([key], aggregates)

        host_call()
        columns = columns_call()
        n = host.n_groups
        assert columns.n_groups == n and columns.row_ids.numpy().tobytes() == host.row_ids[:n].tobytes()
        for a in range(len(aggregates)):
            values, nulls = columns.aggregates[a].read()
            assert values.tobytes() == host.raw[a][:n].tobytes() and not nulls.any() and not host.nulls[a][:n].any()
        close(columns)
        model = sum(8 + 1 / 8 for _ in aggregates) + 8 + 4
        print(f"{title}: {key.rows} rows, {n} groups, parity OK; the finish writes {model:.2f} B per group = {model * n / 1e6:.1f} MB "
              f"(host result: {sum(9 for _ in aggregates) + 8} B per group, staged and copied)", flush=True)
        times = {"hy_aggregate_hash": [], "hy_aggregate_hash_columns": []}
        for step in range(steps):
            for name in (list(times) if step % 2 == 0 else list(times)[::-1]):
                result, host_ms, event_ms = timed(host_call if name == "hy_aggregate_hash" else columns_call)
                times[name].append((host_ms, event_ms))
                if name == "hy_aggregate_hash_columns":
                    close(result)
        base = np.array(times["hy_aggregate_hash"])
        other = np.array(times["hy_aggregate_hash_columns"])
        for name, t in (("hy_aggregate_hash", base), ("hy_aggregate_hash_columns", other)):
            print(f"  {name:28s} host {np.median(t[:, 0]):8.3f} ms (min {t[:, 0].min():.3f})  events {np.median(t[:, 1]):8.3f} ms (min {t[:, 1].min():.3f})  median of {steps}", flush=True)
        print(f"  host call's spread max/min {base[:, 0].max() / base[:, 0].min():.3f}; columns / host {np.median(other[:, 0]) / np.median(base[:, 0]):.3f} (host time), "
              f"not slower in {int(np.sum(other[:, 0] <= base[:, 0]))}/{steps} pairs", flush=True)

    case("case A  GROUP BY l_orderkey, SUM(l_quantity), COUNT(*)", DeviceColumn(storage.make_column(data.l_orderkey, None, abi.ENC_FRAME_OF_REFERENCE)))
    case("case A' GROUP BY l_orderkey & 3, SUM(l_quantity), COUNT(*)", DeviceColumn(storage.make_column((data.l_orderkey & 3).astype(np.int32), None, abi.ENC_DICTIONARY)))
    n_orders = data.n_orders
    del data, quantity
    abi.check(lib.hy_set_stream(None))
    binary = os.path.join(ROOT, "tests", "cpp", "aggregate_columns_tests")
    if os.path.exists(binary) and "--no-chain" not in sys.argv:
        sys.stdout.flush()
        subprocess.run([binary, "--chain-bench", str(max(1, steps // 2)), str(n_orders)], check=True)

if __name__ == "__main__":
    main()

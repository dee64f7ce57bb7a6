"""Times the Q1 charge expression l_extendedprice * (1 - l_discount) * (1 + l_tax) over lineitem at SF10 as one hy_projection_expression
program against the chain of hy_projection_arithmetic calls, alternated in one process, and the Q14 shape CASE WHEN p_type LIKE 'PROMO%'
THEN l_extendedprice * (1 - l_discount) ELSE 0 END (which has no predecessor).  Per form: wall time of the call(s) (they end with a stream
synchronise) and the HIP-event time of the projection kernels.  Usage: python tools/projection_expression_timing.py [--rows N] [--rounds R]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hyrise_amd import abi, storage, tpch   # noqa: E402
from hyrise_amd.operators import ColumnTest, make_predicate, projection_expression   # noqa: E402


def timed(lib, call):
    abi.check(lib.hy_set_profiling(1))
    abi.check(lib.hy_synchronize())
    begin = time.perf_counter()
    result = call()
    abi.check(lib.hy_synchronize())
    wall = (time.perf_counter() - begin) * 1e6
    ms, launches = C.c_float(0), C.c_uint32(0)
    abi.check(lib.hy_profile_read_kernel(abi.KERNEL_PROJECTION, C.byref(ms), C.byref(launches)))
    abi.check(lib.hy_profile_read(C.byref(C.c_float(0)), C.byref(C.c_uint32(0))))
    abi.check(lib.hy_set_profiling(0))
    result.close()
    return wall, ms.value * 1e3, launches.value


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=tpch.LINEITEM_ROWS_SF10)
    parser.add_argument("--rounds", type=int, default=15)
    args = parser.parse_args()
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    rng = np.random.default_rng(1)
    n, chunk = args.rows, abi.CHUNK_DEFAULT_SIZE
    raw = {"l_extendedprice": (rng.integers(90_000, 10_500_000, n) / 100.0).astype(np.float32), "l_discount": (rng.integers(0, 11, n) / 100.0).astype(np.float32),
           "l_tax": (rng.integers(0, 9, n) / 100.0).astype(np.float32)}
    codes = rng.integers(0, 150, n).astype(np.uint8)   # p_type behind the join: 150 distinct strings, 25 of them PROMO ...
    p_type = storage.HostColumn([storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, len(part), 1, part, aux=None, aux_size=150)
                                 for part in (codes[b:b + chunk] for b in range(0, n, chunk))], abi.TYPE_STRING)
    p_type_dev = storage.DeviceColumn(p_type)
    matches = [[v < 25 for v in range(150)]] * p_type.n_chunks
    print(f"rows {n}, chunks {p_type.n_chunks}, rounds {args.rounds}")
    for encoding, name in ((abi.ENC_UNENCODED, "unencoded value segments"), (abi.ENC_DICTIONARY, "dictionary segments (q1_columns' encoding)")):
        columns = {key: storage.DeviceColumn(storage.make_column(values, None, encoding, chunk)) for key, values in raw.items()}
        like = make_predicate(abi.PRED_LIKE, abi.TYPE_STRING, dictionary_matches=matches)
        one = (abi.TYPE_INT, 1)
        q14 = lambda: projection_expression(("case", ColumnTest(p_type_dev, like), ("arith", abi.ARITH_MUL, columns["l_extendedprice"], ("arith", abi.ARITH_SUB, one, columns["l_discount"])), (abi.TYPE_INT, 0)))
        forms = {"chain": lambda: tpch.q1_charge_chain(columns), "program": lambda: tpch.q1_charge_program(columns), "q14": q14}
        a, b = tpch.q1_charge_chain(columns), tpch.q1_charge_program(columns)
        assert a.read()[0].tobytes() == b.read()[0].tobytes(), "chain and program differ"
        a.close(), b.close()
        samples = {key: [] for key in forms}
        for _ in range(args.rounds):   # alternated: chain, program, q14, chain, ...
            for key, call in forms.items():
                samples[key].append(timed(lib, call))
        print(f"-- {name}")
        for key, rows in samples.items():
            wall, kernel = [r[0] for r in rows[2:]], [r[1] for r in rows[2:]]
            print(f"{key:8s} kernel launches {rows[-1][2]}  kernels us median {statistics.median(kernel):8.1f} min {min(kernel):8.1f} max {max(kernel):8.1f}   "
                  f"wall us median {statistics.median(wall):8.1f} min {min(wall):8.1f}")
        for column in columns.values():
            column.close()


if __name__ == "__main__":
    main()

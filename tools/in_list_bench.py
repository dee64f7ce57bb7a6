#!/usr/bin/env python3
"""TableScan IN over a literal list (hy_table_scan_in_list) at SF10 lineitem (59 986 052 rows), one process, results in device memory:
  l_quantity IN (k values), k = 4, 8, 19, on the dictionary copy (DictionarySegment<float>, u8 value ids) and on the unencoded copy
  l_shipmode IN (4 strings) on a string dictionary (u8 value ids, seven modes drawn uniformly: the generator has no such column)
each against
  (1) ONE Equals scan of the same column -- the floor: the IN scan moves the same column bytes
  (2) the only device route there was before: k Equals scans joined by hy_union_positions (a balanced tree of k - 1 unions)
in rotating order within one session.  Usage: python tools/in_list_bench.py [steps]   (not part of the product; DESIGN.md section 4.1 and
profiles/in_list_scan.txt quote its output)

What route (2)'s figure leaves out, in its favour: the unions read reference columns that were built before the timed region (from the
same PosLists); creating those columns from the scans' results (hy_column_create, a counts transfer per scan) is not timed.

Bytes (a model from the shapes): a scan reads the column once (w bytes per row) and writes 8 bytes per match; route (2) reads the column
k times, writes every element's PosList, and every union reads its two inputs and writes their union."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = [b"AIR", b"FOB", b"MAIL", b"RAIL", b"REG AIR", b"SHIP", b"TRUCK"]   # sorted byte-wise: a chunk's dictionary


class DeviceResult:
    """A scan result in device memory (chunk regions), reused by every timed call."""

    def __init__(self, lib, column):
        from hyrise_amd import abi
        self.buffers = []
        r = abi.ScanResult()
        r.mem, r.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS | abi.SCAN_MATERIALIZE_ALL_MATCH
        for field, nbytes in (("matches", 8 * max(1, column.rows)), ("offsets", 8 * (column.n_chunks + 1)), ("counts", 4 * max(1, column.n_chunks)), ("chunk_state", max(1, column.n_chunks))):
            pointer = C.c_void_p()
            abi.check(lib.hy_device_malloc(C.byref(pointer), nbytes + 256))
            self.buffers.append(pointer)
            setattr(r, field, pointer.value)
        r.capacity = max(1, column.rows)
        self.c = r


def shipmode_column(n, chunk_size, seed=7):
    from hyrise_amd import abi, storage
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(MODES), n).astype(np.uint8)
    segments = [storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, min(chunk_size, n - b), 1, ids[b:b + chunk_size].copy(), aux=None, aux_size=len(MODES)) for b in range(0, n, chunk_size)]
    return storage.HostColumn(segments, abi.TYPE_STRING), [MODES] * len(segments)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import in_list_predicate, make_predicate, string_in_list_predicate, string_predicate, table_scan, union_positions
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    data = tpch.TpchData(10.0, 42)
    n = data.n_lineitems
    chunk = abi.CHUNK_DEFAULT_SIZE
    shipmode_host, shipmode_dictionaries = shipmode_column(n, chunk)
    columns = {"l_quantity dictionary u8": (storage.make_column(data.l_quantity, None, abi.ENC_DICTIONARY), 1, None),
               "l_quantity unencoded f32": (storage.make_column(data.l_quantity, None, abi.ENC_UNENCODED), 4, None),
               "l_shipmode dictionary u8": (shipmode_host, 1, shipmode_dictionaries)}
    quantities = [3.0, 17.0, 24.0, 36.0, 49.0, 8.0, 11.0, 42.0, 1.0, 5.0, 13.0, 19.0, 22.0, 27.0, 30.0, 33.0, 39.0, 45.0, 50.0]

    def sync():
        abi.check(lib.hy_synchronize())

    print(f"rows {n}, {steps} steps per figure, ms = median [min .. max] of host-timed calls bracketed by hy_synchronize", flush=True)
    for name, (host, width, dictionaries) in columns.items():
        dev = DeviceColumn(host)
        result = DeviceResult(lib, dev)
        for k in ((4,) if dictionaries is not None else (4, 8, 19)):
            elements = [MODES[i] for i in (0, 2, 4, 5)] if dictionaries is not None else quantities[:k]
            if dictionaries is not None:
                in_list = string_in_list_predicate(dictionaries, elements)
                equals = [string_predicate(abi.PRED_EQUALS, dictionaries, e) for e in elements]
            else:
                in_list = in_list_predicate(abi.TYPE_FLOAT, elements)
                equals = [make_predicate(abi.PRED_EQUALS, abi.TYPE_FLOAT, e) for e in elements]
            # setup of route (2): every element's PosLists and every union of the tree as reference columns (not timed)
            level, unions, matches = [], [], 0
            for p in equals:
                scan = table_scan(dev, p, flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
                lists = [scan.pos_list(c).copy() for c in range(dev.n_chunks)]
                reference = storage.make_reference_column(host, lists, list(range(dev.n_chunks)))
                level.append(DeviceColumn(reference, refs={id(host): dev}))
                matches += scan.total
            union_bytes = 0
            while len(level) > 1:
                above = []
                for i in range(0, len(level) - 1, 2):
                    unions.append((level[i], level[i + 1]))
                    out = union_positions([level[i]], [level[i + 1]])
                    rows = out.numpy()
                    out.close()
                    union_bytes += 8 * (level[i].rows + level[i + 1].rows + len(rows))
                    reference = storage.make_reference_column(host, [rows], [None])
                    above.append(DeviceColumn(reference, refs={id(host): dev}))
                if len(level) % 2:
                    above.append(level[-1])
                level = above
            assert level[0].rows == matches

            def run_in():
                abi.check(lib.hy_table_scan_in_list(dev.handle, C.byref(in_list), None, 0, C.byref(result.c)))

            def run_equals():
                abi.check(lib.hy_table_scan(dev.handle, C.byref(equals[0]), None, 0, C.byref(result.c)))

            def run_union_route():
                for p in equals:
                    abi.check(lib.hy_table_scan(dev.handle, C.byref(p), None, 0, C.byref(result.c)))
                for left, right in unions:
                    union_positions([left], [right]).close()

            routes = [("IN", run_in), ("Equals", run_equals), ("kEquals+union", run_union_route)]
            times = {label: [] for label, _ in routes}
            for _, call in routes:   # warm-up
                call()
                sync()
            for step in range(steps):
                for r in range(len(routes)):   # rotating order
                    label, call = routes[(step + r) % len(routes)]
                    sync()
                    t0 = time.perf_counter()
                    call()
                    sync()
                    times[label].append(1e3 * (time.perf_counter() - t0))
            # the scan kernel alone (HIP events around scan_slices)
            kernel_ms = {}
            for label, call in routes[:2]:
                samples = []
                for _ in range(5):
                    abi.check(lib.hy_set_profiling(1))   # (re-enabling starts a new session: the sums below are of this one launch)
                    call()
                    sync()
                    ms, count = C.c_float(0), C.c_uint32(0)
                    abi.check(lib.hy_profile_read_kernel(abi.KERNEL_SCAN, C.byref(ms), C.byref(count)))
                    assert count.value == 1, count.value
                    samples.append(ms.value)
                    abi.check(lib.hy_profile_read(C.byref(ms), C.byref(count)))   # clears the session
                kernel_ms[label] = float(np.median(samples))
            abi.check(lib.hy_set_profiling(0))
            med = {label: float(np.median(v)) for label, v in times.items()}
            spread = max(max(v) - min(v) for v in times.values())
            in_bytes = n * width + 8 * matches
            route_bytes = k * n * width + 8 * matches + union_bytes
            print(f"{name:26s} k {k:2d} matches {matches:9d} | " +
                  " | ".join(f"{label} {med[label]:7.3f} [{min(times[label]):.3f} .. {max(times[label]):.3f}]" for label, _ in routes) +
                  f" | IN/Equals {med['IN'] / med['Equals']:.2f}  union-route/IN {med['kEquals+union'] / med['IN']:.2f}  largest spread {spread:.3f} ms"
                  f" | kernel: IN {kernel_ms['IN']:.3f} Equals {kernel_ms['Equals']:.3f} ms | bytes IN {in_bytes / 1e6:.0f} MB ({in_bytes / (kernel_ms['IN'] * 1e-3) / 1e12:.2f} TB/s in the kernel)"
                  f" union route {route_bytes / 1e6:.0f} MB", flush=True)
            del level, unions


if __name__ == "__main__":
    main()

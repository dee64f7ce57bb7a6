#!/usr/bin/env python3
"""Sort with a row limit (hy_sort_limit) against Sort (hy_sort) over SF10 lineitem (59 986 052 rows), one process.  Cases (a), (b), (c) of
tools/sort_bench.py, each with k in {1, 100, 10 000, 1 000 000, rows / 8}; per k the four calls
  hy_sort | hy_sort_limit flags 0 | FORCE_SELECT | FORCE_FULL_SORT
run in an order that rotates from step to step, into output blocks acquired before the clock starts; median and minimum per call, hy_sort's own
spread (max / min over the steps), the path flags 0 took, and the candidate rows the selection sorts (restated on the host from the keys).
Every (case, k): the FORCE_SELECT result must equal the first k RowIDs of hy_sort's output -- the full-size parity check.
Usage: python tools/sort_limit_bench.py [steps]   (not part of the product; DESIGN.md section 4.7 quotes its output.  Per-kernel times:
rocprofv3 --kernel-trace --stats -- python tools/sort_limit_bench.py 3)

Bytes of the selection (a model, as sort_bench.py's): definition 0's export and stats pass as in hy_sort, 9 B/row per histogram level and for
the marking pass, 1/4 B/row of masks written and read; the later definitions' export and stats over all rows; then hy_sort's word sorts over
the candidates only, and 12 B per output row."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sort_bench import bytes_moved, order_words  # noqa: E402

DIGIT_BITS, REFINE_SHARE_DIVISOR = 11, 16   # sort.hip: SELECT_DIGIT_BITS, REFINE_SHARE_DIVISOR


def relative_keys(values, descending):
    """Definition 0's key as sort.hip's select_key forms it (no NULLs here), sorted, and its bits."""
    v = np.ascontiguousarray(values)
    wide = v.dtype.itemsize == 8
    u = v.view(np.uint64 if wide else np.uint32).copy()
    sign = np.uint64(1 << 63) if wide else np.uint32(1 << 31)
    if v.dtype.kind == "f":
        u[u == sign] = 0
        u = np.where((u & sign) != 0, ~u, u | sign)
    else:
        u = u ^ sign
    if descending:
        u = ~u
    u = u.astype(np.uint64)
    lo, hi = u & np.uint64(0xFFFFFFFF), u >> np.uint64(32)
    lo_bits = int(int(lo.max()) - int(lo.min())).bit_length()
    hi_bits = int(int(hi.max()) - int(hi.min())).bit_length()
    keys = ((hi - hi.min()) << np.uint64(lo_bits)) | (lo - lo.min())
    keys.sort()
    return keys, lo_bits + hi_bits


def candidates_of(sorted_keys, total_bits, k):
    """(candidate rows, histogram levels) of hy_sort_limit's selection for the first k rows."""
    n, shift, levels, need = len(sorted_keys), total_bits, 0, k
    below, upto = 0, n
    while shift > 0 and (levels == 0 or (upto - below > need and upto - below > n // REFINE_SHARE_DIVISOR)):
        shift -= min(shift, DIGIT_BITS)
        levels += 1
        prefix = int(sorted_keys[k - 1]) >> shift
        new_below = int(np.searchsorted(sorted_keys, np.uint64(prefix << shift), "left"))
        upto = int(np.searchsorted(sorted_keys, np.uint64(((prefix + 1) << shift) - 1), "right"))
        below, need = new_below, k - new_below
    return upto, levels


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import make_predicate, table_scan
    from hyrise_amd.storage import DeviceColumn
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    data = tpch.TpchData(10.0, 42)
    n = data.n_lineitems
    run_start = np.flatnonzero(np.concatenate([[True], data.l_orderkey[1:] != data.l_orderkey[:-1]]))
    l_linenumber = (np.arange(n) - np.repeat(run_start, np.diff(np.concatenate([run_start, [n]])))).astype(np.int32) + 1
    hosts = {"l_extendedprice": storage.make_column(data.l_extendedprice, None, abi.ENC_UNENCODED),
             "l_orderkey": storage.make_column(data.l_orderkey, None, abi.ENC_FRAME_OF_REFERENCE),
             "l_linenumber": storage.make_column(l_linenumber, None, abi.ENC_FRAME_OF_REFERENCE),
             "l_shipdate": storage.make_column(data.l_shipdate, None, abi.ENC_DICTIONARY)}
    devs = {name: DeviceColumn(h) for name, h in hosts.items()}
    stored = {"l_extendedprice": 4, "l_orderkey": 2, "l_linenumber": 1}
    scan = table_scan(devs["l_shipdate"], make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, tpch.DAY_1995_01_01), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    pos_lists = [scan.pos_list(c).copy() for c in range(devs["l_shipdate"].n_chunks)]
    matched = np.concatenate([p[:, 0].astype(np.int64) * abi.CHUNK_DEFAULT_SIZE + p[:, 1] for p in pos_lists])
    ref_hosts = {name: storage.make_reference_column(hosts[name], pos_lists, list(range(len(pos_lists)))) for name in ("l_orderkey", "l_linenumber")}
    refs = {name: DeviceColumn(h, refs={id(hosts[name]): devs[name]}) for name, h in ref_hosts.items()}
    ASC, DESC = abi.SORT_ASCENDING_NULLS_FIRST, abi.SORT_DESCENDING_NULLS_FIRST
    cases = [("(a) ORDER BY l_extendedprice", [devs["l_extendedprice"]], [ASC], [(data.l_extendedprice, None, False)], ["l_extendedprice"]),
             ("(b) ORDER BY l_orderkey DESC, l_linenumber", [devs["l_orderkey"], devs["l_linenumber"]], [DESC, ASC],
              [(data.l_orderkey, None, True), (l_linenumber, None, False)], ["l_orderkey", "l_linenumber"]),
             ("(c) (b) over the l_shipdate < 1995-01-01 scan", [refs["l_orderkey"], refs["l_linenumber"]], [DESC, ASC],
              [(data.l_orderkey[matched], None, True), (l_linenumber[matched], None, False)], ["l_orderkey", "l_linenumber"])]
    variants = [("hy_sort", None), ("flags 0", 0), ("FORCE_SELECT", abi.SORT_LIMIT_FORCE_SELECT), ("FORCE_FULL_SORT", abi.SORT_LIMIT_FORCE_FULL_SORT)]
    for name, columns, modes, keys, stored_names in cases:
        rows = columns[0].rows
        array = (abi.SortKey * len(columns))()
        for i, (column, mode) in enumerate(zip(columns, modes)):
            array[i].column, array[i].mode = column.handle, mode
        blocks = [C.c_void_p() for _ in range(2)]   # [0]: hy_sort's rows, [1]: hy_sort_limit's
        for block in blocks:
            abi.check(lib.hy_result_pool_acquire(8 * rows, C.byref(block)))
        n_out, path = C.c_uint64(0), C.c_uint32(0)

        def call(flags, k):
            t0 = time.perf_counter()
            if flags is None:
                status = lib.hy_sort(array, len(columns), blocks[0].value, rows, C.byref(n_out))
            else:
                status = lib.hy_sort_limit(array, len(columns), k, flags, blocks[1].value, rows, C.byref(n_out), C.byref(path))
            elapsed = time.perf_counter() - t0
            abi.check(status)
            return elapsed

        pos_list_bytes = 8 if name.startswith("(c)") else 0
        stored_bytes = [stored[s] + pos_list_bytes for s in stored_names]
        full_bytes = bytes_moved(rows, stored_bytes, keys)
        sorted_keys, total_bits = relative_keys(keys[0][0], keys[0][2])
        word_bytes = 0   # per candidate row: every sorted word's gather and radix passes
        for key in keys:
            bits, width = order_words(*key)
            word_bytes += sum((4 + width + 1 + 4) + 20 * ((b + 7) // 8) for b in bits)
        call(None, 0)
        full = np.zeros((rows, 2), dtype=np.uint32)
        abi.check(lib.hy_memcpy_d2h(full.ctypes.data, blocks[0].value, full.nbytes))
        print(f"{name}  rows {rows}  hy_sort model {full_bytes / 1e9:.2f} GB", flush=True)
        for k in (1, 100, 10_000, 1_000_000, rows // 8):
            candidates, levels = candidates_of(sorted_keys, total_bits, k)
            select_bytes = (rows * (stored_bytes[0] + 9 + 9 + 9 * levels + 9 + 0.25) + sum(rows * (s + 9 + 9) for s in stored_bytes[1:])
                            + candidates * word_bytes + k * 12)
            for flags in (0, abi.SORT_LIMIT_FORCE_SELECT):   # warm-up, and the parity check of the selection
                call(flags, k)
            assert path.value == 1 and n_out.value == k
            got = np.zeros((k, 2), dtype=np.uint32)
            abi.check(lib.hy_memcpy_d2h(got.ctypes.data, blocks[1].value, got.nbytes))
            assert got.tobytes() == full[:k].tobytes(), f"{name} k={k}: the selection differs from hy_sort's prefix"
            times = {label: [] for label, _ in variants}
            default_path = None
            for step in range(steps):
                for j in range(len(variants)):
                    label, flags = variants[(j + step) % len(variants)]
                    times[label].append(call(flags, k))
                    if flags == 0:
                        default_path = path.value
            base = np.array(times["hy_sort"])
            pairs_won = {label: int(np.sum(np.array(times[label]) < base)) for label, _ in variants[1:]}
            print(f"  k {k:>9d}  candidates {candidates:>9d} ({100.0 * candidates / rows:5.2f} %)  levels {levels}  flags 0 took path {default_path}  parity OK  "
                  f"select model {select_bytes / 1e9:5.2f} GB = {select_bytes / 8e12 * 1e3:5.2f} ms at 8 TB/s", flush=True)
            for label, _ in variants:
                t = 1e3 * np.array(times[label])
                extra = f"  spread max/min {t.max() / t.min():.3f}" if label == "hy_sort" else f"  {np.median(base) * 1e3 / np.median(t):5.2f} x hy_sort, faster in {pairs_won[label]}/{steps} pairs"
                print(f"      {label:16s} {np.median(t):8.3f} ms (median of {steps}, min {t.min():.3f}){extra}", flush=True)
        for block in blocks:
            lib.hy_result_pool_release(block.value)


if __name__ == "__main__":
    main()

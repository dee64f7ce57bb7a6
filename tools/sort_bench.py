#!/usr/bin/env python3
"""Sort (hy_sort) over SF10 lineitem (59 986 052 rows), one process: ms per sort and the bytes the kernels move, for
  (a) ORDER BY l_extendedprice
  (b) ORDER BY l_orderkey DESC, l_linenumber
  (c) (b) over the PosLists of the scan  l_shipdate < '1995-01-01'  (a reference table)
Usage: python tools/sort_bench.py [steps]   (not part of the product; DESIGN.md section 4.7 quotes its output)

Bytes (a model of what the kernels read and write, from the shapes; the random gathers counted as the bytes they ask for): per sort key the
export (stored column read once, 8 B values + 1 B null flag written per row) and the stats pass (9 B read per row); per 32-bit word that is not
the same in every row the gather (4 B permutation read, value + null flag gathered, 4 B key written) and sort_pairs_u32's passes, one per 8
key bits (histogram: 4 B read; scatter: 8 B read, 8 B written per row); then the positions (4 B read, 8 B written per row)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def order_words(values, nulls, descending):
    """The 32-bit words hy_sort sorts for one key and the bits each needs (sort.hip: order_key, the min / max reduction)."""
    v = np.ascontiguousarray(values[~nulls] if nulls is not None else values)
    wide = v.dtype.itemsize == 8
    u = v.view(np.uint64 if wide else np.uint32).copy()
    sign = np.uint64(1 << 63) if wide else np.uint32(1 << 31)
    if v.dtype.kind == "f":
        u[u == sign] = 0
        negative = (u & sign) != 0
        u = np.where(negative, ~u, u | sign)
    else:
        u = u ^ sign
    if descending:
        u = ~u
    words = [u & np.uint64(0xFFFFFFFF), u >> np.uint64(32)] if wide else [u]
    bits = []
    for w in words:
        lo, hi = (int(w.min()), int(w.max())) if len(w) else (0, 0)
        if lo != hi:
            bits.append(int(hi - lo).bit_length())
    if nulls is not None and 0 < int(nulls.sum()) < len(nulls):
        bits.append(1)
    return bits, v.dtype.itemsize


def bytes_moved(rows, stored_bytes_per_row, keys):
    """keys: [(values, nulls, descending)] in the order of the sort definitions."""
    total = 0
    for (values, nulls, descending), stored in zip(keys, stored_bytes_per_row):
        bits, width = order_words(values, nulls, descending)
        total += rows * (stored + 9) + rows * 9
        for b in bits:
            total += rows * (4 + width + 1 + 4) + rows * 20 * ((b + 7) // 8)
    return total + rows * 12


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    from hyrise_amd import abi, storage, tpch
    from hyrise_amd.operators import make_predicate, sort, table_scan
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
    stored = {"l_extendedprice": 4, "l_orderkey": 2, "l_linenumber": 1}   # bytes per row as stored (FoR offsets: u16 / u8)
    # (c): the scan's PosLists as reference columns of the same table
    scan = table_scan(devs["l_shipdate"], make_predicate(abi.PRED_LESS_THAN, abi.TYPE_INT, tpch.DAY_1995_01_01), flags=abi.SCAN_MATERIALIZE_ALL_MATCH)
    pos_lists = [scan.pos_list(c).copy() for c in range(devs["l_shipdate"].n_chunks)]
    matched = np.concatenate([p[:, 0].astype(np.int64) * abi.CHUNK_DEFAULT_SIZE + p[:, 1] for p in pos_lists])
    ref_hosts = {name: storage.make_reference_column(hosts[name], pos_lists, list(range(len(pos_lists)))) for name in ("l_orderkey", "l_linenumber")}
    refs = {name: DeviceColumn(h, refs={id(hosts[name]): devs[name]}) for name, h in ref_hosts.items()}
    cases = [("(a) ORDER BY l_extendedprice", [devs["l_extendedprice"]], [abi.SORT_ASCENDING_NULLS_FIRST],
              [(data.l_extendedprice, None, False)], ["l_extendedprice"]),
             ("(b) ORDER BY l_orderkey DESC, l_linenumber", [devs["l_orderkey"], devs["l_linenumber"]], [abi.SORT_DESCENDING_NULLS_FIRST, abi.SORT_ASCENDING_NULLS_FIRST],
              [(data.l_orderkey, None, True), (l_linenumber, None, False)], ["l_orderkey", "l_linenumber"]),
             ("(c) (b) over the l_shipdate < 1995-01-01 scan", [refs["l_orderkey"], refs["l_linenumber"]], [abi.SORT_DESCENDING_NULLS_FIRST, abi.SORT_ASCENDING_NULLS_FIRST],
              [(data.l_orderkey[matched], None, True), (l_linenumber[matched], None, False)], ["l_orderkey", "l_linenumber"])]
    for name, columns, modes, keys, stored_names in cases:
        rows = columns[0].rows
        pos_list_bytes = 8 if name.startswith("(c)") else 0   # a reference column's export reads its PosList too
        moved = bytes_moved(rows, [stored[s] + pos_list_bytes for s in stored_names], keys)
        for _ in range(2):
            sort(columns, modes).close()
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            out = sort(columns, modes)   # (hy_sort returns when the positions are complete)
            times.append(time.perf_counter() - t0)
            out.close()
        ms = 1e3 * float(np.median(times))
        print(f"{name:48s} rows {rows:>10d}  {ms:8.2f} ms/sort (median of {steps}, min {1e3 * min(times):.2f})  bytes {moved / 1e9:6.2f} GB  "
              f"-> {moved / (ms * 1e-3) / 1e12:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()

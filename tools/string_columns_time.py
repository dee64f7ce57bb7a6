#!/usr/bin/env python3
"""String ColumnVsColumn l_commitdate < l_receiptdate on SF10-shaped lineitem date columns: chunks of 65 535 rows, about 2 500 distinct
ISO dates per chunk and column, u16 value ids.  Medians of HIP-event times, alternating per round which call goes first:
  (a) string_rank, the ranking launch                     the library's event pair (HY_KERNEL_STRING_RANK)
  (b) the row pass of hy_table_scan_columns_strings       the library's event pair (HY_KERNEL_SCAN)
  (c) hy_table_scan_columns_strings, the whole call       an event pair on the call's stream around it (device result: nothing waits)
  (d) hy_table_scan_columns over the two int32 stand-ins  the yardstick: (b) is this kernel; event pair (HY_KERNEL_SCAN) and whole call
Usage: python tools/string_columns_time.py [chunks = 916] [rounds = 21]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 916
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 21
    import numpy as np
    import torch
    from hyrise_amd import abi
    from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn, HostSegment
    import string_columns_oracle as oracle
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    rows_per_chunk = 65_535
    rng = np.random.default_rng(43)
    epoch = np.datetime64("1992-01-01")
    string_segments, twin_segments, dictionaries = ([], []), ([], []), ([], [])
    for c in range(chunks):
        orderdate = rng.integers(0, 2406, rows_per_chunk)
        days = (orderdate + rng.integers(30, 91, rows_per_chunk), orderdate + rng.integers(2, 152, rows_per_chunk))   # l_commitdate, l_receiptdate
        entries = []
        for side in (0, 1):
            distinct, ids = np.unique(days[side], return_inverse=True)          # ISO dates order as their day numbers do
            entries.append([str(epoch + int(d)).encode() for d in distinct])
            dictionaries[side].append(entries[side])
            ids = ids.astype(np.uint16)
            string_segments[side].append(HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, rows_per_chunk, 2, ids, aux=None, aux_size=len(distinct)))
        tables = (np.asarray(oracle.ranks(entries[0], entries[1]), dtype=np.int32), np.arange(0, 2 * len(entries[1]), 2, dtype=np.int32))
        for side in (0, 1):
            s = string_segments[side][-1]
            twin_segments[side].append(HostSegment(abi.ENC_DICTIONARY, abi.TYPE_INT, s.size, 2, s.data, aux=tables[side], aux_size=s.aux_size))
    rows = chunks * rows_per_chunk
    left, right = (DeviceColumn(HostColumn(string_segments[side], abi.TYPE_STRING)) for side in (0, 1))
    left_twin, right_twin = (DeviceColumn(HostColumn(twin_segments[side], abi.TYPE_INT)) for side in (0, 1))
    left_dict, right_dict = (DeviceStringDictionary(dictionaries[side]) for side in (0, 1))
    entries_per_chunk = sum(len(d) for d in dictionaries[0]) / chunks, sum(len(d) for d in dictionaries[1]) / chunks

    stream = torch.cuda.Stream()
    abi.check(lib.hy_set_stream(C.c_void_p(stream.cuda_stream)))
    matches = torch.empty((rows + 2, 2), dtype=torch.int32, device="cuda")
    offsets = torch.zeros(chunks + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(chunks, dtype=torch.int32, device="cuda")
    result = abi.ScanResult()
    result.mem, result.flags = abi.MEM_DEVICE, abi.SCAN_CHUNK_REGIONS
    result.matches, result.capacity, result.offsets, result.counts = matches.data_ptr(), rows, offsets.data_ptr(), counts.data_ptr()

    def strings():
        abi.check(lib.hy_table_scan_columns_strings(left.handle, left_dict.handle, right.handle, right_dict.handle, abi.PRED_LESS_THAN, C.byref(result)))

    def twins():
        abi.check(lib.hy_table_scan_columns(left_twin.handle, right_twin.handle, abi.PRED_LESS_THAN, C.byref(result)))

    def kernel_ms(kind):
        ms, launches = C.c_float(0), C.c_uint32(0)
        abi.check(lib.hy_profile_read_kernel(kind, C.byref(ms), C.byref(launches)))
        return ms.value / max(1, launches.value)

    def timed(call):
        """One call: (event pair around the whole call on its stream, string_rank's pair, the scan kernel's pair), in ms."""
        abi.check(lib.hy_set_profiling(1))
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        call()
        end.record(stream)
        end.synchronize()
        times = begin.elapsed_time(end), kernel_ms(abi.KERNEL_STRING_RANK), kernel_ms(abi.KERNEL_SCAN)
        abi.check(lib.hy_set_profiling(0))
        return times

    for call in (strings, twins, strings, twins):      # warm-up: tables uploaded, scratch grown, code loaded
        call()
    torch.cuda.synchronize()
    strings()
    torch.cuda.synchronize()
    want = counts.clone()
    twins()
    torch.cuda.synchronize()
    assert torch.equal(counts, want), "the string scan and the scan over the stand-ins disagree"
    samples = {"strings": [], "twins": []}
    for r in range(rounds):
        for name, call in ((("strings", strings), ("twins", twins)) if r % 2 == 0 else (("twins", twins), ("strings", strings))):
            samples[name].append(timed(call))
    abi.check(lib.hy_set_stream(None))

    def line(label, values):
        values = sorted(values)
        print(f"  {label:58s} median {1e3 * values[len(values) // 2]:9.1f} us  (min {1e3 * values[0]:.1f}, max {1e3 * values[-1]:.1f}, n = {len(values)})")

    print(f"column pair: {chunks} chunks x {rows_per_chunk} rows, {entries_per_chunk[0]:.0f} / {entries_per_chunk[1]:.0f} distinct dates per chunk, u16 value ids; "
          f"l_commitdate < l_receiptdate: {int(want.sum().item())} of {rows} rows")
    line("(a) string_rank (event pair)", [s[1] for s in samples["strings"]])
    line("(b) row pass of hy_table_scan_columns_strings (event pair)", [s[2] for s in samples["strings"]])
    line("(c) hy_table_scan_columns_strings, whole call (stream events)", [s[0] for s in samples["strings"]])
    line("(d) hy_table_scan_columns over the int32 stand-ins, kernel", [s[2] for s in samples["twins"]])
    line("(d) ... whole call (stream events)", [s[0] for s in samples["twins"]])
    overhead = C.c_float(0)
    abi.check(lib.hy_profile_event_overhead(C.byref(overhead)))
    print(f"  an event pair around an empty kernel: {1e3 * overhead.value:.1f} us")


if __name__ == "__main__":
    main()

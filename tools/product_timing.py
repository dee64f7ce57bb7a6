#!/usr/bin/env python3
"""hy_product against the store-only floor of the memory system, and the mirror's Product -> TableScan chain with and without device-resident
results.  One process, device-memory results, host clock around calls that end in a device synchronise, median of 11 calls per variant in
rotating order.  Usage: python tools/product_timing.py [rounds] > profiles/product.txt

  (a) data x data: 916 chunks of 65 535 rows x 1 chunk of 1 row          (rows(cr) = 1: every output row wraps)
  (b) data x data: 1 000 rows x 60 000 rows, each in Hyrise chunks       (one pair, runs of 60 000 equal left rows)
  (c) (b) with both sides behind device PosLists, as a scan leaves them   (8 bytes read per left run and per right element)
Variants: hy_product with write-back stores (HY_OPT_PRODUCT_NONTEMPORAL = 0), with nontemporal 16-byte stores (= 1), and torch's fill_ of
the same two buffers.  Bytes: 16 written per output row (both lists)."""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyrise_amd import abi  # noqa: E402


def main():
    import torch
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    device = torch.device("cuda:0")
    values = torch.zeros(65_536, dtype=torch.int32, device=device)
    keep = [values]

    def data_column(sizes):
        """Chunks of these sizes over ONE small device buffer (HY_MEM_DEVICE: hy_product reads the layout only)."""
        segments = (abi.Segment * len(sizes))()
        for s, size in zip(segments, sizes):
            s.encoding, s.data_type, s.size, s.width, s.data, s.ref_chunk_id = abi.ENC_UNENCODED, abi.TYPE_INT, size, 4, values.data_ptr(), abi.INVALID_CHUNK_ID
        handle = C.c_void_p()
        abi.check(lib.hy_column_create(segments, len(sizes), abi.MEM_DEVICE, C.byref(handle)))
        keep.append(segments)
        return handle

    def scanned_column(data, rows):
        """One chunk behind a device PosList of `rows` RowIDs (0, i): what a scan that keeps every row of chunk 0 leaves in HBM."""
        row_ids = torch.stack([torch.zeros(rows + 2, dtype=torch.int32, device=device), torch.arange(rows + 2, dtype=torch.int32, device=device)], dim=1).contiguous()
        segments = (abi.Segment * 1)()
        s = segments[0]
        s.encoding, s.data_type, s.size, s.width, s.data, s.ref_chunk_id, s.ref = abi.ENC_REFERENCE, abi.TYPE_INT, rows, 8, row_ids.data_ptr(), 0, data
        handle = C.c_void_p()
        abi.check(lib.hy_column_create(segments, 1, abi.MEM_DEVICE, C.byref(handle)))
        keep.extend([row_ids, segments])
        return handle

    left_b, right_b = data_column([1_000]), data_column([60_000])
    cases = [("(a) data x data, 916 x 65 535 rows x 1 row", data_column([65_535] * 916), data_column([1]), 0),
             ("(b) data x data, 1 000 x 60 000 rows", left_b, right_b, 0),
             ("(c) reference x reference over device PosLists, 1 000 x 60 000 rows", scanned_column(left_b, 1_000), scanned_column(right_b, 60_000), 8 * (1_000 + 60_000))]
    print(f"hy_product against torch.Tensor.fill_ of the same two buffers, median of {rounds} calls in rotating order (ms, synchronised host timing)")
    for name, left, right, read_bytes in cases:
        n = C.c_uint64(0)
        abi.check(lib.hy_product_count(left, right, C.byref(n)))
        n = n.value
        lists = [torch.empty(n + 2, dtype=torch.int64, device=device) for _ in range(2)]
        result = abi.ProductResult()
        result.mem, result.capacity, result.left_pos, result.right_pos = abi.MEM_DEVICE, n, lists[0].data_ptr(), lists[1].data_ptr()

        def run_product(nontemporal):
            abi.check(lib.hy_set_option(abi.OPT_PRODUCT_NONTEMPORAL, nontemporal))
            abi.check(lib.hy_product(left, right, C.byref(result)))   # (returns when the lists are complete)

        def run_fill():
            lists[0].fill_(7)
            lists[1].fill_(9)
            torch.cuda.synchronize()

        variants = [("hy_product, write-back stores", lambda: run_product(0)), ("hy_product, nontemporal stores", lambda: run_product(1)), ("fill_ of both buffers", run_fill)]
        times = {label: [] for label, _ in variants}
        for _, call in variants:   # warm-up
            call()
        torch.cuda.synchronize()
        for r in range(rounds):
            for k in range(len(variants)):
                label, call = variants[(r + k) % len(variants)]
                begin = time.perf_counter()
                call()
                times[label].append((time.perf_counter() - begin) * 1e3)
        print(f"{name}: {n} output rows, {16 * n / 1e6:.0f} MB written, {read_bytes} B of PosLists read per pass")
        for label, _ in variants:
            t = sorted(times[label])
            median = statistics.median(t)
            print(f"  {label:32s} median {median:7.3f} ms  (min {t[0]:.3f}, max {t[-1]:.3f})  {16 * n / median / 1e9:6.2f} TB/s")
        abi.check(lib.hy_set_option(abi.OPT_PRODUCT_NONTEMPORAL, 0))
        del lists
    sys.stdout.flush()
    abi.check(lib.hy_shutdown())
    # the C++ mirror: Product -> TableScan, device-resident results against host results, five alternating pairs (a fresh process)
    chain = subprocess.run([os.path.join(ROOT, "tests", "cpp", "product_tests"), "--chain-timing", "1000", "60000", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(chain.stdout, end="")
    return chain.returncode


if __name__ == "__main__":
    sys.exit(main())

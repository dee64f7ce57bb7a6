#!/usr/bin/env python3
"""What matching a large string dictionary costs on the host and on the device.  Usage: python tools/like_dictionary_time.py [chunks] [rounds]
> profiles/like_dictionary.txt

Shape: a column of 229 chunks x 65 535 rows, every chunk with 65 535 distinct strings of 19 - 78 bytes (o_comment at SF10).  Patterns:
NOT LIKE '%special%requests%' (TPC-H Q13), LIKE 'forest%' (Q20), LIKE '%green%' (Q9).  In ONE process (tests/cpp/like_device_tests --timing),
after a warm-up scan on either path, alternating per round which path goes first:
  (a) the mirror's TableScan with the host matcher: find_matches_in_dictionaries + hy_table_scan with staged bitmaps
  (b) the same TableScan over hy_table_scan_like (dictionaries resident in HBM, the matcher on the scan's stream)
  (c) the matcher launch alone, by the library's event pair around like_match; bytes = chars + offsets of every chunk, read once
Host clock around execute() for (a) and (b): the call ends in a transfer that waits for the stream."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    chunks = sys.argv[1] if len(sys.argv) > 1 else "229"
    rounds = sys.argv[2] if len(sys.argv) > 2 else "7"
    binary = os.path.join(ROOT, "tests", "cpp", "like_device_tests")
    if not os.path.exists(binary):
        sys.exit("tests/cpp/like_device_tests missing: run __graft_entry__.build()")
    run = subprocess.run([binary, "--timing", chunks, rounds], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout, end="")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())

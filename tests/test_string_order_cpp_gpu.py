"""Runs tests/cpp/string_order_tests.cpp: the C++ mirror's Sort by a string column with the ranks made on the device
(device_string_rank_column -> hy_column_string_ranks) against std::stable_sort over the strings row by row -- a data table and a TableScan's
output, both directions, NULLs, two keys, a row limit, a materialised output --, the forced host ranking giving the identical table, a
ValueSegment<pmr_string> chunk through host_key_table, and TableScan -> Sort -> Limit.  Fixture: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_string_order(device):
    binary = os.path.join(ROOT, "tests", "cpp", "string_order_tests")
    assert os.path.exists(binary), "tests/cpp/string_order_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "STRING ORDER TESTS PASSED"
    for name in ("StringOrder.DataTableAgainstStableSort", "StringOrder.OverATableScansOutput", "StringOrder.TwoKeysRowLimitAndMaterialization",
                 "StringOrder.AValueSegmentChunkSortsThroughTheHostKeyTable", "StringOrderChain.ScanSortLimit"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

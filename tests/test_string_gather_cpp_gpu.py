"""Runs tests/cpp/string_gather_tests.cpp: the C++ mirror's AggregateHash with string GROUP BY columns and MIN / MAX / ANY over a string column,
device_string_results() on (hy_string_column_gather, hy_string_ranks_gather: DeviceStringDictionarySegments) against off (the host path) cell
for cell, both against a row-by-row evaluation with std::string comparisons, over a data table and a TableScan's output; and AggregateHash ->
TableScan (LIKE) -> Sort without a segment fetch before the final read.  Fixture: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_string_gather(device):
    binary = os.path.join(ROOT, "tests", "cpp", "string_gather_tests")
    assert os.path.exists(binary), "tests/cpp/string_gather_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "STRING GATHER TESTS PASSED"
    for name in ("StringGather.AggregateOverADataTable", "StringGather.AggregateOverATableScansOutput", "StringGather.HostRanksKeepTheHostPath",
                 "StringGatherChain.AggregateLikeScanSortWithoutAFetch"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

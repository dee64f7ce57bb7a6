"""Runs tests/cpp/substr_tests.cpp: the C++ mirror's Projection with SUBSTR over a string column, device_string_results() on (one
hy_string_column_substr: DeviceStringDictionarySegments) against off (the host loop) cell for cell, both against the formula row by row, over
a data table and a TableScan's output; TableScan -> Projection -> AggregateHash -> Sort (Q9's shape) without a segment fetch before the
final read; a column with a ValueSegment<pmr_string> chunk on the host path.  Fixture: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_substr(device):
    binary = os.path.join(ROOT, "tests", "cpp", "substr_tests")
    assert os.path.exists(binary), "tests/cpp/substr_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "SUBSTR TESTS PASSED"
    for name in ("Substr.HostFormula", "Substr.ProjectionOverADataTable", "Substr.ProjectionOverATableScansOutput", "Substr.AValueSegmentChunkTakesTheHostPath",
                 "Substr.OverAnythingButAColumnFails", "SubstrChain.ScanProjectAggregateSortWithoutAFetch"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

"""Runs tests/cpp/string_forward_tests.cpp: the C++ mirror's Projection with a forwarded string column beside a computed one over a
TableScan's output, device_string_results() on (one hy_string_column_materialize: DeviceStringDictionarySegments) against off (the host
loop) cell for cell, both against the rows; TableScan -> Projection -> AggregateHash (GROUP BY the forwarded string) -> Sort (Q1's shape)
without a segment fetch before the final read; Sort with ForceMaterialization::Yes and a row limit of 20 over a string payload column
(hy_string_column_gather at the sorted positions) on against off; a column with a ValueSegment<pmr_string> chunk on the host path.
Fixture: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_string_forward(device):
    binary = os.path.join(ROOT, "tests", "cpp", "string_forward_tests")
    assert os.path.exists(binary), "tests/cpp/string_forward_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "STRING FORWARD TESTS PASSED"
    for name in ("Forward.ProjectionOverATableScansOutput", "Forward.AValueSegmentChunkTakesTheHostPath", "Forward.SortMaterializesAStringPayloadAtTwentyRows",
                 "ForwardChain.ScanProjectAggregateSortWithoutAFetch"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

"""Runs tests/cpp/like_device_tests.cpp: the C++ mirror's TableScan with the LIKE family over hy_table_scan_like (dictionaries from the
residency cache's device_string_dictionary) against the same scans with the host matcher's bitmaps -- PosLists entry by entry, over the
data table and over another scan's output --, the fallback for a pattern the library refuses, and TableScan(LIKE) -> JoinHash ->
AggregateHash with the PosLists staying in HBM.  Fixtures: tests/golden/tbl/int_string_like*.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_like_on_the_device(device):
    binary = os.path.join(ROOT, "tests", "cpp", "like_device_tests")
    assert os.path.exists(binary), "tests/cpp/like_device_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "LIKE DEVICE TESTS PASSED"
    for name in ("LikeDevice.DataTableAgainstHostBitmaps", "LikeDevice.SpecialCharacters", "LikeDevice.OverAnotherScansOutput",
                 "LikeDevice.PatternTooLongFallsBackToTheHostMatcher", "LikeDeviceChain.ScanJoinAggregateStaysInHbm"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

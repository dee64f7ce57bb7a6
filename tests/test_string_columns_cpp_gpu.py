"""Runs tests/cpp/string_columns_tests.cpp: the C++ mirror's TableScan(in, left, condition, right) on two string columns over
hy_table_scan_columns_strings (dictionaries from the residency cache's device_string_dictionary) against a row-by-row comparison of the
strings -- over the data table and over another scan's output --, a string column against a number (a Fail), and TableScan(strings) ->
AggregateHash with the PosLists staying in HBM.  Fixture: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_string_columns(device):
    binary = os.path.join(ROOT, "tests", "cpp", "string_columns_tests")
    assert os.path.exists(binary), "tests/cpp/string_columns_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "STRING COLUMNS TESTS PASSED"
    for name in ("StringColumns.DataTableAgainstTheStrings", "StringColumns.OverAnotherScansOutput", "StringColumns.StringsAgainstNonStringsFail",
                 "StringColumnsChain.ScanAggregateStaysInHbm"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

"""Runs tests/cpp/aggregate_columns_tests.cpp: the C++ mirror's AggregateHash with its output table in HBM (hy_aggregate_hash_columns,
DeviceValueSegment) against the same operator with host results -- the aggregate_test.cpp fixtures of tests/golden/tbl/aggregateoperator, a
scan -> join -> aggregate -> scan -> sort/limit chain that fetches no aggregate column to the host, and a partial chunk range."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_aggregate_columns(device):
    binary = os.path.join(ROOT, "tests", "cpp", "aggregate_columns_tests")
    assert os.path.exists(binary), "tests/cpp/aggregate_columns_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "AGGREGATE COLUMNS TESTS PASSED"
    assert proc.stdout.count("[  OK  ]") == 3 and "FAILED" not in proc.stdout

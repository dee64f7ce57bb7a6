"""Runs tests/cpp/expression_scan_tests.cpp: the C++ mirror's TableScan over a predicate expression through hy_table_scan_expression -- the
predicates the other scan implementations do not take against a row-by-row host evaluation, over a data table and over another scan's output,
BETWEEN on the spine, a Value root, and TableScan(expression) -> Projection -> AggregateHash with nothing leaving HBM."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_expression_scan(device):
    binary = os.path.join(ROOT, "tests", "cpp", "expression_scan_tests")
    assert os.path.exists(binary), "tests/cpp/expression_scan_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "EXPRESSION SCAN TESTS PASSED"
    assert proc.stdout.count("[  OK  ]") == 4 and "FAILED" not in proc.stdout

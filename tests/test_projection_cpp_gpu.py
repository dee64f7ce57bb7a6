"""Runs tests/cpp/projection_tests.cpp: the C++ mirror's Projection over hy_projection_expression -- the evaluator's recorded series over the
fixture tables, forwarding only, forwarded and computed columns over a scan's output, and TableScan -> Projection (CASE over a string column
test) -> AggregateHash with every column staying in HBM."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_projection(device):
    binary = os.path.join(ROOT, "tests", "cpp", "projection_tests")
    assert os.path.exists(binary), "tests/cpp/projection_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl"), os.path.join(ROOT, "tests", "golden", "expression")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "PROJECTION TESTS PASSED"
    assert proc.stdout.count("[  OK  ]") == 4 and "FAILED" not in proc.stdout

"""Runs the reference's Product tests (src/test/lib/operators/product_test.cpp), re-stated in tests/cpp/product_tests.cpp against the C++ mirror's
Product (hyrise_amd/host/hyrise_host.hpp, over hy_product), and the mirror's own: the output's shape and shared PosLists, device-resident
against host results list by list, the chain TableScan -> Product -> TableScan in HBM, and Product -> TableScan against JoinNestedLoop.
Fixtures: tests/golden/tbl/product (see the MANIFEST.json there; tests/test_product_oracle.py verifies it) and tests/golden/tbl/int.tbl."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_product_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "product_tests")
    assert os.path.exists(binary), "tests/cpp/product_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "PRODUCT TESTS PASSED"
    for name in ("ValueSegments", "ReferenceAndValueSegments", "SelfProduct"):
        assert f"[  OK  ] OperatorsProductTest.{name}" in proc.stdout, name
    assert "[  OK  ] TableScan -> Product -> TableScan" in proc.stdout
    assert proc.stdout.count("[  OK  ] Product -> TableScan(left.a < right.b) == JoinNestedLoop Inner") == 2
    assert "FAILED" not in proc.stdout

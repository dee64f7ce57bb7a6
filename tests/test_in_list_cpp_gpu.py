"""Runs tests/cpp/in_list_tests.cpp: the C++ mirror's TableScan with PredicateCondition::In / NotIn (hyrise_amd/host/hyrise_host.hpp), which
scans on the device through hy_table_scan_in_list, over the reference's JoinTestRunner tables -- and the chain TableScan(In) -> JoinHash ->
AggregateHash whose PosLists are DevicePosLists, against the same chain over the union of the elements' Equals scans."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["InListTest.EveryNumericColumnAndEncoding", "InListTest.MixedTypesNullsAndConstants", "InListTest.StringDictionaries", "InListTest.ReferenceInputs",
         "InListChain.ScanJoinAggregateStaysInHbm"]


@pytest.mark.gpu
def test_cpp_in_list_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "in_list_tests")
    assert os.path.exists(binary), "tests/cpp/in_list_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "IN LIST TESTS PASSED" in proc.stdout
    for name in CASES:
        assert f"[  OK  ] {name}" in proc.stdout, name

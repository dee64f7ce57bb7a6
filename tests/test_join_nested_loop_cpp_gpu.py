"""Runs tests/cpp/join_nested_loop_tests.cpp: the C++ mirror's JoinNestedLoop (hyrise_amd/host/hyrise_host.hpp) over the reference's
JoinTestRunner input tables -- the output's rows in order against a nested loop in the reference's order, every mode x condition, two key
types, secondary predicates, reference inputs, host and device-resident results, and JoinSortMerge's multiset where it accepts the join."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_join_nested_loop_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "join_nested_loop_tests")
    assert os.path.exists(binary), "tests/cpp/join_nested_loop_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "JOIN NESTED LOOP TESTS PASSED" in proc.stdout
    for name in ("JoinNestedLoop refusals", "JoinNestedLoop reference inputs 15 x 15 (results in HBM)", "JoinNestedLoop data inputs 15 x 15 (host results)",
                 "JoinNestedLoop secondary predicates over reference inputs (host results)", "JoinNestedLoop chunks of 3 rows (results in HBM)"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert proc.stdout.count("[  OK  ] JoinNestedLoop data inputs") == 12 and proc.stdout.count("[  OK  ] JoinNestedLoop reference inputs") == 6
    assert proc.stdout.count("[  OK  ] JoinNestedLoop secondary predicates") == 8

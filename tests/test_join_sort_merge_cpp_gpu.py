"""Runs tests/cpp/join_sort_merge_tests.cpp: the C++ mirror's JoinSortMerge (hyrise_amd/host/hyrise_host.hpp) over the reference's
JoinTestRunner input tables -- row multisets against a nested loop, chunk boundaries, the sorted / clustered flags, supports()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_join_sort_merge_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "join_sort_merge_tests")
    assert os.path.exists(binary), "tests/cpp/join_sort_merge_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "JOIN SORT MERGE TESTS PASSED" in proc.stdout
    for name in ("JoinSortMerge::supports", "JoinSortMerge refusals", "JoinSortMerge reference inputs 15 x 15 (results in HBM)", "JoinSortMerge data inputs 15 x 15 (host results)"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert proc.stdout.count("[  OK  ] JoinSortMerge data inputs") == 12 and proc.stdout.count("[  OK  ] JoinSortMerge reference inputs") == 6

"""Runs tests/cpp/string_join_keys_tests.cpp: the C++ mirror's JoinHash and JoinSortMerge on string keys made on the device
(device_string_join_key_columns -> hy_column_string_join_keys) -- JoinHash's output table with the switch on against the switch off, cell for
cell and chunk for chunk (data tables, a TableScan's output, four modes, a secondary predicate), JoinSortMerge against a nested loop over the
strings, a ValueSegment<pmr_string> chunk with NULL keys on the host route, and TableScan (LIKE) -> JoinHash -> AggregateHash without a segment fetch,
also over a string column made in HBM.  Every run that should take the device route is counted.
Fixtures: tests/golden/tbl/tpch/sf-0.001/lineitem.tbl and the join_test_runner tables."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_string_join_keys(device):
    binary = os.path.join(ROOT, "tests", "cpp", "string_join_keys_tests")
    assert os.path.exists(binary), "tests/cpp/string_join_keys_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "STRING JOIN KEYS TESTS PASSED"
    for name in ("StringJoinKeys.JoinHashOnAndOffDataTables", "StringJoinKeys.JoinHashOnAndOffRunnerTables", "StringJoinKeys.JoinHashOverATableScansOutputAndASecondaryPredicate",
                 "StringJoinKeys.JoinSortMergeAgainstANestedLoop", "StringJoinKeys.AValueSegmentChunkKeepsTheHostRoute", "StringJoinKeysChain.ScanJoinAggregateWithoutAFetch", "StringJoinKeysChain.AStringColumnMadeInHBMJoinsWithoutAFetch"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert "FAILED" not in proc.stdout

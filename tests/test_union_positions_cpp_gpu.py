"""Runs the reference's UnionPositions tests (src/test/lib/operators/union_positions_test.cpp), re-stated in tests/cpp/union_positions_tests.cpp
against the C++ mirror's UnionPositions (hyrise_amd/host/hyrise_host.hpp), which unions on the device; plus UnionAll and a chain whose
PosLists stay in HBM.  Fixtures: tests/golden/tbl/union_positions (see the MANIFEST.json there)."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBL = os.path.join(ROOT, "tests", "golden", "tbl", "union_positions")
CASES = ["SelfUnionSimple", "SelfUnionExlusiveRanges", "SelfUnionOverlappingRanges", "EarlyResultLeft", "EarlyResultRight",
         "SelfUnionOverlappingRangesMultipleSegments", "MultipleReferencedTables", "MultipleShuffledPosList", "DifferentTables", "SameColumnsDifferentTables"]


def test_union_positions_fixtures_match_their_manifest():
    manifest = json.load(open(os.path.join(TBL, "MANIFEST.json")))
    assert sorted(manifest) == sorted(f for f in os.listdir(TBL) if f.endswith(".tbl"))
    for name, entry in manifest.items():
        data = open(os.path.join(TBL, name), "rb").read()
        assert len(data) < 200 and hashlib.sha256(data).hexdigest() == entry["sha256"], name


@pytest.mark.gpu
def test_cpp_union_positions_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "union_positions_tests")
    assert os.path.exists(binary), "tests/cpp/union_positions_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "UNION POSITIONS TESTS PASSED" in proc.stdout
    for name in CASES:
        assert f"[  OK  ] UnionPositionsTest.{name}" in proc.stdout, name
    assert "[  OK  ] UnionAllTest.UnionOfTwoScansSharesTheirChunks" in proc.stdout
    assert "[  OK  ] UnionPositionsChain.DeviceListsEqualHostLists" in proc.stdout

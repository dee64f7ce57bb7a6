"""Runs the reference's Sort tests (src/test/lib/operators/sort_test.cpp), re-stated in tests/cpp/sort_tests.cpp against the C++ mirror's
Sort (hyrise_amd/host/hyrise_host.hpp), which sorts on the device.  Fixtures: tests/golden/tbl/sort (see the MANIFEST.json there)."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_TBL = os.path.join(ROOT, "tests", "golden", "tbl", "sort")


def test_sort_fixtures_match_their_manifest():
    manifest = json.load(open(os.path.join(SORT_TBL, "MANIFEST.json")))
    assert sorted(manifest) == sorted(f for f in os.listdir(SORT_TBL) if f.endswith(".tbl"))
    for name, entry in manifest.items():
        assert hashlib.sha256(open(os.path.join(SORT_TBL, name), "rb").read()).hexdigest() == entry["sha256"], name


@pytest.mark.gpu
def test_cpp_sort_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "sort_tests")
    assert os.path.exists(binary), "tests/cpp/sort_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "SORT TESTS PASSED" in proc.stdout
    for name in ("SortTest.JoinProducesReferences", "SortTest.InputReferencesDifferentTables", "SortTest.InputReferencesDifferentColumns"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert proc.stdout.count("[  OK  ] SortTest.Sort Variations/") == 14

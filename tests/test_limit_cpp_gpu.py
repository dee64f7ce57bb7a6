"""Runs the reference's Limit tests (src/test/lib/operators/limit_test.cpp), re-stated in tests/cpp/limit_tests.cpp against the C++ mirror's
Limit (hyrise_amd/host/hyrise_host.hpp), and the mirror's own: Limit over device-resident PosLists, and Sort with a row limit (hy_sort_limit)
against Limit over Sort.  Fixtures: tests/golden/tbl/limit (see the MANIFEST.json there) and tests/golden/tbl/int_int3.tbl."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_TBL = os.path.join(ROOT, "tests", "golden", "tbl", "limit")


def test_limit_fixtures_match_their_manifest():
    manifest = json.load(open(os.path.join(LIMIT_TBL, "MANIFEST.json")))
    assert sorted(manifest) == sorted(f for f in os.listdir(LIMIT_TBL) if f.endswith(".tbl")) == ["int_int3_limit_1.tbl", "int_int3_limit_2.tbl", "int_int3_limit_4.tbl"]
    for name, entry in manifest.items():
        assert hashlib.sha256(open(os.path.join(LIMIT_TBL, name), "rb").read()).hexdigest() == entry["sha256"], name


@pytest.mark.gpu
def test_cpp_limit_operator(device):
    binary = os.path.join(ROOT, "tests", "cpp", "limit_tests")
    assert os.path.exists(binary), "tests/cpp/limit_tests missing: run __graft_entry__.build()"
    proc = subprocess.run([binary, os.path.join(ROOT, "tests", "golden", "tbl")], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    print(proc.stderr)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert proc.stdout.strip().splitlines()[-1] == "LIMIT TESTS PASSED"
    for row_count in (1, 2, 4, 10):
        for segments in ("ValueSegment", "ReferenceSegment"):
            assert f"[  OK  ] OperatorsLimitTest.Limit{row_count}{segments}" in proc.stdout
    for name in ("OperatorsLimitTest.ForwardSortedByFlag", "OperatorsLimitTest.Name"):
        assert f"[  OK  ] {name}" in proc.stdout, name
    assert proc.stdout.count("[  OK  ] Limit(Sort(x), k) == Sort(x, row_limit = k)") == 4
    assert "FAILED" not in proc.stdout

"""The pack / unpack arithmetic of pk_emit's 4-byte staged record and the LDS footprint of its compact flavour
(hyrise_amd/csrc/join_pk_stage.hpp), compiled for the host and checked exhaustively by tests/cpp/pk_stage_record_main.cpp: no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_record_round_trip_and_lds_footprint(tmp_path):
    binary = tmp_path / "pk_stage_record"
    source = os.path.join(ROOT, "tests", "cpp", "pk_stage_record_main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(binary), source])
    result = subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True)
    assert result.returncode == 0 and result.stdout.startswith("ok "), result.stdout

"""hy_join_nested_loop's part of the C ABI: the result struct's layout in ctypes and the two entry points, exported and bound."""
import ctypes as C
import os
import re
import subprocess

from hyrise_amd import abi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "hyrise_amd.h")


def test_result_struct_has_the_c_layout(tmp_path):
    fields = [(name, abi.NestedLoopResult.__dict__[name].offset, abi.NestedLoopResult.__dict__[name].size) for name, _ in abi.NestedLoopResult._fields_]
    assert fields == [("mem", 0, 4), ("reserved", 4, 4), ("left_pos", 8, 8), ("right_pos", 16, 8), ("capacity", 24, 8), ("n_pairs", 32, 8)]
    assert C.sizeof(abi.NestedLoopResult) == 40
    with open(HEADER) as fh:
        header = fh.read()
    body = re.search(r"typedef struct hy_nested_loop_result \{(.*?)\} hy_nested_loop_result;", header, re.S).group(1)
    declared = re.findall(r"^\s*(?:uint32_t|uint64_t|hy_row_id\*)\s+(\w+);", body, re.M)
    assert declared == [name for name, _ in abi.NestedLoopResult._fields_]
    source = tmp_path / "layout.c"   # ... and the C compiler agrees, as do the two limits the header names
    lines = [f'  printf("{name} %zu\\n", offsetof(hy_nested_loop_result, {name}));\n' for name, _ in abi.NestedLoopResult._fields_]
    lines += ['  printf("size %zu\\n", sizeof(hy_nested_loop_result));\n', '  printf("comparisons %llu\\n", (unsigned long long)HY_NLJ_MAX_COMPARISONS);\n',
              '  printf("temporaries %llu\\n", (unsigned long long)HY_NLJ_MAX_TEMPORARY_BYTES);\n']
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    said = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for name, offset, _ in fields:
        assert int(said[name]) == offset, name
    assert int(said["size"]) == 40
    assert int(said["comparisons"]) == abi.NLJ_MAX_COMPARISONS and int(said["temporaries"]) == abi.NLJ_MAX_TEMPORARY_BYTES


def test_entry_points_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    assert bound["hy_join_nested_loop"] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.JoinPredicate), C.c_uint32, C.POINTER(abi.NestedLoopResult)]
    assert bound["hy_join_nested_loop_count"] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.JoinPredicate), C.c_uint32, C.POINTER(C.c_uint64)]
    for name in ("hy_join_nested_loop", "hy_join_nested_loop_count"):
        assert getattr(lib, name).restype is C.c_int32
    assert lib.hy_abi_version() == 4   # (entry points were added; nothing that exists changed)


def test_null_arguments_are_refused_without_a_device():
    lib = abi.load_library()
    assert lib.hy_join_nested_loop(None, None, abi.JOIN_INNER, abi.PRED_LESS_THAN, None, 0, None) == abi.ERR_INVALID
    n = C.c_uint64(7)
    assert lib.hy_join_nested_loop_count(None, None, abi.JOIN_INNER, abi.PRED_LESS_THAN, None, 0, C.byref(n)) == abi.ERR_INVALID and n.value == 0
    assert lib.hy_last_error()

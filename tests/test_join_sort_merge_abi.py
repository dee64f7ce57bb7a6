"""hy_join_sort_merge's part of the C ABI: the result struct's layout in ctypes and the two entry points, exported and bound."""
import ctypes as C
import os
import re

from hyrise_amd import abi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hyrise_amd.h")


def test_result_struct_has_the_c_layout():
    fields = [(name, abi.SortMergeResult.__dict__[name].offset, abi.SortMergeResult.__dict__[name].size) for name, _ in abi.SortMergeResult._fields_]
    assert fields == [("mem", 0, 4), ("reserved", 4, 4), ("left_pos", 8, 8), ("right_pos", 16, 8), ("capacity", 24, 8), ("n_pairs", 32, 8), ("n_matched", 40, 8),
                      ("n_left_outer", 48, 8)]
    assert C.sizeof(abi.SortMergeResult) == 56
    with open(HEADER) as fh:
        header = fh.read()
    body = re.search(r"typedef struct hy_sort_merge_result \{(.*?)\} hy_sort_merge_result;", header, re.S).group(1)
    declared = re.findall(r"^\s*(?:uint32_t|uint64_t|hy_row_id\*)\s+(\w+);", body, re.M)
    assert declared == [name for name, _ in abi.SortMergeResult._fields_]


def test_entry_points_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    assert bound["hy_join_sort_merge"] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.SortMergeResult)]
    assert bound["hy_join_sort_merge_count"] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    for name in ("hy_join_sort_merge", "hy_join_sort_merge_count"):
        assert getattr(lib, name).restype is C.c_int32
    assert lib.hy_abi_version() == 4   # (entry points were added; nothing that exists changed)

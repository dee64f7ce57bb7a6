"""CPU-side checks of hy_sort_limit: declared in the header, bound and exported, the ABI version unchanged, the flag constants of the ctypes
mirror equal to the header's, and the argument errors that are decided before any column or device is touched."""
import ctypes as C
import os
import re

from hyrise_amd import abi, operators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    with open(os.path.join(ROOT, "include", "hyrise_amd.h")) as header:
        return header.read()


def test_sort_limit_is_declared_bound_and_exported():
    lib = abi.load_library()
    assert re.search(r"\bhy_status\s+hy_sort_limit\s*\(", header_text())
    assert "hy_sort_limit" in {name for name, _, _ in abi.SYMBOLS} and hasattr(lib, "hy_sort_limit")
    assert "limit" in operators.sort.__code__.co_varnames and "flags" in operators.sort.__code__.co_varnames


def test_the_abi_version_is_still_four():
    assert abi.load_library().hy_abi_version() == 4
    assert re.search(r"#define\s+HY_ABI_VERSION\s+4\b", header_text())


def test_flag_constants_equal_the_header():
    declared = dict((name, int(value)) for name, value in re.findall(r"\b(HY_SORT_LIMIT_[A-Z_]+)\s*=\s*(\d+)", header_text()))
    assert declared == {"HY_SORT_LIMIT_FORCE_FULL_SORT": abi.SORT_LIMIT_FORCE_FULL_SORT, "HY_SORT_LIMIT_FORCE_SELECT": abi.SORT_LIMIT_FORCE_SELECT}
    assert abi.SORT_LIMIT_FORCE_FULL_SORT == 1 and abi.SORT_LIMIT_FORCE_SELECT == 2


def test_the_header_cites_what_it_replaces():
    comment = header_text().split("hy_status hy_sort_limit")[0].rsplit("/*", 1)[1]
    assert "sort.cpp:287-516" in comment and "limit.cpp:47-127" in comment


def test_argument_errors_before_any_column_is_read():
    lib = abi.load_library()
    keys = (abi.SortKey * 1)()   # (a null column inside)
    n_out, path = C.c_uint64(77), C.c_uint32(77)
    assert lib.hy_sort_limit(None, 1, 10, 0, None, 0, C.byref(n_out), C.byref(path)) == abi.ERR_INVALID
    assert lib.hy_sort_limit(keys, 0, 10, 0, None, 0, C.byref(n_out), C.byref(path)) == abi.ERR_INVALID
    assert lib.hy_sort_limit(keys, 1, 10, 0, None, 0, None, C.byref(path)) == abi.ERR_INVALID
    for flags in (abi.SORT_LIMIT_FORCE_FULL_SORT | abi.SORT_LIMIT_FORCE_SELECT, 4, 1 << 31):
        n_out.value = path.value = 77
        assert lib.hy_sort_limit(keys, 1, 10, flags, None, 0, C.byref(n_out), C.byref(path)) == abi.ERR_INVALID
        assert n_out.value == 0 and path.value == 0 and "flags" in lib.hy_last_error().decode()
    assert lib.hy_sort_limit(keys, 1, 10, 0, None, 0, C.byref(n_out), None) == abi.ERR_INVALID   # the null column
    assert "hy_sort_limit" in lib.hy_last_error().decode()

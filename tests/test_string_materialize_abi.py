"""hy_string_column_materialize and HY_OPT_STRING_SPARSE_GATHER at the C boundary: the symbol declared, exported and bound with the header's
argument count, the option on both sides with its default, and the refusals that need no column -- all without a GPU: a null argument is
answered before anything touches the device.  The refusals that need a column (a column that is no string column, a dictionary that
disagrees, the column of zero chunks) are at the end, on the GPU, as tests/test_string_substr_abi.py has them for its entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hyrise_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "hyrise_amd.h")) as fh:
        return fh.read()


def materialize(lib, column, dictionary, give_result=True, give_dict=True):
    result, result_dict = C.c_void_p(1), C.c_void_p(1)
    status = lib.hy_string_column_materialize(column, dictionary, C.byref(result) if give_result else None, C.byref(result_dict) if give_dict else None)
    if status == abi.OK:
        assert result.value and result_dict.value
        chunks = C.c_uint32(77)
        abi.check(lib.hy_column_chunk_count(result, C.byref(chunks)))
        abi.check(lib.hy_column_destroy(result))
        abi.check(lib.hy_string_dictionary_destroy(result_dict))
        return status, chunks.value
    assert (not give_result or not result.value) and (not give_dict or not result_dict.value)
    return status, None


def test_symbol_is_declared_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    assert hasattr(lib, "hy_string_column_materialize") and len(bound["hy_string_column_materialize"]) == 4
    prototype = re.search(r"hy_status\s+hy_string_column_materialize\s*\(([^;]*)\)\s*;", header())
    assert prototype and len(prototype.group(1).split(",")) == 4
    assert "projection.cpp:201-215" in header()
    assert re.search(r"#define\s+HY_ABI_VERSION\s+4\b", header())


def test_option_19_exists_on_both_sides_with_the_library_deciding_by_default():
    lib = abi.load_library()
    assert re.search(r"HY_OPT_STRING_SPARSE_GATHER\s*=\s*19\b", header()) and re.search(r"HY_OPT_COUNT\s*=\s*20\b", header())
    assert abi.OPT_STRING_SPARSE_GATHER == 19
    value = C.c_int64(-1)
    abi.check(lib.hy_get_option(abi.OPT_STRING_SPARSE_GATHER, C.byref(value)))
    assert value.value == 1
    for setting in (0, 2):
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, setting):
            abi.check(lib.hy_get_option(abi.OPT_STRING_SPARSE_GATHER, C.byref(value)))
            assert value.value == setting
    abi.check(lib.hy_get_option(abi.OPT_STRING_SPARSE_GATHER, C.byref(value)))
    assert value.value == 1
    assert lib.hy_get_option(20, C.byref(value)) == abi.ERR_INVALID


def test_null_arguments_leave_both_outputs_null():
    """(The handles are never read: every call fails on a null argument first.)"""
    lib = abi.load_library()
    fake_column, fake_dictionary = C.c_void_p(1), C.c_void_p(1)
    for column, dictionary, give_result, give_dict in ((None, fake_dictionary, True, True), (fake_column, None, True, True), (None, None, True, True),
                                                       (None, fake_dictionary, False, True), (None, fake_dictionary, True, False)):
        status, _ = materialize(lib, column, dictionary, give_result, give_dict)
        assert status == abi.ERR_INVALID and b"hy_string_column_materialize: null argument" in lib.hy_last_error()


@pytest.mark.gpu
def test_refusals_with_a_column(device):
    """A column that is no string column, a dictionary with another chunk count or other entry counts: both outputs NULL after each, and
    nothing is launched for any of them."""
    from hyrise_amd import storage
    lib = abi.load_library()
    encoded = [storage.encode_string_dictionary(v) for v in ([b"a", b"b", b"a"], [b"c", b"c"])]
    column = storage.DeviceColumn(storage.HostColumn([segment for segment, _ in encoded], abi.TYPE_STRING))
    dictionaries = [dictionary for _, dictionary in encoded]
    good = storage.DeviceStringDictionary(dictionaries)
    for setting in (0, 2):
        with abi.option(abi.OPT_STRING_SPARSE_GATHER, setting):
            assert materialize(lib, column.handle, good.handle) == (abi.OK, 2)
    abi.check(lib.hy_set_profiling(1))
    try:
        assert materialize(lib, column.handle, storage.DeviceStringDictionary(dictionaries[:1]).handle)[0] == abi.ERR_INVALID
        assert materialize(lib, column.handle, storage.DeviceStringDictionary([dictionaries[0], dictionaries[1] + [b"z"]]).handle)[0] == abi.ERR_INVALID
        ints = storage.DeviceColumn(storage.make_column(np.arange(6, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
        assert materialize(lib, ints.handle, storage.DeviceStringDictionary([[b"a", b"b", b"c"]] * 2).handle)[0] == abi.ERR_INVALID
        assert b"string column" in lib.hy_last_error()
        empty = storage.DeviceColumn(storage.HostColumn([], abi.TYPE_STRING))
        assert materialize(lib, empty.handle, storage.DeviceStringDictionary([]).handle) == (abi.OK, 0)
        milliseconds, launches = C.c_float(0), C.c_uint32(77)
        abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(milliseconds), C.byref(launches)))
        assert launches.value == 0
    finally:
        abi.check(lib.hy_set_profiling(0))

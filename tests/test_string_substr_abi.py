"""hy_string_column_substr at the C boundary: the symbol exported and bound with the header's argument count, and every refusal -- before
any launch, with both out pointers NULL.  hy_projection_expression still refuses HY_PROJ_FUNCTION: this call is the route.
A dictionary on another device is refused by the check that hy_column_string_ranks shares (tests/cpp/multi_gpu_tests.cpp has the devices).
(A column of 2^32 rows needs 4 GiB of attribute vectors before the call could refuse it: that refusal is one comparison in front of the
first allocation and is not run here; the one for an output chunk of 2^32 bytes of chars is the gather's own, behind the same sums.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hyrise_amd import abi, storage
from test_like_device_abi import CallerOwnedDictionary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def substr(lib, column, dictionary, start, length, give_result=True, give_dict=True):
    result, result_dict = C.c_void_p(1), C.c_void_p(1)
    status = lib.hy_string_column_substr(column, dictionary, start, length, C.byref(result) if give_result else None, C.byref(result_dict) if give_dict else None)
    if status == abi.OK:
        assert result.value and result_dict.value
        chunks = C.c_uint32(77)
        abi.check(lib.hy_column_chunk_count(result, C.byref(chunks)))
        abi.check(lib.hy_column_destroy(result))
        abi.check(lib.hy_string_dictionary_destroy(result_dict))
        return status, chunks.value
    assert (not give_result or not result.value) and (not give_dict or not result_dict.value)
    return status, None


def test_symbol_is_exported_and_bound(device):
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    assert hasattr(lib, "hy_string_column_substr") and len(bound["hy_string_column_substr"]) == 6
    with open(os.path.join(ROOT, "include", "hyrise_amd.h")) as fh:
        prototype = re.search(r"hy_status\s+hy_string_column_substr\s*\(([^;]*)\)\s*;", fh.read())
    assert prototype and len(prototype.group(1).split(",")) == 6


def test_null_arguments_leave_both_outputs_null(device):
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([3, 0, 65])
    fake_column = C.c_void_p(1)   # (never read: every call below fails on another argument first)
    for column, dict_handle, give_result, give_dict in ((None, dictionary.handle, True, True), (fake_column, None, True, True), (None, None, True, True),
                                                        (None, dictionary.handle, False, True), (None, dictionary.handle, True, False)):
        status, _ = substr(lib, column, dict_handle, 1, 4, give_result, give_dict)
        assert status == abi.ERR_INVALID and b"null argument" in lib.hy_last_error()


def test_refusals_with_a_column(device):
    """A column that is no string column, a dictionary with another chunk count or other entry counts: both outputs NULL after each.
    (Unencoded and LZ4 string segments never become an hy_column -- hy_column_create refuses them.)"""
    lib = abi.load_library()
    encoded = [storage.encode_string_dictionary(v) for v in ([b"a", b"b", b"a"], [b"c", b"c"])]
    column = storage.DeviceColumn(storage.HostColumn([segment for segment, _ in encoded], abi.TYPE_STRING))
    dictionaries = [dictionary for _, dictionary in encoded]
    good = storage.DeviceStringDictionary(dictionaries)
    assert substr(lib, column.handle, good.handle, 1, 4) == (abi.OK, 2)
    assert substr(lib, column.handle, good.handle, 2**31 - 1, 2**31 - 1) == (abi.OK, 2)
    assert substr(lib, column.handle, good.handle, -2**31, -2**31) == (abi.OK, 2)
    assert substr(lib, column.handle, storage.DeviceStringDictionary(dictionaries[:1]).handle, 1, 4)[0] == abi.ERR_INVALID
    assert substr(lib, column.handle, storage.DeviceStringDictionary([dictionaries[0], dictionaries[1] + [b"z"]]).handle, 1, 4)[0] == abi.ERR_INVALID
    ints = storage.DeviceColumn(storage.make_column(np.arange(6, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    assert substr(lib, ints.handle, storage.DeviceStringDictionary([[b"a", b"b", b"c"]] * 2).handle, 1, 4)[0] == abi.ERR_INVALID
    assert b"string column" in lib.hy_last_error()


def test_a_column_of_zero_chunks_is_answered_without_a_launch(device):
    lib = abi.load_library()
    column = storage.DeviceColumn(storage.HostColumn([], abi.TYPE_STRING))
    dictionary = storage.DeviceStringDictionary([])
    abi.check(lib.hy_set_profiling(1))
    try:
        assert substr(lib, column.handle, dictionary.handle, 1, 4) == (abi.OK, 0)
        milliseconds, launches = C.c_float(0), C.c_uint32(77)
        abi.check(lib.hy_profile_read_kernel(abi.KERNEL_STRING_RANK, C.byref(milliseconds), C.byref(launches)))
        assert launches.value == 0
    finally:
        abi.check(lib.hy_set_profiling(0))


def test_two_to_the_thirty_one_entries_are_unsupported(device):
    """Two chunks whose dictionaries have 2^30 entries each: refused before anything is allocated or read (the buffers are 16 bytes)."""
    lib = abi.load_library()
    segments = [storage.HostSegment(abi.ENC_DICTIONARY, abi.TYPE_STRING, 2, 4, np.zeros(2, dtype=np.uint32), aux=None, aux_size=1 << 30) for _ in range(2)]
    column = storage.DeviceColumn(storage.HostColumn(segments, abi.TYPE_STRING))
    keep = np.zeros(16, dtype=np.uint8)
    chunks = (abi.StringDictionaryChunk * 2)()
    for c in range(2):
        chunks[c].n_entries, chunks[c].string_length, chunks[c].chars, chunks[c].offsets = 1 << 30, 1, keep.ctypes.data, None
    handle = C.c_void_p()
    assert lib.hy_string_dictionary_create(chunks, 2, abi.MEM_DEVICE, C.byref(handle)) == abi.OK
    assert substr(lib, column.handle, handle, 1, 4)[0] == abi.ERR_UNSUPPORTED and b"int32 ranks" in lib.hy_last_error()
    lib.hy_string_dictionary_destroy(handle)


def test_function_expressions_are_still_refused_by_the_expression_programs(device):
    from hyrise_amd.operators import projection_program
    lib = abi.load_library()
    out = C.c_void_p(0xDEAD)
    program = projection_program(("function", (abi.TYPE_INT, 1)))[0]
    assert lib.hy_projection_expression(C.byref(program), C.byref(out)) == abi.ERR_UNSUPPORTED and out.value is None

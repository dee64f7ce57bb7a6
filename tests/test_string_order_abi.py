"""hy_string_dictionary_order and hy_column_string_ranks at the C boundary: symbols exported and bound with the header's argument counts, the
ABI version and the kernel kinds unchanged, and every argument check that returns before any launch.  Dictionaries over caller-owned device
buffers are created by pure host work, so these run without a device -- all but the checks of a dictionary against a column's segments,
which need a column and therefore a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hyrise_amd import abi, storage
from test_like_device_abi import CallerOwnedDictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"hy_string_dictionary_order": 4, "hy_column_string_ranks": 3}
UNTOUCHED = 0x5A5A5A5A


def header_text():
    with open(os.path.join(ROOT, "include", "hyrise_amd.h")) as fh:
        return fh.read()


def test_symbols_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    header = header_text()
    for name, n_arguments in NEW_SYMBOLS.items():
        assert hasattr(lib, name), f"{name} not exported"
        assert name in bound and len(bound[name]) == n_arguments
        prototype = re.search(r"hy_status\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert prototype and len(prototype.group(1).split(",")) == n_arguments


def test_abi_version_and_kernel_kinds_are_unchanged():
    lib = abi.load_library()
    header = header_text()
    assert lib.hy_abi_version() == 4 and re.search(r"#define\s+HY_ABI_VERSION\s+4\b", header)
    assert re.search(r"HY_KERNEL_STRING_RANK\s*=\s*8\b", header) and re.search(r"HY_KERNEL_KINDS\s*=\s*9\b", header)
    assert abi.KERNEL_STRING_RANK == 8


def test_order_refusals_come_before_any_launch():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([3, 0, 65])
    ranks = np.full(80, UNTOUCHED, dtype=np.int32)
    n_distinct = C.c_uint32(77)
    assert lib.hy_string_dictionary_order(None, abi.MEM_HOST, ranks.ctypes.data, C.byref(n_distinct)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_order(dictionary.handle, abi.MEM_HOST, None, C.byref(n_distinct)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_order(dictionary.handle, abi.MEM_DEVICE, None, None) == abi.ERR_INVALID
    for mem in (2, 5, 0xFFFFFFFF):
        assert lib.hy_string_dictionary_order(dictionary.handle, mem, ranks.ctypes.data, C.byref(n_distinct)) == abi.ERR_INVALID
        assert b"memory space" in lib.hy_last_error()
    for off in (1, 2, 3):
        assert lib.hy_string_dictionary_order(dictionary.handle, abi.MEM_DEVICE, ranks.ctypes.data + off, None) == abi.ERR_INVALID
        assert b"4-byte" in lib.hy_last_error()
    assert (ranks == UNTOUCHED).all() and n_distinct.value == 77


def test_a_dictionary_without_entries_is_ordered_without_a_launch():
    lib = abi.load_library()
    ranks = np.full(4, UNTOUCHED, dtype=np.int32)
    for counts in ([], [0], [0, 0, 0]):
        dictionary = CallerOwnedDictionary(counts)
        for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
            n_distinct = C.c_uint32(77)
            assert lib.hy_string_dictionary_order(dictionary.handle, mem, ranks.ctypes.data, C.byref(n_distinct)) == abi.OK
            assert n_distinct.value == 0
            assert lib.hy_string_dictionary_order(dictionary.handle, mem, ranks.ctypes.data, None) == abi.OK
    assert (ranks == UNTOUCHED).all()


def test_two_to_the_thirty_one_entries_are_unsupported():
    """Ranks are int32.  Two chunks of 2^30 one-byte slots each: 2 GiB of chars that nothing reads before a launch."""
    lib = abi.load_library()
    keep = np.zeros(16, dtype=np.uint8)
    chunks = (abi.StringDictionaryChunk * 2)()
    for c in range(2):
        chunks[c].n_entries, chunks[c].string_length, chunks[c].chars, chunks[c].offsets = 1 << 30, 1, keep.ctypes.data, None
    handle = C.c_void_p()
    assert lib.hy_string_dictionary_create(chunks, 2, abi.MEM_DEVICE, C.byref(handle)) == abi.OK
    ranks = np.full(8, UNTOUCHED, dtype=np.int32)
    n_distinct = C.c_uint32(77)
    for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        assert lib.hy_string_dictionary_order(handle, mem, ranks.ctypes.data, C.byref(n_distinct)) == abi.ERR_UNSUPPORTED
        assert b"int32 ranks" in lib.hy_last_error()
    assert (ranks == UNTOUCHED).all() and n_distinct.value == 77
    lib.hy_string_dictionary_destroy(handle)


def test_column_string_ranks_null_arguments():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([1])
    out = C.c_void_p(1)
    assert lib.hy_column_string_ranks(None, dictionary.handle, C.byref(out)) == abi.ERR_INVALID and not out.value
    out = C.c_void_p(1)
    assert lib.hy_column_string_ranks(None, None, C.byref(out)) == abi.ERR_INVALID and not out.value
    assert lib.hy_column_string_ranks(None, dictionary.handle, None) == abi.ERR_INVALID


@pytest.mark.gpu
def test_a_column_or_dictionary_that_does_not_fit_is_refused(device):
    """A non-string column; a dictionary whose chunk count or any n_entries differs from the data column's dictionary segments (aux_size),
    for a data column and behind a reference column.  *out is NULL after each.  (Needs a column, and a column needs a device.)"""
    lib = abi.load_library()
    values = [[b"a", b"b", b"a"], [b"c", b"c"], [b"d", b"e", b"f", b"g"]]
    encoded = [storage.encode_string_dictionary(v) for v in values]
    host = storage.HostColumn([segment for segment, _ in encoded], abi.TYPE_STRING)
    column = storage.DeviceColumn(host)
    dictionaries = [dictionary for _, dictionary in encoded]
    reference = storage.DeviceColumn(storage.make_reference_column(host, [np.array([[c, 0]], dtype=np.uint32) for c in range(3)], [0, 1, 2]), refs={id(host): column})

    def ranks(dev_column, dev_dict):
        out = C.c_void_p(1)
        status = lib.hy_column_string_ranks(dev_column.handle, dev_dict.handle, C.byref(out))
        if status == abi.OK:
            assert out.value
            abi.check(lib.hy_column_destroy(out))
        else:
            assert not out.value
        return status

    good = storage.DeviceStringDictionary(dictionaries)
    for dev_column in (column, reference):
        assert ranks(dev_column, good) == abi.OK
        assert ranks(dev_column, storage.DeviceStringDictionary(dictionaries[:2])) == abi.ERR_INVALID
        assert ranks(dev_column, storage.DeviceStringDictionary(dictionaries + [[b"x"]])) == abi.ERR_INVALID
        assert ranks(dev_column, storage.DeviceStringDictionary([dictionaries[0], dictionaries[1] + [b"z"], dictionaries[2]])) == abi.ERR_INVALID
        assert ranks(dev_column, storage.DeviceStringDictionary([dictionaries[0], dictionaries[1], dictionaries[2][:3]])) == abi.ERR_INVALID
    ints = storage.DeviceColumn(storage.make_column(np.arange(9, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    assert ranks(ints, storage.DeviceStringDictionary([[b"a", b"b", b"c"]] * 3)) == abi.ERR_INVALID
    assert b"string column" in lib.hy_last_error()
    out = C.c_void_p(1)
    assert lib.hy_column_string_ranks(column.handle, None, C.byref(out)) == abi.ERR_INVALID and not out.value

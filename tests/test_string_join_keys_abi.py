"""hy_string_dictionary_order_pair, hy_string_dictionary_join_ids and hy_column_string_join_keys at the C boundary: symbols exported and bound
with the header's argument counts, the ABI version, the kernel kinds and the option count unchanged, and every argument check that returns
before any launch.  Dictionaries over caller-owned device buffers are created by pure host work, so these run without a device."""
import ctypes as C
import os
import re

import numpy as np

from hyrise_amd import abi
from test_like_device_abi import CallerOwnedDictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"hy_string_dictionary_order_pair": 6, "hy_string_dictionary_join_ids": 5, "hy_column_string_join_keys": 7}
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
    assert re.search(r"HY_STRING_KEYS_RANKS\s*=\s*0\b", header) and re.search(r"HY_STRING_KEYS_HASH_IDS\s*=\s*1\b", header)
    assert (abi.STRING_KEYS_RANKS, abi.STRING_KEYS_HASH_IDS) == (0, 1)


def test_abi_version_kernel_kinds_and_options_are_unchanged():
    lib = abi.load_library()
    header = header_text()
    assert lib.hy_abi_version() == 4 and re.search(r"#define\s+HY_ABI_VERSION\s+4\b", header)
    assert re.search(r"HY_KERNEL_STRING_RANK\s*=\s*8\b", header) and re.search(r"HY_KERNEL_KINDS\s*=\s*9\b", header)
    assert re.search(r"HY_OPT_COUNT\s*=\s*20\b", header)
    assert abi.KERNEL_STRING_RANK == 8 and abi.OPT_STRING_SPARSE_GATHER == 19


def calls(lib):
    """(name, width, call(left, right, mem, left_out, right_out, n_distinct)) for the two dictionary-level entry points"""
    def ids(left, right, mem, left_out, right_out, n_distinct):
        return lib.hy_string_dictionary_join_ids(left, right, mem, left_out, right_out)
    return [("ranks", 4, lib.hy_string_dictionary_order_pair), ("ids", 8, ids)]


def test_refusals_come_before_any_launch():
    lib = abi.load_library()
    left, right = CallerOwnedDictionary([3, 0, 65]), CallerOwnedDictionary([2, 9])   # (different chunk counts: legal)
    for name, width, call in calls(lib):
        dtype = np.int32 if width == 4 else np.int64
        a, b = np.full(80, UNTOUCHED, dtype=dtype), np.full(80, UNTOUCHED, dtype=dtype)
        n_distinct = C.c_uint32(77)
        n = C.byref(n_distinct)
        assert call(None, right.handle, abi.MEM_HOST, a.ctypes.data, b.ctypes.data, n) == abi.ERR_INVALID
        assert call(left.handle, None, abi.MEM_HOST, a.ctypes.data, b.ctypes.data, n) == abi.ERR_INVALID
        assert call(left.handle, right.handle, abi.MEM_HOST, None, b.ctypes.data, n) == abi.ERR_INVALID
        assert call(left.handle, right.handle, abi.MEM_DEVICE, a.ctypes.data, None, None) == abi.ERR_INVALID
        for mem in (2, 5, 0xFFFFFFFF):
            assert call(left.handle, right.handle, mem, a.ctypes.data, b.ctypes.data, n) == abi.ERR_INVALID
            assert b"memory space" in lib.hy_last_error()
        for off in range(1, width):
            assert call(left.handle, right.handle, abi.MEM_DEVICE, a.ctypes.data + off, b.ctypes.data, None) == abi.ERR_INVALID
            assert (b"%d-byte" % width) in lib.hy_last_error()
            assert call(left.handle, right.handle, abi.MEM_DEVICE, a.ctypes.data, b.ctypes.data + off, None) == abi.ERR_INVALID
            assert call(left.handle, left.handle, abi.MEM_DEVICE, a.ctypes.data, b.ctypes.data + off, None) == abi.ERR_INVALID   # (a self join is checked alike)
        assert (a == UNTOUCHED).all() and (b == UNTOUCHED).all() and n_distinct.value == 77, name


def test_two_sides_without_entries_launch_nothing():
    lib = abi.load_library()
    for name, width, call in calls(lib):
        a, b = np.full(4, UNTOUCHED, dtype=np.int64), np.full(4, UNTOUCHED, dtype=np.int64)
        for left_counts, right_counts in (([], []), ([0], []), ([0, 0, 0], [0, 0])):
            left, right = CallerOwnedDictionary(left_counts), CallerOwnedDictionary(right_counts)
            for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
                n_distinct = C.c_uint32(77)
                assert call(left.handle, right.handle, mem, a.ctypes.data, b.ctypes.data, C.byref(n_distinct)) == abi.OK
                assert n_distinct.value == (0 if name == "ranks" else 77)
                assert call(left.handle, right.handle, mem, a.ctypes.data, b.ctypes.data, None) == abi.OK
        assert (a == UNTOUCHED).all() and (b == UNTOUCHED).all()


def test_a_joint_total_of_two_to_the_thirty_one_entries_is_unsupported():
    """Ranks are int32 over both sides together.  Each side: one chunk of 2^30 one-byte slots, legal alone, that nothing reads before a launch."""
    lib = abi.load_library()
    keep = np.zeros(16, dtype=np.uint8)
    handles = []
    for _ in range(2):
        chunks = (abi.StringDictionaryChunk * 1)()
        chunks[0].n_entries, chunks[0].string_length, chunks[0].chars, chunks[0].offsets = 1 << 30, 1, keep.ctypes.data, None
        handle = C.c_void_p()
        assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.OK
        handles.append(handle)
    for name, width, call in calls(lib):
        a, b = np.full(8, UNTOUCHED, dtype=np.int64), np.full(8, UNTOUCHED, dtype=np.int64)
        n_distinct = C.c_uint32(77)
        for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
            for left, right in ((handles[0], handles[1]), (handles[0], handles[0])):
                assert call(left, right, mem, a.ctypes.data, b.ctypes.data, C.byref(n_distinct)) == abi.ERR_UNSUPPORTED
                assert b"int32 ranks" in lib.hy_last_error()
        assert (a == UNTOUCHED).all() and (b == UNTOUCHED).all() and n_distinct.value == 77
    for handle in handles:
        lib.hy_string_dictionary_destroy(handle)


def test_column_string_join_keys_null_arguments_and_kind():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([1])
    d = dictionary.handle
    for kind in (abi.STRING_KEYS_RANKS, abi.STRING_KEYS_HASH_IDS, 2, 0xFFFFFFFF):
        for arguments in ((None, d, None, d), (None, None, None, None), (None, d, None, None)):
            left, right = C.c_void_p(1), C.c_void_p(1)
            assert lib.hy_column_string_join_keys(*arguments, kind, C.byref(left), C.byref(right)) == abi.ERR_INVALID
            assert not left.value and not right.value
        left = C.c_void_p(1)
        assert lib.hy_column_string_join_keys(None, d, None, d, kind, C.byref(left), None) == abi.ERR_INVALID and not left.value
        right = C.c_void_p(1)
        assert lib.hy_column_string_join_keys(None, d, None, d, kind, None, C.byref(right)) == abi.ERR_INVALID and not right.value

"""hy_string_column_gather, hy_string_ranks_gather and the two dictionary read-back calls at the C boundary: symbols exported and bound with
the header's argument counts, the ABI version and the kernel kinds unchanged, and every refusal that needs no column -- it returns before
any launch, with both out pointers NULL.  The read-back of a host-created dictionary and the refusal of fixed-slot chunks need a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hyrise_amd import abi, storage
from test_like_device_abi import CallerOwnedDictionary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"hy_string_column_gather": 7, "hy_string_ranks_gather": 4, "hy_string_dictionary_chunk_size": 4, "hy_string_dictionary_read_chunk": 4}
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


def test_gather_null_arguments_leave_both_outputs_null():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([3, 0, 65])
    positions = np.full(8, UNTOUCHED, dtype=np.uint32)
    fake_column = C.c_void_p(1)   # (never read: every call below fails on another argument first)
    for column, dict_handle, give_result, give_dict in ((None, dictionary.handle, True, True), (fake_column, None, True, True), (None, None, True, True),
                                                        (None, dictionary.handle, False, True), (None, dictionary.handle, True, False)):
        result, result_dict = C.c_void_p(1), C.c_void_p(1)
        status = lib.hy_string_column_gather(column, dict_handle, positions.ctypes.data, 4, 2, C.byref(result) if give_result else None, C.byref(result_dict) if give_dict else None)
        assert status == abi.ERR_INVALID and b"null argument" in lib.hy_last_error()
        assert (not give_result or not result.value) and (not give_dict or not result_dict.value)
    for dict_handle, ranks, give_result, give_dict in ((None, fake_column, True, True), (dictionary.handle, None, True, True), (dictionary.handle, None, False, True),
                                                       (dictionary.handle, None, True, False)):
        result, result_dict = C.c_void_p(1), C.c_void_p(1)
        status = lib.hy_string_ranks_gather(dict_handle, ranks, C.byref(result) if give_result else None, C.byref(result_dict) if give_dict else None)
        assert status == abi.ERR_INVALID and b"null argument" in lib.hy_last_error()
        assert (not give_result or not result.value) and (not give_dict or not result_dict.value)
    assert (positions == UNTOUCHED).all()


def test_read_back_refusals_touch_nothing():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([3, 0])
    n_entries, chars_bytes = C.c_uint32(77), C.c_uint64(77)
    offsets = np.full(8, UNTOUCHED, dtype=np.uint32)
    chars = np.full(8, 0x5A, dtype=np.uint8)
    assert lib.hy_string_dictionary_chunk_size(None, 0, C.byref(n_entries), C.byref(chars_bytes)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_chunk_size(dictionary.handle, 0, None, C.byref(chars_bytes)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_chunk_size(dictionary.handle, 0, C.byref(n_entries), None) == abi.ERR_INVALID
    for chunk in (2, 3, 0xFFFFFFFF):
        assert lib.hy_string_dictionary_chunk_size(dictionary.handle, chunk, C.byref(n_entries), C.byref(chars_bytes)) == abi.ERR_INVALID
        assert lib.hy_string_dictionary_read_chunk(dictionary.handle, chunk, chars.ctypes.data, offsets.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_read_chunk(None, 0, chars.ctypes.data, offsets.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_read_chunk(dictionary.handle, 0, chars.ctypes.data, None) == abi.ERR_INVALID
    assert n_entries.value == 77 and chars_bytes.value == 77 and (offsets == UNTOUCHED).all() and (chars == 0x5A).all()
    # a chunk without entries is answered by the host alone
    assert lib.hy_string_dictionary_chunk_size(dictionary.handle, 1, C.byref(n_entries), C.byref(chars_bytes)) == abi.OK
    assert n_entries.value == 0 and chars_bytes.value == 0
    assert lib.hy_string_dictionary_read_chunk(dictionary.handle, 1, None, offsets.ctypes.data) == abi.OK
    assert offsets[0] == 0 and (offsets[1:] == UNTOUCHED).all()


@pytest.mark.gpu
def test_read_back_returns_the_original_bytes(device):
    lib = abi.load_library()
    dictionaries = [[b"", b"a\x00b", b"ab", b"\x80\xff"], [], [b"x" * 1000, b"y"]]
    dev_dict = storage.DeviceStringDictionary(dictionaries)
    for c, dictionary in enumerate(dictionaries):
        entries, chars, offsets = dev_dict.read_chunk(c)
        want_chars, want_offsets = storage.pack_string_dictionary(dictionary)
        assert entries == dictionary and chars.tobytes() == want_chars.tobytes() and offsets.tobytes() == want_offsets.tobytes()
    # around the caller's arrays nothing is written
    chars = np.full(16 + 7 + 16, 0x5A, dtype=np.uint8)
    offsets = np.full(4 + 5 + 4, UNTOUCHED, dtype=np.uint32)
    abi.check(lib.hy_string_dictionary_read_chunk(dev_dict.handle, 0, chars[16:].ctypes.data, offsets[4:].ctypes.data))
    assert chars[16:23].tobytes() == b"a\x00bab\x80\xff" and (chars[:16] == 0x5A).all() and (chars[23:] == 0x5A).all()
    assert offsets[4:9].tolist() == [0, 0, 3, 5, 7] and (offsets[:4] == UNTOUCHED).all() and (offsets[9:] == UNTOUCHED).all()


@pytest.mark.gpu
def test_fixed_slot_chunks_are_refused_by_both_read_back_calls(device):
    lib = abi.load_library()
    dev_dict = storage.DeviceStringDictionary([[b"a", b"bc"], []], fixed_length=4)
    n_entries, chars_bytes = C.c_uint32(77), C.c_uint64(77)
    offsets = np.full(4, UNTOUCHED, dtype=np.uint32)
    chars = np.full(16, 0x5A, dtype=np.uint8)
    assert lib.hy_string_dictionary_chunk_size(dev_dict.handle, 0, C.byref(n_entries), C.byref(chars_bytes)) == abi.ERR_UNSUPPORTED
    assert b"fixed-slot" in lib.hy_last_error()
    assert lib.hy_string_dictionary_read_chunk(dev_dict.handle, 0, chars.ctypes.data, offsets.ctypes.data) == abi.ERR_UNSUPPORTED
    assert n_entries.value == 77 and chars_bytes.value == 77 and (offsets == UNTOUCHED).all() and (chars == 0x5A).all()


@pytest.mark.gpu
def test_gather_refusals_with_a_column_come_before_any_allocation(device):
    """chunk_rows == 0, positions off an 8-byte boundary, a column that is no string column (an int dictionary column), a dictionary that
    does not fit, n >= 2^32: both outputs NULL after each.  (Unencoded and LZ4 string segments never become an hy_column -- hy_column_create
    refuses them -- so the call's own refusal of them cannot be reached through the ABI.)"""
    import torch
    lib = abi.load_library()
    encoded = [storage.encode_string_dictionary(v) for v in ([b"a", b"b", b"a"], [b"c", b"c"])]
    column = storage.DeviceColumn(storage.HostColumn([segment for segment, _ in encoded], abi.TYPE_STRING))
    dictionaries = [dictionary for _, dictionary in encoded]
    good = storage.DeviceStringDictionary(dictionaries)
    positions = torch.zeros(64, dtype=torch.uint8, device="cuda")
    pointer = positions.data_ptr()
    assert pointer % 8 == 0

    def gather(dev_column, dev_dict, at, n, chunk_rows):
        result, result_dict = C.c_void_p(1), C.c_void_p(1)
        status = lib.hy_string_column_gather(dev_column.handle, dev_dict.handle, at, n, chunk_rows, C.byref(result), C.byref(result_dict))
        if status == abi.OK:
            assert result.value and result_dict.value
            abi.check(lib.hy_column_destroy(result))
            abi.check(lib.hy_string_dictionary_destroy(result_dict))
        else:
            assert not result.value and not result_dict.value
        return status

    assert gather(column, good, pointer, 4, 2) == abi.OK
    assert gather(column, good, pointer, 4, 0) == abi.ERR_INVALID
    assert gather(column, good, None, 4, 2) == abi.ERR_INVALID
    for off in (1, 2, 4, 7):
        assert gather(column, good, pointer + off, 4, 2) == abi.ERR_INVALID and b"8-byte" in lib.hy_last_error()
    assert gather(column, storage.DeviceStringDictionary(dictionaries[:1]), pointer, 4, 2) == abi.ERR_INVALID
    assert gather(column, storage.DeviceStringDictionary([dictionaries[0], dictionaries[1] + [b"z"]]), pointer, 4, 2) == abi.ERR_INVALID
    ints = storage.DeviceColumn(storage.make_column(np.arange(6, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    assert gather(ints, storage.DeviceStringDictionary([[b"a", b"b", b"c"]] * 2), pointer, 4, 2) == abi.ERR_INVALID
    assert b"string column" in lib.hy_last_error()
    assert gather(column, good, None, 0, 2) == abi.OK   # no rows: zero chunks, nothing launched
    assert gather(column, good, pointer, 1 << 32, 65_535) == abi.ERR_UNSUPPORTED and b"32-bit" in lib.hy_last_error()
    # hy_column_read_chunk gives value ids for string dictionary segments only: a numeric dictionary column is refused as before
    got = np.full(4, UNTOUCHED, dtype=np.uint32)
    assert lib.hy_column_read_chunk(ints.handle, 0, got.ctypes.data, None) == abi.ERR_UNSUPPORTED and (got == UNTOUCHED).all()
    ids = np.full(8, 0x5A, dtype=np.uint8)   # (this column's value ids are one byte wide)
    abi.check(lib.hy_column_read_chunk(column.handle, 0, ids.ctypes.data, None))
    assert ids[:3].tolist() == [0, 1, 0] and (ids[3:] == 0x5A).all()


@pytest.mark.gpu
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
    import torch
    positions = torch.zeros(64, dtype=torch.uint8, device="cuda")
    result, result_dict = C.c_void_p(1), C.c_void_p(1)
    assert lib.hy_string_column_gather(column.handle, handle, positions.data_ptr(), 4, 2, C.byref(result), C.byref(result_dict)) == abi.ERR_UNSUPPORTED
    assert b"int32 ranks" in lib.hy_last_error() and not result.value and not result_dict.value
    lib.hy_string_dictionary_destroy(handle)

"""The device LIKE entry points at the C boundary: symbols exported and bound, hy_string_dictionary_chunk laid out as abi.py says, the
pattern tokeniser and the dictionary packing (host-only pieces), hy_string_dictionary_match_layout, and every argument check that returns
before any launch.  A dictionary over caller-owned device buffers is created by pure host work, so these run without a device -- all but
the check of a dictionary against a column's segments, which needs a column and therefore a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.like import dictionary_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIKE_CONDITIONS = (abi.PRED_LIKE, abi.PRED_NOT_LIKE, abi.PRED_LIKE_INSENSITIVE, abi.PRED_NOT_LIKE_INSENSITIVE)
NEW_SYMBOLS = {"hy_string_dictionary_create": 4, "hy_string_dictionary_destroy": 1, "hy_string_dictionary_match_layout": 2, "hy_like_tokenize": 5, "hy_like_matches": 6,
               "hy_table_scan_like": 9}


class CallerOwnedDictionary:
    """An hy_string_dictionary over HY_MEM_DEVICE descriptors whose buffers nothing reads before a launch: `entry_counts` entries of one
    byte each per chunk.  (The pointers name host arrays here; no test of this file launches anything over them.)"""

    def __init__(self, entry_counts):
        self.lib = abi.load_library()
        self.keep = []
        chunks = (abi.StringDictionaryChunk * max(1, len(entry_counts)))()
        for c, n in enumerate(entry_counts):
            chars, offsets = storage.pack_string_dictionary([b"x"] * n)
            self.keep += [chars, offsets]
            chunks[c].n_entries, chunks[c].string_length = n, 0
            chunks[c].chars, chunks[c].offsets = (chars.ctypes.data if n else None), offsets.ctypes.data
        self.handle = C.c_void_p()
        assert self.lib.hy_string_dictionary_create(chunks, len(entry_counts), abi.MEM_DEVICE, C.byref(self.handle)) == abi.OK
        self.n_chunks = len(entry_counts)

    def layout(self):
        out = np.full(self.n_chunks + 1, 0xDEAD, dtype=np.uint64)
        assert self.lib.hy_string_dictionary_match_layout(self.handle, out.ctypes.data) == abi.OK
        return out.tolist()

    def __del__(self):
        if self.handle:
            self.lib.hy_string_dictionary_destroy(self.handle)


def test_symbols_are_exported_and_bound():
    lib = abi.load_library()
    bound = {name: argtypes for name, _, argtypes in abi.SYMBOLS}
    for name, n_arguments in NEW_SYMBOLS.items():
        assert hasattr(lib, name), f"{name} not exported"
        assert name in bound and len(bound[name]) == n_arguments
    assert lib.hy_abi_version() == 4
    assert abi.MAX_LIKE_PATTERN == 256 and abi.KERNEL_LIKE == 7


def test_chunk_descriptor_layout_matches_the_header(tmp_path):
    fields = [name for name, _ in abi.StringDictionaryChunk._fields_]
    assert fields == ["n_entries", "string_length", "chars", "offsets"]
    lines = ['  printf("size %zu\\n", sizeof(hy_string_dictionary_chunk));\n', '  printf("max %d\\n", HY_MAX_LIKE_PATTERN);\n', '  printf("kernel %d\\n", HY_KERNEL_LIKE);\n']
    lines += [f'  printf("{f} %zu\\n", offsetof(hy_string_dictionary_chunk, {f}));\n' for f in fields]
    source = tmp_path / "like_sizes.c"
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hyrise_amd.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    binary = tmp_path / "like_sizes"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(binary), str(source)])
    sizes = dict(line.split() for line in subprocess.run([str(binary)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(sizes["size"]) == C.sizeof(abi.StringDictionaryChunk) == 24
    assert int(sizes["max"]) == abi.MAX_LIKE_PATTERN and int(sizes["kernel"]) == abi.KERNEL_LIKE
    for f in fields:
        assert int(sizes[f]) == getattr(abi.StringDictionaryChunk, f).offset, f


def tokenize(pattern, condition):
    lib = abi.load_library()
    tokens = np.full(abi.MAX_LIKE_PATTERN + 1, 0xBEEF, dtype=np.uint16)
    n = C.c_uint32(77)
    status = lib.hy_like_tokenize(pattern, len(pattern), condition, tokens.ctypes.data, C.byref(n))
    assert tokens[abi.MAX_LIKE_PATTERN] == 0xBEEF
    return status, tokens[:n.value].tolist()


def test_pattern_tokens():
    one, run = abi.LIKE_ANY_ONE, abi.LIKE_ANY_RUN
    assert tokenize(b"", abi.PRED_LIKE) == (abi.OK, [])
    assert tokenize(b"%", abi.PRED_NOT_LIKE) == (abi.OK, [run])
    assert tokenize(b"%%%", abi.PRED_LIKE) == (abi.OK, [run])
    assert tokenize(b"_%_", abi.PRED_LIKE) == (abi.OK, [one, run, one])
    assert tokenize(b"%_%%_", abi.PRED_LIKE) == (abi.OK, [run, one, run, one])
    assert tokenize(b"aB%\x00\xff_Z", abi.PRED_LIKE) == (abi.OK, [0x61, 0x42, run, 0x00, 0xFF, one, 0x5A])
    assert tokenize(b"aB%\x00\xff_Z@[", abi.PRED_LIKE_INSENSITIVE) == (abi.OK, [0x61, 0x62, run, 0x00, 0xFF, one, 0x7A, 0x40, 0x5B])   # only A-Z folds
    assert tokenize(b"aB", abi.PRED_NOT_LIKE_INSENSITIVE) == (abi.OK, [0x61, 0x62])
    status, tokens = tokenize(b"a" * 256, abi.PRED_LIKE)
    assert status == abi.OK and tokens == [0x61] * 256
    assert tokenize(b"a" * 257, abi.PRED_LIKE) == (abi.ERR_UNSUPPORTED, [])
    assert tokenize(b"%" * 257, abi.PRED_LIKE) == (abi.ERR_UNSUPPORTED, [])   # the limit is on the pattern's bytes
    for condition in (abi.PRED_EQUALS, abi.PRED_NOT_IN, abi.PRED_IS_NULL, 99):
        assert tokenize(b"a", condition) == (abi.ERR_INVALID, [])
    lib = abi.load_library()
    n = C.c_uint32(0)
    assert lib.hy_like_tokenize(b"a", 1, abi.PRED_LIKE, None, C.byref(n)) == abi.ERR_INVALID
    assert lib.hy_like_tokenize(None, 1, abi.PRED_LIKE, np.zeros(256, np.uint16).ctypes.data, C.byref(n)) == abi.ERR_INVALID


def test_the_tokens_describe_the_host_matchers_language():
    """A matcher that walks the tokens the way the kernel does (two pointers, one backtracking point) agrees with like.dictionary_matches."""
    def token_match(tokens, text, fold):
        t = p = resume = 0
        star = None
        while t < len(text):
            token = tokens[p] if p < len(tokens) else 0xFFFF
            if token == abi.LIKE_ANY_RUN:
                star, resume = p, t
                p += 1
                continue
            c = text[t] + 32 if fold and 0x41 <= text[t] <= 0x5A else text[t]
            if token == abi.LIKE_ANY_ONE or token == c:
                p, t = p + 1, t + 1
            elif star is not None:
                resume += 1
                p, t = star + 1, resume
            else:
                return False
        while p < len(tokens) and tokens[p] == abi.LIKE_ANY_RUN:
            p += 1
        return p == len(tokens)

    rng = np.random.default_rng(5)
    entries = [bytes(rng.choice(list(b"abA"), rng.integers(0, 9)).tolist()) for _ in range(200)]
    for _ in range(300):
        pattern = bytes(rng.choice(list(b"abA%_"), rng.integers(0, 7)).tolist())
        for condition in LIKE_CONDITIONS:
            status, tokens = tokenize(pattern, condition)
            assert status == abi.OK
            fold = condition in (abi.PRED_LIKE_INSENSITIVE, abi.PRED_NOT_LIKE_INSENSITIVE)
            negated = condition in (abi.PRED_NOT_LIKE, abi.PRED_NOT_LIKE_INSENSITIVE)
            got = [token_match(tokens, e, fold) != negated for e in entries]
            assert got == dictionary_matches([entries], pattern, condition)[0].tolist(), (pattern, condition)


def test_the_host_matcher_anchors_at_the_end_of_the_input():
    """`$` would also match in front of a trailing newline; LikeMatcher (and the kernel) end the match at the last byte only."""
    entries = [b"", b"\n", b"a", b"a\n", b"a\n\n", b"\na"]
    assert dictionary_matches([entries], b"", abi.PRED_LIKE)[0].tolist() == [True, False, False, False, False, False]
    assert dictionary_matches([entries], b"a", abi.PRED_LIKE)[0].tolist() == [False, False, True, False, False, False]
    assert dictionary_matches([entries], b"a_", abi.PRED_LIKE)[0].tolist() == [False, False, False, True, False, False]
    assert dictionary_matches([entries], b"a", abi.PRED_NOT_LIKE)[0].tolist() == [True, True, False, True, True, True]
    assert dictionary_matches([entries], b"%a", abi.PRED_LIKE_INSENSITIVE)[0].tolist() == [False, False, True, False, False, True]


def test_caller_owned_chunks_need_their_chars():
    """HY_MEM_DEVICE offsets are not read at creation, so a chunk with entries and no chars is refused; a host chunk of empty strings is not
    (that refusal comes first: no device is needed to see it)."""
    lib = abi.load_library()
    handle = C.c_void_p()
    offsets = np.zeros(3, dtype=np.uint32)
    chunks = (abi.StringDictionaryChunk * 1)()
    chunks[0].n_entries, chunks[0].string_length, chunks[0].chars, chunks[0].offsets = 2, 0, None, offsets.ctypes.data
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.ERR_INVALID and not handle.value
    chunks[0].n_entries = 0
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.OK
    assert lib.hy_string_dictionary_destroy(handle) == abi.OK


def test_dictionary_packing():
    chars, offsets = storage.pack_string_dictionary([b"", b"ab", b"\x00c\xff", b""])
    assert chars.tobytes() == b"ab\x00c\xff" and offsets.tolist() == [0, 0, 2, 5, 5] and offsets.dtype == np.uint32
    chars, offsets = storage.pack_string_dictionary([])
    assert len(chars) == 0 and offsets.tolist() == [0]
    chars, offsets = storage.pack_string_dictionary([b"", b"ab", b"abc"], fixed_length=3)
    assert chars.tobytes() == b"\x00\x00\x00ab\x00abc" and offsets is None
    with pytest.raises(AssertionError):
        storage.pack_string_dictionary([b"abcd"], fixed_length=3)


def test_match_layout():
    assert CallerOwnedDictionary([0, 1, 63, 64, 65]).layout() == [0, 0, 1, 2, 3, 5]
    assert CallerOwnedDictionary([65, 0, 64, 63, 1, 257]).layout() == [0, 2, 2, 3, 4, 5, 10]
    assert CallerOwnedDictionary([]).layout() == [0]
    lib = abi.load_library()
    assert lib.hy_string_dictionary_match_layout(None, np.zeros(2, np.uint64).ctypes.data) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_match_layout(CallerOwnedDictionary([1]).handle, None) == abi.ERR_INVALID


def test_dictionary_create_refusals():
    lib = abi.load_library()
    handle = C.c_void_p(1)
    chunks = (abi.StringDictionaryChunk * 1)()
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, None) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_create(None, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.ERR_INVALID and not handle.value
    assert lib.hy_string_dictionary_create(chunks, 1, 7, C.byref(handle)) == abi.ERR_INVALID
    keep = np.zeros(64, dtype=np.uint8)
    chunks[0].n_entries, chunks[0].string_length, chunks[0].chars, chunks[0].offsets = 1 << 20, 1 << 12, keep.ctypes.data, None   # 2^32 bytes of slots
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.ERR_UNSUPPORTED and not handle.value
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_HOST, C.byref(handle)) == abi.ERR_UNSUPPORTED and not handle.value
    chunks[0].n_entries, chunks[0].string_length, chunks[0].chars = 2, 4, None                  # slots without chars
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.ERR_INVALID
    offsets = np.array([0, 3, 2], dtype=np.uint32)                                              # host offsets that descend
    chunks[0].n_entries, chunks[0].string_length, chunks[0].chars, chunks[0].offsets = 2, 0, keep.ctypes.data, offsets.ctypes.data
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_HOST, C.byref(handle)) == abi.ERR_INVALID and not handle.value
    chunks[0].offsets = keep.ctypes.data + 2                                                   # offsets off 4 bytes
    assert lib.hy_string_dictionary_create(chunks, 1, abi.MEM_DEVICE, C.byref(handle)) == abi.ERR_INVALID
    assert lib.hy_string_dictionary_destroy(None) == abi.OK


def test_like_matches_refusals_come_before_any_launch():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([3, 0, 65])
    words = np.full(8, 0xABCD, dtype=np.uint64)
    assert lib.hy_like_matches(None, b"a", 1, abi.PRED_LIKE, abi.MEM_HOST, words.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_like_matches(dictionary.handle, b"a", 1, abi.PRED_LIKE, abi.MEM_HOST, None) == abi.ERR_INVALID
    assert lib.hy_like_matches(dictionary.handle, None, 1, abi.PRED_LIKE, abi.MEM_HOST, words.ctypes.data) == abi.ERR_INVALID
    assert lib.hy_like_matches(dictionary.handle, b"a", 1, abi.PRED_LIKE, 5, words.ctypes.data) == abi.ERR_INVALID
    for condition in (abi.PRED_EQUALS, abi.PRED_NOT_IN, abi.PRED_IS_NULL, 1000):
        assert lib.hy_like_matches(dictionary.handle, b"a", 1, condition, abi.MEM_HOST, words.ctypes.data) == abi.ERR_INVALID
    for condition in LIKE_CONDITIONS:
        assert lib.hy_like_matches(dictionary.handle, b"a" * 257, 257, condition, abi.MEM_HOST, words.ctypes.data) == abi.ERR_UNSUPPORTED
        assert lib.hy_like_matches(dictionary.handle, b"a" * 257, 257, condition, abi.MEM_DEVICE, words.ctypes.data) == abi.ERR_UNSUPPORTED
    for off in (1, 2, 4, 7):
        assert lib.hy_like_matches(dictionary.handle, b"a", 1, abi.PRED_LIKE, abi.MEM_DEVICE, words.ctypes.data + off) == abi.ERR_INVALID
    assert lib.hy_last_error()
    assert (words == 0xABCD).all()


def test_table_scan_like_null_arguments_and_patterns():
    lib = abi.load_library()
    dictionary = CallerOwnedDictionary([1])
    result = abi.ScanResult()
    assert lib.hy_table_scan_like(None, dictionary.handle, b"a", 1, abi.PRED_LIKE, 0, None, 0, C.byref(result)) == abi.ERR_INVALID
    assert lib.hy_table_scan_like(None, None, b"a", 1, abi.PRED_LIKE, 0, None, 0, C.byref(result)) == abi.ERR_INVALID
    assert lib.hy_table_scan_like(None, dictionary.handle, b"a", 1, abi.PRED_LIKE, 0, None, 0, None) == abi.ERR_INVALID


@pytest.mark.gpu
def test_a_dictionary_that_disagrees_with_the_column_is_invalid(device):
    """Chunk count and every n_entries are checked against the data column's dictionary segments (aux_size) before any launch; so are the
    condition and the pattern's length.  (Needs a column, and a column needs a device.)"""
    from hyrise_amd.operators import HostScanResult
    lib = abi.load_library()
    values = [[b"a", b"b", b"a"], [b"c", b"c"], [b"d", b"e", b"f", b"g"]]
    encoded = [storage.encode_string_dictionary(v) for v in values]
    host = storage.HostColumn([segment for segment, _ in encoded], abi.TYPE_STRING)
    column = storage.DeviceColumn(host)
    dictionaries = [dictionary for _, dictionary in encoded]

    def scan(dev_dict, pattern=b"%", condition=abi.PRED_LIKE, dev_column=column):
        result = HostScanResult(dev_column.n_chunks, dev_column.rows)
        result.matches[:] = 0xEEEEEEEE
        status = lib.hy_table_scan_like(dev_column.handle, dev_dict.handle, pattern, len(pattern), condition, 0, None, 0, C.byref(result.c))
        assert status == abi.OK or (result.matches == 0xEEEEEEEE).all()   # a refused call writes nothing
        return status

    assert scan(storage.DeviceStringDictionary(dictionaries)) == abi.OK
    assert scan(storage.DeviceStringDictionary(dictionaries[:2])) == abi.ERR_INVALID
    assert scan(storage.DeviceStringDictionary(dictionaries + [[b"x"]])) == abi.ERR_INVALID
    assert scan(storage.DeviceStringDictionary([dictionaries[0], dictionaries[1] + [b"z"], dictionaries[2]])) == abi.ERR_INVALID
    assert scan(storage.DeviceStringDictionary([dictionaries[0], dictionaries[1], dictionaries[2][:3]])) == abi.ERR_INVALID
    good = storage.DeviceStringDictionary(dictionaries)
    assert scan(good, b"a" * 257) == abi.ERR_UNSUPPORTED
    assert scan(good, condition=abi.PRED_EQUALS) == abi.ERR_INVALID
    pos_lists = [np.array([[c, 0]], dtype=np.uint32) for c in range(3)]
    referencing = storage.make_reference_column(host, pos_lists, [0, 1, 2])
    reference = storage.DeviceColumn(referencing, refs={id(host): column})
    assert scan(good, dev_column=reference) == abi.OK
    result = HostScanResult(3, 3)
    excluded = np.array([1], dtype=np.uint32)
    assert lib.hy_table_scan_like(reference.handle, good.handle, b"%", 1, abi.PRED_LIKE, 0, excluded.ctypes.data, 1, C.byref(result.c)) == abi.ERR_INVALID   # data tables only
    assert b"excluded chunks" in lib.hy_last_error()
    ints = storage.DeviceColumn(storage.make_column(np.arange(9, dtype=np.int32), None, abi.ENC_DICTIONARY, chunk_size=3))
    assert scan(storage.DeviceStringDictionary([[b"a", b"b", b"c"]] * 3), dev_column=ints) == abi.ERR_INVALID   # "LIKE operator only applicable on string columns"

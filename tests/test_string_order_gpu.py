"""hy_string_dictionary_order (csrc/string_order.hip): one column's dictionaries ordered against each other in HBM, against
tests/string_order_oracle.py bit for bit -- every chunk count that changes the shape of the merge rounds, empty chunks anywhere, shared
and disjoint entries, bytes as bytes, both dictionary layouts, runs that cross many workgroups, caller-owned buffers."""
import ctypes as C

import numpy as np
import pytest

from hyrise_amd import abi, storage
from hyrise_amd.operators import string_dictionary_order
from hyrise_amd.storage import DeviceStringDictionary
from placed_columns import PlacedArray
from test_like_device_gpu import BYTE_ENTRIES, PlacedDictionary
import string_order_oracle as oracle

pytestmark = pytest.mark.gpu

ENTRY_COUNTS = (0, 1, 63, 64, 65, 257)


def random_entries(rng, n, alphabet=b"ab\x00\xff", longest=6):
    """n distinct sorted entries (the alphabet is small and the strings short: the chunks share many entries)."""
    out = set()
    while len(out) < n:
        out.add(bytes(rng.choice(list(alphabet), rng.integers(0, longest + 1)).tolist()))
    return sorted(out)


def assert_order(dictionaries, context, dev_dict=None):
    got, n_distinct = string_dictionary_order(dev_dict or DeviceStringDictionary(dictionaries))
    want, want_distinct = oracle.column_order(dictionaries)
    assert n_distinct == want_distinct, context
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.tolist() == w, f"{context}: chunk {c} of {len(dictionaries)} ({len(dictionaries[c])} entries)"
    return got


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 5, 8, 9, 33])
def test_chunk_counts(device, n_chunks):
    """One run; an odd run carried through one or several rounds; powers of two on both sides.  Entry counts cycle through 0 .. 257."""
    rng = np.random.default_rng(n_chunks)
    counts = [ENTRY_COUNTS[(c + n_chunks) % len(ENTRY_COUNTS)] for c in range(n_chunks)]
    assert_order([random_entries(rng, n) for n in counts], f"{n_chunks} chunks")
    assert_order([random_entries(rng, 65) for _ in range(n_chunks)], f"{n_chunks} chunks of 65")


@pytest.mark.parametrize("counts", [(0, 64, 257), (65, 0, 63), (1, 257, 0), (0, 0, 65, 0, 0), (0, 1, 0, 1, 0, 1, 0), (0,), (0, 0, 0), ()],
                         ids=lambda counts: "x".join(map(str, counts)) or "none")
def test_empty_chunks_first_in_the_middle_and_last(device, counts):
    rng = np.random.default_rng(len(counts))
    assert_order([random_entries(rng, n) for n in counts], f"counts {counts}")


def test_structure_of_five_chunks(device):
    rng = np.random.default_rng(3)
    base = [e for e in random_entries(rng, 301, alphabet=b"bcd", longest=8) if e][:300]       # (the empty string lies below everything)
    got = assert_order([base] * 5, "all identical")
    assert all(g.tolist() == list(range(300)) for g in got) and string_dictionary_order(DeviceStringDictionary([base] * 5))[1] == 300
    disjoint = [sorted({bytes([0x61 + c]) + e for e in base}) for c in range(5)]
    assert_order(disjoint[::2] + disjoint[1::2], "pairwise disjoint")
    assert_order(disjoint[::-1], "each chunk wholly below its predecessor")
    twins = [sorted({e + b"\x00" * c for e in base}) for c in range(5)]
    assert_order(twins, "each entry's twin + \\0 in the next chunk")


def test_bytes_are_bytes(device):
    """The empty string, \\0 inside an entry, 0x80-0xFF against ASCII, a / ab / aab, two 400-byte entries that differ in the last byte
    only, one of them the other's prefix -- dealt round-robin over 4 chunks, with overlap."""
    entries = sorted(set(BYTE_ENTRIES))
    assert entries[0] == b"" and b"a\x00b" in entries and b"a" * 400 in entries and b"a" * 400 + b"b" in entries
    chunks = [sorted(set(entries[c::4] + entries[(c + 1) % 4::8])) for c in range(4)]
    assert any(set(chunks[a]) & set(chunks[b]) for a in range(4) for b in range(a + 1, 4))
    assert_order(chunks, "byte entries")
    assert_order([[b"a" * 400 + b"b"], [b"a" * 400], [b"a" * 400 + b"a", b"a" * 400 + b"b"]], "long twins")


class MixedDictionary:
    """An uploaded hy_string_dictionary whose chunk c has the fixed-slot layout of fixed_lengths[c] bytes, or (None) the offsets layout."""

    def __init__(self, dictionaries, fixed_lengths):
        self.lib = abi.load_library()
        self.n_chunks, self.n_entries = len(dictionaries), [len(d) for d in dictionaries]
        self.packed = [storage.pack_string_dictionary(d, length) for d, length in zip(dictionaries, fixed_lengths)]
        chunks = (abi.StringDictionaryChunk * max(1, self.n_chunks))()
        for c, (chars, offsets) in enumerate(self.packed):
            chunks[c].n_entries, chunks[c].string_length = self.n_entries[c], fixed_lengths[c] or 0
            chunks[c].chars = chars.ctypes.data if len(chars) else None
            chunks[c].offsets = offsets.ctypes.data if offsets is not None else None
        self.handle = C.c_void_p()
        abi.check(self.lib.hy_string_dictionary_create(chunks, self.n_chunks, abi.MEM_HOST, C.byref(self.handle)))

    def __del__(self):
        if self.handle:
            self.lib.hy_string_dictionary_destroy(self.handle)


@pytest.mark.parametrize("fixed_lengths", [(6, 6, 6, 6, 6), (6, None, 9, None, 6), (None, 6, None, 6, 7)], ids=["fixed", "mixed", "mixed_other"])
def test_fixed_length_layouts_alone_and_mixed(device, fixed_lengths):
    """Slots of 6 bytes hold entries of 0 .. 6 bytes: some fill the whole slot, and a slot's entry ends at its first \\0."""
    rng = np.random.default_rng(7)
    dictionaries = [random_entries(rng, n, alphabet=b"ab\xff") for n in (257, 64, 65, 0, 100)]
    assert all(any(len(e) == 6 for e in d) for d in dictionaries if d)
    assert_order(dictionaries, f"layouts {fixed_lengths}", MixedDictionary(dictionaries, fixed_lengths))


def test_three_chunks_of_seventy_thousand(device):
    """Runs that cross hundreds of workgroups, value ids past 65 535; half of every chunk's entries are shared with the others."""
    shared = [b"s%06d" % i for i in range(35_000)]
    dictionaries = [sorted(shared + [b"%c%06d" % (0x61 + c, 3 * i + c) for i in range(35_000)]) for c in range(3)]
    assert all(len(d) == 70_000 for d in dictionaries)
    assert_order(dictionaries, "3 x 70 000")


@pytest.mark.parametrize("chars_residue", [1, 3, 8])
def test_device_ranks_and_caller_owned_dictionaries(device, chars_residue):
    """HY_MEM_DEVICE: dictionary buffers at odd byte addresses, the rank buffer at 4 modulo 16 with canaries on both sides; the result is the
    HY_MEM_HOST result; inputs stay as they were."""
    lib = abi.load_library()
    rng = np.random.default_rng(chars_residue)
    dictionaries = [random_entries(rng, n) for n in (65, 0, 257, 1, 64, 63)]
    want = np.array([r for chunk in oracle.column_order(dictionaries)[0] for r in chunk], dtype=np.int32)
    fill = 0xFF if chars_residue == 3 else 0x00
    placed = PlacedDictionary(dictionaries, chars_residue, fill)
    for dev_dict in (placed, DeviceStringDictionary(dictionaries)):
        ranks = PlacedArray(4 * len(want), 4, fill, guard=64)
        n_distinct = C.c_uint32(0)
        abi.check(lib.hy_string_dictionary_order(dev_dict.handle, abi.MEM_DEVICE, ranks.pointer, C.byref(n_distinct)))
        inside, guards_intact = ranks.read(np.int32)
        assert guards_intact and np.array_equal(inside, want) and n_distinct.value == int(want.max()) + 1
        ranks = PlacedArray(4 * len(want), 4, fill, guard=64)
        abi.check(lib.hy_string_dictionary_order(dev_dict.handle, abi.MEM_DEVICE, ranks.pointer, None))   # (no host round trip: stream order)
        abi.check(lib.hy_synchronize())
        inside, guards_intact = ranks.read(np.int32)
        assert guards_intact and np.array_equal(inside, want)
    placed.assert_untouched()
    host = np.full(len(want) + 8, 0x5A5A5A5A, dtype=np.int32)
    abi.check(lib.hy_string_dictionary_order(placed.handle, abi.MEM_HOST, host[4:].ctypes.data, None))
    assert np.array_equal(host[4:4 + len(want)], want) and (host[:4] == 0x5A5A5A5A).all() and (host[4 + len(want):] == 0x5A5A5A5A).all()


def test_calling_twice_gives_the_same_bytes(device):
    rng = np.random.default_rng(9)
    dev_dict = DeviceStringDictionary([random_entries(rng, n) for n in (257, 65, 0, 64, 300, 1, 63)])
    first, first_distinct = string_dictionary_order(dev_dict)
    second, second_distinct = string_dictionary_order(dev_dict)
    assert first_distinct == second_distinct and all(a.tobytes() == b.tobytes() for a, b in zip(first, second))

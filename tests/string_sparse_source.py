"""The source column of the sparse-route tests (test_string_gather_sparse_gpu.py, test_string_materialize_gpu.py): five chunks whose
dictionaries have 0, 1, 300, 2 049 and 70 000 entries -- attribute vectors of 1, 2 and 4 bytes and a bit-packed one --, strings shared
between chunks, the empty string, bytes 0x00 and 0x80-0xFF, one 100 000-byte entry, NULL rows in every chunk."""
import ctypes as C

import numpy as np

from hyrise_amd import abi, storage
from hyrise_amd.storage import DeviceColumn, DeviceStringDictionary, HostColumn

NULL = 0xFFFFFFFF
ENTRY_COUNTS = [0, 1, 300, 2_049, 70_000]
DENSE, SPARSE = 0, 2   # HY_OPT_STRING_SPARSE_GATHER


def entries_of(count, chunk):
    """`count` distinct strings: the first ones the same in every chunk, the rest the chunk's own."""
    special = [b"", b"\x00", b"\x00\x00a", b"a\x00b", b"\x80", b"\xff\xfe\x80", b"a", b"ab", b"abc\xff"]
    entries = special[:count]
    entries += [b"s%05d" % i for i in range(min(100, count - len(entries)))]   # shared with the other chunks
    entries += [b"%c%06d\x80" % (0x62 + chunk, i) for i in range(count - len(entries))]
    assert len(set(entries)) == count
    return entries


class SparseSource:
    def __init__(self):
        long_entry = bytes(np.random.default_rng(11).integers(0, 256, 100_000, dtype=np.uint8))
        self.chunks = []
        for c, count in enumerate(ENTRY_COUNTS):
            entries = entries_of(count, c)
            if count == 2_049:
                entries[-1] = long_entry
            rows = entries + [None, None] + entries[:3] + [None]
            self.chunks.append(rows[1:] + rows[:1])   # (not in dictionary order)
        encoded = [storage.encode_string_dictionary([v if v is not None else b"" for v in chunk], [v is None for v in chunk]) for chunk in self.chunks]
        self.dictionaries = [dictionary for _, dictionary in encoded]
        assert [len(d) for d in self.dictionaries] == ENTRY_COUNTS
        segments = [segment for segment, _ in encoded]
        assert [s.width for s in segments] == [1, 1, 2, 2, 4]
        segments[2] = storage.bit_pack_segment(segments[2])   # 9 bits per element
        self.host = HostColumn(segments, abi.TYPE_STRING)
        self.dev = DeviceColumn(self.host)
        self.dev_dict = DeviceStringDictionary(self.dictionaries)
        self.rows = sum(len(chunk) for chunk in self.chunks)

    def row(self, position):
        """The string at a RowID, None for NULL: a NULL RowID, one outside the table, a NULL row."""
        chunk, offset = position
        if offset == NULL or chunk >= len(self.chunks) or offset >= len(self.chunks[chunk]):
            return None
        return self.chunks[chunk][offset]


def temporary_pool_largest_block(lib):
    largest = C.c_uint64(0)
    abi.check(lib.hy_temporary_pool_stats(None, C.byref(largest)))
    return largest.value

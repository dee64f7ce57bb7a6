"""The layout arithmetic of tests/placed_columns.py, over a numpy array in place of the device tensor."""
import numpy as np
import pytest

import placed_columns as pc
from hyrise_amd import abi, storage


def test_residues_per_placement_and_element_size():
    for w in (1, 2, 4, 8):
        assert [pc.residue("aligned", role, w) for role in ("data", "aux", "nulls")] == [0, 0, 0]
        assert [pc.residue("natural", role, w) for role in ("data", "aux", "nulls")] == [w, w, w]
        assert [pc.residue("eight", role, w) for role in ("data", "aux", "nulls")] == [8, 8, 8]
        assert [pc.residue("last", role, w) for role in ("data", "aux", "nulls")] == [16 - w] * 3
        assert [pc.residue("aux_only", role, w) for role in ("data", "aux", "nulls")] == [0, w, 0]
        for placement in pc.PLACEMENTS:
            assert pc.residue(placement, "data", w) % w == 0   # offsets are multiples of the element size
    assert pc.placements_for(8) == ["aligned", "natural"]      # duplicates collapse: 0 and 8
    assert pc.placements_for(4) == ["aligned", "natural", "eight", "last"]
    assert pc.placements_for(1) == ["aligned", "natural", "eight", "last"]


def columns():
    rng = np.random.default_rng(1)
    n = 8_203 + 2_051 + 5
    sizes = (8_203, 2_051, 5)
    ints = rng.integers(-300, 300, n).astype(np.int32)
    nulls = rng.random(n) < 0.1
    out = []

    def chunks(make):
        begin, segments = 0, []
        for size in sizes:
            segments.append(make(ints[begin:begin + size], nulls[begin:begin + size]))
            begin += size
        return storage.HostColumn(segments, abi.TYPE_INT)

    out.append(chunks(lambda v, m: storage.encode_segment(v, m, abi.ENC_UNENCODED)))
    out.append(chunks(lambda v, m: storage.encode_segment(v.astype(np.float64), m, abi.ENC_DICTIONARY)))
    out.append(chunks(lambda v, m: storage.encode_segment(v, m, abi.ENC_FRAME_OF_REFERENCE)))
    out.append(chunks(lambda v, m: storage.encode_run_length(v // 100, m)))
    out.append(chunks(lambda v, m: storage.bit_pack_segment(storage.encode_segment(v, m, abi.ENC_DICTIONARY))))
    out.append(storage.make_mvcc_column(np.arange(100), np.arange(100), np.arange(100), chunk_size=33))
    base = out[0]
    out.append(storage.make_reference_column(base, [np.array([[0, 1], [2, 3], [0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32), 1], [None, 1]))
    return out


@pytest.mark.parametrize("placement", pc.PLACEMENTS)
@pytest.mark.parametrize("fill", pc.FILLS)
def test_layout_over_a_numpy_array(placement, fill):
    for host in columns():
        buffers = pc.column_buffers(host)
        assert buffers
        for skew in (0, 1, 7, 12):   # whatever the allocation's own address is
            allocation = np.empty(pc.upper_bound(buffers) + 16, dtype=np.uint8)
            base = allocation.ctypes.data + skew
            length = pc.lay_out(base, buffers, placement)
            assert skew + length <= len(allocation)
            image = pc.image_of(buffers, length, fill)
            allocation[skew:skew + length] = image
            mask = pc.filler_mask(buffers, length)
            assert np.all(image[mask] == fill)
            # addresses, gaps, leading and trailing filler
            assert pc.LEADING <= buffers[0].offset <= pc.LEADING + 15
            assert length - (buffers[-1].offset + len(buffers[-1].bytes)) == pc.TRAILING == 4096
            for before, after in zip(buffers[:-1], buffers[1:]):
                assert pc.GAP <= after.offset - (before.offset + len(before.bytes)) <= pc.GAP + 15
            for b in buffers:
                address = base + b.offset
                assert address % 16 == pc.residue(placement, b.role, b.w)
                assert address % b.w == 0
                # every buffer reads back byte for byte, through its absolute address
                assert allocation[address - allocation.ctypes.data:][:len(b.bytes)].tobytes() == b.bytes.tobytes()


def test_buffers_of_every_segment_kind():
    value, dictionary, frame, runs, packed, mvcc, reference = columns()
    assert [(b.field, b.w) for b in pc.column_buffers(value) if b.chunk == 0] == [("data", 4), ("nulls", 8)]
    assert [(b.field, b.role, b.w) for b in pc.column_buffers(dictionary) if b.chunk == 0] == [("data", "data", 2), ("aux", "aux", 8)]
    assert [(b.field, b.w) for b in pc.column_buffers(frame) if b.chunk == 0] == [("data", 2), ("aux", 4), ("nulls", 8)]
    assert [(b.field, b.w) for b in pc.column_buffers(runs) if b.chunk == 0] == [("data", 4), ("aux", 4), ("nulls", 1)]
    assert [(b.field, b.w) for b in pc.column_buffers(packed) if b.chunk == 0] == [("data", 8), ("aux", 4)]
    assert [(b.field, b.w) for b in pc.column_buffers(mvcc) if b.chunk == 0] == [("data", 4), ("aux", 4), ("nulls", 4)]
    assert [(b.chunk, b.field, b.w) for b in pc.column_buffers(reference)] == [(0, "data", 8)]   # the EntireChunkPosList has no buffer
    first = pc.column_buffers(value)[0]
    assert first.bytes.tobytes() == value.segments[0].data.tobytes()


def test_lz4_segments_are_refused():
    segment = storage.HostSegment(abi.ENC_LZ4, abi.TYPE_INT, 4, 4, None)
    with pytest.raises(ValueError):
        pc.column_buffers(storage.HostColumn([segment], abi.TYPE_INT))

"""Columns in caller-owned device memory (HY_MEM_DEVICE) with every buffer at a chosen address modulo 16.

storage.DeviceColumn uploads through the library's arena: every buffer starts on a 256-byte boundary and has 16 spare bytes behind it.  A
caller's buffers start wherever the caller's vectors do and are followed by the next buffer.  PlacedColumn lays every buffer of every
segment of a HostColumn out in ONE torch.uint8 tensor, each at the residue its placement asks for, with known filler bytes around it, and
creates the column over those addresses.  The layout arithmetic is plain Python over an address and a list of buffers (tests/
test_placed_columns.py checks it without a GPU, over a numpy array)."""
import ctypes as C

import numpy as np

from hyrise_amd import abi

PLACEMENTS = ("aligned", "natural", "eight", "last", "aux_only")
FILLS = (0x00, 0xFF)
LEADING, GAP, TRAILING = 256, 32, 4096   # filler in front of the first buffer (256 .. 271), between two buffers (32 .. 47), behind the last one


def residue(placement, role, w):
    """The address modulo 16 a buffer of `w`-byte elements gets.  role: "data", "aux" or "nulls"."""
    assert w in (1, 2, 4, 8) and role in ("data", "aux", "nulls")
    if placement == "aligned":
        return 0
    if placement == "natural":
        return w
    if placement == "eight":
        return 8
    if placement == "last":
        return 16 - w
    if placement == "aux_only":
        return w if role == "aux" else 0
    raise ValueError(f"placement {placement}")


def placements_for(w):
    """The placements that differ for a `w`-byte buffer (duplicates collapse: an 8-byte buffer has two)."""
    seen, out = set(), []
    for placement in ("aligned", "natural", "eight", "last"):
        r = residue(placement, "data", w)
        if r not in seen:
            seen.add(r)
            out.append(placement)
    return out


class Buffer:
    """One buffer of one segment: which descriptor field it fills, its element size and its bytes."""

    def __init__(self, chunk, field, role, w, array):
        array = np.ascontiguousarray(array)
        self.chunk, self.field, self.role, self.w = chunk, field, role, w
        self.bytes = array.view(np.uint8).reshape(-1) if array.size else np.zeros(0, dtype=np.uint8)
        assert len(self.bytes) % w == 0
        self.offset = None


def column_buffers(host_column):
    """Every device buffer of a HostColumn's segments, in descriptor order (data, aux, nulls per chunk).  Empty buffers are left out: their
    descriptor field stays NULL, as after an upload."""
    out = []
    for c, s in enumerate(host_column.segments):
        if s.encoding == abi.ENC_LZ4:
            raise ValueError("LZ4 segments are handed over as host memory only")
        packed = s.width == 0 and s.bits and s.encoding in (abi.ENC_DICTIONARY, abi.ENC_FRAME_OF_REFERENCE)
        if s.encoding == abi.ENC_REFERENCE:
            fields = [("data", "data", 8, s.data)]                       # the PosList (RowIDs); None: an EntireChunkPosList
        elif s.encoding == abi.ENC_MVCC:
            fields = [("data", "data", 4, s.data), ("aux", "aux", 4, s.aux), ("nulls", "nulls", 4, s.nulls)]   # tids, begin cids, end cids
        elif s.encoding == abi.ENC_RUN_LENGTH:
            fields = [("data", "data", s.width, s.data), ("aux", "aux", 4, s.aux), ("nulls", "nulls", 1, s.nulls)]   # run values, run ends, run null bytes
        else:
            aux_w = 4 if s.encoding == abi.ENC_FRAME_OF_REFERENCE else (s.aux.dtype.itemsize if s.aux is not None else 4)
            fields = [("data", "data", 8 if packed else s.width, s.data), ("aux", "aux", aux_w, s.aux), ("nulls", "nulls", 8, s.nulls)]
        for field, role, w, array in fields:
            if array is not None and np.asarray(array).size:
                out.append(Buffer(c, field, role, w, array))
    return out


def upper_bound(buffers):
    """Bytes that hold any layout of `buffers` at any base address."""
    return LEADING + 16 + sum(len(b.bytes) + GAP + 16 for b in buffers) + TRAILING


def lay_out(base_address, buffers, placement):
    """Sets every buffer's offset from `base_address` -> the layout's length in bytes (the last buffer's end + TRAILING)."""
    cursor = LEADING
    for b in buffers:
        want = residue(placement, b.role, b.w)
        cursor += (want - (base_address + cursor)) % 16
        b.offset = cursor
        assert (base_address + b.offset) % 16 == want and (base_address + b.offset) % b.w == 0
        cursor += len(b.bytes) + GAP
    return (cursor - GAP if buffers else LEADING) + TRAILING


def image_of(buffers, length, fill):
    """The layout's bytes: `fill` everywhere but in the buffers."""
    image = np.full(length, fill, dtype=np.uint8)
    for b in buffers:
        image[b.offset:b.offset + len(b.bytes)] = b.bytes
    return image


def filler_mask(buffers, length):
    mask = np.ones(length, dtype=bool)
    for b in buffers:
        mask[b.offset:b.offset + len(b.bytes)] = False
    return mask


class PlacedColumn:
    """A HostColumn as an HY_MEM_DEVICE column over one torch.uint8 tensor (usable wherever a storage.DeviceColumn is).
    refs: {id(referenced HostColumn): its device column} for reference segments."""

    def __init__(self, host_column, placement, fill, refs=None, device="cuda"):
        import torch
        assert placement in PLACEMENTS and fill in FILLS
        self.lib = abi.load_library()
        self.host, self.placement, self.fill = host_column, placement, fill
        self._refs = refs or {}
        self.buffers = column_buffers(host_column)
        allocation = torch.empty(upper_bound(self.buffers), dtype=torch.uint8, device=device)
        self.base = allocation.data_ptr()
        length = lay_out(self.base, self.buffers, placement)
        assert length <= allocation.numel()
        self.tensor = allocation[:length]          # (ends TRAILING bytes behind the last buffer; the allocation behind it stays alive with the view)
        self.image = image_of(self.buffers, length, fill)
        self.tensor.copy_(torch.from_numpy(self.image))
        torch.cuda.synchronize()
        self._filler = filler_mask(self.buffers, length)

        arr = host_column.descriptors(lambda ref_host: self._refs[id(ref_host)].handle)
        for c in range(host_column.n_chunks):
            arr[c].data = arr[c].aux = arr[c].nulls = None
        self.addresses = {}
        for b in self.buffers:
            address = self.base + b.offset
            assert address % 16 == residue(placement, b.role, b.w), (placement, b.field, b.w, address % 16)
            assert b.offset >= LEADING and b.offset + len(b.bytes) + TRAILING <= length   # never at the end of the allocation
            setattr(arr[b.chunk], b.field, address)
            self.addresses[(b.chunk, b.field)] = address
        self._descriptors = arr
        handle = C.c_void_p()
        abi.check(self.lib.hy_column_create(arr, host_column.n_chunks, abi.MEM_DEVICE, C.byref(handle)))
        self.handle = handle
        self.n_chunks, self.rows, self.data_type = host_column.n_chunks, host_column.rows, host_column.data_type

    def assert_untouched(self):
        """Inputs are const: every filler byte still holds `fill`, every buffer its bytes."""
        import torch
        torch.cuda.synchronize()
        now = self.tensor.cpu().numpy()
        touched = np.flatnonzero(now != self.image)
        if len(touched):
            where = "filler" if self._filler[touched[0]] else "a buffer"
            raise AssertionError(f"{len(touched)} bytes of a {self.placement}/{self.fill:#04x} input were written, the first at offset {touched[0]} ({where})")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.hy_column_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlacedArray:
    """A plain device array at `residue` modulo 16 inside one torch.uint8 tensor with `guard` filler bytes on both sides (and 4096 behind):
    positions, tables and outputs of the calls that take raw device pointers."""

    def __init__(self, nbytes, residue_16, fill, guard=64, contents=None, device="cuda"):
        import torch
        self.nbytes, self.fill, self.guard = int(nbytes), fill, guard
        allocation = torch.empty(guard + 16 + self.nbytes + guard + TRAILING, dtype=torch.uint8, device=device)
        self.offset = guard + (residue_16 - (allocation.data_ptr() + guard)) % 16
        self.tensor = allocation[:self.offset + self.nbytes + guard + TRAILING]
        self.pointer = allocation.data_ptr() + self.offset
        assert self.pointer % 16 == residue_16
        self.image = np.full(self.tensor.numel(), fill, dtype=np.uint8)
        if contents is not None:
            raw = np.ascontiguousarray(contents).view(np.uint8).reshape(-1)
            assert len(raw) == self.nbytes
            self.image[self.offset:self.offset + self.nbytes] = raw
        self.tensor.copy_(torch.from_numpy(self.image))
        torch.cuda.synchronize()

    def read(self, dtype=np.uint8):
        """(the array's bytes as `dtype`, True if every guard byte still holds the fill)"""
        import torch
        torch.cuda.synchronize()
        now = self.tensor.cpu().numpy()
        inside = now[self.offset:self.offset + self.nbytes].copy()
        outside = np.concatenate([now[:self.offset], now[self.offset + self.nbytes:]])
        return inside.view(dtype), bool(np.all(outside == self.fill))

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(self.tensor.cpu().numpy(), self.image), "a const input array was written"

// string_order.hip -- ColumnVsColumn on two string columns (column_vs_column_table_scan_impl.cpp:145-187 applied to pmr_string): per chunk
// the left column's dictionary is ordered against the right column's, on the device, and the row pass is the numeric two-column scan.
//
//   lo(v)   = number of right entries < L[v]          (lower_bound)
//   eq(v)   = lo(v) < n_r && R[lo(v)] == L[v]
//   rank(v) = 2 * lo(v) - (eq(v) ? 0 : 1)             rank of right entry r: 2 * r
//
// L[v] <cond> R[r]  <=>  rank(v) <cond> 2r  for all six comparisons: with eq, L[v] = R[lo] and 2lo against 2r decides; without,
// R[lo - 1] < L[v] < R[lo] and the odd 2lo - 1 lies strictly between 2(lo - 1) and 2lo.
//
// string_rank, ONE launch per dictionary pair: a workgroup owns 256 consecutive left entries of one chunk (the LikeBlock table of the left
// dictionary, like.hip), a lane one entry; it binary-searches the right chunk's dictionary and writes one int32.  Order is std::string's:
// bytes as unsigned, the shorter string first when it is the other's prefix.  Entries are compared four bytes at a time (one load each side
// at whatever byte address the entry has, byte-swapped so that the words order as the bytes do) while four bytes remain in BOTH, byte by byte
// after that: no byte outside an entry is read, so not even the slack behind the buffers is needed.  Nothing is staged in LDS: the left
// entry is a lane's own 12 or so re-reads of one line, and the right entries are a data-dependent gather over a dictionary of any size
// whose first probes are the same for all lanes (one broadcast line each).
// Offsets are clamped to the chunk's byte range [0, offsets[n_entries]] on both sides: a dictionary that is not sorted, or offsets that do
// not ascend, give unspecified ranks and no read outside the two chunks' bytes.
#include "hy_device.hpp"

#include <algorithm>

namespace hy {

namespace {

constexpr uint32_t RANK_WG = 256;   // = like.hip's LIKE_WG: the block table is the matcher's

struct RankArgs {
  const LikeChunk* left;
  const LikeChunk* right;
  const LikeBlock* blocks;          // of the left dictionary
  const uint64_t* entry_offsets;    // of the left dictionary
  int32_t* ranks;
};

struct Entry {
  const uint8_t* bytes;
  uint32_t length;
};

// bytes in the chunk's chars: what the entries may be read from
__device__ __forceinline__ uint32_t chunk_bytes(const LikeChunk& chunk) {
  if (chunk.n_entries == 0) return 0;
  return chunk.offsets ? chunk.offsets[chunk.n_entries] : chunk.n_entries * chunk.string_length;
}

__device__ __forceinline__ Entry entry_of(const LikeChunk& chunk, uint32_t v, uint32_t end) {
  const uint8_t* chars = reinterpret_cast<const uint8_t*>(chunk.chars);
  if (chunk.offsets) {
    const uint32_t from = min(chunk.offsets[v], end);
    const uint32_t to = min(max(chunk.offsets[v + 1], from), end);
    return Entry{chars + from, to - from};
  }
  const uint8_t* slot = chars + size_t{v} * chunk.string_length;   // FixedString: strnlen(slot, L), fixed_string.cpp:86-99
  uint32_t length = 0;
  while (length < chunk.string_length && slot[length] != 0) ++length;
  return Entry{slot, length};
}

__device__ __forceinline__ uint32_t load_word(const uint8_t* p) {   // four bytes at any address, first byte most significant
  uint32_t w;
  __builtin_memcpy(&w, p, 4);
  return __builtin_bswap32(w);
}

// < 0, 0, > 0 as x.compare(y) of two std::strings
__device__ __forceinline__ int compare_entries(const Entry& x, const Entry& y) {
  const uint32_t common = min(x.length, y.length);
  uint32_t i = 0;
  for (; i + 4 <= common; i += 4) {
    const uint32_t p = load_word(x.bytes + i), q = load_word(y.bytes + i);
    if (p != q) return p < q ? -1 : 1;
  }
  for (; i < common; ++i) {
    const uint32_t p = x.bytes[i], q = y.bytes[i];
    if (p != q) return p < q ? -1 : 1;
  }
  return x.length == y.length ? 0 : x.length < y.length ? -1 : 1;
}

__global__ __launch_bounds__(RANK_WG) void string_rank(RankArgs a) {
  const LikeBlock block = a.blocks[blockIdx.x];
  const LikeChunk left = a.left[block.chunk], right = a.right[block.chunk];
  const uint32_t v = block.first_entry + threadIdx.x;
  if (v >= left.n_entries) return;
  const uint32_t left_end = chunk_bytes(left), right_end = chunk_bytes(right);
  const Entry mine = entry_of(left, v, left_end);
  uint32_t lo = 0, hi = right.n_entries;
  bool equal = false;   // R[hi] == L[v], for the hi a probe has set
  while (lo < hi) {
    const uint32_t middle = lo + (hi - lo) / 2;
    const int order = compare_entries(entry_of(right, middle, right_end), mine);
    if (order < 0) lo = middle + 1;
    else { hi = middle; equal = order == 0; }
  }
  // (lo == hi: R[lo] is the entry of the last probe that lowered hi, or lo == n_r and `equal` was never set)
  a.ranks[a.entry_offsets[block.chunk] + v] = static_cast<int32_t>(2 * lo) - (equal ? 0 : 1);
}

__global__ __launch_bounds__(256) void string_twins(StringTwins t) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < t.n_evens) t.evens[i] = static_cast<int32_t>(2 * i);
  // (a descriptor is copied, then patched where it lies: a patched local copy becomes a private array)
  if (i < t.n_data_chunks) {
    DevSegment& l = t.left_data_twin[i];
    DevSegment& r = t.right_data_twin[i];
    l = t.left_data[i];
    r = t.right_data[i];
    l.aux = t.ranks + t.entry_offsets[i];
    r.aux = t.evens;
    l.data_type = r.data_type = HY_TYPE_INT;
  }
  if (i < t.n_chunks && t.left_reference) {
    DevSegment& l = t.left_reference_twin[i];
    l = t.left_reference[i];
    l.ref = t.left_data_twin;
    l.data_type = HY_TYPE_INT;
  }
  if (i < t.n_chunks && t.right_reference) {
    DevSegment& r = t.right_reference_twin[i];
    r = t.right_reference[i];
    r.ref = t.right_data_twin;
    r.data_type = HY_TYPE_INT;
  }
}

}  // namespace

hy_status string_order_check(const hy_string_dictionary* left, const hy_string_dictionary* right, const char* entry_point) {
  if (left->n_chunks != right->n_chunks) return fail(HY_ERR_INVALID, "%s: the left dictionary has %u chunks, the right one %u", entry_point, left->n_chunks, right->n_chunks);
  if (left->device != right->device) return fail(HY_ERR_INVALID, "%s: the left dictionary lives on device %d, the right one on device %d", entry_point, left->device, right->device);
  if (left->device != this_thread_device()) return fail(HY_ERR_INVALID, "%s: the dictionaries live on device %d, the calling thread works on device %d", entry_point, left->device, this_thread_device());
  for (uint32_t c = 0; c < right->n_chunks; ++c) {
    if (right->chunks[c].n_entries >= (1u << 30)) return fail(HY_ERR_UNSUPPORTED, "%s: chunk %u: a right dictionary of %u entries does not fit int32 ranks (2 * lo)", entry_point, c, right->chunks[c].n_entries);
  }
  return HY_OK;
}

hy_status string_order_launch(const hy_string_dictionary* left, const hy_string_dictionary* right, int32_t* d_ranks, hipStream_t stream) {
  HY_TRY(like_dictionary_tables(left));
  HY_TRY(like_dictionary_tables(right));
  if (left->blocks.empty()) return HY_OK;
  RankArgs args{left->d_chunks, right->d_chunks, left->d_blocks, left->d_entry_offsets, d_ranks};
  hipEvent_t started = nullptr, stopped = nullptr;
  profile_events(&started, &stopped, HY_KERNEL_STRING_RANK);
  hipExtLaunchKernelGGL(string_rank, dim3(static_cast<uint32_t>(left->blocks.size())), dim3(RANK_WG), 0, stream, started, stopped, 0, args);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

hy_status string_twins_launch(const StringTwins& twins, hipStream_t stream) {
  const uint32_t lanes = std::max(twins.n_evens, std::max(twins.n_data_chunks, twins.n_chunks));
  if (!lanes) return HY_OK;
  hipLaunchKernelGGL(string_twins, dim3((lanes + 255) / 256), dim3(256), 0, stream, twins);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_string_dictionary_ranks(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem, int32_t* ranks) {
  if (!left || !right || !ranks) return fail(HY_ERR_INVALID, "hy_string_dictionary_ranks: null argument");
  if (mem != HY_MEM_HOST && mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "hy_string_dictionary_ranks: bad memory space %u", mem);
  HY_TRY(string_order_check(left, right, "hy_string_dictionary_ranks"));
  if (mem == HY_MEM_DEVICE && reinterpret_cast<uintptr_t>(ranks) % 4 != 0) return fail(HY_ERR_INVALID, "hy_string_dictionary_ranks: ranks not on a 4-byte boundary");
  const uint64_t total = left->entry_offsets[left->n_chunks];
  if (!total) return HY_OK;
  hipStream_t stream = current_stream();
  if (mem == HY_MEM_DEVICE) return string_order_launch(left, right, ranks, stream);   // (complete in the order of the calling thread's stream)
  Scratch& sc = scratch();
  HY_TRY(sc.reserve(4 * total + 4096));
  int32_t* d_ranks = carve<int32_t>(sc, total);
  if (!d_ranks) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
  HY_TRY(string_order_launch(left, right, d_ranks, stream));
  HY_HIP(hipMemcpyAsync(ranks, d_ranks, 4 * total, hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));
  return HY_OK;
}

}  // extern "C"

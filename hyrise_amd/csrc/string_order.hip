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
#include "string_entries.hpp"

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

// ---- one column's global string order (hy_string_dictionary_order) ----------------------------------------------------------------------
// Every chunk's dictionary is a sorted run already: the runs are merged pairwise in ceil(log2(n_chunks)) rounds, rank-based.  An element
// is a packed word (chunk << 32 | value id); position p of a buffer is entry_offsets[c] + v for the (c, v) that lies there before round 0
// (order_identity).  In round r a run is 2^r consecutive chunks, and the merged pair takes exactly the positions its two runs had, so every
// boundary comes from entry_offsets.  A workgroup owns the 256 positions of one LikeBlock, a lane one position: it reads its element,
// binary-searches the sibling run (lower_bound for an element of the left run, upper_bound for one of the right: equal strings keep the
// left one first) and stores the element at its merged position in the other buffer -- one plain 8-byte store, no atomics, no LDS, nothing
// that depends on lane order.  A run without a sibling finds an empty one and stays where it is.
// Then: a head flag per position (the element differs from its predecessor), counted inclusively inside a workgroup's 256 positions
// (order_heads), the workgroups' totals scanned by one workgroup (scan_tiles, string_entries.hpp), and rank = heads at or before the position - 1
// scattered to ranks[entry_offsets[c] + v] (order_scatter).
// Robustness: an element read from a buffer is clamped to a chunk and an entry that exist, offsets to the chunk's bytes; merged positions
// are run begin + own index + a count of at most the sibling's length, so they stay inside the pair.  Dictionaries that are not sorted
// leave positions unwritten and others written twice: unspecified ranks, nothing outside the buffers, no loop whose length is data.
constexpr uint32_t ORDER_WG = 256;       // = LIKE_WG: the block table is the matcher's

struct OrderArgs {
  const LikeChunk* chunks;
  const LikeBlock* blocks;
  const uint64_t* entry_offsets;    // [n_chunks + 1]
  uint32_t n_chunks;
  const EntryWindow* windows;       // [entry_offsets[n_chunks]]: what of every entry is compared, or nullptr: all of it
  uint64_t run_positions;           // 0: round 0 merges whole chunks (each one a sorted run); else single positions (windows that do not ascend)
  // The positions: entry_offsets[c] + v of the dictionary's entries (table == nullptr: run_offsets == entry_offsets, a workgroup owns a LikeBlock),
  // or -- the sparse route of string_gather.hip -- the n_positions entries of a table, chunk c's run at [run_offsets[c], run_offsets[c + 1]),
  // a workgroup owning 256 consecutive positions; an element is then the entry's index into the table.
  const SubsetEntry* table;
  const uint64_t* run_offsets;      // [n_chunks + 1]
  uint64_t n_positions;
};

__device__ __forceinline__ Entry element_entry(const OrderArgs& a, uint64_t element) {
  if (a.table) return entry_of(a.table[min(element, a.n_positions - 1)]);
  const uint32_t c = min(static_cast<uint32_t>(element >> 32), a.n_chunks - 1);
  const LikeChunk chunk = a.chunks[c];
  if (chunk.n_entries == 0) return Entry{nullptr, 0};
  return entry_of(chunk, min(static_cast<uint32_t>(element), chunk.n_entries - 1), chunk_bytes(chunk), a.windows ? a.windows + a.entry_offsets[c] : nullptr);
}

// The position a lane owns, the chunk whose run it lies in and the element that lies there before round 0; false: the lane has none
__device__ __forceinline__ bool own_position(const OrderArgs& a, uint64_t* position, uint32_t* chunk, uint64_t* element) {
  if (a.table) {
    const uint64_t p = uint64_t{blockIdx.x} * ORDER_WG + threadIdx.x;
    if (p >= a.n_positions) return false;
    *position = *element = p;
    *chunk = last_at_or_below(a.run_offsets, a.n_chunks, p);   // (of equal offsets the last: the chunk that has the position)
    return true;
  }
  const LikeBlock block = a.blocks[blockIdx.x];
  const uint32_t v = block.first_entry + threadIdx.x;
  if (v >= a.chunks[block.chunk].n_entries) return false;
  *position = a.entry_offsets[block.chunk] + v;
  *chunk = block.chunk;
  *element = uint64_t{block.chunk} << 32 | v;
  return true;
}

__global__ __launch_bounds__(ORDER_WG) void order_identity(OrderArgs a, uint64_t* elements) {
  uint64_t position, element;
  uint32_t chunk;
  if (own_position(a, &position, &chunk, &element)) elements[position] = element;
}

__global__ __launch_bounds__(ORDER_WG) void order_merge(OrderArgs a, const uint64_t* in, uint64_t* out, uint32_t round) {
  uint64_t position, identity;
  uint32_t chunk;
  if (!own_position(a, &position, &chunk, &identity)) return;
  // the pair of runs the position lies in: chunks [first, middle) and [middle, last)
  const uint64_t run = uint64_t{1} << round;
  uint64_t left_begin, right_begin, right_end;
  if (a.run_positions) {   // runs of 2^round positions
    const uint64_t total = a.run_offsets[a.n_chunks];
    left_begin = position >> (round + 1) << (round + 1);
    right_begin = min(left_begin + run, total);
    right_end = min(left_begin + 2 * run, total);
  } else {
    const uint64_t first = (chunk >> round & ~1u) * run;
    const uint64_t middle = min(first + run, uint64_t{a.n_chunks}), last = min(first + 2 * run, uint64_t{a.n_chunks});
    left_begin = a.run_offsets[first], right_begin = a.run_offsets[middle], right_end = a.run_offsets[last];
  }
  const uint64_t element = in[position];
  const Entry mine = element_entry(a, element);
  const bool in_left = position < right_begin;
  // left: the sibling's entries < mine; right: the sibling's entries <= mine
  uint64_t lo = in_left ? right_begin : left_begin, hi = in_left ? right_end : right_begin;
  const uint64_t sibling_begin = lo;
  while (lo < hi) {
    const uint64_t at = lo + (hi - lo) / 2;
    const int order = compare_entries(element_entry(a, in[at]), mine);
    if (in_left ? order < 0 : order <= 0) lo = at + 1;
    else hi = at;
  }
  const uint64_t own = position - (in_left ? left_begin : right_begin);
  out[left_begin + own + (lo - sibling_begin)] = element;
}

// local[p] = heads among the positions of p's workgroup up to and including p; tile_heads[workgroup] = its heads
__global__ __launch_bounds__(ORDER_WG) void order_heads(OrderArgs a, const uint64_t* sorted, uint64_t n, uint32_t* local, uint32_t* tile_heads) {
  __shared__ uint32_t s_wave_heads[ORDER_WG / 64];
  const uint64_t p = uint64_t{blockIdx.x} * ORDER_WG + threadIdx.x;
  bool head = false;
  if (p < n) head = p == 0 || compare_entries(element_entry(a, sorted[p - 1]), element_entry(a, sorted[p])) != 0;
  const uint64_t ballot = __ballot(head);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave_heads[wave] = __popcll(ballot);
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += s_wave_heads[w];
  if (p < n) local[p] = before + __popcll(ballot & (~0ull >> (63 - lane)));
  if (threadIdx.x == ORDER_WG - 1) tile_heads[blockIdx.x] = before + s_wave_heads[wave];
}

// (split: the joint order of two dictionaries, below -- a position at or behind it is an entry of the right one and goes to right_ranks)
__global__ __launch_bounds__(ORDER_WG) void order_scatter(OrderArgs a, const uint64_t* sorted, uint64_t n, const uint32_t* local, const uint32_t* tile_heads, int32_t* ranks,
                                                          int32_t* right_ranks, uint64_t split) {
  const uint64_t p = uint64_t{blockIdx.x} * ORDER_WG + threadIdx.x;
  if (p >= n) return;
  const uint64_t element = sorted[p];
  if (a.table) {   // ranks by table index
    ranks[min(element, a.n_positions - 1)] = static_cast<int32_t>(tile_heads[blockIdx.x] + local[p] - 1);
    return;
  }
  const uint32_t c = min(static_cast<uint32_t>(element >> 32), a.n_chunks - 1);
  const uint32_t n_entries = a.chunks[c].n_entries;
  if (n_entries == 0) return;
  const uint32_t v = min(static_cast<uint32_t>(element), n_entries - 1);
  const uint64_t position = a.entry_offsets[c] + v;
  const int32_t rank = static_cast<int32_t>(tile_heads[blockIdx.x] + local[p] - 1);   // (position 0 is a head: never below 0)
  if (position >= split) right_ranks[position - split] = rank;
  else ranks[position] = rank;
}

}  // namespace

// The merge sequence's temporaries for `total` positions: two buffers of elements (the one the last round read then holds the tile-local head
// counts), the tiles' heads and the number of distinct strings.
void merge_layout(Carver& carver, uint64_t total, MergeBlocks& blocks) {
  blocks.ping = carver.take<uint64_t>(total);
  blocks.pong = carver.take<uint64_t>(total);
  blocks.tile_heads = carver.take<uint32_t>((total + ORDER_WG - 1) / ORDER_WG);
  blocks.n_distinct = carver.take<uint32_t>(1);
}

// The launch sequence, once, for its three callers: identity, the merge rounds over `n_runs` runs, heads, the scan of the tiles' heads, the
// scatter (positions at or behind `split` to d_right_ranks).  `merge_workgroups`: what order_identity and order_merge are launched with (a
// block table's size, or the tiles of a table of entries); a.n_positions > 0.
static hy_status order_sequence(const OrderArgs& a, uint32_t merge_workgroups, uint64_t n_runs, const MergeBlocks& blocks, int32_t* d_ranks, int32_t* d_right_ranks, uint64_t split,
                                hipStream_t stream) {
  const uint64_t total = a.n_positions;
  const uint32_t n_tiles = static_cast<uint32_t>((total + ORDER_WG - 1) / ORDER_WG);
  uint64_t* ping = blocks.ping;
  uint64_t* pong = blocks.pong;
  profile_begin(stream, HY_KERNEL_STRING_RANK);
  hipLaunchKernelGGL(order_identity, dim3(merge_workgroups), dim3(ORDER_WG), 0, stream, a, ping);
  for (uint32_t round = 0; (uint64_t{1} << round) < n_runs; ++round) {
    hipLaunchKernelGGL(order_merge, dim3(merge_workgroups), dim3(ORDER_WG), 0, stream, a, ping, pong, round);
    std::swap(ping, pong);
  }
  uint32_t* local = reinterpret_cast<uint32_t*>(pong);   // (the buffer the last round read: free again)
  hipLaunchKernelGGL(order_heads, dim3(n_tiles), dim3(ORDER_WG), 0, stream, a, ping, total, local, blocks.tile_heads);
  hipLaunchKernelGGL(scan_tiles<uint32_t>, dim3(1), dim3(SCAN_WG), 0, stream, blocks.tile_heads, n_tiles, blocks.n_distinct);
  hipLaunchKernelGGL(order_scatter, dim3(n_tiles), dim3(ORDER_WG), 0, stream, a, ping, total, local, blocks.tile_heads, d_ranks, d_right_ranks, split);
  profile_end(stream);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

// Queues the whole sequence on `stream`: d_ranks[entry_offsets[c] + v] and *blocks.n_distinct.  total = entry_offsets[n_chunks] > 0.
hy_status column_order_launch(const hy_string_dictionary* dict, const MergeBlocks& blocks, int32_t* d_ranks, hipStream_t stream, const EntryWindow* d_windows, bool sorted_chunks) {
  HY_TRY(like_dictionary_tables(dict));
  const uint64_t total = dict->entry_offsets[dict->n_chunks];
  const bool by_position = d_windows && !sorted_chunks;
  const OrderArgs args{dict->d_chunks, dict->d_blocks, dict->d_entry_offsets, dict->n_chunks, d_windows, by_position ? 1u : 0u, nullptr, dict->d_entry_offsets, total};
  return order_sequence(args, static_cast<uint32_t>(dict->blocks.size()), by_position ? total : dict->n_chunks, blocks, d_ranks, nullptr, ~0ull, stream);
}

// The same sequence over a table of entries (the sparse route of string_gather.hip): `total` > 0 positions, 256 per workgroup
hy_status table_order_launch(const SubsetEntry* d_table, const uint64_t* d_run_offsets, uint32_t n_chunks, uint64_t total, bool by_position, const MergeBlocks& blocks, int32_t* d_ranks,
                             hipStream_t stream) {
  const OrderArgs args{nullptr, nullptr, nullptr, n_chunks, nullptr, by_position ? 1u : 0u, d_table, d_run_offsets, total};
  return order_sequence(args, static_cast<uint32_t>((total + ORDER_WG - 1) / ORDER_WG), by_position ? total : n_chunks, blocks, d_ranks, nullptr, ~0ull, stream);
}

// The same sequence over the chunks of TWO dictionaries laid end to end (string_join_keys.hip builds the tables): left's chunks are runs
// 0 .. n_l - 1, right's follow, so equal strings of either side get one rank.  Positions below t.split are left's entries and go to
// d_left_ranks, the others to d_right_ranks[position - split].  t.total > 0.
hy_status pair_order_launch(const PairTables& t, const MergeBlocks& blocks, int32_t* d_left_ranks, int32_t* d_right_ranks, hipStream_t stream) {
  const OrderArgs args{t.chunks, t.blocks, t.entry_offsets, t.n_chunks, nullptr, 0u, nullptr, t.entry_offsets, t.total};
  return order_sequence(args, t.n_blocks, t.n_chunks, blocks, d_left_ranks, d_right_ranks, t.split, stream);
}

// ---- the refusals, before any launch and any allocation -----------------------------------------------------------------------------------
hy_status dictionary_device_check(const hy_string_dictionary* dict, const char* entry_point) {
  if (dict->device == this_thread_device()) return HY_OK;
  return fail(HY_ERR_INVALID, "%s: the dictionary lives on device %d, the calling thread works on device %d", entry_point, dict->device, this_thread_device());
}

hy_status entries_fit_ranks(uint64_t total, const char* entry_point) {
  if (total < (uint64_t{1} << 31)) return HY_OK;
  return fail(HY_ERR_UNSUPPORTED, "%s: %llu dictionary entries do not fit int32 ranks", entry_point, static_cast<unsigned long long>(total));
}

hy_status column_order_check(const hy_string_dictionary* dict, const char* entry_point) {
  HY_TRY(dictionary_device_check(dict, entry_point));
  return entries_fit_ranks(dict->entry_offsets[dict->n_chunks], entry_point);
}

hy_status string_column_check(const hy_column* column, const hy_string_dictionary* dict, const char* entry_point) {
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->data_type != HY_TYPE_STRING && column->n_chunks)) return fail(HY_ERR_INVALID, "%s: not a string column (type %u)", entry_point, column->data_type);
  HY_TRY(check_dictionary(dict, column, "", entry_point));
  return column_order_check(dict, entry_point);
}

hy_status string_order_check(const hy_string_dictionary* left, const hy_string_dictionary* right, const char* entry_point) {
  if (left->n_chunks != right->n_chunks) return fail(HY_ERR_INVALID, "%s: the left dictionary has %u chunks, the right one %u", entry_point, left->n_chunks, right->n_chunks);
  if (left->device != right->device) return fail(HY_ERR_INVALID, "%s: the left dictionary lives on device %d, the right one on device %d", entry_point, left->device, right->device);
  HY_TRY(dictionary_device_check(left, entry_point));
  for (uint32_t c = 0; c < right->n_chunks; ++c) {
    if (right->chunks[c].n_entries >= (1u << 30)) return fail(HY_ERR_UNSUPPORTED, "%s: chunk %u: a right dictionary of %u entries does not fit int32 ranks (2 * lo)", entry_point, c, right->chunks[c].n_entries);
  }
  return HY_OK;
}

hy_status outputs_to_caller(uint32_t mem, const TwinPart* parts, uint32_t n_parts, const uint32_t* d_n_distinct, uint32_t* n_distinct, hipStream_t stream) {
  for (uint32_t p = 0; mem == HY_MEM_HOST && p < n_parts; ++p)
    if (parts[p].bytes) HY_HIP(hipMemcpyAsync(parts[p].host, parts[p].device, parts[p].bytes, hipMemcpyDeviceToHost, stream));
  if (n_distinct) HY_HIP(hipMemcpyAsync(n_distinct, d_n_distinct, 4, hipMemcpyDeviceToHost, stream));
  if (mem == HY_MEM_HOST || n_distinct) HY_HIP(hipStreamSynchronize(stream));
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

// The int32 stand-in of a string column (a data column, or a reference column over one) over a table of E int32_t in device memory: entry v
// of data chunk c reads table[entry_offsets[c] + v].  (data_type HY_TYPE_LONG: a table of E int64_t and an int64 stand-in, string_join_keys.hip.)  The data stand-in has DictionarySegment<int32> chunks over the caller's attribute
// vectors, whatever their width or packing, with the NULL value id still aux_size; a reference column gets the same PosLists over it, and
// owns it (hy_column::stand_in).  The table stays the caller's.
hy_status string_stand_in(const hy_column* column, const hy_string_dictionary* dict, void* d_table, hy_column** out, uint32_t data_type) {
  *out = nullptr;
  const hy_column* data_column = column->is_reference ? column->ref : column;
  const uint32_t n_data_chunks = data_column->n_chunks;
  std::vector<hy_segment> segments(data_column->host_segments);
  for (uint32_t c = 0; c < n_data_chunks; ++c) {
    segments[c].data_type = data_type;
    segments[c].aux = static_cast<char*>(d_table) + (data_type == HY_TYPE_LONG ? 8 : 4) * dict->entry_offsets[c];
  }
  hy_column* stand_in = nullptr;
  HY_TRY(hy_column_create(segments.data(), n_data_chunks, HY_MEM_DEVICE, &stand_in));
  hy_column* result = stand_in;
  if (column->is_reference) {   // the same PosLists over the stand-in
    segments = column->host_segments;
    for (hy_segment& segment : segments) {
      segment.data_type = data_type;
      segment.ref = stand_in;
      // (an uploaded PosList without rows has no device buffer: as a descriptor over device memory it reads as an entire-chunk list, whose
      // chunk id must exist -- of no rows, so which chunk does not matter)
      if (!segment.data && !segment.size && n_data_chunks && segment.ref_chunk_id >= n_data_chunks) segment.ref_chunk_id = 0;
    }
    const hy_status status = hy_column_create(segments.data(), column->n_chunks, HY_MEM_DEVICE, &result);
    if (status != HY_OK) {
      (void)hy_column_destroy(stand_in);
      return status;
    }
    result->stand_in = stand_in;
  }
  *out = result;
  return HY_OK;
}

hy_status KeyColumn::alloc(size_t bytes) {
  HY_HIP(hipMalloc(&d_keys, bytes));
  return HY_OK;
}

hy_status KeyColumn::make_stand_in(const hy_column* column, const hy_string_dictionary* dict, uint32_t data_type) {
  HY_TRY(string_stand_in(column, dict, d_keys, &stand_in, data_type));
  (stand_in->stand_in ? stand_in->stand_in : stand_in)->owned.push_back(d_keys);
  return HY_OK;
}

void KeyColumn::drop() {
  if (stand_in) (void)hy_column_destroy(stand_in);
  else if (d_keys) (void)hipFree(d_keys);
  stand_in = nullptr;
  d_keys = nullptr;
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
  int32_t* d_ranks = ranks;
  if (mem == HY_MEM_HOST) HY_TRY(reserve_and_carve([&](Carver& carver) { d_ranks = carver.take<int32_t>(total); }));   // the twin
  HY_TRY(string_order_launch(left, right, d_ranks, stream));
  const TwinPart part{ranks, d_ranks, 4 * total};
  return outputs_to_caller(mem, &part, 1, nullptr, nullptr, stream);
}

hy_status hy_string_dictionary_order(const hy_string_dictionary* dict, uint32_t mem, int32_t* ranks, uint32_t* n_distinct) {
  const char* name = "hy_string_dictionary_order";
  if (!dict || !ranks) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (mem != HY_MEM_HOST && mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "%s: bad memory space %u", name, mem);
  HY_TRY(column_order_check(dict, name));
  if (mem == HY_MEM_DEVICE && reinterpret_cast<uintptr_t>(ranks) % 4 != 0) return fail(HY_ERR_INVALID, "%s: ranks not on a 4-byte boundary", name);
  const uint64_t total = dict->entry_offsets[dict->n_chunks];
  if (!total) {
    if (n_distinct) *n_distinct = 0;
    return HY_OK;
  }
  hipStream_t stream = current_stream();
  MergeBlocks merge;
  int32_t* d_ranks = ranks;
  HY_TRY(reserve_and_carve([&](Carver& carver) {
    if (mem == HY_MEM_HOST) d_ranks = carver.take<int32_t>(total);   // the twin
    merge_layout(carver, total, merge);
  }));
  HY_TRY(column_order_launch(dict, merge, d_ranks, stream));
  const TwinPart part{ranks, d_ranks, 4 * total};
  return outputs_to_caller(mem, &part, 1, merge.n_distinct, n_distinct, stream);
}

hy_status hy_column_string_ranks(const hy_column* column, const hy_string_dictionary* dict, hy_column** out) {
  const char* name = "hy_column_string_ranks";
  if (!out) return fail(HY_ERR_INVALID, "%s: null output", name);
  *out = nullptr;
  if (!column || !dict) return fail(HY_ERR_INVALID, "%s: null argument", name);
  HY_TRY(string_column_check(column, dict, name));
  const uint64_t total = dict->entry_offsets[dict->n_chunks];

  // the ranks: a buffer the stand-in owns (16 bytes of slack behind the last rank, like every dictionary of a column)
  hipStream_t stream = current_stream();
  KeyColumn keys;
  HY_TRY(keys.alloc(align_up(4 * total + 16, 256)));
  auto give_up = [&](hy_status status) {
    (void)hipStreamSynchronize(stream);
    keys.drop();
    return status;
  };
  if (total) {
    MergeBlocks merge;
    hy_status status = reserve_and_carve([&](Carver& carver) { merge_layout(carver, total, merge); });
    if (status == HY_OK) status = column_order_launch(dict, merge, static_cast<int32_t*>(keys.d_keys), stream);
    if (status != HY_OK) return give_up(status);
  }
  const hy_status status = keys.make_stand_in(column, dict, HY_TYPE_INT);
  if (status != HY_OK) return give_up(status);
  // (the dictionary may die as soon as the call has returned: nothing queued reads it any more)
  const hipError_t err = hipStreamSynchronize(stream);
  if (err != hipSuccess) return give_up(fail(HY_ERR_DEVICE, "%s: ranking failed: %s", name, hipGetErrorString(err)));
  *out = keys.stand_in;
  return HY_OK;
}

}  // extern "C"

// string_substr.hip -- SUBSTR(column, start, length) over a dictionary-encoded string column (hy_string_column_substr), the result a new
// dictionary-encoded string column in HBM: the pair hy_string_column_gather documents, in the input column's own chunk layout.
//
// The substring of a dictionary entry is a WINDOW into chars that are in HBM already -- a byte begin and a byte length, 8 bytes per source
// entry -- and no intermediate string is ever written:
//   1  entry_windows, one launch over the source dictionary (a workgroup owns the 256 entries of one LikeBlock, a lane one entry): the entry's
//      length n (an offsets difference, or strnlen of a fixed slot read four bytes at a time where the slot is aligned), then the reference's
//      _evaluate_substring (expression_evaluator.cpp:1597-1638) in 64-bit arithmetic:
//        length <= 0: ""      start < 0: s = start + n      start == 0: s = 0, length - 1      start > 0: s = start - 1
//        e = min(s + length, n), s = max(s, 0); bytes [s, e) when s < n and e > s, else ""
//   2  the windowed entries ranked by hy_string_dictionary_order's launches (column_order_launch with the windows): equal substrings get one
//      rank, whichever source entries or chunks they came from.  A window that begins at the entry's first byte (start 0 or 1, or an empty
//      result) keeps every chunk's entries ascending, and the merge starts from whole chunks as it does for the entries themselves; any other
//      window does not, and the merge starts from single entries (log2(E) rounds, not log2(chunks));
//   3  every row's global source entry, or -1 for a NULL row: the column's int32 stand-in over the table 0, 1, 2, ... exported once
//      (string_stand_in: attribute vectors of any width or packing, PosLists in either memory space read in place);
//   4  gather_entries (string_gather.hip) with the windows: rows ordered by (output chunk, rank), head flags, prefix sums, offsets and the
//      byte-parallel copy, whose source is the window's first byte -- at any byte address, as the copy has always read.
// Temporaries: string_gather.hip's, plus 8 bytes per source entry for the windows (scratch arena).  The host side is string_gather.hip's
// request (string_request, string_request_run): this file holds the two kernels that only these entry points launch.
#include "hy_device.hpp"
#include "sort_words.hpp"
#include "string_entries.hpp"

#include <algorithm>

namespace hy {

namespace {

constexpr uint32_t WG = 256;   // = like.hip's LIKE_WG: the block table is the matcher's

__global__ __launch_bounds__(WG) void entry_windows(const LikeChunk* chunks, const LikeBlock* blocks, const uint64_t* entry_offsets, int32_t start, int32_t length, EntryWindow* windows) {
  const LikeBlock block = blocks[blockIdx.x];
  const LikeChunk chunk = chunks[block.chunk];
  const uint32_t v = block.first_entry + threadIdx.x;
  if (v >= chunk.n_entries) return;
  uint32_t n;
  if (chunk.offsets) {   // (clamped as entry_of clamps: the window stays inside the chunk's bytes)
    const uint32_t end = chunk_bytes(chunk);
    const uint32_t from = min(chunk.offsets[v], end);
    n = min(max(chunk.offsets[v + 1], from), end) - from;
  } else {
    n = slot_length(reinterpret_cast<const uint8_t*>(chunk.chars) + size_t{v} * chunk.string_length, chunk.string_length);
  }
  windows[entry_offsets[block.chunk] + v] = substr_window(n, start, length);
}

// values / nulls: the stand-in over the table 0, 1, 2, ..., exported
__global__ __launch_bounds__(WG) void entries_of_rows(const int32_t* values, const uint8_t* nulls, uint32_t n, uint32_t n_source_entries, int32_t* entry) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) entry[i] = (!nulls[i] && static_cast<uint32_t>(values[i]) < n_source_entries) ? values[i] : -1;
}

}  // namespace

void entry_windows_launch(const hy_string_dictionary* dict, const SubstrArguments& substr, EntryWindow* d_windows, hipStream_t stream) {
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the windows: a bracket of their own)
  hipLaunchKernelGGL(entry_windows, dim3(static_cast<uint32_t>(dict->blocks.size())), dim3(WG), 0, stream, dict->d_chunks, dict->d_blocks, dict->d_entry_offsets, substr.start, substr.length,
                     d_windows);
  profile_end(stream);
}

void entries_of_rows_launch(const int32_t* values, const uint8_t* nulls, uint64_t n, uint64_t n_source_entries, int32_t* d_entry, hipStream_t stream) {
  hipLaunchKernelGGL(entries_of_rows, dim3(grid_for(n)), dim3(WG), 0, stream, values, nulls, static_cast<uint32_t>(n), static_cast<uint32_t>(n_source_entries), d_entry);
}

// The rows of `column` themselves as a new string column in its own chunk layout, every entry seen through SUBSTR's window (`substr`) or
// whole (nullptr): hy_string_column_substr and hy_string_column_materialize.
static hy_status column_rows_strings(const hy_column* column, const hy_string_dictionary* dict, const SubstrArguments* substr, const char* name, hy_column** result,
                                     hy_string_dictionary** result_dict) {
  StringRequest request;
  bool answered = false;
  HY_TRY(string_request(StringRoute::ColumnRows, name, column, dict, nullptr, 0, 0, substr, result, result_dict, &request, &answered));
  return answered ? HY_OK : string_request_run(request);
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_string_column_substr(const hy_column* column, const hy_string_dictionary* dict, int32_t start, int32_t length, hy_column** result, hy_string_dictionary** result_dict) {
  const SubstrArguments substr{start, length};
  return column_rows_strings(column, dict, &substr, "hy_string_column_substr", result, result_dict);
}

hy_status hy_string_column_materialize(const hy_column* column, const hy_string_dictionary* dict, hy_column** result, hy_string_dictionary** result_dict) {
  return column_rows_strings(column, dict, nullptr, "hy_string_column_materialize", result, result_dict);
}

}  // extern "C"

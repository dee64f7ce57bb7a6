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
// Temporaries: string_gather.hip's, plus 8 bytes per source entry for the windows (scratch arena).
#include "hy_device.hpp"
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

__global__ __launch_bounds__(WG) void iota_entries(int32_t* table, uint32_t n) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) table[i] = static_cast<int32_t>(i);
}

uint32_t grid_of(uint64_t items) { return static_cast<uint32_t>(std::min<uint64_t>((items + WG - 1) / WG, 4096)); }

struct ColumnGuard {
  hy_column* column = nullptr;
  ~ColumnGuard() { if (column) (void)hy_column_destroy(column); }
};

// The rows of `column` themselves as a new string column in its own chunk layout, every entry seen through SUBSTR's window (`substr`) or
// whole (nullptr): hy_string_column_substr and hy_string_column_materialize.
hy_status column_rows_strings(const hy_column* column, const hy_string_dictionary* dict, const SubstrArguments* substr, const char* name, hy_column** result,
                              hy_string_dictionary** result_dict) {
  const int32_t start = substr ? substr->start : 1, length = substr ? substr->length : 0;
  if (result) *result = nullptr;
  if (result_dict) *result_dict = nullptr;
  if (!result || !result_dict || !column || !dict) return fail(HY_ERR_INVALID, "%s: null argument", name);
  HY_TRY(string_column_check(column, dict, name));
  if (column->rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows (32-bit row ids)", name, static_cast<unsigned long long>(column->rows));
  if (!column->n_chunks) return empty_string_results(result, result_dict);
  OutChunks out;
  out.n = column->rows;
  for (const hy_segment& segment : column->host_segments) out.sizes.push_back(segment.size);

  hipStream_t stream = current_stream();
  const uint64_t n = column->rows, n_source_entries = dict->entry_offsets[dict->n_chunks];
  if (string_sparse_route(n, n, n_source_entries)) {   // few rows against the dictionary: the column read row by row, the entries they reference windowed and ranked
    DeviceBuffer entry;
    HY_TRY(entry.alloc(4 * n + 16));
    Scratch& sc = scratch();
    HY_TRY(sc.reserve(sparse_gather_scratch_bytes(n_source_entries, dict->n_chunks, n, out.sizes.size())));
    HY_TRY(like_dictionary_tables(dict));
    SparseSubset subset;
    hy_status st = HY_OK;
    if (n) st = sparse_entries(column, dict, nullptr, n, substr, sc, entry.as<int32_t>(), stream, name, &subset);
    if (st == HY_OK) st = gather_entries(dict, out, entry.as<int32_t>(), subset.ranks, nullptr, sc, stream, name, result, result_dict, &subset);
    (void)hipStreamSynchronize(stream);   // (the temporaries go back to the pool)
    return st;
  }
  DeviceBuffer table, values, nulls, entry;
  ColumnGuard stand_in;
  HY_TRY(table.alloc(4 * n_source_entries + 16));
  HY_TRY(values.alloc(4 * n + 16));
  HY_TRY(nulls.alloc(n + 16));
  HY_TRY(entry.alloc(4 * n + 16));
  Scratch& sc = scratch();
  HY_TRY(sc.reserve(gather_scratch_bytes(n_source_entries, n, out.sizes.size(), false) + (substr ? align_up(sizeof(EntryWindow) * n_source_entries + 16, 256) : 0)));
  HY_TRY(like_dictionary_tables(dict));
  int32_t* d_ranks = nullptr;
  EntryWindow* d_windows = nullptr;
  if (n_source_entries) {
    d_ranks = carve<int32_t>(sc, n_source_entries);
    if (!d_ranks) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
    if (substr) {
      d_windows = carve<EntryWindow>(sc, n_source_entries);
      if (!d_windows) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
      profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the windows: a bracket of their own)
      hipLaunchKernelGGL(entry_windows, dim3(static_cast<uint32_t>(dict->blocks.size())), dim3(WG), 0, stream, dict->d_chunks, dict->d_blocks, dict->d_entry_offsets, start, length, d_windows);
      profile_end(stream);
    }
    uint32_t* d_n_distinct = nullptr;
    // a window at the entry's first byte keeps a sorted dictionary sorted
    const hy_status ranked = column_order_launch(dict, sc, d_ranks, &d_n_distinct, stream, d_windows, !substr || length <= 0 || start == 0 || start == 1);
    if (ranked != HY_OK) {   // (launches may be queued: the temporaries go back to the pool behind them)
      (void)hipStreamSynchronize(stream);
      return ranked;
    }
  }
  hy_status st = string_stand_in(column, dict, table.as<int32_t>(), &stand_in.column);
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  if (st == HY_OK && n_source_entries) hipLaunchKernelGGL(iota_entries, dim3(grid_of(n_source_entries)), dim3(WG), 0, stream, table.as<int32_t>(), static_cast<uint32_t>(n_source_entries));
  if (st == HY_OK && n) {
    st = export_column_at(stand_in.column, values.ptr, nulls.as<uint8_t>(), nullptr);
    if (st == HY_OK)
      hipLaunchKernelGGL(entries_of_rows, dim3(grid_of(n)), dim3(WG), 0, stream, values.as<int32_t>(), nulls.as<uint8_t>(), static_cast<uint32_t>(n), static_cast<uint32_t>(n_source_entries),
                         entry.as<int32_t>());
  }
  profile_end(stream);
  if (st == HY_OK) st = gather_entries(dict, out, entry.as<int32_t>(), d_ranks, d_windows, sc, stream, name, result, result_dict);
  (void)hipStreamSynchronize(stream);   // (the temporaries go back to the pool, the stand-in dies)
  return st;
}

}  // namespace

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

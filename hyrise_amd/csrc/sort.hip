// sort.hip -- Sort (operators/sort.cpp:287-516) on the device: one stable lexicographic sort of a table's rows by several columns, and the
// gather that materialises a column in that order (write_materialized_output_table, sort.cpp:58-150).
//
// sort.cpp applies the sort definitions from the last to the first, each one a stable sort of the order the previous ones left; NULLs go
// first in both directions and keep their order among themselves (:435-443).  Here every definition becomes one to three 32-bit words --
// the low and high half of an order-preserving unsigned key (integers: sign bit flipped; floats: the sign-flip transform after -0.0 is
// made +0.0, so that std::less ties stay ties; descending: all bits inverted), then a 1-bit "is not NULL" word -- and every word is one
// stable LSD radix sort of (word, row) pairs by sort_pairs_u32 (join.hip), least significant word first.  A word whose value is the same
// in every row is skipped (a reduction over the exported column decides it), and a word sorts only the bits its range needs.
#include "hy_device.hpp"
#include "sort_words.hpp"
#include "sort_keys.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hy {

namespace {

// hy_column_gather: output row i = flat row row_base[p.chunk_id] + p.chunk_offset of the exported column, p = positions[i]; one wave per
// 64 rows of one output chunk, so that the wave's NULL flags are one word of the chunk's null vector (written by lane 0).
template <typename U>
__global__ __launch_bounds__(256) void gather_column_rows(const U* values, const uint8_t* nulls, const uint64_t* row_base, uint32_t n_chunks, const hy_row_id* positions,
                                                          uint64_t n, uint32_t chunk_rows, uint32_t words_per_chunk, uint64_t value_stride, uint64_t null_stride,
                                                          char* out_values, uint64_t* out_nulls, uint64_t groups) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t g = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) / 64; g < groups; g += static_cast<uint64_t>(gridDim.x) * 4) {
    const uint64_t chunk = g / words_per_chunk, word = g % words_per_chunk;
    const uint64_t chunk_begin = chunk * chunk_rows;
    const uint64_t rows_here = n - chunk_begin < chunk_rows ? n - chunk_begin : chunk_rows;
    const uint64_t offset = word * 64 + lane;
    bool is_null = false;
    if (offset < rows_here) {
      const hy_row_id p = positions[chunk_begin + offset];
      U value = 0;
      is_null = true;
      if (p.chunk_offset != 0xFFFFFFFFu && p.chunk_id < n_chunks && row_base[p.chunk_id] + p.chunk_offset < row_base[p.chunk_id + 1]) {
        const uint64_t row = row_base[p.chunk_id] + p.chunk_offset;
        is_null = nulls[row] != 0;
        value = is_null ? U{0} : values[row];
      }
      reinterpret_cast<U*>(out_values + chunk * value_stride)[offset] = value;
    }
    const uint64_t bits = __ballot(is_null);
    if (lane == 0) out_nulls[chunk * null_stride + word] = bits;
  }
}

// ---- Sort with a row limit: which rows can be among the first k ------------------------------------------------------------------------------
// Definition 0's key relative to the column's minima: (high word - its minimum) << lo_bits | (low word - its minimum), the words and bit counts
// that sort_word_stats / word_range give.  It orders the non-NULL rows as the two value words do and uses hi_bits + lo_bits bits.
struct SelectKey {
  uint32_t lo_min, hi_min, lo_bits;
  bool is_float, descending;
};

template <typename U>
__device__ __forceinline__ uint64_t select_key(U bits, const SelectKey& k) {
  const U key = order_key<U>(bits, k.is_float, k.descending);
  const uint64_t lo = static_cast<uint32_t>(key) - k.lo_min;
  if constexpr (sizeof(U) == 4) return lo;
  else return (static_cast<uint64_t>(static_cast<uint32_t>(key >> 31 >> 1) - k.hi_min) << k.lo_bits) | lo;
}

constexpr uint32_t SELECT_DIGIT_BITS = 11;
constexpr uint32_t SELECT_BINS = 1u << SELECT_DIGIT_BITS;   // 8 KiB of LDS per workgroup
constexpr uint32_t SELECT_HISTOGRAM_WGS = 256;              // of 1024 threads: 16 waves on every CU, and as many rows of bins to add up
constexpr uint32_t SELECT_TILE = SLICE_ROWS;                // rows per workgroup of select_mark / select_emit: 128 mask words
constexpr uint32_t SELECT_TILE_WORDS = SELECT_TILE / 64;

// One digit of the key -- (key >> shift) & digit_mask -- counted over the non-NULL rows, from the second level on only over the rows whose
// key >> prefix_shift is `prefix` (the bucket the threshold fell into).  Bins in LDS; a wave whose rows all fall into one bin (a long run of
// equal values, a refinement's dense cluster) adds them with one atomic.  The workgroup writes its bins as row blockIdx.x of `partial` with
// plain stores: select_sum_bins adds the rows up, so no workgroup touches another one's words.
template <typename U>
__global__ __launch_bounds__(1024) void select_histogram(const U* values, const uint8_t* nulls, uint32_t n, SelectKey key, bool filtered, uint32_t prefix_shift, uint64_t prefix,
                                                         uint32_t shift, uint32_t digit_mask, uint32_t* partial) {
  __shared__ uint32_t s_bins[SELECT_BINS];
  for (uint32_t b = threadIdx.x; b < SELECT_BINS; b += 1024) s_bins[b] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t base = uint64_t{blockIdx.x} * 1024; base < n; base += uint64_t{gridDim.x} * 1024) {   // (whole waves: the ballots below)
    const uint64_t i = base + threadIdx.x;
    bool counted = false;
    uint32_t digit = 0;
    if (i < n && !nulls[i]) {
      const uint64_t k = select_key<U>(values[i], key);
      if (!filtered || (k >> prefix_shift) == prefix) {
        counted = true;
        digit = static_cast<uint32_t>(k >> shift) & digit_mask;
      }
    }
    const uint64_t active = __ballot(counted);
    if (!active) continue;
    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(active))) - 1;
    const uint32_t leader_digit = static_cast<uint32_t>(__shfl(static_cast<int>(digit), static_cast<int>(leader)));
    if (__ballot(counted && digit == leader_digit) == active) {
      if (lane == leader) atomicAdd(&s_bins[digit], static_cast<uint32_t>(__popcll(active)));
    } else if (counted) {
      atomicAdd(&s_bins[digit], 1u);
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < SELECT_BINS; b += 1024) partial[size_t{blockIdx.x} * SELECT_BINS + b] = s_bins[b];
}

// totals[b] = the sum of bin b over the `rows` rows of `partial`; 64 bins per workgroup, a wave per quarter of the rows.  `totals` is pinned
// host memory: the host picks the bucket.
__global__ __launch_bounds__(256) void select_sum_bins(const uint32_t* partial, uint32_t rows, uint32_t* totals) {
  __shared__ uint32_t s_part[4][64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t bin = blockIdx.x * 64 + lane;
  uint32_t sum = 0;
  for (uint32_t r = wave; r < rows; r += 4) sum += partial[size_t{r} * SELECT_BINS + bin];
  s_part[wave][lane] = sum;
  __syncthreads();
  if (wave == 0) totals[bin] = s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane];
}

// A row is a candidate if it is NULL, or -- with_values -- if key >> shift <= threshold (below: certainly among the first k; equal: undecided,
// or a true tie once the bits have run out).  One workgroup per tile: bit l of masks[w] = row 64 w + l is a candidate, counts[tile] = how many.
template <typename U>
__global__ __launch_bounds__(256) void select_mark(const U* values, const uint8_t* nulls, uint32_t n, SelectKey key, bool with_values, uint32_t shift, uint64_t threshold,
                                                   uint64_t* masks, uint32_t* counts) {
  __shared__ uint32_t s_count[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t count = 0;
  for (uint32_t step = 0; step < SELECT_TILE_WORDS / 4; ++step) {
    const uint64_t word = uint64_t{blockIdx.x} * SELECT_TILE_WORDS + wave * (SELECT_TILE_WORDS / 4) + step;
    const uint64_t row = word * 64 + lane;
    bool candidate = false;
    if (row < n) candidate = nulls[row] ? true : (with_values && (select_key<U>(values[row], key) >> shift) <= threshold);
    const uint64_t mask = __ballot(candidate);
    if (lane == 0) masks[word] = mask;
    count += static_cast<uint32_t>(__popcll(mask));
  }
  if (lane == 0) s_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

// The candidates' row numbers in ascending order: a wave takes a quarter of the tile's mask words, lane l of it word l's count (a wave scan
// gives every word its place), then word by word lane l writes row 64 w + l behind the candidates below it.
__global__ __launch_bounds__(256) void select_emit(const uint64_t* masks, const uint32_t* offsets, uint32_t* rows_out, uint32_t capacity) {
  __shared__ uint32_t s_wave[4];
  constexpr uint32_t WORDS = SELECT_TILE_WORDS / 4;   // per wave: 32
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first_word = uint64_t{blockIdx.x} * SELECT_TILE_WORDS + wave * WORDS;
  const uint32_t mine = lane < WORDS ? static_cast<uint32_t>(__popcll(masks[first_word + lane])) : 0;
  uint32_t scan = mine;   // inclusive over the wave
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan), step));
    if (lane >= step) scan += up;
  }
  if (lane == 63) s_wave[wave] = scan;
  __syncthreads();
  uint32_t at = offsets[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
  const uint32_t before = scan - mine;
  const uint64_t below = (uint64_t{1} << lane) - 1;
  for (uint32_t w = 0; w < WORDS; ++w) {
    const uint64_t mask = masks[first_word + w];
    if (!mask) continue;
    const uint32_t place = at + static_cast<uint32_t>(__shfl(static_cast<int>(before), static_cast<int>(w))) + static_cast<uint32_t>(__popcll(mask & below));
    if ((mask >> lane & 1) && place < capacity) rows_out[place] = static_cast<uint32_t>((first_word + w) * 64 + lane);
  }
}

bool numeric_type(uint32_t t) { return t >= HY_TYPE_INT && t <= HY_TYPE_DOUBLE; }

hy_status check_sortable(const hy_column* column, const char* entry_point) {
  if (!column) return fail(HY_ERR_INVALID, "%s: null column", entry_point);
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_INVALID, "MVCC columns are read by hy_validate only");
  if (!numeric_type(column->data_type)) return fail(HY_ERR_UNSUPPORTED, "%s: numeric columns only (a string column is passed as ranks)", entry_point);
  if (column->has_dictionary_without_values) return fail(HY_ERR_UNSUPPORTED, "%s: the dictionary values are not on the device", entry_point);
  return HY_OK;
}

// hy_sort's argument checks, word for word, under hy_sort_limit's name.
hy_status check_sort_keys(const hy_sort_key* keys, uint32_t n_keys, const char* entry_point) {
  for (uint32_t k = 0; k < n_keys; ++k) {
    HY_TRY(check_sortable(keys[k].column, entry_point));
    if (keys[k].mode != HY_SORT_ASCENDING_NULLS_FIRST && keys[k].mode != HY_SORT_DESCENDING_NULLS_FIRST)
      return fail(HY_ERR_INVALID, "%s: Sort does not support NULLS LAST (sort mode %u)", entry_point, keys[k].mode);
    const hy_column* a = keys[0].column;
    const hy_column* b = keys[k].column;
    bool same = a->n_chunks == b->n_chunks;
    for (uint32_t c = 0; same && c < a->n_chunks; ++c) same = a->host_segments[c].size == b->host_segments[c].size;
    if (!same) return fail(HY_ERR_INVALID, "%s: the sort columns do not belong to one table (chunk layouts differ)", entry_point);
  }
  if (keys[0].column->rows >= (uint64_t{1} << 32))
    return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows (32-bit row ids)", entry_point, static_cast<unsigned long long>(keys[0].column->rows));
  return HY_OK;
}

// Path 0: every row sorted by hy_sort into a temporary, the first k RowIDs copied out.
hy_status full_sort_and_cut(const hy_sort_key* keys, uint32_t n_keys, uint64_t rows, uint64_t k, hy_row_id* out) {
  DeviceBuffer sorted;
  HY_TRY(sorted.alloc(8 * rows + 16));
  uint64_t n_sorted = 0;
  HY_TRY(hy_sort(keys, n_keys, sorted.as<hy_row_id>(), rows, &n_sorted));
  hipStream_t stream = current_stream();
  HY_HIP(hipMemcpyAsync(out, sorted.ptr, 8 * k, hipMemcpyDeviceToDevice, stream));
  HY_HIP(hipStreamSynchronize(stream));
  return HY_OK;
}

// The default's switch-over: with flags == 0 the selection runs while the candidates are at most 1 / SELECT_SHARE_DIVISOR of the table.  A limit
// above the share goes straight to the full sort; a candidate set above it (heavy ties on definition 0) falls back after the histogram.
// PROVISIONAL: 1/4 comes from DESIGN.md section 4.7's byte model (40 B/row of selection in front of some 130 B per sorted candidate), not
// from a measurement -- tools/sort_limit_bench.py has not been run on the device yet (no profiles/sort_limit_bench.txt); set it from there.
constexpr uint64_t SELECT_SHARE_DIVISOR = 4;
// A bucket is refined on its next digits while it holds more than this share of the table: one more pass over the exported values (9 B/row)
// against sorting the bucket's rows (some 130 B/row by section 4.7's model).
constexpr uint64_t REFINE_SHARE_DIVISOR = 16;

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_sort(const hy_sort_key* keys, uint32_t n_keys, hy_row_id* out, uint64_t capacity, uint64_t* n_out) {
  if (!keys || !n_keys || !n_out) return fail(HY_ERR_INVALID, "hy_sort: null argument or no sort key");
  *n_out = 0;
  for (uint32_t k = 0; k < n_keys; ++k) {
    HY_TRY(check_sortable(keys[k].column, "hy_sort"));
    if (keys[k].mode != HY_SORT_ASCENDING_NULLS_FIRST && keys[k].mode != HY_SORT_DESCENDING_NULLS_FIRST)
      return fail(HY_ERR_INVALID, "hy_sort: Sort does not support NULLS LAST (sort mode %u)", keys[k].mode);
    const hy_column* a = keys[0].column;
    const hy_column* b = keys[k].column;
    bool same = a->n_chunks == b->n_chunks;
    for (uint32_t c = 0; same && c < a->n_chunks; ++c) same = a->host_segments[c].size == b->host_segments[c].size;
    if (!same) return fail(HY_ERR_INVALID, "hy_sort: the sort columns do not belong to one table (chunk layouts differ)");
  }
  const hy_column* shape = keys[0].column;
  const uint64_t rows = shape->rows;
  if (rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "hy_sort: %llu rows (32-bit row ids)", static_cast<unsigned long long>(rows));
  *n_out = rows;
  if (rows > capacity) return fail(HY_ERR_CAPACITY, "hy_sort: %llu rows, capacity %llu", static_cast<unsigned long long>(rows), static_cast<unsigned long long>(capacity));
  if (!rows) return HY_OK;
  if (!out) return fail(HY_ERR_INVALID, "hy_sort: null output");
  const uint32_t n = static_cast<uint32_t>(rows);
  hipStream_t stream = current_stream();

  DeviceBuffer values, nulls, stats_buffer;
  WordSort order;   // order.perm == nullptr: the identity (no word sorted yet)
  if (n > 1) {
    HY_TRY(order.alloc(n));
    HY_TRY(values.alloc(8 * size_t{n} + 16));
    HY_TRY(nulls.alloc(size_t{n} + 16));
    HY_TRY(stats_buffer.alloc(64));
  }
  for (uint32_t k = n > 1 ? n_keys : 0; k-- > 0;) {   // sort.cpp:322-336: the last definition first
    const hy_column* column = keys[k].column;
    const bool wide = column->data_type == HY_TYPE_LONG || column->data_type == HY_TYPE_DOUBLE;
    const bool is_float = column->data_type == HY_TYPE_FLOAT || column->data_type == HY_TYPE_DOUBLE;
    const bool descending = keys[k].mode == HY_SORT_DESCENDING_NULLS_FIRST;
    HY_TRY(export_column_at(column, values.ptr, nulls.as<uint8_t>(), nullptr));
    uint32_t* stats = stats_buffer.as<uint32_t>();
    HY_HIP(hipMemsetAsync(stats, 0xFF, 8, stream));
    HY_HIP(hipMemsetAsync(stats + 2, 0, 12, stream));
    const uint32_t stats_grid = std::min<uint32_t>(grid_for(n / 16), 1024);
    if (wide) hipLaunchKernelGGL(sort_word_stats<uint64_t>, dim3(stats_grid), dim3(256), 0, stream, values.as<uint64_t>(), nulls.as<uint8_t>(), n, is_float, descending, stats);
    else hipLaunchKernelGGL(sort_word_stats<uint32_t>, dim3(stats_grid), dim3(256), 0, stream, values.as<uint32_t>(), nulls.as<uint8_t>(), n, is_float, descending, stats);
    uint32_t s[5];
    HY_HIP(hipMemcpyAsync(s, stats, sizeof(s), hipMemcpyDeviceToHost, stream));
    HY_HIP(hipStreamSynchronize(stream));
    const uint32_t null_rows = s[4];
    for (uint32_t word = 0; word < 3; ++word) {
      uint32_t minimum = 0, bits = 1;
      if (word < 2) {
        if (word == 1 && !wide) continue;
        if (null_rows == n || !word_range(s[word], s[2 + word], &minimum, &bits)) continue;   // the same in every row: nothing to order
      } else if (null_rows == 0 || null_rows == n) {
        continue;
      }
      if (wide) hipLaunchKernelGGL(sort_gather_word<uint64_t>, dim3(grid_for(n / 4)), dim3(256), 0, stream, values.as<uint64_t>(), nulls.as<uint8_t>(), order.perm, order.key_words(), order.ids(), n, word, is_float, descending, minimum);
      else hipLaunchKernelGGL(sort_gather_word<uint32_t>, dim3(grid_for(n / 4)), dim3(256), 0, stream, values.as<uint32_t>(), nulls.as<uint8_t>(), order.perm, order.key_words(), order.ids(), n, word, is_float, descending, minimum);
      HY_HIP(hipGetLastError());
      HY_TRY(order.sort(n, bits, stream));
    }
  }
  hipLaunchKernelGGL(sort_positions, dim3(grid_for(n / 2)), dim3(256), 0, stream, order.perm, shape->d_row_base, shape->n_chunks, n, out);
  HY_HIP(hipGetLastError());
  HY_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool; the caller reads `out` next)
  return HY_OK;
}

hy_status hy_sort_limit(const hy_sort_key* keys, uint32_t n_keys, uint64_t limit, uint32_t flags, hy_row_id* out, uint64_t capacity, uint64_t* n_out, uint32_t* path) {
  if (!keys || !n_keys || !n_out) return fail(HY_ERR_INVALID, "hy_sort_limit: null argument or no sort key");
  *n_out = 0;
  if (path) *path = 0;
  constexpr uint32_t BOTH = HY_SORT_LIMIT_FORCE_FULL_SORT | HY_SORT_LIMIT_FORCE_SELECT;
  if ((flags & ~BOTH) || (flags & BOTH) == BOTH) return fail(HY_ERR_INVALID, "hy_sort_limit: flags %#x (0, FORCE_FULL_SORT or FORCE_SELECT)", flags);
  HY_TRY(check_sort_keys(keys, n_keys, "hy_sort_limit"));
  const hy_column* shape = keys[0].column;
  const uint64_t rows = shape->rows;
  const uint64_t k = std::min(limit, rows);
  *n_out = k;
  if (k > capacity) return fail(HY_ERR_CAPACITY, "hy_sort_limit: %llu rows, capacity %llu", static_cast<unsigned long long>(k), static_cast<unsigned long long>(capacity));
  const bool force_select = (flags & HY_SORT_LIMIT_FORCE_SELECT) != 0;
  if (!k) {
    if (path && force_select) *path = 1;   // (no row to select: the forced path in name, as hy_union_positions answers a forced sort of no rows)
    return HY_OK;
  }
  if (!out) return fail(HY_ERR_INVALID, "hy_sort_limit: null output");
  if ((flags & HY_SORT_LIMIT_FORCE_FULL_SORT) || (!force_select && (k >= rows || k > rows / SELECT_SHARE_DIVISOR))) return full_sort_and_cut(keys, n_keys, rows, k, out);
  const uint32_t n = static_cast<uint32_t>(rows);
  hipStream_t stream = current_stream();

  // definition 0: exported, and its words' ranges
  DeviceBuffer stats_buffer;
  HY_TRY(stats_buffer.alloc(64));
  ExportedKey first;
  HY_TRY(first.alloc(n));
  HY_TRY(first.load(keys[0], n, stats_buffer.as<uint32_t>(), stream));
  const uint32_t null_rows = first.stats[4];
  SelectKey key{first.stats[0], first.stats[1], 0, first.is_float, first.descending};
  uint32_t total_bits = 0, unused = 0;
  if (null_rows < n) {
    if (word_range(first.stats[0], first.stats[2], &unused, &key.lo_bits)) total_bits = key.lo_bits;
    uint32_t hi_bits = 0;
    if (first.wide && word_range(first.stats[1], first.stats[3], &unused, &hi_bits)) total_bits += hi_bits;
  }

  // the bucket the k-th row falls into: one histogram over the key's most significant digit, refined on the next digits while the bucket is large
  uint64_t candidates = null_rows;   // (null_rows >= k: the NULL rows alone)
  uint32_t shift = 0;
  uint64_t threshold = 0;
  const bool with_values = null_rows < k;
  if (with_values) {
    uint64_t need = k - null_rows, certain = 0, undecided = n - null_rows;
    DeviceBuffer partial;
    shift = total_bits;
    if (total_bits) HY_TRY(partial.alloc(size_t{4} * SELECT_HISTOGRAM_WGS * SELECT_BINS));
    for (bool filtered = false; shift > 0 && (!filtered || (undecided > need && undecided > n / REFINE_SHARE_DIVISOR)); filtered = true) {
      const uint32_t prefix_shift = filtered ? shift : 0;
      const uint32_t digit_bits = std::min(shift, SELECT_DIGIT_BITS);
      shift -= digit_bits;
      uint32_t* totals = nullptr;
      uint32_t* d_totals = nullptr;
      HY_TRY(pinned_staging(4 * SELECT_BINS, reinterpret_cast<void**>(&totals), reinterpret_cast<void**>(&d_totals)));
      const uint32_t grid = std::min<uint32_t>((n + 4095) / 4096, SELECT_HISTOGRAM_WGS);
      if (first.wide) hipLaunchKernelGGL(select_histogram<uint64_t>, dim3(grid), dim3(1024), 0, stream, first.values.as<uint64_t>(), first.nulls.as<uint8_t>(), n, key, filtered, prefix_shift, threshold, shift, (1u << digit_bits) - 1, partial.as<uint32_t>());
      else hipLaunchKernelGGL(select_histogram<uint32_t>, dim3(grid), dim3(1024), 0, stream, first.values.as<uint32_t>(), first.nulls.as<uint8_t>(), n, key, filtered, prefix_shift, threshold, shift, (1u << digit_bits) - 1, partial.as<uint32_t>());
      HY_HIP(hipGetLastError());
      hipLaunchKernelGGL(select_sum_bins, dim3(SELECT_BINS / 64), dim3(256), 0, stream, partial.as<uint32_t>(), grid, d_totals);
      HY_HIP(hipGetLastError());
      HY_HIP(hipStreamSynchronize(stream));
      uint32_t bucket = 0;
      uint64_t below = 0;
      while (bucket + 1 < (1u << digit_bits) && below + totals[bucket] < need) below += totals[bucket++];
      if (below + totals[bucket] < need) return fail(HY_ERR_DEVICE, "hy_sort_limit: the histogram holds %llu rows where %llu were expected", static_cast<unsigned long long>(below + totals[bucket]), static_cast<unsigned long long>(need));
      certain += below;
      need -= below;
      undecided = totals[bucket];
      threshold = (threshold << digit_bits) | bucket;
    }
    candidates = null_rows + certain + undecided;
  }
  if (!force_select && candidates > rows / SELECT_SHARE_DIVISOR) return full_sort_and_cut(keys, n_keys, rows, k, out);   // (first's buffers go back to the pool as it returns)
  if (path) *path = 1;

  // the candidates' row numbers, ascending, as the permutation the word sorts start from
  const uint32_t m = static_cast<uint32_t>(candidates);
  WordSort order;
  HY_TRY(order.alloc(m));
  uint32_t* d_total = stats_buffer.as<uint32_t>() + 8;   // (behind sort_word_stats' five words)
  {
    const uint32_t n_tiles = (n + SELECT_TILE - 1) / SELECT_TILE;
    DeviceBuffer masks, counts, offsets;
    HY_TRY(masks.alloc(size_t{8} * n_tiles * SELECT_TILE_WORDS));
    HY_TRY(counts.alloc(size_t{4} * n_tiles));
    HY_TRY(offsets.alloc(size_t{4} * n_tiles));
    if (first.wide) hipLaunchKernelGGL(select_mark<uint64_t>, dim3(n_tiles), dim3(256), 0, stream, first.values.as<uint64_t>(), first.nulls.as<uint8_t>(), n, key, with_values, shift, threshold, masks.as<uint64_t>(), counts.as<uint32_t>());
    else hipLaunchKernelGGL(select_mark<uint32_t>, dim3(n_tiles), dim3(256), 0, stream, first.values.as<uint32_t>(), first.nulls.as<uint8_t>(), n, key, with_values, shift, threshold, masks.as<uint64_t>(), counts.as<uint32_t>());
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(select_scan_tiles, dim3(1), dim3(1024), 0, stream, counts.as<uint32_t>(), n_tiles, offsets.as<uint32_t>(), d_total);
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(select_emit, dim3(n_tiles), dim3(256), 0, stream, masks.as<uint64_t>(), offsets.as<uint32_t>(), order.perm_a.as<uint32_t>(), m);
    HY_HIP(hipGetLastError());
    order.perm = order.perm_a.as<uint32_t>();
  }

  // hy_sort's chain over the candidates only: the last definition first, definition 0 from the export above
  if (m > 1) {
    ExportedKey later;
    if (n_keys > 1) HY_TRY(later.alloc(n));
    for (uint32_t d = n_keys; d-- > 1;) {
      HY_TRY(later.load(keys[d], n, stats_buffer.as<uint32_t>(), stream));
      HY_TRY(later.sort_words(order, n, m, stream));
    }
    HY_TRY(first.sort_words(order, n, m, stream));
  }
  hipLaunchKernelGGL(sort_positions, dim3(grid_for(k / 2)), dim3(256), 0, stream, order.perm, shape->d_row_base, shape->n_chunks, static_cast<uint32_t>(k), out);
  HY_HIP(hipGetLastError());
  uint32_t marked = 0;
  HY_HIP(hipMemcpyAsync(&marked, d_total, sizeof(marked), hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));
  if (marked != m) return fail(HY_ERR_DEVICE, "hy_sort_limit: %u candidates marked, %u expected", marked, m);
  return HY_OK;
}

hy_status hy_column_gather(const hy_column* column, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows, hy_column** result) {
  if (!result) return fail(HY_ERR_INVALID, "hy_column_gather: null argument");
  *result = nullptr;
  HY_TRY(check_sortable(column, "hy_column_gather"));
  if (!chunk_rows || (n && !positions)) return fail(HY_ERR_INVALID, "hy_column_gather: positions missing or chunk_rows == 0");
  const uint32_t type = column->data_type;
  const uint32_t width = (type == HY_TYPE_INT || type == HY_TYPE_FLOAT) ? 4 : 8;
  hipStream_t stream = current_stream();
  const uint64_t n_chunks64 = (n + chunk_rows - 1) / chunk_rows;
  if (n_chunks64 >= 0xFFFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "hy_column_gather: too many output chunks");
  const uint32_t n_chunks = static_cast<uint32_t>(n_chunks64);
  // one allocation: chunk c's values at c * value_stride (256-byte aligned), then every chunk's null vector at c * null_stride words
  const uint64_t value_stride = align_up(uint64_t{chunk_rows} * width + 16, 256);
  const uint32_t words_per_chunk = (chunk_rows + 63) / 64;
  const uint64_t null_stride = align_up(words_per_chunk, 32);
  const uint64_t values_bytes = value_stride * n_chunks;
  char* arena = nullptr;
  size_t arena_capacity = 0;
  HY_TRY(pool_acquire(values_bytes + 8 * null_stride * n_chunks + 256, reinterpret_cast<void**>(&arena), &arena_capacity));
  auto release = [&](hy_status status) { pool_release(arena, arena_capacity); return status; };
  uint64_t* out_nulls = reinterpret_cast<uint64_t*>(arena + values_bytes);
  if (n && column->rows) {
    DeviceBuffer values, nulls;
    hy_status st = values.alloc(size_t{width} * column->rows + 16);
    if (st == HY_OK) st = nulls.alloc(column->rows + 16);
    if (st == HY_OK) st = export_column_at(column, values.ptr, nulls.as<uint8_t>(), nullptr);
    if (st != HY_OK) return release(st);
    const uint64_t groups = uint64_t{n_chunks} * words_per_chunk;
    const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((groups + 3) / 4, 8192)));
    if (width == 8) hipLaunchKernelGGL(gather_column_rows<uint64_t>, dim3(grid), dim3(256), 0, stream, values.as<uint64_t>(), nulls.as<uint8_t>(), column->d_row_base, column->n_chunks, positions, n,
                                       chunk_rows, words_per_chunk, value_stride, null_stride, arena, out_nulls, groups);
    else hipLaunchKernelGGL(gather_column_rows<uint32_t>, dim3(grid), dim3(256), 0, stream, values.as<uint32_t>(), nulls.as<uint8_t>(), column->d_row_base, column->n_chunks, positions, n,
                            chunk_rows, words_per_chunk, value_stride, null_stride, arena, out_nulls, groups);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return release(fail(HY_ERR_DEVICE, "hy_column_gather: kernel failed"));
  } else if (n) {   // positions into an empty column: every row NULL
    return release(fail(HY_ERR_INVALID, "hy_column_gather: positions into an empty column"));
  }
  // the result as a column over the device buffers (HY_MEM_DEVICE: nothing is copied), which then owns them
  std::vector<hy_segment> segments(n_chunks ? n_chunks : 1);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    hy_segment& s = segments[c];
    std::memset(&s, 0, sizeof(s));
    s.encoding = HY_ENC_UNENCODED;
    s.data_type = type;
    s.size = static_cast<uint32_t>(std::min<uint64_t>(chunk_rows, n - uint64_t{c} * chunk_rows));
    s.width = width;
    s.data = arena + c * value_stride;
    s.nulls = out_nulls + c * null_stride;
    s.ref_chunk_id = 0xFFFFFFFFu;
  }
  hy_column* gathered = nullptr;
  const hy_status status = hy_column_create(segments.data(), n_chunks, HY_MEM_DEVICE, &gathered);
  if (status != HY_OK) return release(status);
  gathered->pooled.emplace_back(arena_capacity, arena);
  *result = gathered;
  return HY_OK;
}

}  // extern "C"

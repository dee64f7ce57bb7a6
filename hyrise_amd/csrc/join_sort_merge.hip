// join_sort_merge.hip -- JoinSortMerge (operators/join_sort_merge.cpp) on the device: the join the translator takes where JoinHash does not
// apply -- a primary predicate <, <=, >, >= or <>, or FULL OUTER.  Both inputs are sorted by key, so the partners of a left row are one
// range of the sorted right side (two for <>), and the join is a bounds search, a scan and a range expansion:
//   sort            per side: the column exported, its word statistics, then hy_sort's chain of stable word sorts (sort_keys.hpp) with the
//                   "is not NULL" word last, so the non-NULL rows are the tail of the permutation, ascending by key, ties by position;
//   smj_sorted_keys, sort_positions   per side: the sorted order-preserving keys (u32 / u64) and the sorted RowIDs as contiguous arrays;
//   smj_bounds      per sorted left row: [lower, upper) of its key in the right keys.  A workgroup takes a tile of left rows; the tile's
//                   first and last key bound the window of right keys all its searches fall into (both sequences ascend), which is searched
//                   in LDS where it fits and in global memory where a run of duplicates makes it larger.  It also writes the tile's pairs
//                   and its rows that have partners;
//   smj_scan_tiles  one workgroup: exclusive scan of both tile sums (64-bit pairs), the totals go to the host through pinned memory;
//   smj_mark, select_scan_tiles   outer modes: one bit per INPUT row "has no partner" (NULL keys included), counted per tile and scanned;
//   -- the host reads the totals here: HY_ERR_CAPACITY, or hy_join_sort_merge_count's answer --
//   smj_compact     the left rows that have partners, in sorted order, with the 64-bit offset of each one's first pair;
//   smj_emit        a workgroup per tile of output pairs: one binary search of the offsets for the tile's first row, the row starts written
//                   to LDS and spread by a max scan, then consecutive lanes write consecutive pairs of both lists;
//   smj_outer_emit  the marked rows in position order behind the pairs, NULL_ROW_ID on the other side.
// No kernel takes an output position from a global atomic: the result is a pure function of the inputs.
#include "hy_device.hpp"
#include "sort_words.hpp"
#include "sort_keys.hpp"
#include "join_outer_emit.hpp"

#include <algorithm>

namespace hy {

namespace {

constexpr uint32_t BOUNDS_ROWS = 4;                     // left rows per thread
constexpr uint32_t BOUNDS_TILE = 256 * BOUNDS_ROWS;     // left rows per workgroup of smj_bounds / smj_compact
constexpr uint32_t WINDOW_BYTES = 32768;                // right keys of a tile in LDS: 8192 u32 or 4096 u64
constexpr uint32_t EMIT_ITEMS = 8;
constexpr uint32_t EMIT_TILE = 256 * EMIT_ITEMS;        // output pairs per workgroup of smj_emit (8 KiB of LDS)
enum : uint32_t { TEST_EQUALS = 0, TEST_BELOW_MAX = 1, TEST_UP_TO_MAX = 2, TEST_ABOVE_MIN = 3, TEST_FROM_MIN = 4 };

// How many partners a left row has whose key spans [lower, upper) of the m_right sorted right keys, and where partner j lies.
__device__ __forceinline__ uint32_t partner_count(uint32_t condition, uint32_t lower, uint32_t upper, uint32_t m_right) {
  switch (condition) {
    case HY_PRED_EQUALS: return upper - lower;
    case HY_PRED_LESS_THAN: return m_right - upper;
    case HY_PRED_LESS_THAN_EQUALS: return m_right - lower;
    case HY_PRED_GREATER_THAN: return lower;
    case HY_PRED_GREATER_THAN_EQUALS: return upper;
    default: return lower + (m_right - upper);   // <>: the keys below, then the keys above
  }
}
__device__ __forceinline__ uint32_t partner_index(uint32_t condition, uint32_t lower, uint32_t upper, uint32_t j) {
  switch (condition) {
    case HY_PRED_EQUALS: case HY_PRED_LESS_THAN_EQUALS: return lower + j;
    case HY_PRED_LESS_THAN: return upper + j;
    case HY_PRED_GREATER_THAN: case HY_PRED_GREATER_THAN_EQUALS: return j;
    default: return j < lower ? j : j - lower + upper;
  }
}

// The first index in [lo, hi) whose key is >= / > `key` (hi if none).
template <typename K>
__device__ __forceinline__ uint32_t lower_bound_of(const K* keys, uint32_t lo, uint32_t hi, K key) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
template <typename K>
__device__ __forceinline__ uint32_t upper_bound_of(const K* keys, uint32_t lo, uint32_t hi, K key) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, uint32_t step) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v)), step));
  const uint32_t hi = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v >> 32)), step));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// keys[i] = the order-preserving key of the i-th non-NULL row in sorted order: row perm[first + i] (perm == nullptr: the identity).
template <typename U>
__global__ __launch_bounds__(256) void smj_sorted_keys(const U* values, const uint32_t* perm, uint32_t first, uint32_t m, bool is_float, U* keys) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
    const uint32_t row = perm ? perm[first + i] : first + i;
    keys[i] = order_key<U>(values[row], is_float, false);
  }
}

template <typename K>
__global__ __launch_bounds__(256) void smj_bounds(const K* left_keys, uint32_t m_left, const K* right_keys, uint32_t m_right, uint32_t condition, uint32_t* lower, uint32_t* upper,
                                                  uint64_t* tile_pairs, uint32_t* tile_rows) {
  constexpr uint32_t WINDOW = WINDOW_BYTES / sizeof(K);
  __shared__ K s_window[WINDOW];
  __shared__ uint32_t s_range[2];
  __shared__ uint64_t s_pairs[4];
  __shared__ uint32_t s_rows[4];
  const uint32_t tile_begin = blockIdx.x * BOUNDS_TILE;
  const uint32_t tile_end = min(m_left, tile_begin + BOUNDS_TILE);   // (the grid has no empty tile)
  if (threadIdx.x == 0) s_range[0] = lower_bound_of<K>(right_keys, 0, m_right, left_keys[tile_begin]);
  if (threadIdx.x == 64) s_range[1] = upper_bound_of<K>(right_keys, 0, m_right, left_keys[tile_end - 1]);
  __syncthreads();
  // every bound of the tile's keys lies in [window_begin, window_end]: the keys before are smaller than the tile's first, those behind larger than its last
  const uint32_t window_begin = s_range[0], window_end = s_range[1];
  const uint32_t window = window_end - window_begin;
  const bool in_lds = window <= WINDOW;
  if (in_lds) {
    for (uint32_t w = threadIdx.x; w < window; w += 256) s_window[w] = right_keys[window_begin + w];
    __syncthreads();
  }
  uint64_t pairs = 0;
  uint32_t rows = 0;
  for (uint32_t step = 0; step < BOUNDS_ROWS; ++step) {
    const uint32_t i = tile_begin + step * 256 + threadIdx.x;
    if (i >= tile_end) break;
    const K key = left_keys[i];
    uint32_t lo, hi;
    if (in_lds) {
      lo = window_begin + lower_bound_of<K>(s_window, 0, window, key);
      hi = window_begin + upper_bound_of<K>(s_window, lo - window_begin, window, key);
    } else {
      lo = lower_bound_of<K>(right_keys, window_begin, window_end, key);
      hi = upper_bound_of<K>(right_keys, lo, window_end, key);
    }
    lower[i] = lo;
    upper[i] = hi;
    const uint32_t count = partner_count(condition, lo, hi, m_right);
    pairs += count;
    rows += count != 0;
  }
  for (int offset = 32; offset > 0; offset >>= 1) {
    pairs += (static_cast<uint64_t>(static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(pairs >> 32)), offset))) << 32) |
             static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(pairs)), offset));
    rows += static_cast<uint32_t>(__shfl_xor(static_cast<int>(rows), offset));
  }
  if ((threadIdx.x & 63) == 0) { s_pairs[threadIdx.x >> 6] = pairs; s_rows[threadIdx.x >> 6] = rows; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_pairs[blockIdx.x] = s_pairs[0] + s_pairs[1] + s_pairs[2] + s_pairs[3];
    tile_rows[blockIdx.x] = s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3];
  }
}

// pair_offsets[t] / row_offsets[t] = the pairs / the rows with partners in the tiles before t; totals[0] / totals[1] = all of them (pinned host
// memory).  One workgroup, select_scan_tiles' shape with a 64-bit sum next to the 32-bit one.
__global__ __launch_bounds__(1024) void smj_scan_tiles(const uint64_t* tile_pairs, const uint32_t* tile_rows, uint32_t n_tiles, uint64_t* pair_offsets, uint32_t* row_offsets,
                                                       uint64_t* totals) {
  __shared__ uint64_t s_pairs[1024];
  __shared__ uint32_t s_rows[1024];
  const uint32_t per_thread = (n_tiles + 1023) / 1024;
  const uint32_t begin = min(n_tiles, threadIdx.x * per_thread), end = min(n_tiles, begin + per_thread);
  uint64_t pairs = 0;
  uint32_t rows = 0;
  for (uint32_t t = begin; t < end; ++t) { pairs += tile_pairs[t]; rows += tile_rows[t]; }
  s_pairs[threadIdx.x] = pairs;
  s_rows[threadIdx.x] = rows;
  __syncthreads();
  for (uint32_t step = 1; step < 1024; step <<= 1) {   // (inclusive scan of the threads' sums)
    const uint64_t add_pairs = threadIdx.x >= step ? s_pairs[threadIdx.x - step] : 0;
    const uint32_t add_rows = threadIdx.x >= step ? s_rows[threadIdx.x - step] : 0;
    __syncthreads();
    s_pairs[threadIdx.x] += add_pairs;
    s_rows[threadIdx.x] += add_rows;
    __syncthreads();
  }
  uint64_t run_pairs = s_pairs[threadIdx.x] - pairs;
  uint32_t run_rows = s_rows[threadIdx.x] - rows;
  for (uint32_t t = begin; t < end; ++t) {
    pair_offsets[t] = run_pairs; run_pairs += tile_pairs[t];
    row_offsets[t] = run_rows; run_rows += tile_rows[t];
  }
  if (threadIdx.x == 1023) { totals[0] = s_pairs[1023]; totals[1] = s_rows[1023]; }
}

// The sorted left rows that have partners: compact_row[k] = the row, compact_offset[k] = the output position of its first pair.  A thread
// takes BOUNDS_ROWS consecutive rows of smj_bounds' tile; the workgroup scans the threads' sums.
__global__ __launch_bounds__(256) void smj_compact(const uint32_t* lower, const uint32_t* upper, uint32_t m_left, uint32_t m_right, uint32_t condition, const uint64_t* pair_offsets,
                                                   const uint32_t* row_offsets, uint32_t* compact_row, uint64_t* compact_offset) {
  __shared__ uint64_t s_pairs[4];
  __shared__ uint32_t s_rows[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t first = blockIdx.x * BOUNDS_TILE + threadIdx.x * BOUNDS_ROWS;
  uint32_t counts[BOUNDS_ROWS];
  uint64_t pairs = 0;
  uint32_t rows = 0;
  for (uint32_t r = 0; r < BOUNDS_ROWS; ++r) {
    counts[r] = first + r < m_left ? partner_count(condition, lower[first + r], upper[first + r], m_right) : 0;
    pairs += counts[r];
    rows += counts[r] != 0;
  }
  uint64_t scan_pairs = pairs;   // inclusive over the wave
  uint32_t scan_rows = rows;
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint64_t up_pairs = shfl_up_u64(scan_pairs, step);
    const uint32_t up_rows = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan_rows), step));
    if (lane >= step) { scan_pairs += up_pairs; scan_rows += up_rows; }
  }
  if (lane == 63) { s_pairs[wave] = scan_pairs; s_rows[wave] = scan_rows; }
  __syncthreads();
  uint64_t at_pair = pair_offsets[blockIdx.x] + scan_pairs - pairs;
  uint32_t at_row = row_offsets[blockIdx.x] + scan_rows - rows;
  for (uint32_t w = 0; w < wave; ++w) { at_pair += s_pairs[w]; at_row += s_rows[w]; }
  for (uint32_t r = 0; r < BOUNDS_ROWS; ++r) {
    if (!counts[r]) continue;
    compact_row[at_row] = first + r;
    compact_offset[at_row] = at_pair;
    ++at_row;
    at_pair += counts[r];
  }
}

// Output pairs [tile * EMIT_TILE, + EMIT_TILE).  s_row[e] = which of the compacted rows, counted from the tile's first, pair e belongs to:
// the rows that begin inside the tile write their number at their first pair (at most EMIT_TILE - 1 of them, every one has a pair: a fixed
// EMIT_ITEMS steps whatever the data), a max scan spreads it over the row's pairs -- one row with 10^5 partners is 49 tiles that find
// nothing to write and scan zeros, 10^5 rows without partners are not in the compacted list.
__global__ __launch_bounds__(256) void smj_emit(const uint32_t* compact_row, const uint64_t* compact_offset, uint32_t n_rows, uint64_t total, const uint32_t* lower,
                                                const uint32_t* upper, uint32_t condition, const uint64_t* left_rows, const uint64_t* right_rows, uint64_t* left_out,
                                                uint64_t* right_out) {
  __shared__ u32x4_t s_row4[EMIT_TILE / 4];
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_first;
  uint32_t* s_row = reinterpret_cast<uint32_t*>(s_row4);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t tile_begin = uint64_t{blockIdx.x} * EMIT_TILE;
  const uint32_t count = static_cast<uint32_t>(min(uint64_t{EMIT_TILE}, total - tile_begin));
  if (threadIdx.x == 0) {   // the last compacted row that begins at or before the tile (compact_offset[0] == 0, and the offsets ascend strictly)
    uint32_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (compact_offset[mid] <= tile_begin) lo = mid; else hi = mid;
    }
    s_first = lo;
  }
  s_row4[threadIdx.x] = u32x4_t{0, 0, 0, 0};
  s_row4[256 + threadIdx.x] = u32x4_t{0, 0, 0, 0};
  __syncthreads();
  const uint32_t first = s_first;
  for (uint32_t step = 0; step < EMIT_ITEMS; ++step) {
    const uint64_t k = uint64_t{first} + 1 + step * 256 + threadIdx.x;
    if (k >= n_rows) break;
    const uint64_t offset = compact_offset[k];
    if (offset >= tile_begin + count) break;
    s_row[offset - tile_begin] = static_cast<uint32_t>(k - first);
  }
  __syncthreads();
  // inclusive max scan: a thread's EMIT_ITEMS consecutive entries, the wave's threads, the workgroup's waves
  u32x4_t a = s_row4[2 * threadIdx.x], b = s_row4[2 * threadIdx.x + 1];
  a.y = max(a.y, a.x); a.z = max(a.z, a.y); a.w = max(a.w, a.z);
  b.x = max(b.x, a.w); b.y = max(b.y, b.x); b.z = max(b.z, b.y); b.w = max(b.w, b.z);
  uint32_t scan = b.w;
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan), step));
    if (lane >= step) scan = max(scan, up);
  }
  if (lane == 63) s_wave[wave] = scan;
  uint32_t before = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan), 1));
  if (lane == 0) before = 0;
  __syncthreads();
  for (uint32_t w = 0; w < wave; ++w) before = max(before, s_wave[w]);
  a.x = max(a.x, before); a.y = max(a.y, before); a.z = max(a.z, before); a.w = max(a.w, before);
  b.x = max(b.x, before); b.y = max(b.y, before); b.z = max(b.z, before); b.w = max(b.w, before);
  s_row4[2 * threadIdx.x] = a;
  s_row4[2 * threadIdx.x + 1] = b;
  __syncthreads();
  for (uint32_t step = 0; step < EMIT_ITEMS; ++step) {
    const uint32_t e = step * 256 + threadIdx.x;
    if (e >= count) break;
    const uint32_t k = first + s_row[e];
    const uint32_t row = compact_row[k];
    const uint32_t j = static_cast<uint32_t>(tile_begin + e - compact_offset[k]);
    left_out[tile_begin + e] = left_rows[row];
    right_out[tile_begin + e] = right_rows[partner_index(condition, lower[row], upper[row], j)];
  }
}

// Bit l of masks[w] = input row 64 w + l has no partner: its key is NULL, the other side has no non-NULL row, or `test` fails -- TEST_EQUALS:
// the key is among other_keys (a binary search); the others: a comparison with the other side's largest / smallest key.  counts[tile] = how
// many.  One workgroup per MARK_TILE rows (select_mark's shape).
template <typename U>
__global__ __launch_bounds__(256) void smj_mark(const U* values, const uint8_t* nulls, uint32_t n, bool is_float, const U* other_keys, uint32_t m_other, uint32_t test,
                                                uint64_t* masks, uint32_t* counts) {
  __shared__ uint32_t s_count[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  U bound = 0;
  if (m_other && test != TEST_EQUALS) bound = (test == TEST_BELOW_MAX || test == TEST_UP_TO_MAX) ? other_keys[m_other - 1] : other_keys[0];
  uint32_t count = 0;
  for (uint32_t step = 0; step < MARK_TILE_WORDS / 4; ++step) {
    const uint64_t word = uint64_t{blockIdx.x} * MARK_TILE_WORDS + wave * (MARK_TILE_WORDS / 4) + step;
    const uint64_t row = word * 64 + lane;
    bool unmatched = false;
    if (row < n) {
      unmatched = true;
      if (m_other && !nulls[row]) {
        const U key = order_key<U>(values[row], is_float, false);
        bool partner;
        if (test == TEST_EQUALS) {
          const uint32_t at = lower_bound_of<U>(other_keys, 0, m_other, key);
          partner = at < m_other && other_keys[at] == key;
        } else {
          partner = test == TEST_BELOW_MAX ? key < bound : test == TEST_UP_TO_MAX ? key <= bound : test == TEST_ABOVE_MIN ? key > bound : key >= bound;
        }
        unmatched = !partner;
      }
    }
    const uint64_t mask = __ballot(unmatched);
    if (lane == 0) masks[word] = mask;
    count += static_cast<uint32_t>(__popcll(mask));
  }
  if (lane == 0) s_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// One input: the column by position (for smj_mark), and its non-NULL rows in key order as keys and RowIDs.
struct SortedSide {
  ExportedKey column;
  DeviceBuffer keys, positions;
  uint32_t n = 0, m = 0;   // rows, non-NULL rows
};

hy_status sort_side(const hy_column* input, SortedSide& side, uint32_t* d_stats, bool with_positions, hipStream_t stream) {
  const uint32_t n = side.n = static_cast<uint32_t>(input->rows);
  if (!n) return HY_OK;
  HY_TRY(side.column.alloc(n));
  const hy_sort_key key{input, HY_SORT_ASCENDING_NULLS_FIRST, 0};
  HY_TRY(side.column.load(key, n, d_stats, stream));
  const uint32_t null_rows = side.column.stats[4];
  const uint32_t m = side.m = n - null_rows;
  if (!m) return HY_OK;
  WordSort order;   // order.perm == nullptr: the identity (then no row is NULL, or the side has one row)
  if (n > 1) {
    HY_TRY(order.alloc(n));
    HY_TRY(side.column.sort_words(order, n, n, stream));   // NULLs first: the non-NULL rows are perm[null_rows, n)
  }
  const bool wide = side.column.wide;
  HY_TRY(side.keys.alloc((wide ? 8 : 4) * size_t{m} + 16));
  if (wide) hipLaunchKernelGGL(smj_sorted_keys<uint64_t>, dim3(grid_for(m)), dim3(256), 0, stream, side.column.values.as<uint64_t>(), order.perm, null_rows, m, side.column.is_float, side.keys.as<uint64_t>());
  else hipLaunchKernelGGL(smj_sorted_keys<uint32_t>, dim3(grid_for(m)), dim3(256), 0, stream, side.column.values.as<uint32_t>(), order.perm, null_rows, m, side.column.is_float, side.keys.as<uint32_t>());
  HY_HIP(hipGetLastError());
  if (with_positions) {
    HY_TRY(side.positions.alloc(8 * size_t{m} + 16));
    hipLaunchKernelGGL(sort_positions, dim3(grid_for(m / 2)), dim3(256), 0, stream, order.perm ? order.perm + null_rows : nullptr, input->d_row_base, input->n_chunks, m, side.positions.as<hy_row_id>());
    HY_HIP(hipGetLastError());
  }
  return HY_OK;   // (the permutation goes back to the pool, which hands blocks on in stream order)
}

// The unmatched rows of one side under an outer mode: the mask words, the tiles' offsets, and (after the host has read `total`) how many.
struct OuterRows {
  DeviceBuffer masks, counts, offsets;
  uint32_t n_tiles = 0;
};

hy_status mark_side(const SortedSide& side, const SortedSide& other, uint32_t test, OuterRows& outer, uint32_t* d_total, hipStream_t stream) {
  const uint32_t n_tiles = outer.n_tiles = (side.n + MARK_TILE - 1) / MARK_TILE;
  if (!n_tiles) return HY_OK;
  HY_TRY(outer.masks.alloc(size_t{8} * n_tiles * MARK_TILE_WORDS));
  HY_TRY(outer.counts.alloc(size_t{4} * n_tiles));
  HY_TRY(outer.offsets.alloc(size_t{4} * n_tiles));
  if (side.column.wide) hipLaunchKernelGGL(smj_mark<uint64_t>, dim3(n_tiles), dim3(256), 0, stream, side.column.values.as<uint64_t>(), side.column.nulls.as<uint8_t>(), side.n, side.column.is_float,
                                           other.keys.as<uint64_t>(), other.m, test, outer.masks.as<uint64_t>(), outer.counts.as<uint32_t>());
  else hipLaunchKernelGGL(smj_mark<uint32_t>, dim3(n_tiles), dim3(256), 0, stream, side.column.values.as<uint32_t>(), side.column.nulls.as<uint8_t>(), side.n, side.column.is_float,
                          other.keys.as<uint32_t>(), other.m, test, outer.masks.as<uint64_t>(), outer.counts.as<uint32_t>());
  HY_HIP(hipGetLastError());
  hipLaunchKernelGGL(select_scan_tiles, dim3(1), dim3(1024), 0, stream, outer.counts.as<uint32_t>(), n_tiles, outer.offsets.as<uint32_t>(), d_total);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

hy_status check_input(const hy_column* column, const char* entry_point) {
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_INVALID, "MVCC columns are read by hy_validate only");
  if (column->data_type < HY_TYPE_INT || column->data_type > HY_TYPE_DOUBLE) return fail(HY_ERR_UNSUPPORTED, "%s: string join keys stay on the stock operator", entry_point);
  if (column->has_dictionary_without_values) return fail(HY_ERR_UNSUPPORTED, "%s: the dictionary values are not on the device", entry_point);
  if (column->rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows on one side (32-bit row ids)", entry_point, static_cast<unsigned long long>(column->rows));
  return HY_OK;
}

// result == nullptr: the counting passes only.
hy_status run_sort_merge(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, hy_sort_merge_result* result, uint64_t* n_pairs_out, const char* entry_point) {
  if (!left || !right) return fail(HY_ERR_INVALID, "%s: null column", entry_point);
  if (mode > HY_JOIN_FULL_OUTER) return fail(HY_ERR_UNSUPPORTED, "%s: JoinSortMerge does not support join mode %u (Semi, Anti and Cross stay on the stock operator)", entry_point, mode);
  if (condition > HY_PRED_GREATER_THAN_EQUALS) return fail(HY_ERR_UNSUPPORTED, "%s: condition %u is no comparison of two columns", entry_point, condition);
  if (condition == HY_PRED_NOT_EQUALS && mode != HY_JOIN_INNER) return fail(HY_ERR_UNSUPPORTED, "%s: <> with an outer join mode (join_sort_merge.cpp:43-47)", entry_point);
  HY_TRY(check_input(left, entry_point));
  HY_TRY(check_input(right, entry_point));
  // (a column without chunks -- an input table without rows -- carries no type of its own: hy_column_create calls it int)
  if (left->n_chunks && right->n_chunks && left->data_type != right->data_type) return fail(HY_ERR_UNSUPPORTED, "%s: key columns of different types (%u and %u) stay on the stock operator", entry_point, left->data_type, right->data_type);
  if (result) {
    if (result->mem != HY_MEM_HOST && result->mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "%s: result->mem %u", entry_point, result->mem);
    result->n_pairs = result->n_matched = result->n_left_outer = 0;
    if (result->capacity && (!result->left_pos || !result->right_pos)) return fail(HY_ERR_INVALID, "%s: null output list", entry_point);
    if (reinterpret_cast<uintptr_t>(result->left_pos) % 8 != 0 || reinterpret_cast<uintptr_t>(result->right_pos) % 8 != 0) return fail(HY_ERR_INVALID, "%s: output list not on an 8-byte boundary", entry_point);
  }
  hipStream_t stream = current_stream();
  const bool left_outer = mode == HY_JOIN_LEFT || mode == HY_JOIN_FULL_OUTER, right_outer = mode == HY_JOIN_RIGHT || mode == HY_JOIN_FULL_OUTER;

  DeviceBuffer stats_buffer;
  HY_TRY(stats_buffer.alloc(64));
  profile_begin(stream);   // (hy_set_profiling: one event pair around the call's kernels, the host's reads in between included)
  struct ProfileEnd { hipStream_t stream; ~ProfileEnd() { profile_end(stream); } } profile_bracket{stream};
  SortedSide l, r;
  HY_TRY(sort_side(left, l, stats_buffer.as<uint32_t>(), result != nullptr, stream));
  HY_TRY(sort_side(right, r, stats_buffer.as<uint32_t>(), result != nullptr, stream));

  // totals: [0] matched pairs, [1] left rows with partners (64-bit words); then 32-bit words [4] unmatched left rows, [5] unmatched right rows
  uint64_t* totals = nullptr;
  uint64_t* d_totals = nullptr;
  HY_TRY(pinned_staging(64, reinterpret_cast<void**>(&totals), reinterpret_cast<void**>(&d_totals)));
  totals[0] = totals[1] = totals[2] = 0;
  const volatile uint32_t* outer_totals = reinterpret_cast<const uint32_t*>(totals) + 4;
  uint32_t* d_outer_totals = reinterpret_cast<uint32_t*>(d_totals) + 4;

  const bool any_pairs = l.m && r.m;
  const uint32_t n_tiles = any_pairs ? (l.m + BOUNDS_TILE - 1) / BOUNDS_TILE : 0;
  DeviceBuffer lower, upper, tile_pairs, tile_rows, pair_offsets, row_offsets;
  if (any_pairs) {
    HY_TRY(lower.alloc(4 * size_t{l.m} + 16));
    HY_TRY(upper.alloc(4 * size_t{l.m} + 16));
    HY_TRY(tile_pairs.alloc(8 * size_t{n_tiles}));
    HY_TRY(tile_rows.alloc(4 * size_t{n_tiles}));
    HY_TRY(pair_offsets.alloc(8 * size_t{n_tiles}));
    HY_TRY(row_offsets.alloc(4 * size_t{n_tiles}));
    if (l.column.wide) hipLaunchKernelGGL(smj_bounds<uint64_t>, dim3(n_tiles), dim3(256), 0, stream, l.keys.as<uint64_t>(), l.m, r.keys.as<uint64_t>(), r.m, condition, lower.as<uint32_t>(), upper.as<uint32_t>(),
                                 tile_pairs.as<uint64_t>(), tile_rows.as<uint32_t>());
    else hipLaunchKernelGGL(smj_bounds<uint32_t>, dim3(n_tiles), dim3(256), 0, stream, l.keys.as<uint32_t>(), l.m, r.keys.as<uint32_t>(), r.m, condition, lower.as<uint32_t>(), upper.as<uint32_t>(),
                            tile_pairs.as<uint64_t>(), tile_rows.as<uint32_t>());
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(smj_scan_tiles, dim3(1), dim3(1024), 0, stream, tile_pairs.as<uint64_t>(), tile_rows.as<uint32_t>(), n_tiles, pair_offsets.as<uint64_t>(), row_offsets.as<uint32_t>(), d_totals);
    HY_HIP(hipGetLastError());
  }
  // a left row finds a partner iff ... (a right row: the mirrored comparison)
  static constexpr uint32_t LEFT_TEST[6] = {TEST_EQUALS, TEST_EQUALS, TEST_BELOW_MAX, TEST_UP_TO_MAX, TEST_ABOVE_MIN, TEST_FROM_MIN};
  static constexpr uint32_t RIGHT_TEST[6] = {TEST_EQUALS, TEST_EQUALS, TEST_ABOVE_MIN, TEST_FROM_MIN, TEST_BELOW_MAX, TEST_UP_TO_MAX};
  OuterRows outer_left, outer_right;
  if (left_outer) HY_TRY(mark_side(l, r, LEFT_TEST[condition], outer_left, d_outer_totals, stream));
  if (right_outer) HY_TRY(mark_side(r, l, RIGHT_TEST[condition], outer_right, d_outer_totals + 1, stream));
  HY_HIP(hipStreamSynchronize(stream));

  const uint64_t n_matched = totals[0];
  const uint64_t rows_with_partners = totals[1];
  const uint64_t n_left_outer = outer_left.n_tiles ? outer_totals[0] : 0, n_right_outer = outer_right.n_tiles ? outer_totals[1] : 0;
  const uint64_t n_pairs = n_matched + n_left_outer + n_right_outer;
  if (n_pairs_out) *n_pairs_out = n_pairs;
  if (!result) return HY_OK;
  result->n_pairs = n_pairs;
  result->n_matched = n_matched;
  result->n_left_outer = n_left_outer;
  if (n_pairs > result->capacity) return fail(HY_ERR_CAPACITY, "%s: %llu pairs, capacity %llu", entry_point, static_cast<unsigned long long>(n_pairs), static_cast<unsigned long long>(result->capacity));
  if (!n_pairs) return HY_OK;
  const uint64_t emit_tiles = (n_matched + EMIT_TILE - 1) / EMIT_TILE;
  if (emit_tiles > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "%s: %llu pairs are more than one launch emits", entry_point, static_cast<unsigned long long>(n_matched));

  const bool host_result = result->mem == HY_MEM_HOST;
  DeviceBuffer left_list, right_list;   // a host result: the lists in device memory first
  uint64_t* left_out = reinterpret_cast<uint64_t*>(result->left_pos);
  uint64_t* right_out = reinterpret_cast<uint64_t*>(result->right_pos);
  if (host_result) {
    HY_TRY(left_list.alloc(8 * n_pairs));
    HY_TRY(right_list.alloc(8 * n_pairs));
    left_out = left_list.as<uint64_t>();
    right_out = right_list.as<uint64_t>();
  }
  DeviceBuffer compact_row, compact_offset;
  if (n_matched) {
    HY_TRY(compact_row.alloc(4 * rows_with_partners));
    HY_TRY(compact_offset.alloc(8 * rows_with_partners));
    hipLaunchKernelGGL(smj_compact, dim3(n_tiles), dim3(256), 0, stream, lower.as<uint32_t>(), upper.as<uint32_t>(), l.m, r.m, condition, pair_offsets.as<uint64_t>(), row_offsets.as<uint32_t>(),
                       compact_row.as<uint32_t>(), compact_offset.as<uint64_t>());
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(smj_emit, dim3(static_cast<uint32_t>(emit_tiles)), dim3(256), 0, stream, compact_row.as<uint32_t>(), compact_offset.as<uint64_t>(), static_cast<uint32_t>(rows_with_partners), n_matched,
                       lower.as<uint32_t>(), upper.as<uint32_t>(), condition, l.positions.as<uint64_t>(), r.positions.as<uint64_t>(), left_out, right_out);
    HY_HIP(hipGetLastError());
  }
  if (n_left_outer) {
    hipLaunchKernelGGL(smj_outer_emit, dim3(outer_left.n_tiles), dim3(256), 0, stream, outer_left.masks.as<uint64_t>(), outer_left.offsets.as<uint32_t>(), left->d_row_base, left->n_chunks, n_matched, left_out,
                       right_out);
    HY_HIP(hipGetLastError());
  }
  if (n_right_outer) {
    hipLaunchKernelGGL(smj_outer_emit, dim3(outer_right.n_tiles), dim3(256), 0, stream, outer_right.masks.as<uint64_t>(), outer_right.offsets.as<uint32_t>(), right->d_row_base, right->n_chunks,
                       n_matched + n_left_outer, right_out, left_out);
    HY_HIP(hipGetLastError());
  }
  if (host_result) {
    HY_HIP(hipMemcpyAsync(result->left_pos, left_out, 8 * n_pairs, hipMemcpyDeviceToHost, stream));
    HY_HIP(hipMemcpyAsync(result->right_pos, right_out, 8 * n_pairs, hipMemcpyDeviceToHost, stream));
  }
  HY_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool; the caller reads the lists next)
  return HY_OK;
}

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_join_sort_merge(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, hy_sort_merge_result* result) {
  if (!result) return fail(HY_ERR_INVALID, "hy_join_sort_merge: null result");
  return run_sort_merge(left, right, mode, condition, result, nullptr, "hy_join_sort_merge");
}

hy_status hy_join_sort_merge_count(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, uint64_t* n_pairs) {
  if (!n_pairs) return fail(HY_ERR_INVALID, "hy_join_sort_merge_count: null argument");
  *n_pairs = 0;
  return run_sort_merge(left, right, mode, condition, nullptr, n_pairs, "hy_join_sort_merge_count");
}

}  // extern "C"

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

#include <algorithm>
#include <cstring>
#include <vector>

namespace hy {

namespace {

// The order-preserving unsigned key of a value's bits (4- or 8-byte types; NULL rows never get here).
template <typename U>
__device__ __forceinline__ U order_key(U bits, bool is_float, bool descending) {
  constexpr U SIGN = U{1} << (8 * sizeof(U) - 1);
  U key;
  if (is_float) {
    if (bits == SIGN) bits = 0;                       // -0.0 == 0.0 under std::less: one key
    key = (bits & SIGN) ? static_cast<U>(~bits) : static_cast<U>(bits | SIGN);
  } else {
    key = bits ^ SIGN;
  }
  return descending ? static_cast<U>(~key) : key;
}

// word 0 / 1: the low / high 32 bits of the key; word 2: "is not NULL" (NULLs first).  NULL rows: 0 in the value words -- the same for
// every NULL, so they keep the order they had.
template <typename U>
__device__ __forceinline__ uint32_t key_word(const U* values, const uint8_t* nulls, uint32_t row, uint32_t word, bool is_float, bool descending, uint32_t minimum) {
  if (word == 2) return nulls[row] ? 0u : 1u;
  if (nulls[row]) return 0u;
  const U key = order_key<U>(values[row], is_float, descending);
  return static_cast<uint32_t>(word == 0 ? key : static_cast<U>(key >> 31 >> 1)) - minimum;
}

// The smallest and largest value of both key words over the non-NULL rows, and the number of NULL rows.
// stats: [0] min word 0, [1] min word 1, [2] max word 0, [3] max word 1, [4] NULL rows (set to ~0 / ~0 / 0 / 0 / 0 before).
template <typename U>
__global__ __launch_bounds__(256) void sort_word_stats(const U* values, const uint8_t* nulls, uint32_t n, bool is_float, bool descending, uint32_t* stats) {
  uint32_t lo_min = ~0u, hi_min = ~0u, lo_max = 0, hi_max = 0, null_rows = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if (nulls[i]) { ++null_rows; continue; }
    const U key = order_key<U>(values[i], is_float, descending);
    const uint32_t lo = static_cast<uint32_t>(key), hi = static_cast<uint32_t>(key >> 31 >> 1);
    lo_min = min(lo_min, lo); lo_max = max(lo_max, lo);
    hi_min = min(hi_min, hi); hi_max = max(hi_max, hi);
  }
  for (int offset = 32; offset > 0; offset >>= 1) {
    lo_min = min(lo_min, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo_min), offset)));
    hi_min = min(hi_min, static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi_min), offset)));
    lo_max = max(lo_max, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo_max), offset)));
    hi_max = max(hi_max, static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi_max), offset)));
    null_rows += static_cast<uint32_t>(__shfl_xor(static_cast<int>(null_rows), offset));
  }
  // the workgroup's four waves through LDS, then one set of atomics per workgroup (one per wave: 1.2 ms at 60 M rows, contention)
  __shared__ uint32_t s_part[4][5];
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_part[wave][0] = lo_min; s_part[wave][1] = hi_min; s_part[wave][2] = lo_max; s_part[wave][3] = hi_max; s_part[wave][4] = null_rows;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < 4; ++w) {
      lo_min = min(lo_min, s_part[w][0]); hi_min = min(hi_min, s_part[w][1]);
      lo_max = max(lo_max, s_part[w][2]); hi_max = max(hi_max, s_part[w][3]); null_rows += s_part[w][4];
    }
    atomicMin(stats + 0, lo_min);
    atomicMin(stats + 1, hi_min);
    atomicMax(stats + 2, lo_max);
    atomicMax(stats + 3, hi_max);
    if (null_rows) atomicAdd(stats + 4, null_rows);
  }
}

// keys[i] = word(transform(values[perm[i]])) - minimum, four rows per thread and step: perm is read and keys written as 16-byte vectors,
// only the values (and null bytes) are gathered.  perm == nullptr: the identity, which is then written to ids_out (the first word sorted).
template <typename U>
__global__ __launch_bounds__(256) void sort_gather_word(const U* values, const uint8_t* nulls, const uint32_t* perm, uint32_t* keys, uint32_t* ids_out, uint32_t n,
                                                        uint32_t word, bool is_float, bool descending, uint32_t minimum) {
  const uint32_t quads = n / 4;
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
    u32x4_t p;
    if (perm) p = reinterpret_cast<const u32x4_t*>(perm)[q];
    else p = u32x4_t{4 * q, 4 * q + 1, 4 * q + 2, 4 * q + 3};
    const u32x4_t k{key_word<U>(values, nulls, p.x, word, is_float, descending, minimum), key_word<U>(values, nulls, p.y, word, is_float, descending, minimum),
                    key_word<U>(values, nulls, p.z, word, is_float, descending, minimum), key_word<U>(values, nulls, p.w, word, is_float, descending, minimum)};
    reinterpret_cast<u32x4_t*>(keys)[q] = k;
    if (!perm) reinterpret_cast<u32x4_t*>(ids_out)[q] = p;
  }
  for (uint32_t i = 4 * quads + blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {   // (the last n % 4 rows)
    const uint32_t row = perm ? perm[i] : i;
    keys[i] = key_word<U>(values, nulls, row, word, is_float, descending, minimum);
    if (!perm) ids_out[i] = row;
  }
}

// Flat row index -> the input table's position (chunk, offset): a binary search of row_base [n_chunks + 1].  Two rows per thread and step.
__device__ __forceinline__ hy_row_id position_of(uint32_t row, const uint64_t* row_base, uint32_t n_chunks) {
  uint32_t lo = 0, hi = n_chunks;   // the last chunk c with row_base[c] <= row (empty chunks: the first one after them)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (row_base[mid] <= row) lo = mid; else hi = mid;
  }
  return hy_row_id{lo, static_cast<uint32_t>(row - row_base[lo])};
}

__global__ __launch_bounds__(256) void sort_positions(const uint32_t* perm, const uint64_t* row_base, uint32_t n_chunks, uint32_t n, hy_row_id* out) {
  const uint32_t pairs = reinterpret_cast<uintptr_t>(out) % 16 == 0 ? n / 2 : 0;   // (an output that is not 16-byte aligned: one row at a time)
  const uint32_t stride = gridDim.x * 256;
  for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < pairs; q += stride) {
    const uint32_t a = perm ? perm[2 * q] : 2 * q, b = perm ? perm[2 * q + 1] : 2 * q + 1;
    const hy_row_id ra = position_of(a, row_base, n_chunks), rb = position_of(b, row_base, n_chunks);
    reinterpret_cast<u32x4_t*>(out)[q] = u32x4_t{ra.chunk_id, ra.chunk_offset, rb.chunk_id, rb.chunk_offset};
  }
  for (uint32_t i = 2 * pairs + blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = position_of(perm ? perm[i] : i, row_base, n_chunks);
}

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

bool numeric_type(uint32_t t) { return t >= HY_TYPE_INT && t <= HY_TYPE_DOUBLE; }

hy_status check_sortable(const hy_column* column, const char* entry_point) {
  if (!column) return fail(HY_ERR_INVALID, "%s: null column", entry_point);
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_INVALID, "MVCC columns are read by hy_validate only");
  if (!numeric_type(column->data_type)) return fail(HY_ERR_UNSUPPORTED, "%s: numeric columns only (a string column is passed as ranks)", entry_point);
  if (column->has_dictionary_without_values) return fail(HY_ERR_UNSUPPORTED, "%s: the dictionary values are not on the device", entry_point);
  return HY_OK;
}

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

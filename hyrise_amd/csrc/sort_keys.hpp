// sort_keys.hpp -- the kernels that turn an exported column into sort words and positions, shared by the operators that order rows by a
// column's values (sort.hip: Sort and Sort with a row limit; join_sort_merge.hip: JoinSortMerge): the order-preserving key, its word
// statistics, the word gather in front of every sort_pairs_u32 pass, the positions of the sorted rows, and the one-workgroup scan of tile
// counts that the compactions use.  Every translation unit that includes this gets its own copy of the kernels (anonymous namespace).
#pragma once

#include "hy_device.hpp"
#include "sort_words.hpp"

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

// offsets[t] = the candidates in the tiles before t; *total = all of them (union_scan_tiles' scan: one workgroup, 7 323 tiles for 60 M rows).
__global__ __launch_bounds__(1024) void select_scan_tiles(const uint32_t* counts, uint32_t n_tiles, uint32_t* offsets, uint32_t* total) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t per_thread = (n_tiles + 1023) / 1024;
  const uint32_t begin = min(n_tiles, threadIdx.x * per_thread), end = min(n_tiles, begin + per_thread);
  uint32_t sum = 0;
  for (uint32_t t = begin; t < end; ++t) sum += counts[t];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t step = 1; step < 1024; step <<= 1) {   // (inclusive scan of the threads' sums)
    const uint32_t add = threadIdx.x >= step ? s_sum[threadIdx.x - step] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = s_sum[threadIdx.x] - sum;
  for (uint32_t t = begin; t < end; ++t) { offsets[t] = run; run += counts[t]; }
  if (threadIdx.x == 1023) *total = s_sum[1023];
}

// One sort definition on its way through the word sorts: the column exported, and its word statistics on the host.
struct ExportedKey {
  DeviceBuffer values, nulls;
  bool wide = false, is_float = false, descending = false;
  uint32_t stats[5] = {0, 0, 0, 0, 0};   // sort_word_stats' five words
  hy_status alloc(uint32_t n) {
    HY_TRY(values.alloc(8 * size_t{n} + 16));
    return nulls.alloc(size_t{n} + 16);
  }
  hy_status load(const hy_sort_key& key, uint32_t n, uint32_t* d_stats, hipStream_t stream) {
    const hy_column* column = key.column;
    wide = column->data_type == HY_TYPE_LONG || column->data_type == HY_TYPE_DOUBLE;
    is_float = column->data_type == HY_TYPE_FLOAT || column->data_type == HY_TYPE_DOUBLE;
    descending = key.mode == HY_SORT_DESCENDING_NULLS_FIRST;
    HY_TRY(export_column_at(column, values.ptr, nulls.as<uint8_t>(), nullptr));
    HY_HIP(hipMemsetAsync(d_stats, 0xFF, 8, stream));
    HY_HIP(hipMemsetAsync(d_stats + 2, 0, 12, stream));
    const uint32_t grid = std::min<uint32_t>(grid_for(n / 16), 1024);
    if (wide) hipLaunchKernelGGL(sort_word_stats<uint64_t>, dim3(grid), dim3(256), 0, stream, values.as<uint64_t>(), nulls.as<uint8_t>(), n, is_float, descending, d_stats);
    else hipLaunchKernelGGL(sort_word_stats<uint32_t>, dim3(grid), dim3(256), 0, stream, values.as<uint32_t>(), nulls.as<uint8_t>(), n, is_float, descending, d_stats);
    HY_HIP(hipGetLastError());
    HY_HIP(hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, stream));
    HY_HIP(hipStreamSynchronize(stream));
    return HY_OK;
  }
  // hy_sort's loop over the definition's words, over the m rows of order.perm (stats of the whole column bound those of any subset of it)
  hy_status sort_words(WordSort& order, uint32_t n, uint32_t m, hipStream_t stream) const {
    const uint32_t null_rows = stats[4];
    for (uint32_t word = 0; word < 3; ++word) {
      uint32_t minimum = 0, bits = 1;
      if (word < 2) {
        if (word == 1 && !wide) continue;
        if (null_rows == n || !word_range(stats[word], stats[2 + word], &minimum, &bits)) continue;
      } else if (null_rows == 0 || null_rows == n) {
        continue;
      }
      if (wide) hipLaunchKernelGGL(sort_gather_word<uint64_t>, dim3(grid_for(m / 4)), dim3(256), 0, stream, values.as<uint64_t>(), nulls.as<uint8_t>(), order.perm, order.key_words(), order.ids(), m, word, is_float, descending, minimum);
      else hipLaunchKernelGGL(sort_gather_word<uint32_t>, dim3(grid_for(m / 4)), dim3(256), 0, stream, values.as<uint32_t>(), nulls.as<uint8_t>(), order.perm, order.key_words(), order.ids(), m, word, is_float, descending, minimum);
      HY_HIP(hipGetLastError());
      HY_TRY(order.sort(m, bits, stream));
    }
    return HY_OK;
  }
};

}  // namespace

}  // namespace hy

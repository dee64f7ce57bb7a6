// join_outer_emit.hpp -- the unmatched rows of one join input behind the pairs of an outer join: one bit per input row in 64-row mask words,
// counted per MARK_TILE rows, scanned by select_scan_tiles (sort_keys.hpp) and written by smj_outer_emit.  Shared by join_sort_merge.hip and
// join_nested_loop.hip; every translation unit that includes this gets its own copy of the kernel (anonymous namespace).
#pragma once

#include "hy_device.hpp"
#include "sort_keys.hpp"

namespace hy {

namespace {

constexpr uint32_t MARK_TILE = SLICE_ROWS;              // input rows per workgroup of smj_mark / smj_outer_emit: 128 mask words
constexpr uint32_t MARK_TILE_WORDS = MARK_TILE / 64;
constexpr uint64_t NULL_ROW = ~uint64_t{0};             // NULL_ROW_ID as it lies in memory

// The marked rows in position order at own_out[base ...] as RowIDs of the input table, NULL_ROW_ID in other_out (select_emit's shape).
__global__ __launch_bounds__(256) void smj_outer_emit(const uint64_t* masks, const uint32_t* offsets, const uint64_t* row_base, uint32_t n_chunks, uint64_t base, uint64_t* own_out,
                                                      uint64_t* other_out) {
  __shared__ uint32_t s_wave[4];
  constexpr uint32_t WORDS = MARK_TILE_WORDS / 4;   // per wave: 32
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first_word = uint64_t{blockIdx.x} * MARK_TILE_WORDS + wave * WORDS;
  const uint32_t mine = lane < WORDS ? static_cast<uint32_t>(__popcll(masks[first_word + lane])) : 0;
  uint32_t scan = mine;   // inclusive over the wave
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan), step));
    if (lane >= step) scan += up;
  }
  if (lane == 63) s_wave[wave] = scan;
  __syncthreads();
  uint64_t at = base + offsets[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
  const uint32_t before = scan - mine;
  const uint64_t below = (uint64_t{1} << lane) - 1;
  for (uint32_t w = 0; w < WORDS; ++w) {
    const uint64_t mask = masks[first_word + w];
    if (!mask) continue;
    const uint64_t place = at + static_cast<uint32_t>(__shfl(static_cast<int>(before), static_cast<int>(w))) + static_cast<uint32_t>(__popcll(mask & below));
    if (mask >> lane & 1) {
      const hy_row_id position = position_of(static_cast<uint32_t>((first_word + w) * 64 + lane), row_base, n_chunks);
      own_out[place] = (static_cast<uint64_t>(position.chunk_offset) << 32) | position.chunk_id;
      other_out[place] = NULL_ROW;
    }
  }
}

}  // namespace

}  // namespace hy

// sort_words.hpp -- what the operators that order rows word by word share (sort.hip: Sort; union_positions.hip: UnionPositions): a row order
// is built as a chain of stable LSD radix sorts of (32-bit word, row) pairs by sort_pairs_u32 (join.hip), least significant word first.  A word
// that has the same value in every row is skipped, and a word sorts only the bits its range needs.
#pragma once

#include "hy_device.hpp"

#include <algorithm>

namespace hy {

struct u32x4_t { uint32_t x, y, z, w; };

inline uint32_t grid_for(uint64_t items) { return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, 4096))); }

// A word whose values span [lowest, highest]: false if it orders nothing (constant), else what to subtract and how many bits are left to sort.
inline bool word_range(uint32_t lowest, uint32_t highest, uint32_t* minimum, uint32_t* bits) {
  if (lowest >= highest) return false;
  *minimum = lowest;
  *bits = 32 - static_cast<uint32_t>(__builtin_clz(highest - lowest));
  return true;
}

// Smallest / largest of a value over the wave (every lane gets it).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  for (int offset = 32; offset > 0; offset >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), offset)));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int offset = 32; offset > 0; offset >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), offset)));
  return v;
}

// The permutation as it grows: perm == nullptr is the identity (no word sorted yet).  For every word the caller's kernel writes
// key_words()[i] = word of row perm[i] (and, while perm == nullptr, ids()[i] = i), then sort() orders the pairs.
struct WordSort {
  DeviceBuffer perm_a, perm_b, keys_a, keys_b;
  uint32_t* perm = nullptr;
  hy_status alloc(uint32_t n) {
    HY_TRY(perm_a.alloc(4 * size_t{n} + 16));
    HY_TRY(perm_b.alloc(4 * size_t{n} + 16));
    HY_TRY(keys_a.alloc(4 * size_t{n} + 16));
    HY_TRY(keys_b.alloc(4 * size_t{n} + 16));
    return HY_OK;
  }
  uint32_t* key_words() const { return keys_a.as<uint32_t>(); }
  uint32_t* ids() const { return perm ? perm : perm_a.as<uint32_t>(); }
  hy_status sort(uint32_t n, uint32_t bits, hipStream_t stream) {
    uint32_t* id_words = ids();
    uint32_t* spare_ids = id_words == perm_a.as<uint32_t>() ? perm_b.as<uint32_t>() : perm_a.as<uint32_t>();
    uint32_t* words = key_words();
    HY_TRY(sort_pairs_u32(&words, &id_words, keys_b.as<uint32_t>(), spare_ids, n, bits, stream));
    perm = id_words;
    return HY_OK;
  }
};

}  // namespace hy

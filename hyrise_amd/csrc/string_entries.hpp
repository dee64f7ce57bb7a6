// string_entries.hpp -- one dictionary entry as the kernels over string dictionaries read it (string_order.hip: the rankings; string_gather.hip:
// the gather): where its bytes lie and how many they are, in either chunk layout, and std::string's order of two entries; and the scan over
// tile sums that both run behind their head flags.  Every translation unit that includes this gets its own copy (anonymous namespace).
#pragma once

#include "hy_device.hpp"

namespace hy {

namespace {

struct Entry {
  const uint8_t* bytes;
  uint32_t length;
};

// the last i in [0, n) with table[i] <= x, for an ascending table whose first element is <= x (equal elements: the last of them)
template <typename T>
__device__ __forceinline__ uint32_t last_at_or_below(const T* table, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (table[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

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

// strnlen(slot, L) of a fixed slot, four bytes at a time where the slot lies on a 4-byte boundary
__device__ __forceinline__ uint32_t slot_length(const uint8_t* slot, uint32_t L) {
  uint32_t length = 0;
  if (reinterpret_cast<uintptr_t>(slot) % 4 == 0) {
    for (; length + 4 <= L; length += 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(slot + length);
      if ((w - 0x01010101u) & ~w & 0x80808080u) break;   // a zero byte among the four
    }
  }
  while (length < L && slot[length] != 0) ++length;
  return length;
}

// The entry seen through a window (SUBSTR, string_substr.hip): bytes [begin, begin + length) of it.  `windows` are the chunk's, one per entry,
// made from the entries' own lengths (entry_windows: begin + length never exceeds the entry); nullptr is the identity window, the whole entry.
__device__ __forceinline__ Entry entry_of(const LikeChunk& chunk, uint32_t v, uint32_t end, const EntryWindow* windows) {
  if (!windows) return entry_of(chunk, v, end);
  const uint8_t* chars = reinterpret_cast<const uint8_t*>(chunk.chars);
  const EntryWindow window = windows[v];
  const uint8_t* entry = chunk.offsets ? chars + min(chunk.offsets[v], end) : chars + size_t{v} * chunk.string_length;
  return Entry{entry + window.begin, window.length};
}

// SUBSTR(entry of n bytes, start, length) as a window: the reference's _evaluate_substring (expression_evaluator.cpp:1597-1638) in 64-bit arithmetic
__device__ __forceinline__ EntryWindow substr_window(uint32_t n, int32_t start, int32_t length) {
  if (length <= 0) return EntryWindow{0, 0};
  int64_t s, l = length;
  if (start < 0) s = int64_t{start} + n;
  else if (start == 0) { s = 0; l -= 1; }
  else s = int64_t{start} - 1;
  const int64_t e = min(s + l, int64_t{n});
  s = max(s, int64_t{0});
  if (s < int64_t{n} && e > s) return EntryWindow{static_cast<uint32_t>(s), static_cast<uint32_t>(e - s)};
  return EntryWindow{0, 0};
}

// An entry of the sparse route's table (hy_device.hpp: SubsetEntry), as the comparisons and the copy read it
__device__ __forceinline__ Entry entry_of(const SubsetEntry& e) { return Entry{e.bytes, e.length}; }

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

constexpr uint32_t SCAN_WG = 1024;

// tiles[t] becomes the sum of the tiles before t; *total = the sum of all.  One workgroup: a thread sums a contiguous share, the shares' sums
// are scanned in LDS, the thread walks its share again.
template <typename T>
__global__ __launch_bounds__(SCAN_WG) void scan_tiles(T* tiles, uint32_t n_tiles, T* total) {
  __shared__ T s_sums[SCAN_WG];
  const uint32_t share = (n_tiles + SCAN_WG - 1) / SCAN_WG;
  const uint32_t begin = min(threadIdx.x * share, n_tiles), end = min(begin + share, n_tiles);
  T sum = 0;
  for (uint32_t i = begin; i < end; ++i) sum += tiles[i];
  s_sums[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t step = 1; step < SCAN_WG; step <<= 1) {   // Hillis-Steele, inclusive
    const T add = threadIdx.x >= step ? s_sums[threadIdx.x - step] : 0;
    __syncthreads();
    s_sums[threadIdx.x] += add;
    __syncthreads();
  }
  T running = s_sums[threadIdx.x] - sum;
  for (uint32_t i = begin; i < end; ++i) {
    const T here = tiles[i];
    tiles[i] = running;
    running += here;
  }
  if (threadIdx.x == SCAN_WG - 1) *total = s_sums[SCAN_WG - 1];
}

}  // namespace

}  // namespace hy

// string_gather.hip -- string columns MADE on the device: the rows of a dictionary-encoded string column at RowIDs (hy_string_column_gather)
// and the strings an int32 column of dense ranks stands for (hy_string_ranks_gather), each as a new dictionary-encoded string column in HBM --
// uint32_t attribute vectors plus an hy_string_dictionary with one sorted, duplicate-free dictionary per output chunk -- and the read-back of
// an offsets-layout dictionary chunk.
//
// Both entry points make, per output row, the row's GLOBAL ENTRY INDEX (entry_offsets[source chunk] + value id) or -1 for a NULL row:
//   RowIDs   the column's int32 stand-in over the table 0, 1, 2, ... (string_stand_in: the caller's attribute vectors of any width or packing
//            and the PosLists of a reference column, read in place) exported once, then one lookup per RowID (entries_at_positions);
//   ranks    an inverse table rank -> smallest entry index with that rank (inverse_ranks: one vector atomicMin per entry, whose result does
//            not depend on any order), then one lookup per row (entries_of_ranks); a rank that no entry has finds the table's filler, -1.
// The back end (gather_entries) is the same for both:
//   1  the source dictionary ranked by hy_string_dictionary_order's launches: equal strings of different source chunks get one rank;
//   2  the rows ordered by (output chunk, rank), a NULL row's rank above every other: two stable word sorts of (word, row) pairs
//      (sort_words.hpp), the rank first, then the output chunk -- skipped for one output chunk;
//   3  a head flag per sorted row (its key differs from its predecessor's; NULL rows are never heads), counted inclusively per 256 rows and
//      scanned over the tiles: a row's value id = heads at or before it - heads before its chunk - 1 (a NULL row, behind all heads of its chunk,
//      gets the chunk's entry count), stored by the sorted row into its place; a head also records its entry as the next output entry;
//   4  every output entry's source address and length (offsets difference, or strnlen of a fixed slot), the lengths scanned as 64-bit sums;
//      per output chunk the entry count and the chars' bytes go to the host in ONE copy of 16 bytes per chunk -- all it ever learns;
//   5  the output offsets (per chunk, relative to the chunk's first byte) and the bytes: copy_entry_bytes is byte-parallel, a lane owns 16
//      consecutive output bytes of the whole column's char stream, finds the entry its first byte lies in by binary search over the
//      workgroup's stretch of entry starts (staged in LDS while it has at most COPY_TILE entries, else read where they are), gathers from
//      as many entries as its 16 bytes span -- 8, 4 or 1 source bytes at a time at any byte address, never a byte outside an entry -- and
//      stores one 16-byte vector.  A 100 kB entry is copied by 6 250 lanes.
// Temporaries.  Scratch arena: per source entry 16 bytes of ranking (merge_layout) + 4 of ranks (+ 4 of inverse table for the rank front
// end); per output row 4 (entry) + 4 (tile-local heads) + 4 (output entry's source entry) + 8 (its address) + 8 (tile-local byte sums), per
// 256 rows 12, per output chunk 20.  Pool blocks: the word sort's 16 bytes per row; for the RowID front end the stand-in's table (4 per
// source entry) and its export (5 per SOURCE row).  Results: the attribute vectors and null-free segments in one pooled arena owned by the
// column (hy_column_gather's layout); offsets and chars in one allocation owned by the dictionary.
// The sparse route (HY_OPT_STRING_SPARSE_GATHER) is for few rows out of a large column: the column is read AT the rows
// (sparse_mark: PosLists and attribute vectors of any width or packing in place, no stand-in, no export), the entries they reference are
// marked in a bitmap over E and compacted into a table of (address, length), only those are ranked (table_order_launch), and the back end
// reads entries by table index.  Its temporaries follow n and the subset, plus one bit per source entry (sparse_layout, subset_layout).
// The host side: the four producers of string columns (these two, hy_string_column_substr, hy_string_column_materialize) are one StringRequest,
// resolved once (string_request) and run as stages (string_request_run): reserve by layout, rank the source, row entries, gather_entries.
#include "hy_device.hpp"
#include "sort_words.hpp"
#include "string_entries.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hy {

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t COPY_SPAN = 16;      // output bytes per lane: one vector store
constexpr uint32_t COPY_TILE = 1024;    // entry starts a workgroup stages in LDS (4 KiB of output hold that many entries of 4 bytes)

// The output chunks: chunk_rows rows each (the last one shorter), or, with row_base, the chunks of another column.
struct OutLayout {
  const uint64_t* row_base;     // [n_chunks + 1] in device memory, or nullptr
  const uint64_t* vector_at;    // [n_chunks] where a chunk's attribute vector begins in the arena (bytes), or nullptr: chunk * vector_stride
  uint64_t vector_stride;
  uint32_t chunk_rows;
  uint32_t n_chunks;
  uint32_t n;                   // rows
};

struct ChunkTotals {   // what crosses to the host, per output chunk
  uint64_t chars_bytes;
  uint32_t n_entries;
  uint32_t reserved;
};

__device__ __forceinline__ uint32_t chunk_of(const OutLayout& l, uint32_t row) {
  return l.row_base ? last_at_or_below(l.row_base, l.n_chunks, row) : row / l.chunk_rows;
}

__device__ __forceinline__ uint64_t chunk_begin(const OutLayout& l, uint32_t chunk) {   // chunk <= n_chunks
  return l.row_base ? l.row_base[chunk] : min(uint64_t{chunk} * l.chunk_rows, uint64_t{l.n});
}

// ---- front ends: a row's global entry index, or -1 ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void iota_table(int32_t* table, uint32_t n) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) table[i] = static_cast<int32_t>(i);
}

// values / nulls: the stand-in over iota_table, exported (row row_base[c] + o of the column's table)
__global__ __launch_bounds__(WG) void entries_at_positions(const int32_t* values, const uint8_t* nulls, const uint64_t* row_base, uint32_t n_chunks, const hy_row_id* positions,
                                                           uint32_t n, uint32_t n_source_entries, int32_t* entry) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
    const hy_row_id p = positions[i];
    int32_t e = -1;
    if (p.chunk_offset != 0xFFFFFFFFu && p.chunk_id < n_chunks && row_base[p.chunk_id] + p.chunk_offset < row_base[p.chunk_id + 1]) {
      const uint64_t row = row_base[p.chunk_id] + p.chunk_offset;
      if (!nulls[row] && static_cast<uint32_t>(values[row]) < n_source_entries) e = values[row];
    }
    entry[i] = e;
  }
}

// inverse[r] = the smallest entry index whose rank is r (filled with 0xFFFFFFFF before)
__global__ __launch_bounds__(WG) void inverse_ranks(const int32_t* ranks, uint32_t n_source_entries, uint32_t* inverse) {
  for (uint32_t e = blockIdx.x * WG + threadIdx.x; e < n_source_entries; e += gridDim.x * WG) {
    const uint32_t r = static_cast<uint32_t>(ranks[e]);
    if (r < n_source_entries) atomicMin(&inverse[r], e);
  }
}

// values / nulls: the caller's column of ranks, exported
__global__ __launch_bounds__(WG) void entries_of_ranks(const int32_t* values, const uint8_t* nulls, const uint32_t* inverse, uint32_t n, uint32_t n_source_entries, int32_t* entry) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
    const uint32_t r = static_cast<uint32_t>(values[i]);
    entry[i] = (!nulls[i] && r < n_source_entries) ? static_cast<int32_t>(inverse[r]) : -1;   // (the filler 0xFFFFFFFF: -1)
  }
}

// ---- step 2: the sort words --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rank_word(const int32_t* entry, const int32_t* ranks, uint32_t n_source_entries, uint32_t row) {
  const int32_t e = entry[row];
  return e < 0 ? n_source_entries : static_cast<uint32_t>(ranks[e]);   // (ranks run below the entry count)
}

__global__ __launch_bounds__(WG) void rank_words(const int32_t* entry, const int32_t* ranks, uint32_t n_source_entries, uint32_t n, uint32_t* words, uint32_t* ids) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
    words[i] = rank_word(entry, ranks, n_source_entries, i);
    ids[i] = i;
  }
}

__global__ __launch_bounds__(WG) void chunk_words(OutLayout l, const uint32_t* perm, uint32_t* words) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < l.n; i += gridDim.x * WG) words[i] = chunk_of(l, perm[i]);
}

// ---- step 3: heads, value ids, the output entries ----------------------------------------------------------------------------------------------
// local[p] = heads among the sorted rows of p's workgroup up to and including p; tile_heads[workgroup] = its heads
__global__ __launch_bounds__(WG) void key_heads(OutLayout l, const int32_t* entry, const int32_t* ranks, uint32_t n_source_entries, const uint32_t* perm, uint32_t* local,
                                                uint32_t* tile_heads) {
  __shared__ uint32_t s_wave_heads[WG / 64];
  const uint64_t p = uint64_t{blockIdx.x} * WG + threadIdx.x;
  bool head = false;
  if (p < l.n) {
    const uint32_t row = perm[p];
    const uint32_t word = rank_word(entry, ranks, n_source_entries, row);
    head = word != n_source_entries;
    if (head && p > 0) {
      const uint32_t before = perm[p - 1];
      head = word != rank_word(entry, ranks, n_source_entries, before) || chunk_of(l, row) != chunk_of(l, before);
    }
  }
  const uint64_t ballot = __ballot(head);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave_heads[wave] = __popcll(ballot);
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += s_wave_heads[w];
  if (p < l.n) local[p] = before + __popcll(ballot & (~0ull >> (63 - lane)));
  if (threadIdx.x == WG - 1) tile_heads[blockIdx.x] = before + s_wave_heads[wave];
}

// the sum of the first `count` elements of a sequence kept as tile-local inclusive sums and scanned tile sums
template <typename T>
__device__ __forceinline__ T sum_before(const T* local, const T* tiles, uint64_t count) {
  return count == 0 ? T{0} : tiles[(count - 1) / WG] + local[count - 1];
}

// chunk_first[c] = output entries in the chunks before c, c <= n_chunks
__global__ __launch_bounds__(WG) void chunk_firsts(OutLayout l, const uint32_t* local, const uint32_t* tile_heads, uint32_t* chunk_first) {
  const uint32_t c = blockIdx.x * WG + threadIdx.x;
  if (c <= l.n_chunks) chunk_first[c] = sum_before(local, tile_heads, chunk_begin(l, c));
}

__global__ __launch_bounds__(WG) void value_ids(OutLayout l, const int32_t* entry, const uint32_t* perm, const uint32_t* local, const uint32_t* tile_heads, const uint32_t* chunk_first,
                                                char* arena, int32_t* unique_entry) {
  const uint64_t p = uint64_t{blockIdx.x} * WG + threadIdx.x;
  if (p >= l.n) return;
  const uint32_t row = perm[p];
  const int32_t e = entry[row];
  const uint32_t chunk = chunk_of(l, row);
  const uint32_t heads = sum_before(local, tile_heads, p + 1);
  uint32_t* vector = reinterpret_cast<uint32_t*>(arena + (l.vector_at ? l.vector_at[chunk] : chunk * l.vector_stride));
  vector[row - chunk_begin(l, chunk)] = heads - chunk_first[chunk] - (e >= 0 ? 1 : 0);
  if (e >= 0 && heads != sum_before(local, tile_heads, p)) unique_entry[heads - 1] = e;   // a head: output entry heads - 1
}

// ---- step 4: where every output entry's bytes are, and how many ---------------------------------------------------------------------------------
// (windows: what of every source entry the output holds -- SUBSTR -- or nullptr: all of it)
__global__ __launch_bounds__(WG) void unique_lengths(const LikeChunk* chunks, const uint64_t* entry_offsets, uint32_t n_source_chunks, const EntryWindow* windows,
                                                     const SubsetEntry* table, uint32_t n_table, const int32_t* unique_entry, const uint32_t* n_unique, const uint8_t** source,
                                                     uint64_t* local_bytes, uint64_t* tile_bytes) {
  __shared__ uint64_t s_sums[WG];
  const uint64_t u = uint64_t{blockIdx.x} * WG + threadIdx.x;
  const bool mine = u < *n_unique;
  uint64_t length = 0;
  if (mine && table) {   // the sparse route: the entry is an index into the subset's table, the window applied already
    const SubsetEntry found = table[min(static_cast<uint32_t>(unique_entry[u]), n_table - 1)];
    source[u] = found.bytes;
    length = found.length;
  } else if (mine) {
    const uint32_t e = static_cast<uint32_t>(unique_entry[u]);
    const uint32_t c = last_at_or_below(entry_offsets, n_source_chunks, e);
    const LikeChunk chunk = chunks[c];
    const Entry found = entry_of(chunk, min(static_cast<uint32_t>(e - entry_offsets[c]), chunk.n_entries - 1), chunk_bytes(chunk), windows ? windows + entry_offsets[c] : nullptr);
    source[u] = found.bytes;
    length = found.length;
  }
  s_sums[threadIdx.x] = length;
  __syncthreads();
  for (uint32_t step = 1; step < WG; step <<= 1) {   // Hillis-Steele, inclusive
    const uint64_t add = threadIdx.x >= step ? s_sums[threadIdx.x - step] : 0;
    __syncthreads();
    s_sums[threadIdx.x] += add;
    __syncthreads();
  }
  if (mine) local_bytes[u] = s_sums[threadIdx.x];
  if (threadIdx.x == WG - 1) tile_bytes[blockIdx.x] = s_sums[WG - 1];
}

__global__ __launch_bounds__(WG) void chunk_totals(const uint32_t* chunk_first, uint32_t n_chunks, const uint64_t* local_bytes, const uint64_t* tile_bytes, ChunkTotals* totals) {
  const uint32_t c = blockIdx.x * WG + threadIdx.x;
  if (c >= n_chunks) return;
  totals[c] = ChunkTotals{sum_before(local_bytes, tile_bytes, chunk_first[c + 1]) - sum_before(local_bytes, tile_bytes, chunk_first[c]), chunk_first[c + 1] - chunk_first[c], 0};
}

// ---- step 5: offsets and bytes ------------------------------------------------------------------------------------------------------------------
// Chunk c's n_entries + 1 offsets begin at offsets[chunk_first[c] + c], relative to the chunk's first byte.
__global__ __launch_bounds__(WG) void dictionary_offsets(const uint32_t* chunk_first, uint32_t n_chunks, const uint64_t* local_bytes, const uint64_t* tile_bytes, uint32_t n_unique,
                                                         uint32_t* offsets) {
  const uint64_t i = uint64_t{blockIdx.x} * WG + threadIdx.x;
  if (i < n_unique) {
    const uint32_t c = last_at_or_below(chunk_first, n_chunks, i);
    offsets[i + c] = static_cast<uint32_t>(sum_before(local_bytes, tile_bytes, i) - sum_before(local_bytes, tile_bytes, chunk_first[c]));
  }
  if (i < n_chunks)   // the chunk's end
    offsets[chunk_first[i + 1] + i] = static_cast<uint32_t>(sum_before(local_bytes, tile_bytes, chunk_first[i + 1]) - sum_before(local_bytes, tile_bytes, chunk_first[i]));
}

// `count` <= 8 bytes (the low ones of `bytes`, the others zero) to byte `at` of the 16 bytes low | high; at + count <= 16
__device__ __forceinline__ void put_bytes(uint64_t& low, uint64_t& high, uint64_t bytes, uint32_t at) {
  const uint32_t shift = 8 * (at & 7);
  if (at < 8) {
    low |= bytes << shift;
    if (shift) high |= bytes >> (64 - shift);
  } else {
    high |= bytes << shift;
  }
}

// The chars of all output chunks are one stream of `total` bytes, entry u's at [before(u), before(u + 1)); chars: 16-byte aligned, 16 bytes of
// slack behind the stream (the last lane's vector ends there, zero-filled).
__global__ __launch_bounds__(WG) void copy_entry_bytes(const uint8_t* const* source, const uint64_t* local_bytes, const uint64_t* tile_bytes, uint32_t n_unique, uint64_t total,
                                                       uint8_t* chars) {
  __shared__ uint64_t s_before[COPY_TILE + 1];
  const uint64_t first_byte = uint64_t{blockIdx.x} * (WG * COPY_SPAN);   // (< total: the grid covers the stream)
  const uint64_t last_byte = min(first_byte + WG * COPY_SPAN, total) - 1;
  // the entries the workgroup's bytes lie in: [u_first, u_last]
  uint32_t u_first = 0, u_last = 0;
  {
    uint32_t lo = 0, hi = n_unique;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (sum_before(local_bytes, tile_bytes, mid) <= first_byte) lo = mid; else hi = mid;
    }
    u_first = lo;
    hi = n_unique;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (sum_before(local_bytes, tile_bytes, mid) <= last_byte) lo = mid; else hi = mid;
    }
    u_last = lo;
  }
  const bool staged = u_last - u_first < COPY_TILE;   // before(u_first) .. before(u_last + 1): at most COPY_TILE + 1 sums
  if (staged)
    for (uint32_t k = threadIdx.x; k <= u_last - u_first + 1; k += WG) s_before[k] = sum_before(local_bytes, tile_bytes, uint64_t{u_first} + k);
  __syncthreads();
  auto before = [&](uint32_t u) { return staged ? s_before[u - u_first] : sum_before(local_bytes, tile_bytes, u); };
  const uint64_t at = first_byte + threadIdx.x * COPY_SPAN;
  if (at >= total) return;
  uint32_t u = u_first;
  for (uint32_t hi = u_last + 1; hi - u > 1;) {   // the last entry that begins at or before the lane's first byte
    const uint32_t mid = u + (hi - u) / 2;
    if (before(mid) <= at) u = mid; else hi = mid;
  }
  uint64_t low = 0, high = 0;
  uint32_t filled = 0;
  while (filled < COPY_SPAN && at + filled < total) {   // (before(n_unique) == total: u stays below n_unique)
    const uint64_t here = at + filled, end = before(u + 1);
    if (end <= here) { ++u; continue; }   // an empty entry, or the entry is used up
    const uint32_t take = static_cast<uint32_t>(min(end - here, uint64_t{COPY_SPAN - filled}));
    const uint8_t* from = source[u] + (here - before(u));
    uint32_t done = 0;
    for (; done + 8 <= take; done += 8) {
      uint64_t w;
      __builtin_memcpy(&w, from + done, 8);
      put_bytes(low, high, w, filled + done);
    }
    if (done + 4 <= take) {
      uint32_t w;
      __builtin_memcpy(&w, from + done, 4);
      put_bytes(low, high, w, filled + done);
      done += 4;
    }
    for (; done < take; ++done) put_bytes(low, high, from[done], filled + done);
    filled += take;
  }
  *reinterpret_cast<u32x4_t*>(chars + at) = u32x4_t{static_cast<uint32_t>(low), static_cast<uint32_t>(low >> 32), static_cast<uint32_t>(high), static_cast<uint32_t>(high >> 32)};
}

// ---- the sparse route: the column read AT the rows, the entries they reference as a table ---------------------------------------------------
// Which entries the rows reference is a bitmap over the E entries (bit e of word e / 64), set with one vector atomicOr per non-NULL row: the
// result does not depend on any order, an entry's subset index is a popcount (bits below it), and the entries come out ascending -- chunk
// by chunk, inside a chunk in dictionary order -- without a sort.
struct RowSource {
  const DevSegment* segments;       // the column's: dictionary segments, or reference segments over them
  const uint64_t* row_base;         // [n_chunks + 1]
  const uint64_t* entry_offsets;    // [n_data_chunks + 1], the data column's dictionaries
  uint32_t n_chunks;
  uint32_t n_data_chunks;
};

// element `row` of an attribute vector of 1, 2 or 4 bytes at any byte address, or of a bit-packed one (little-endian stream of 64-bit words)
__device__ __forceinline__ uint32_t value_id_at(const DevSegment& s, uint32_t row) {
  if (seg_is_packed(s)) {
    const uint64_t* words = static_cast<const uint64_t*>(s.data);
    const uint32_t bits = seg_bits(s);
    const uint64_t at = uint64_t{row} * bits;
    const uint32_t shift = static_cast<uint32_t>(at & 63);
    uint64_t value = words[at >> 6] >> shift;
    if (shift + bits > 64) value |= words[(at >> 6) + 1] << (64 - shift);
    return static_cast<uint32_t>(value & ((1ull << bits) - 1));
  }
  const uint8_t* data = static_cast<const uint8_t*>(s.data);
  if (s.width == 1) return data[row];
  if (s.width == 2) {
    uint16_t v;
    __builtin_memcpy(&v, data + 2 * size_t{row}, 2);
    return v;
  }
  uint32_t v;
  __builtin_memcpy(&v, data + 4 * size_t{row}, 4);
  return v;
}

// The global entry index of row (chunk_id, chunk_offset) of the column, or -1: a NULL RowID, a RowID outside the table, a NULL row
__device__ __forceinline__ int32_t entry_at_row(const RowSource& src, uint32_t chunk_id, uint32_t chunk_offset) {
  if (chunk_offset == 0xFFFFFFFFu || chunk_id >= src.n_chunks) return -1;
  const DevSegment* s = src.segments + chunk_id;
  if (chunk_offset >= s->size) return -1;
  if (s->encoding == HY_ENC_REFERENCE) {
    hy_row_id r{s->ref_chunk_id, chunk_offset};   // (no list: an EntireChunkPosList)
    if (s->data) r = static_cast<const hy_row_id*>(s->data)[chunk_offset];
    if (r.chunk_offset == 0xFFFFFFFFu || r.chunk_id >= src.n_data_chunks) return -1;
    chunk_id = r.chunk_id;
    chunk_offset = r.chunk_offset;
    s = s->ref + chunk_id;
    if (chunk_offset >= s->size) return -1;
  }
  if (s->encoding != HY_ENC_DICTIONARY || chunk_id >= src.n_data_chunks) return -1;
  const uint32_t value_id = value_id_at(*s, chunk_offset);
  const uint64_t first = src.entry_offsets[chunk_id];
  if (value_id >= s->aux_size || value_id >= src.entry_offsets[chunk_id + 1] - first) return -1;   // (the NULL value id, or one no entry has)
  return static_cast<int32_t>(first + value_id);
}

// entry[i] = the global entry index of row positions[i] -- positions == nullptr: of row i of the column -- and its bit in the bitmap
__global__ __launch_bounds__(WG) void sparse_mark(RowSource src, const hy_row_id* positions, uint32_t n, int32_t* entry, unsigned long long* bitmap) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
    hy_row_id p;
    if (positions) {
      p = positions[i];
    } else {
      p.chunk_id = last_at_or_below(src.row_base, src.n_chunks, i);
      p.chunk_offset = static_cast<uint32_t>(i - src.row_base[p.chunk_id]);
    }
    const int32_t e = entry_at_row(src, p.chunk_id, p.chunk_offset);
    entry[i] = e;
    if (e >= 0) atomicOr(bitmap + (static_cast<uint32_t>(e) >> 6), 1ull << (e & 63));
  }
}

// local[w] = set bits in the words of w's workgroup up to and including w; tile_bits[workgroup] = its bits
__global__ __launch_bounds__(WG) void sparse_count(const unsigned long long* bitmap, uint32_t n_words, uint32_t* local, uint32_t* tile_bits) {
  __shared__ uint32_t s_sums[WG];
  const uint32_t w = blockIdx.x * WG + threadIdx.x;
  s_sums[threadIdx.x] = w < n_words ? static_cast<uint32_t>(__popcll(bitmap[w])) : 0;
  __syncthreads();
  for (uint32_t step = 1; step < WG; step <<= 1) {   // Hillis-Steele, inclusive
    const uint32_t add = threadIdx.x >= step ? s_sums[threadIdx.x - step] : 0;
    __syncthreads();
    s_sums[threadIdx.x] += add;
    __syncthreads();
  }
  if (w < n_words) local[w] = s_sums[threadIdx.x];
  if (threadIdx.x == WG - 1) tile_bits[blockIdx.x] = s_sums[WG - 1];
}

// set bits below bit e of the bitmap: the subset index of entry e, if it is in the subset (e <= E: word e / 64 exists, the bitmap has E / 64 + 1)
__device__ __forceinline__ uint32_t bits_below(const unsigned long long* bitmap, const uint32_t* local, const uint32_t* tile_bits, uint64_t e) {
  return sum_before(local, tile_bits, e >> 6) + static_cast<uint32_t>(__popcll(bitmap[e >> 6] & ((1ull << (e & 63)) - 1)));
}

// The subset's table.  A lane loads one bitmap word, the wave then takes its non-zero words one after the other, lane l the word's bit l:
// the entry's chunk (binary search over entry_offsets), its bytes and length, through the window if there is one.
__global__ __launch_bounds__(WG) void sparse_table(const unsigned long long* bitmap, uint32_t n_words, const uint32_t* local, const uint32_t* tile_bits, const LikeChunk* chunks,
                                                   const uint64_t* entry_offsets, uint32_t n_source_chunks, bool windowed, SubstrArguments substr, uint32_t n_subset, SubsetEntry* table) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_waves = gridDim.x * (WG / 64);
  for (uint64_t base = (uint64_t{blockIdx.x} * (WG / 64) + (threadIdx.x >> 6)) * 64; base < n_words; base += uint64_t{n_waves} * 64) {   // (whole waves)
    const uint64_t w = base + lane;
    const unsigned long long mine = w < n_words ? bitmap[w] : 0ull;
    const uint32_t before_mine = mine ? sum_before(local, tile_bits, w) : 0;
    for (uint64_t pending = __ballot(mine != 0); pending; pending &= pending - 1) {
      const int from = __ffsll(static_cast<unsigned long long>(pending)) - 1;
      const unsigned long long word = __shfl(mine, from);
      const uint32_t before = __shfl(before_mine, from);
      if (!((word >> lane) & 1)) continue;
      const uint32_t index = before + static_cast<uint32_t>(__popcll(word & ((1ull << lane) - 1)));
      if (index >= n_subset) continue;   // (cannot happen: the counts are the bitmap's)
      const uint64_t e = (base + from) * 64 + lane;
      const uint32_t c = last_at_or_below(entry_offsets, n_source_chunks, e);
      const LikeChunk chunk = chunks[c];
      Entry found = entry_of(chunk, min(static_cast<uint32_t>(e - entry_offsets[c]), chunk.n_entries - 1), chunk_bytes(chunk));
      if (windowed) {
        const EntryWindow window = substr_window(found.length, substr.start, substr.length);
        found = Entry{found.bytes + window.begin, window.length};
      }
      table[index] = SubsetEntry{found.bytes, found.length, 0};
    }
  }
}

// entry[i]: global entry index -> subset index; run_offsets[c] = subset entries of the source chunks before c, c <= n_source_chunks
__global__ __launch_bounds__(WG) void sparse_indices(const unsigned long long* bitmap, const uint32_t* local, const uint32_t* tile_bits, const uint64_t* entry_offsets,
                                                     uint32_t n_source_chunks, uint32_t n, int32_t* entry, uint64_t* run_offsets) {
  for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n || i <= n_source_chunks; i += gridDim.x * WG) {
    if (i < n && entry[i] >= 0) entry[i] = static_cast<int32_t>(bits_below(bitmap, local, tile_bits, static_cast<uint32_t>(entry[i])));
    if (i <= n_source_chunks) run_offsets[i] = bits_below(bitmap, local, tile_bits, entry_offsets[i]);
  }
}

uint32_t tiles_of(uint64_t items) { return static_cast<uint32_t>((items + WG - 1) / WG); }

uint64_t entries_of(const hy_string_dictionary* dict) { return dict->entry_offsets[dict->n_chunks]; }

// Destroys a column when the scope ends (the stand-in of the RowID front end: it lives as long as the launches that read it)
struct ColumnGuard {
  hy_column* column = nullptr;
  ~ColumnGuard() { if (column) (void)hy_column_destroy(column); }
};

// ---- the temporaries in the scratch arena, as layouts: sizing is a dry run of them ----------------------------------------------------------
struct SourceBlocks {   // the dense routes: the dictionary ranked
  int32_t* ranks;         // [E]
  EntryWindow* windows;   // [E], with SUBSTR
  uint32_t* inverse;      // [E], the rank front end
  MergeBlocks merge;
};
struct SparseBlocks {   // the sparse front end, before the subset's size is known
  unsigned long long* bitmap;
  uint32_t* local;
  uint32_t* tile_bits;
  uint32_t* n_subset;
  uint64_t* run_offsets;
};
struct SubsetBlocks {   // ... and behind it
  SubsetEntry* table;
  int32_t* ranks;
  MergeBlocks merge;
};
struct BackEndBlocks {
  uint32_t* local;
  uint32_t* tile_heads;
  uint32_t* chunk_first;
  int32_t* unique_entry;
  const uint8_t** source;
  uint64_t* local_bytes;
  uint64_t* tile_bytes;
  ChunkTotals* totals;
  uint32_t* n_unique;
  uint64_t* total_bytes;
  uint64_t* row_base;    // the chunks of another column: their first rows and where their vectors begin
  uint64_t* vector_at;
};
struct RequestBlocks {
  SourceBlocks source;
  SparseBlocks sparse;
  SubsetBlocks subset;
  BackEndBlocks back;
};

void source_layout(Carver& carver, const StringRequest& rq, SourceBlocks& b) {
  const uint64_t n_source_entries = entries_of(rq.dict);
  b = SourceBlocks{};
  if (rq.route == StringRoute::Ranks) b.inverse = carver.take<uint32_t>(n_source_entries);
  if (!n_source_entries) return;
  b.ranks = carver.take<int32_t>(n_source_entries);
  if (rq.substr) b.windows = carver.take<EntryWindow>(n_source_entries);
  merge_layout(carver, n_source_entries, b.merge);
}

// one bit per source entry with 4 bytes of counts per 64 entries, per source chunk 8 -- nothing else that grows with E or the column's rows
void sparse_layout(Carver& carver, const hy_string_dictionary* dict, SparseBlocks& b) {
  const uint64_t n_words = entries_of(dict) / 64 + 1;
  b.bitmap = carver.take<unsigned long long>(n_words);
  b.local = carver.take<uint32_t>(n_words);
  b.tile_bits = carver.take<uint32_t>(tiles_of(n_words));
  b.n_subset = carver.take<uint32_t>(1);
  b.run_offsets = carver.take<uint64_t>(size_t{dict->n_chunks} + 1);
}

// per subset entry 16 bytes of table, 4 of ranks and the merge's 16; sized at the bound min(n, E), carved at the U the device counted
void subset_layout(Carver& carver, uint64_t n_subset, SubsetBlocks& b) {
  b = SubsetBlocks{};
  if (!n_subset) return;
  b.table = carver.take<SubsetEntry>(n_subset);
  b.ranks = carver.take<int32_t>(n_subset);
  merge_layout(carver, n_subset, b.merge);
}

void back_end_layout(Carver& carver, const OutChunks& out, BackEndBlocks& b) {
  const uint64_t n = out.n, n_chunks = out.sizes.size(), n_tiles = tiles_of(n);
  b.local = carver.take<uint32_t>(n);
  b.tile_heads = carver.take<uint32_t>(n_tiles);
  b.chunk_first = carver.take<uint32_t>(n_chunks + 1);
  b.unique_entry = carver.take<int32_t>(n);
  b.source = carver.take<const uint8_t*>(n);
  b.local_bytes = carver.take<uint64_t>(n);
  b.tile_bytes = carver.take<uint64_t>(n_tiles);
  b.totals = carver.take<ChunkTotals>(n_chunks);
  b.n_unique = carver.take<uint32_t>(1);
  b.total_bytes = carver.take<uint64_t>(1);
  b.row_base = out.chunk_rows ? nullptr : carver.take<uint64_t>(n_chunks + 1);
  b.vector_at = out.chunk_rows ? nullptr : carver.take<uint64_t>(n_chunks + 1);
}

void request_layout(Carver& carver, const StringRequest& rq, uint64_t n_subset, RequestBlocks& b) {
  if (rq.route == StringRoute::Sparse) {
    sparse_layout(carver, rq.dict, b.sparse);
    subset_layout(carver, n_subset, b.subset);
  } else {
    source_layout(carver, rq, b.source);
  }
  back_end_layout(carver, rq.out, b.back);
}

// Stage 1: the arena sized for the whole request (the subset at its bound), then everything carved that does not wait for the subset's size
hy_status reserve_request(const StringRequest& rq, RequestBlocks& blocks) {
  Carver sizing;
  request_layout(sizing, rq, std::min(rq.n, entries_of(rq.dict)), blocks);
  HY_TRY(scratch().reserve(sizing.used));
  Carver carver{&scratch()};
  request_layout(carver, rq, 0, blocks);
  return carver.failed ? fail(HY_ERR_DEVICE, "scratch arena exhausted") : HY_OK;
}

// The pool blocks of the front ends: the stand-in's table and its export (RowIDs, rows), the export of the ranks, every row's entry
struct FrontBuffers {
  DeviceBuffer table, values, nulls, entry;
  ColumnGuard stand_in;
  hy_status alloc(const StringRequest& rq) {
    if (rq.route != StringRoute::Sparse) {
      if (rq.route != StringRoute::Ranks) HY_TRY(table.alloc(4 * entries_of(rq.dict) + 16));
      HY_TRY(values.alloc(4 * rq.column->rows + 16));
      HY_TRY(nulls.alloc(rq.column->rows + 16));
    }
    return entry.alloc(4 * rq.n + 16);
  }
};

// What the back end reads of the source: the dictionary with its order (d_ranks: nullptr for a dictionary without entries) and, with SUBSTR, what
// of every entry the output holds; or -- `subset`, the sparse route -- a table of the referenced entries with its order, windows applied already.
struct SparseSubset {
  const SubsetEntry* table = nullptr;   // [n]
  const int32_t* ranks = nullptr;       // [n]: equal strings (of different source chunks, or equal windows) have one rank
  uint32_t n = 0;                       // U
};
struct RankedSource {
  const hy_string_dictionary* dict;
  const int32_t* d_ranks;
  const EntryWindow* d_windows;
  const SparseSubset* subset;
};

hy_status device_status(hipError_t err, const char* name) { return err == hipSuccess ? HY_OK : fail(HY_ERR_DEVICE, "%s: %s", name, hipGetErrorString(err)); }

// Stage 2, dense routes: the windows, then the dictionary's order as they read.  A dictionary without entries has neither.
hy_status rank_dictionary(const StringRequest& rq, const SourceBlocks& b, hipStream_t stream, RankedSource* source) {
  if (!entries_of(rq.dict)) return HY_OK;
  if (rq.substr) entry_windows_launch(rq.dict, *rq.substr, b.windows, stream);
  HY_TRY(column_order_launch(rq.dict, b.merge, b.ranks, stream, b.windows, windows_keep_order(rq.substr)));
  source->d_ranks = b.ranks;
  source->d_windows = b.windows;
  return HY_OK;
}

// Stage 3, rows of the column or at RowIDs: the column's stand-in over 0, 1, 2, ... exported -- every source row's global entry index --
// then one lookup per output row
hy_status stand_in_entries(const StringRequest& rq, FrontBuffers& f, hipStream_t stream) {
  const uint64_t n_source_entries = entries_of(rq.dict);
  hy_status st = string_stand_in(rq.column, rq.dict, f.table.as<int32_t>(), &f.stand_in.column);
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  if (st == HY_OK && n_source_entries) hipLaunchKernelGGL(iota_table, dim3(grid_for(n_source_entries)), dim3(WG), 0, stream, f.table.as<int32_t>(), static_cast<uint32_t>(n_source_entries));
  if (st == HY_OK && rq.n) st = export_column_at(f.stand_in.column, f.values.ptr, f.nulls.as<uint8_t>(), nullptr);
  if (st == HY_OK && rq.n && rq.route == StringRoute::RowIds)
    hipLaunchKernelGGL(entries_at_positions, dim3(grid_for(rq.n)), dim3(WG), 0, stream, f.values.as<int32_t>(), f.nulls.as<uint8_t>(), rq.column->d_row_base, rq.column->n_chunks, rq.positions,
                       static_cast<uint32_t>(rq.n), static_cast<uint32_t>(n_source_entries), f.entry.as<int32_t>());
  else if (st == HY_OK && rq.n) entries_of_rows_launch(f.values.as<int32_t>(), f.nulls.as<uint8_t>(), rq.n, n_source_entries, f.entry.as<int32_t>(), stream);
  profile_end(stream);
  return st;
}

// Stage 3, ranks: the inverse table rank -> smallest entry with that rank, then one lookup per row of the exported ranks
hy_status rank_entries(const StringRequest& rq, const SourceBlocks& b, FrontBuffers& f, hipStream_t stream) {
  const uint64_t n_source_entries = entries_of(rq.dict);
  hy_status st = HY_OK;
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  if (n_source_entries) {
    st = device_status(hipMemsetAsync(b.inverse, 0xFF, 4 * n_source_entries, stream), rq.name);
    if (st == HY_OK) hipLaunchKernelGGL(inverse_ranks, dim3(grid_for(n_source_entries)), dim3(WG), 0, stream, b.ranks, static_cast<uint32_t>(n_source_entries), b.inverse);
  }
  if (st == HY_OK && rq.n) st = export_column_at(rq.column, f.values.ptr, f.nulls.as<uint8_t>(), nullptr);
  if (st == HY_OK && rq.n)
    hipLaunchKernelGGL(entries_of_ranks, dim3(grid_for(rq.n)), dim3(WG), 0, stream, f.values.as<int32_t>(), f.nulls.as<uint8_t>(), b.inverse, static_cast<uint32_t>(rq.n),
                       static_cast<uint32_t>(n_source_entries), f.entry.as<int32_t>());
  profile_end(stream);
  return st;
}

// Stage 3, sparse: the column read at the rows, the entries they reference marked and counted; *n_subset = U crosses to the host (4 bytes)
hy_status sparse_mark_and_count(const StringRequest& rq, const SparseBlocks& b, int32_t* d_entry, hipStream_t stream, uint32_t* n_subset) {
  const uint64_t n_source_entries = entries_of(rq.dict);
  const uint32_t n_words = static_cast<uint32_t>(n_source_entries / 64 + 1), n_word_tiles = tiles_of(n_words);
  const hy_column* data_column = rq.column->is_reference ? rq.column->ref : rq.column;
  const RowSource src{rq.column->d_segments, rq.column->d_row_base, rq.dict->d_entry_offsets, rq.column->n_chunks, data_column ? data_column->n_chunks : 0};
  HY_TRY(device_status(hipMemsetAsync(b.bitmap, 0, 8 * size_t{n_words}, stream), rq.name));
  hipLaunchKernelGGL(sparse_mark, dim3(grid_for(rq.n)), dim3(WG), 0, stream, src, rq.positions, static_cast<uint32_t>(rq.n), d_entry, b.bitmap);
  hipLaunchKernelGGL(sparse_count, dim3(n_word_tiles), dim3(WG), 0, stream, b.bitmap, n_words, b.local, b.tile_bits);
  hipLaunchKernelGGL(scan_tiles<uint32_t>, dim3(1), dim3(SCAN_WG), 0, stream, b.tile_bits, n_word_tiles, b.n_subset);
  HY_TRY(device_status(hipGetLastError(), rq.name));
  HY_TRY(device_status(hipMemcpyAsync(n_subset, b.n_subset, 4, hipMemcpyDeviceToHost, stream), rq.name));
  HY_TRY(device_status(hipStreamSynchronize(stream), rq.name));
  if (*n_subset > std::min(rq.n, n_source_entries)) return fail(HY_ERR_DEVICE, "%s: %u entries marked by %llu rows", rq.name, *n_subset, static_cast<unsigned long long>(rq.n));
  return HY_OK;
}

// ... the subset's table, every row's index into it, and (stage 2 of this route) the subset ranked.  U == 0: every row is NULL, every entry -1 already.
hy_status sparse_entries(const StringRequest& rq, RequestBlocks& blocks, int32_t* d_entry, hipStream_t stream, SparseSubset* subset) {
  const SparseBlocks& b = blocks.sparse;
  const hy_string_dictionary* dict = rq.dict;
  const uint32_t n_words = static_cast<uint32_t>(entries_of(dict) / 64 + 1);
  uint32_t n_subset = 0;
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  hy_status st = sparse_mark_and_count(rq, b, d_entry, stream, &n_subset);
  if (st == HY_OK && n_subset) {
    Carver carver{&scratch()};
    subset_layout(carver, n_subset, blocks.subset);
    if (carver.failed) st = fail(HY_ERR_DEVICE, "scratch arena exhausted");
  }
  if (st == HY_OK && n_subset) {
    const SubstrArguments window = rq.substr ? *rq.substr : SubstrArguments{0, 0};
    hipLaunchKernelGGL(sparse_table, dim3(std::min<uint32_t>(tiles_of(n_words), 4096)), dim3(WG), 0, stream, b.bitmap, n_words, b.local, b.tile_bits, dict->d_chunks, dict->d_entry_offsets,
                       dict->n_chunks, rq.substr != nullptr, window, n_subset, blocks.subset.table);
    hipLaunchKernelGGL(sparse_indices, dim3(grid_for(std::max<uint64_t>(rq.n, uint64_t{dict->n_chunks} + 1))), dim3(WG), 0, stream, b.bitmap, b.local, b.tile_bits, dict->d_entry_offsets,
                       dict->n_chunks, static_cast<uint32_t>(rq.n), d_entry, b.run_offsets);
    st = device_status(hipGetLastError(), rq.name);
  }
  profile_end(stream);
  if (st != HY_OK || !n_subset) return st;
  // sorted runs stay runs; single positions where a window unsorts them, and where the entries are fewer than the chunks (fewer rounds)
  HY_TRY(table_order_launch(blocks.subset.table, b.run_offsets, dict->n_chunks, n_subset, !windows_keep_order(rq.substr) || n_subset < dict->n_chunks, blocks.subset.merge,
                            blocks.subset.ranks, stream));
  *subset = SparseSubset{blocks.subset.table, blocks.subset.ranks, n_subset};
  return HY_OK;
}

// ---- stage 4, the back end -----------------------------------------------------------------------------------------------------------------
// The results' own memory -- the pooled arena of the attribute vectors (chunk c's vector 256-byte aligned with 16 bytes of slack,
// hy_column_gather's layout) and the dictionary's block of offsets and chars -- given back unless the results took it
struct ResultMemory {
  char* arena = nullptr;
  size_t arena_capacity = 0;
  void* dictionary_block = nullptr;
  ~ResultMemory() {
    if (arena) pool_release(arena, arena_capacity);
    if (dictionary_block) (void)hipFree(dictionary_block);
  }
};

struct Gather {
  const StringRequest& rq;
  const RankedSource& source;
  const int32_t* d_entry;
  const BackEndBlocks& b;
  hipStream_t stream;
  const uint32_t n, n_chunks, n_tiles;
  const uint32_t n_source_entries;   // what the ranks run below and d_entry indexes: the dictionary's entries, or the subset's
  std::vector<uint64_t> row_base, vector_at;
  std::vector<ChunkTotals> totals;   // (chunks without rows -- a column of empty chunks -- have no entries: nothing is launched for them)
  OutLayout layout{};
  WordSort order;
  ResultMemory memory;
  uint64_t n_unique = 0, total_bytes = 0;
  uint32_t* d_offsets = nullptr;
  uint8_t* d_chars = nullptr;

  Gather(const StringRequest& request, const RankedSource& ranked, const int32_t* entry, const BackEndBlocks& blocks, hipStream_t on)
      : rq(request), source(ranked), d_entry(entry), b(blocks), stream(on), n(static_cast<uint32_t>(request.out.n)), n_chunks(static_cast<uint32_t>(request.out.sizes.size())),
        n_tiles(tiles_of(request.out.n)), n_source_entries(ranked.subset ? ranked.subset->n : static_cast<uint32_t>(entries_of(ranked.dict))), row_base(size_t{n_chunks} + 1, 0),
        vector_at(size_t{n_chunks} + 1, 0), totals(n_chunks) {}

  hy_status check(hipError_t err) const { return device_status(err, rq.name); }

  // where every output chunk's rows and attribute vector begin; the arena; for the chunks of another column the two tables uploaded
  hy_status output_layout() {
    const OutChunks& out = rq.out;
    for (uint32_t c = 0; c < n_chunks; ++c) {
      row_base[c + 1] = row_base[c] + out.sizes[c];
      vector_at[c + 1] = vector_at[c] + align_up(4 * uint64_t{out.sizes[c]} + 16, 256);
    }
    HY_TRY(pool_acquire(vector_at[n_chunks] + 256, reinterpret_cast<void**>(&memory.arena), &memory.arena_capacity));
    layout = OutLayout{nullptr, nullptr, n_chunks ? vector_at[1] : 0, out.chunk_rows, n_chunks, n};
    if (out.chunk_rows) return HY_OK;
    HY_TRY(check(hipMemcpyAsync(b.row_base, row_base.data(), 8 * row_base.size(), hipMemcpyHostToDevice, stream)));
    HY_TRY(check(hipMemcpyAsync(b.vector_at, vector_at.data(), 8 * vector_at.size(), hipMemcpyHostToDevice, stream)));
    HY_TRY(check(hipStreamSynchronize(stream)));   // (the host vectors are pageable)
    layout.row_base = b.row_base;
    layout.vector_at = b.vector_at;
    return HY_OK;
  }

  // 2: the rows by (output chunk, rank)
  hy_status order_rows() {
    hipLaunchKernelGGL(rank_words, dim3(grid_for(n)), dim3(WG), 0, stream, d_entry, source.d_ranks, n_source_entries, n, order.key_words(), order.ids());
    HY_TRY(order.sort(n, n_source_entries ? 32 - static_cast<uint32_t>(__builtin_clz(n_source_entries)) : 0, stream));
    if (n_chunks == 1) return HY_OK;
    hipLaunchKernelGGL(chunk_words, dim3(grid_for(n)), dim3(WG), 0, stream, layout, order.perm, order.key_words());
    return order.sort(n, 32 - static_cast<uint32_t>(__builtin_clz(n_chunks - 1)), stream);
  }

  // 3: heads and value ids
  void heads_and_value_ids() {
    hipLaunchKernelGGL(key_heads, dim3(n_tiles), dim3(WG), 0, stream, layout, d_entry, source.d_ranks, n_source_entries, order.perm, b.local, b.tile_heads);
    hipLaunchKernelGGL(scan_tiles<uint32_t>, dim3(1), dim3(SCAN_WG), 0, stream, b.tile_heads, n_tiles, b.n_unique);
    hipLaunchKernelGGL(chunk_firsts, dim3(tiles_of(uint64_t{n_chunks} + 1)), dim3(WG), 0, stream, layout, b.local, b.tile_heads, b.chunk_first);
    hipLaunchKernelGGL(value_ids, dim3(n_tiles), dim3(WG), 0, stream, layout, d_entry, order.perm, b.local, b.tile_heads, b.chunk_first, memory.arena, b.unique_entry);
  }

  // 4: every output entry's bytes, and per output chunk the entry count and the chars' bytes to the host in ONE copy
  hy_status entry_bytes() {
    const SparseSubset* subset = source.subset;
    hipLaunchKernelGGL(unique_lengths, dim3(n_tiles), dim3(WG), 0, stream, source.dict->d_chunks, source.dict->d_entry_offsets, source.dict->n_chunks, source.d_windows,
                       subset ? subset->table : nullptr, subset ? subset->n : 0, b.unique_entry, b.n_unique, b.source, b.local_bytes, b.tile_bytes);
    hipLaunchKernelGGL(scan_tiles<uint64_t>, dim3(1), dim3(SCAN_WG), 0, stream, b.tile_bytes, n_tiles, b.total_bytes);
    hipLaunchKernelGGL(chunk_totals, dim3(tiles_of(n_chunks)), dim3(WG), 0, stream, b.chunk_first, n_chunks, b.local_bytes, b.tile_bytes, b.totals);
    HY_TRY(check(hipGetLastError()));
    HY_TRY(check(hipMemcpyAsync(totals.data(), b.totals, sizeof(ChunkTotals) * n_chunks, hipMemcpyDeviceToHost, stream)));
    return check(hipStreamSynchronize(stream));
  }

  // 5: offsets and chars, one allocation that the dictionary will own
  hy_status dictionary_block() {
    for (uint32_t c = 0; c < n_chunks; ++c) {
      if (totals[c].chars_bytes >= (uint64_t{1} << 32))
        return fail(HY_ERR_UNSUPPORTED, "%s: output chunk %u: %llu bytes of chars do not fit 32-bit offsets", rq.name, c, static_cast<unsigned long long>(totals[c].chars_bytes));
      n_unique += totals[c].n_entries;
      total_bytes += totals[c].chars_bytes;
    }
    const size_t offsets_bytes = align_up(4 * (n_unique + n_chunks) + 16, 256);
    const hy_status allocated = check(hipMalloc(&memory.dictionary_block, offsets_bytes + align_up(total_bytes + 2 * COPY_SPAN, 256)));
    if (allocated != HY_OK) { memory.dictionary_block = nullptr; return allocated; }
    d_offsets = static_cast<uint32_t*>(memory.dictionary_block);
    d_chars = static_cast<uint8_t*>(memory.dictionary_block) + offsets_bytes;
    if (n) hipLaunchKernelGGL(dictionary_offsets, dim3(tiles_of(std::max<uint64_t>(n_unique, n_chunks))), dim3(WG), 0, stream, b.chunk_first, n_chunks, b.local_bytes, b.tile_bytes,
                              static_cast<uint32_t>(n_unique), d_offsets);
    else HY_TRY(check(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream)));   // (every chunk's one offset)
    if (total_bytes)
      hipLaunchKernelGGL(copy_entry_bytes, dim3(static_cast<uint32_t>((total_bytes + WG * COPY_SPAN - 1) / (WG * COPY_SPAN))), dim3(WG), 0, stream, b.source, b.local_bytes, b.tile_bytes,
                         static_cast<uint32_t>(n_unique), total_bytes, d_chars);
    profile_end(stream);
    HY_TRY(check(hipGetLastError()));
    return check(hipStreamSynchronize(stream));
  }

  // the handles: a dictionary over the block (caller-owned layout: pure host work), which it then owns; a column over the arena
  hy_status handles() {
    std::vector<hy_string_dictionary_chunk> chunks(n_chunks ? n_chunks : 1);
    std::vector<hy_segment> segments(n_chunks ? n_chunks : 1);
    uint64_t first_entry = 0, first_byte = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
      chunks[c] = hy_string_dictionary_chunk{totals[c].n_entries, 0, reinterpret_cast<const char*>(d_chars + first_byte), d_offsets + first_entry + c};
      hy_segment& s = segments[c];
      std::memset(&s, 0, sizeof(s));
      s.encoding = HY_ENC_DICTIONARY;
      s.data_type = HY_TYPE_STRING;
      s.size = rq.out.sizes[c];
      s.width = 4;
      s.data = memory.arena + vector_at[c];
      s.aux_size = totals[c].n_entries;
      s.ref_chunk_id = 0xFFFFFFFFu;
      first_entry += totals[c].n_entries;
      first_byte += totals[c].chars_bytes;
    }
    hy_string_dictionary* made = nullptr;
    HY_TRY(hy_string_dictionary_create(chunks.data(), n_chunks, HY_MEM_DEVICE, &made));
    hy_column* gathered = nullptr;
    const hy_status st = hy_column_create(segments.data(), n_chunks, HY_MEM_DEVICE, &gathered);
    if (st != HY_OK) {
      (void)hy_string_dictionary_destroy(made);
      return st;
    }
    made->owned.push_back(memory.dictionary_block);
    for (uint32_t c = 0; c < n_chunks; ++c) made->chars_bytes[c] = totals[c].chars_bytes;
    gathered->pooled.emplace_back(memory.arena_capacity, memory.arena);
    memory = ResultMemory{};
    *rq.result = gathered;
    *rq.result_dict = made;
    return HY_OK;
  }
};

// d_entry: per output row the global entry index into the dictionary (the sparse route: into the subset's table), or -1; the source's order
// is queued on `stream` already.  Steps 2 to 5 of the file's header, then the handles.
hy_status gather_entries(const StringRequest& rq, const RankedSource& source, const int32_t* d_entry, const BackEndBlocks& blocks, hipStream_t stream) {
  Gather g(rq, source, d_entry, blocks, stream);
  hy_status st = g.output_layout();
  if (st == HY_OK) st = g.order.alloc(g.n);
  if (st == HY_OK && g.n) {
    profile_begin(stream, HY_KERNEL_STRING_RANK);
    st = g.order_rows();
    if (st == HY_OK) g.heads_and_value_ids();
    if (st == HY_OK) st = g.entry_bytes();
  }
  if (st == HY_OK) st = g.dictionary_block();
  if (st == HY_OK) st = g.handles();
  if (st != HY_OK) {   // (launches may be queued: the arena and the block go back behind them)
    profile_end(stream);
    (void)hipStreamSynchronize(stream);
  }
  return st;
}

// Results without rows: a column and a dictionary of zero chunks
hy_status empty_string_results(hy_column** result, hy_string_dictionary** result_dict) {
  hy_string_dictionary_chunk no_chunk{};
  hy_segment no_segment{};
  HY_TRY(hy_string_dictionary_create(&no_chunk, 0, HY_MEM_DEVICE, result_dict));
  const hy_status st = hy_column_create(&no_segment, 0, HY_MEM_DEVICE, result);
  if (st != HY_OK) {
    (void)hy_string_dictionary_destroy(*result_dict);
    *result_dict = nullptr;
  }
  return st;
}

// Which route n rows out of a column of `column_rows` rows and E entries take: column_rows + E is what the dense route reads whatever n is
bool string_sparse_route(uint64_t n, uint64_t column_rows, uint64_t n_source_entries) {
  const int64_t mode = option(HY_OPT_STRING_SPARSE_GATHER);
  if (mode == 2) return true;
  if (mode != 1 || STRING_SPARSE_DIVISOR <= 0) return false;
  return n <= (column_rows + n_source_entries) / static_cast<uint64_t>(STRING_SPARSE_DIVISOR);
}

// the refusals of hy_string_ranks_gather's column of ranks
hy_status ranks_column_check(const hy_column* ranks, const char* name) {
  HY_TRY(on_this_device(ranks, name));
  if (ranks->is_mvcc || ranks->is_reference || (ranks->data_type != HY_TYPE_INT && ranks->n_chunks)) return fail(HY_ERR_INVALID, "%s: ranks are an int32 data column", name);
  for (const hy_segment& segment : ranks->host_segments)
    if (segment.encoding != HY_ENC_UNENCODED) return fail(HY_ERR_INVALID, "%s: ranks are unencoded segments", name);
  return HY_OK;
}

}  // namespace

hy_status string_request(StringRoute route, const char* name, const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows,
                         const SubstrArguments* substr, hy_column** result, hy_string_dictionary** result_dict, StringRequest* rq, bool* answered) {
  *answered = true;   // (a refusal, or results without rows: there is nothing to run)
  if (result) *result = nullptr;
  if (result_dict) *result_dict = nullptr;
  if (!result || !result_dict || !column || !dict) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (route == StringRoute::RowIds) {
    if (!chunk_rows || (n && !positions)) return fail(HY_ERR_INVALID, "%s: positions missing or chunk_rows == 0", name);
    if (reinterpret_cast<uintptr_t>(positions) % 8 != 0) return fail(HY_ERR_INVALID, "%s: positions not on an 8-byte boundary", name);
  }
  if (route == StringRoute::Ranks) {
    HY_TRY(ranks_column_check(column, name));
    HY_TRY(column_order_check(dict, name));
  } else {
    HY_TRY(string_column_check(column, dict, name));
  }
  const uint64_t rows = route == StringRoute::RowIds ? n : column->rows;
  if (rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows (32-bit row ids)", name, static_cast<unsigned long long>(rows));
  if (route == StringRoute::RowIds ? !rows : !column->n_chunks) return empty_string_results(result, result_dict);
  *rq = StringRequest{name, column, dict, positions, rows, substr, OutChunks{}, route, result, result_dict};
  rq->out.n = rows;
  rq->out.chunk_rows = route == StringRoute::RowIds ? chunk_rows : 0;
  if (route == StringRoute::RowIds)
    for (uint64_t begin = 0; begin < rows; begin += chunk_rows) rq->out.sizes.push_back(static_cast<uint32_t>(std::min<uint64_t>(chunk_rows, rows - begin)));
  else
    for (const hy_segment& segment : column->host_segments) rq->out.sizes.push_back(segment.size);
  if (route != StringRoute::Ranks && string_sparse_route(rows, column->rows, entries_of(dict))) rq->route = StringRoute::Sparse;   // few rows out of a large column
  *answered = false;
  return HY_OK;
}

// The stages of a request.  Every exit behind the first queued launch passes the synchronise at the end, before a temporary goes back to the pool.
hy_status string_request_run(const StringRequest& rq) {
  hipStream_t stream = current_stream();
  FrontBuffers front;
  HY_TRY(front.alloc(rq));
  RequestBlocks blocks;
  HY_TRY(reserve_request(rq, blocks));
  HY_TRY(like_dictionary_tables(rq.dict));
  int32_t* d_entry = front.entry.as<int32_t>();
  SparseSubset subset;
  RankedSource source{rq.dict, nullptr, nullptr, nullptr};
  hy_status st = HY_OK;
  if (rq.route == StringRoute::Sparse) {   // the rows' entries first: they say which entries there are to rank
    if (rq.n) st = sparse_entries(rq, blocks, d_entry, stream, &subset);
    source.subset = &subset;
    source.d_ranks = subset.ranks;
  } else {
    st = rank_dictionary(rq, blocks.source, stream, &source);
    if (st == HY_OK) st = rq.route == StringRoute::Ranks ? rank_entries(rq, blocks.source, front, stream) : stand_in_entries(rq, front, stream);
  }
  if (st == HY_OK) st = gather_entries(rq, source, d_entry, blocks.back, stream);
  (void)hipStreamSynchronize(stream);   // (the temporaries go back to the pool, the stand-in dies)
  return st;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_string_column_gather(const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows, hy_column** result,
                                  hy_string_dictionary** result_dict) {
  StringRequest request;
  bool answered = false;
  HY_TRY(string_request(StringRoute::RowIds, "hy_string_column_gather", column, dict, positions, n, chunk_rows, nullptr, result, result_dict, &request, &answered));
  return answered ? HY_OK : string_request_run(request);
}

hy_status hy_string_ranks_gather(const hy_string_dictionary* dict, const hy_column* ranks, hy_column** result, hy_string_dictionary** result_dict) {
  StringRequest request;
  bool answered = false;
  HY_TRY(string_request(StringRoute::Ranks, "hy_string_ranks_gather", ranks, dict, nullptr, 0, 0, nullptr, result, result_dict, &request, &answered));
  return answered ? HY_OK : string_request_run(request);
}

hy_status hy_string_dictionary_chunk_size(const hy_string_dictionary* dict, uint32_t chunk, uint32_t* n_entries, uint64_t* chars_bytes) {
  const char* name = "hy_string_dictionary_chunk_size";
  if (!dict || !n_entries || !chars_bytes) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (chunk >= dict->n_chunks) return fail(HY_ERR_INVALID, "%s: chunk %u of %u", name, chunk, dict->n_chunks);
  const LikeChunk& c = dict->chunks[chunk];
  if (c.n_entries && !c.offsets) return fail(HY_ERR_UNSUPPORTED, "%s: chunk %u has the fixed-slot layout (the caller holds its bytes)", name, chunk);
  *n_entries = c.n_entries;
  *chars_bytes = 0;
  if (!c.n_entries) return HY_OK;
  HY_TRY(dictionary_device_check(dict, name));
  if (dict->chars_bytes[chunk] == ~0ull) {   // caller-owned offsets, not read yet: once
    uint32_t end = 0;
    hipStream_t stream = current_stream();
    HY_HIP(hipMemcpyAsync(&end, c.offsets + c.n_entries, 4, hipMemcpyDeviceToHost, stream));
    HY_HIP(hipStreamSynchronize(stream));
    dict->chars_bytes[chunk] = end;
  }
  *chars_bytes = dict->chars_bytes[chunk];
  return HY_OK;
}

hy_status hy_string_dictionary_read_chunk(const hy_string_dictionary* dict, uint32_t chunk, char* chars, uint32_t* offsets) {
  const char* name = "hy_string_dictionary_read_chunk";
  if (!dict || !offsets) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (chunk >= dict->n_chunks) return fail(HY_ERR_INVALID, "%s: chunk %u of %u", name, chunk, dict->n_chunks);
  const LikeChunk& c = dict->chunks[chunk];
  if (c.n_entries && !c.offsets) return fail(HY_ERR_UNSUPPORTED, "%s: chunk %u has the fixed-slot layout (the caller holds its bytes)", name, chunk);
  offsets[0] = 0;
  if (!c.n_entries) return HY_OK;
  HY_TRY(dictionary_device_check(dict, name));
  hipStream_t stream = current_stream();
  HY_HIP(hipMemcpyAsync(offsets, c.offsets, 4 * (size_t{c.n_entries} + 1), hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));
  const uint32_t end = offsets[c.n_entries];   // (the offsets are returned as they are: they index the chunk's chars from their first byte)
  if (end) {
    if (!chars) return fail(HY_ERR_INVALID, "%s: null chars for %u bytes", name, end);
    HY_HIP(hipMemcpyAsync(chars, c.chars, end, hipMemcpyDeviceToHost, stream));
    HY_HIP(hipStreamSynchronize(stream));
  }
  return HY_OK;
}

}  // extern "C"

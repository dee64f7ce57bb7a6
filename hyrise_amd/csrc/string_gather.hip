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
// Temporaries.  Scratch arena: per source entry 16 bytes of ranking (order_scratch_bytes) + 4 of ranks (+ 4 of inverse table for the rank front
// end); per output row 4 (entry) + 4 (tile-local heads) + 4 (output entry's source entry) + 8 (its address) + 8 (tile-local byte sums), per
// 256 rows 12, per output chunk 20.  Pool blocks: the word sort's 16 bytes per row; for the RowID front end the stand-in's table (4 per
// source entry) and its export (5 per SOURCE row).  Results: the attribute vectors and null-free segments in one pooled arena owned by the
// column (hy_column_gather's layout); offsets and chars in one allocation owned by the dictionary.
// The sparse route (HY_OPT_STRING_SPARSE_GATHER) is for few rows out of a large column: the column is read AT the rows
// (sparse_mark: PosLists and attribute vectors of any width or packing in place, no stand-in, no export), the entries they reference are
// marked in a bitmap over E and compacted into a table of (address, length), only those are ranked (table_order_launch), and the back end
// reads entries by table index.  Its temporaries follow n and the subset, plus one bit per source entry (sparse_gather_scratch_bytes).
#include "hy_device.hpp"
#include "sort_words.hpp"
#include "string_entries.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace hy {

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t SCAN_WG = 1024;
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

// what gather_entries itself carves
size_t back_end_scratch_bytes(uint64_t n, uint64_t n_chunks) {
  const uint64_t tiles = tiles_of(n);
  return 3 * align_up(4 * n + 16, 256) + 2 * align_up(8 * n + 16, 256) + align_up(4 * tiles, 256) + align_up(8 * tiles, 256) + align_up(4 * (n_chunks + 1), 256) +
         align_up(sizeof(ChunkTotals) * n_chunks, 256) + 2 * align_up(8 * (n_chunks + 1), 256) + 16 * 256 + 4096;
}

}  // namespace

// What gather_entries and the front ends in front of it carve from the scratch arena
size_t gather_scratch_bytes(uint64_t n_source_entries, uint64_t n, uint64_t n_chunks, bool inverse) {
  return (n_source_entries ? order_scratch_bytes(n_source_entries) : 0) + (inverse ? 2 : 1) * align_up(4 * n_source_entries + 16, 256) + back_end_scratch_bytes(n, n_chunks);
}

// Which route n rows out of a column of `column_rows` rows and E entries take: column_rows + E is what the dense route reads whatever n is
bool string_sparse_route(uint64_t n, uint64_t column_rows, uint64_t n_source_entries) {
  const int64_t mode = option(HY_OPT_STRING_SPARSE_GATHER);
  if (mode == 2) return true;
  if (mode != 1 || STRING_SPARSE_DIVISOR <= 0) return false;
  return n <= (column_rows + n_source_entries) / static_cast<uint64_t>(STRING_SPARSE_DIVISOR);
}

// What sparse_entries and gather_entries behind it carve: the bitmap (one bit per source entry) with 4 bytes of counts per 64 entries, per
// subset entry (U <= min(n, E)) 16 of table + 4 of ranks + 16 of ranking, per source chunk 8 -- nothing else that grows with E or the column's rows
size_t sparse_gather_scratch_bytes(uint64_t n_source_entries, uint64_t n_source_chunks, uint64_t n, uint64_t n_chunks) {
  const uint64_t n_words = n_source_entries / 64 + 1, n_subset = std::min(n, n_source_entries);
  return align_up(8 * n_words, 256) + align_up(4 * n_words, 256) + align_up(4 * tiles_of(n_words), 256) + 256 + align_up(8 * (n_source_chunks + 1), 256) +
         align_up(sizeof(SubsetEntry) * n_subset + 16, 256) + align_up(4 * n_subset + 16, 256) + (n_subset ? order_scratch_bytes(n_subset) : 0) + back_end_scratch_bytes(n, n_chunks) + 4096;
}

hy_status sparse_entries(const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, const SubstrArguments* substr, Scratch& sc,
                         int32_t* d_entry, hipStream_t stream, const char* name, SparseSubset* subset) {
  *subset = SparseSubset{};
  const uint64_t n_source_entries = dict->entry_offsets[dict->n_chunks];
  const uint32_t n_words = static_cast<uint32_t>(n_source_entries / 64 + 1), n_word_tiles = tiles_of(n_words);
  unsigned long long* bitmap = carve<unsigned long long>(sc, n_words);
  uint32_t* local = carve<uint32_t>(sc, n_words);
  uint32_t* tile_bits = carve<uint32_t>(sc, n_word_tiles);
  uint32_t* d_n_subset = carve<uint32_t>(sc, 1);
  uint64_t* run_offsets = carve<uint64_t>(sc, size_t{dict->n_chunks} + 1);
  if (!bitmap || !local || !tile_bits || !d_n_subset || !run_offsets) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
  auto check = [&](hipError_t err) { return err == hipSuccess ? HY_OK : fail(HY_ERR_DEVICE, "%s: %s", name, hipGetErrorString(err)); };
  const hy_column* data_column = column->is_reference ? column->ref : column;
  const RowSource src{column->d_segments, column->d_row_base, dict->d_entry_offsets, column->n_chunks, data_column ? data_column->n_chunks : 0};
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  hy_status st = check(hipMemsetAsync(bitmap, 0, 8 * size_t{n_words}, stream));
  uint32_t n_subset = 0;
  if (st == HY_OK) {
    hipLaunchKernelGGL(sparse_mark, dim3(grid_for(n)), dim3(WG), 0, stream, src, positions, static_cast<uint32_t>(n), d_entry, bitmap);
    hipLaunchKernelGGL(sparse_count, dim3(n_word_tiles), dim3(WG), 0, stream, bitmap, n_words, local, tile_bits);
    hipLaunchKernelGGL(scan_tiles<uint32_t>, dim3(1), dim3(SCAN_WG), 0, stream, tile_bits, n_word_tiles, d_n_subset);
    st = check(hipGetLastError());
    if (st == HY_OK) st = check(hipMemcpyAsync(&n_subset, d_n_subset, 4, hipMemcpyDeviceToHost, stream));
    if (st == HY_OK) st = check(hipStreamSynchronize(stream));
  }
  if (st == HY_OK && n_subset > std::min(n, n_source_entries)) st = fail(HY_ERR_DEVICE, "%s: %u entries marked by %llu rows", name, n_subset, static_cast<unsigned long long>(n));
  SubsetEntry* table = nullptr;
  int32_t* ranks = nullptr;
  if (st == HY_OK && n_subset) {   // (none: every row is NULL, every entry -1 already)
    table = carve<SubsetEntry>(sc, n_subset);
    ranks = carve<int32_t>(sc, n_subset);
    if (!table || !ranks) st = fail(HY_ERR_DEVICE, "scratch arena exhausted");
  }
  if (st == HY_OK && n_subset) {
    const SubstrArguments window = substr ? *substr : SubstrArguments{0, 0};
    hipLaunchKernelGGL(sparse_table, dim3(std::min<uint32_t>(tiles_of(n_words), 4096)), dim3(WG), 0, stream, bitmap, n_words, local, tile_bits, dict->d_chunks, dict->d_entry_offsets,
                       dict->n_chunks, substr != nullptr, window, n_subset, table);
    hipLaunchKernelGGL(sparse_indices, dim3(grid_for(std::max<uint64_t>(n, uint64_t{dict->n_chunks} + 1))), dim3(WG), 0, stream, bitmap, local, tile_bits, dict->d_entry_offsets,
                       dict->n_chunks, static_cast<uint32_t>(n), d_entry, run_offsets);
    st = check(hipGetLastError());
  }
  profile_end(stream);
  if (st == HY_OK && n_subset) {
    // a window at the entry's first byte keeps a sorted run sorted; single positions also where they are fewer than the chunks (fewer rounds)
    const bool sorted_runs = !substr || substr->length <= 0 || substr->start == 0 || substr->start == 1;
    st = table_order_launch(table, run_offsets, dict->n_chunks, n_subset, !sorted_runs || n_subset < dict->n_chunks, sc, ranks, stream);
  }
  if (st != HY_OK) {   // (launches may be queued: the temporaries go back to the pool behind them)
    (void)hipStreamSynchronize(stream);
    return st;
  }
  subset->table = table;
  subset->ranks = ranks;
  subset->n = n_subset;
  return HY_OK;
}

// The back end.  d_entry: per output row the global entry index into `dict`, or -1; d_ranks: the dictionary's order (column_order_launch), queued
// on `stream` already (nullptr for a dictionary without entries); d_windows: what of every entry the output holds, ranked as such, or nullptr.  The arena `sc` is reserved by the caller (gather_scratch_bytes).
hy_status gather_entries(const hy_string_dictionary* dict, const OutChunks& out, const int32_t* d_entry, const int32_t* d_ranks, const EntryWindow* d_windows, Scratch& sc,
                         hipStream_t stream, const char* name, hy_column** result, hy_string_dictionary** result_dict, const SparseSubset* subset) {
  const uint32_t n = static_cast<uint32_t>(out.n);
  const uint32_t n_chunks = static_cast<uint32_t>(out.sizes.size());
  // (what the ranks run below and d_entry indexes: the dictionary's entries, or the subset's)
  const uint32_t n_source_entries = subset ? subset->n : static_cast<uint32_t>(dict->entry_offsets[dict->n_chunks]);
  const uint32_t n_tiles = tiles_of(n);

  // the attribute vectors: one pooled arena, chunk c's vector 256-byte aligned with 16 bytes of slack (hy_column_gather's layout)
  std::vector<uint64_t> row_base(size_t{n_chunks} + 1, 0), vector_at(size_t{n_chunks} + 1, 0);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    row_base[c + 1] = row_base[c] + out.sizes[c];
    vector_at[c + 1] = vector_at[c] + align_up(4 * uint64_t{out.sizes[c]} + 16, 256);
  }
  char* arena = nullptr;
  size_t arena_capacity = 0;
  HY_TRY(pool_acquire(vector_at[n_chunks] + 256, reinterpret_cast<void**>(&arena), &arena_capacity));
  void* dictionary_block = nullptr;
  auto release = [&](hy_status status) {
    profile_end(stream);
    (void)hipStreamSynchronize(stream);
    pool_release(arena, arena_capacity);
    if (dictionary_block) (void)hipFree(dictionary_block);
    return status;
  };
  auto check = [&](hipError_t err) { return err == hipSuccess ? HY_OK : fail(HY_ERR_DEVICE, "%s: %s", name, hipGetErrorString(err)); };

  OutLayout layout{nullptr, nullptr, n_chunks ? vector_at[1] : 0, out.chunk_rows, n_chunks, n};
  uint32_t* local = carve<uint32_t>(sc, n);
  uint32_t* tile_heads = carve<uint32_t>(sc, n_tiles);
  uint32_t* chunk_first = carve<uint32_t>(sc, size_t{n_chunks} + 1);
  int32_t* unique_entry = carve<int32_t>(sc, n);
  const uint8_t** source = carve<const uint8_t*>(sc, n);
  uint64_t* local_bytes = carve<uint64_t>(sc, n);
  uint64_t* tile_bytes = carve<uint64_t>(sc, n_tiles);
  ChunkTotals* d_totals = carve<ChunkTotals>(sc, n_chunks);
  uint32_t* d_n_unique = carve<uint32_t>(sc, 1);
  uint64_t* d_total_bytes = carve<uint64_t>(sc, 1);
  uint64_t* d_row_base = out.chunk_rows ? nullptr : carve<uint64_t>(sc, size_t{n_chunks} + 1);
  uint64_t* d_vector_at = out.chunk_rows ? nullptr : carve<uint64_t>(sc, size_t{n_chunks} + 1);
  if (!local || !tile_heads || !chunk_first || !unique_entry || !source || !local_bytes || !tile_bytes || !d_totals || !d_n_unique || !d_total_bytes ||
      (!out.chunk_rows && (!d_row_base || !d_vector_at)))
    return release(fail(HY_ERR_DEVICE, "scratch arena exhausted"));
  if (!out.chunk_rows) {
    hy_status st = check(hipMemcpyAsync(d_row_base, row_base.data(), 8 * row_base.size(), hipMemcpyHostToDevice, stream));
    if (st == HY_OK) st = check(hipMemcpyAsync(d_vector_at, vector_at.data(), 8 * vector_at.size(), hipMemcpyHostToDevice, stream));
    if (st == HY_OK) st = check(hipStreamSynchronize(stream));   // (the host vectors are pageable)
    if (st != HY_OK) return release(st);
    layout.row_base = d_row_base;
    layout.vector_at = d_vector_at;
  }

  // 2: the rows by (output chunk, rank)
  WordSort order;
  hy_status st = order.alloc(n);
  if (st != HY_OK) return release(st);
  std::vector<ChunkTotals> totals(n_chunks);   // (chunks without rows -- a column of empty chunks -- have no entries: nothing is launched for them)
  if (n) {
  profile_begin(stream, HY_KERNEL_STRING_RANK);
  hipLaunchKernelGGL(rank_words, dim3(grid_for(n)), dim3(WG), 0, stream, d_entry, d_ranks, n_source_entries, n, order.key_words(), order.ids());
  st = order.sort(n, n_source_entries ? 32 - static_cast<uint32_t>(__builtin_clz(n_source_entries)) : 0, stream);
  if (st == HY_OK && n_chunks > 1) {
    hipLaunchKernelGGL(chunk_words, dim3(grid_for(n)), dim3(WG), 0, stream, layout, order.perm, order.key_words());
    st = order.sort(n, 32 - static_cast<uint32_t>(__builtin_clz(n_chunks - 1)), stream);
  }
  if (st != HY_OK) return release(st);
  // 3 and 4
  hipLaunchKernelGGL(key_heads, dim3(n_tiles), dim3(WG), 0, stream, layout, d_entry, d_ranks, n_source_entries, order.perm, local, tile_heads);
  hipLaunchKernelGGL(scan_tiles<uint32_t>, dim3(1), dim3(SCAN_WG), 0, stream, tile_heads, n_tiles, d_n_unique);
  hipLaunchKernelGGL(chunk_firsts, dim3(tiles_of(uint64_t{n_chunks} + 1)), dim3(WG), 0, stream, layout, local, tile_heads, chunk_first);
  hipLaunchKernelGGL(value_ids, dim3(n_tiles), dim3(WG), 0, stream, layout, d_entry, order.perm, local, tile_heads, chunk_first, arena, unique_entry);
  hipLaunchKernelGGL(unique_lengths, dim3(n_tiles), dim3(WG), 0, stream, dict->d_chunks, dict->d_entry_offsets, dict->n_chunks, d_windows,
                     subset ? subset->table : nullptr, subset ? subset->n : 0, unique_entry, d_n_unique, source, local_bytes, tile_bytes);
  hipLaunchKernelGGL(scan_tiles<uint64_t>, dim3(1), dim3(SCAN_WG), 0, stream, tile_bytes, n_tiles, d_total_bytes);
  hipLaunchKernelGGL(chunk_totals, dim3(tiles_of(n_chunks)), dim3(WG), 0, stream, chunk_first, n_chunks, local_bytes, tile_bytes, d_totals);
  st = check(hipGetLastError());
  if (st == HY_OK) st = check(hipMemcpyAsync(totals.data(), d_totals, sizeof(ChunkTotals) * n_chunks, hipMemcpyDeviceToHost, stream));
  if (st == HY_OK) st = check(hipStreamSynchronize(stream));
  if (st != HY_OK) return release(st);
  }
  uint64_t n_unique = 0, total_bytes = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    if (totals[c].chars_bytes >= (uint64_t{1} << 32))
      return release(fail(HY_ERR_UNSUPPORTED, "%s: output chunk %u: %llu bytes of chars do not fit 32-bit offsets", name, c, static_cast<unsigned long long>(totals[c].chars_bytes)));
    n_unique += totals[c].n_entries;
    total_bytes += totals[c].chars_bytes;
  }
  // 5: offsets and chars, one allocation the dictionary owns
  const size_t offsets_bytes = align_up(4 * (n_unique + n_chunks) + 16, 256);
  st = check(hipMalloc(&dictionary_block, offsets_bytes + align_up(total_bytes + 2 * COPY_SPAN, 256)));
  if (st != HY_OK) { dictionary_block = nullptr; return release(st); }
  uint32_t* d_offsets = static_cast<uint32_t*>(dictionary_block);
  uint8_t* d_chars = static_cast<uint8_t*>(dictionary_block) + offsets_bytes;
  if (n) hipLaunchKernelGGL(dictionary_offsets, dim3(tiles_of(std::max<uint64_t>(n_unique, n_chunks))), dim3(WG), 0, stream, chunk_first, n_chunks, local_bytes, tile_bytes,
                            static_cast<uint32_t>(n_unique), d_offsets);
  else st = check(hipMemsetAsync(d_offsets, 0, offsets_bytes, stream));   // (every chunk's one offset)
  if (st != HY_OK) return release(st);
  if (total_bytes)
    hipLaunchKernelGGL(copy_entry_bytes, dim3(static_cast<uint32_t>((total_bytes + WG * COPY_SPAN - 1) / (WG * COPY_SPAN))), dim3(WG), 0, stream, source, local_bytes, tile_bytes,
                       static_cast<uint32_t>(n_unique), total_bytes, d_chars);
  profile_end(stream);
  st = check(hipGetLastError());
  if (st == HY_OK) st = check(hipStreamSynchronize(stream));
  if (st != HY_OK) return release(st);

  // the handles: a dictionary over the block (caller-owned layout: pure host work), which it then owns; a column over the arena
  std::vector<hy_string_dictionary_chunk> chunks(n_chunks ? n_chunks : 1);
  std::vector<hy_segment> segments(n_chunks ? n_chunks : 1);
  uint64_t first_entry = 0, first_byte = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    chunks[c] = hy_string_dictionary_chunk{totals[c].n_entries, 0, reinterpret_cast<const char*>(d_chars + first_byte), d_offsets + first_entry + c};
    hy_segment& s = segments[c];
    std::memset(&s, 0, sizeof(s));
    s.encoding = HY_ENC_DICTIONARY;
    s.data_type = HY_TYPE_STRING;
    s.size = out.sizes[c];
    s.width = 4;
    s.data = arena + vector_at[c];
    s.aux_size = totals[c].n_entries;
    s.ref_chunk_id = 0xFFFFFFFFu;
    first_entry += totals[c].n_entries;
    first_byte += totals[c].chars_bytes;
  }
  hy_string_dictionary* made = nullptr;
  st = hy_string_dictionary_create(chunks.data(), n_chunks, HY_MEM_DEVICE, &made);
  if (st != HY_OK) return release(st);
  hy_column* gathered = nullptr;
  st = hy_column_create(segments.data(), n_chunks, HY_MEM_DEVICE, &gathered);
  if (st != HY_OK) {
    (void)hy_string_dictionary_destroy(made);
    return release(st);
  }
  made->owned.push_back(dictionary_block);
  for (uint32_t c = 0; c < n_chunks; ++c) made->chars_bytes[c] = totals[c].chars_bytes;
  gathered->pooled.emplace_back(arena_capacity, arena);
  *result = gathered;
  *result_dict = made;
  return HY_OK;
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

namespace {

// Destroys a column when the scope ends (the stand-in of the RowID front end: it lives as long as the launches that read it)
struct ColumnGuard {
  hy_column* column = nullptr;
  ~ColumnGuard() { if (column) (void)hy_column_destroy(column); }
};

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_string_column_gather(const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows, hy_column** result,
                                  hy_string_dictionary** result_dict) {
  const char* name = "hy_string_column_gather";
  if (result) *result = nullptr;
  if (result_dict) *result_dict = nullptr;
  if (!result || !result_dict || !column || !dict) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (!chunk_rows || (n && !positions)) return fail(HY_ERR_INVALID, "%s: positions missing or chunk_rows == 0", name);
  if (reinterpret_cast<uintptr_t>(positions) % 8 != 0) return fail(HY_ERR_INVALID, "%s: positions not on an 8-byte boundary", name);
  HY_TRY(string_column_check(column, dict, name));
  if (n >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows (32-bit row ids)", name, static_cast<unsigned long long>(n));
  if (!n) return empty_string_results(result, result_dict);
  OutChunks out;
  out.n = n;
  out.chunk_rows = chunk_rows;
  for (uint64_t begin = 0; begin < n; begin += chunk_rows) out.sizes.push_back(static_cast<uint32_t>(std::min<uint64_t>(chunk_rows, n - begin)));

  hipStream_t stream = current_stream();
  const uint64_t n_source_entries = dict->entry_offsets[dict->n_chunks];
  if (string_sparse_route(n, column->rows, n_source_entries)) {   // the column read at the RowIDs, the entries they reference ranked
    DeviceBuffer entry;
    HY_TRY(entry.alloc(4 * n + 16));
    Scratch& sc = scratch();
    HY_TRY(sc.reserve(sparse_gather_scratch_bytes(n_source_entries, dict->n_chunks, n, out.sizes.size())));
    HY_TRY(like_dictionary_tables(dict));
    SparseSubset subset;
    hy_status st = sparse_entries(column, dict, positions, n, nullptr, sc, entry.as<int32_t>(), stream, name, &subset);
    if (st == HY_OK) st = gather_entries(dict, out, entry.as<int32_t>(), subset.ranks, nullptr, sc, stream, name, result, result_dict, &subset);
    (void)hipStreamSynchronize(stream);   // (the temporaries go back to the pool)
    return st;
  }
  // the column's stand-in over 0, 1, 2, ... exported: every source row's global entry index
  DeviceBuffer table, values, nulls, entry;
  ColumnGuard stand_in;
  HY_TRY(table.alloc(4 * n_source_entries + 16));
  HY_TRY(values.alloc(4 * column->rows + 16));
  HY_TRY(nulls.alloc(column->rows + 16));
  HY_TRY(entry.alloc(4 * n + 16));
  Scratch& sc = scratch();
  HY_TRY(sc.reserve(gather_scratch_bytes(n_source_entries, n, out.sizes.size(), false)));
  HY_TRY(like_dictionary_tables(dict));
  int32_t* d_ranks = nullptr;
  if (n_source_entries) {
    d_ranks = carve<int32_t>(sc, n_source_entries);
    if (!d_ranks) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
    uint32_t* d_n_distinct = nullptr;
    const hy_status ranked = column_order_launch(dict, sc, d_ranks, &d_n_distinct, stream);
    if (ranked != HY_OK) {   // (launches may be queued: the temporaries go back to the pool behind them)
      (void)hipStreamSynchronize(stream);
      return ranked;
    }
  }
  hy_status st = string_stand_in(column, dict, table.as<int32_t>(), &stand_in.column);
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  if (st == HY_OK && n_source_entries) hipLaunchKernelGGL(iota_table, dim3(grid_for(n_source_entries)), dim3(WG), 0, stream, table.as<int32_t>(), static_cast<uint32_t>(n_source_entries));
  if (st == HY_OK) st = export_column_at(stand_in.column, values.ptr, nulls.as<uint8_t>(), nullptr);
  if (st == HY_OK) hipLaunchKernelGGL(entries_at_positions, dim3(grid_for(n)), dim3(WG), 0, stream, values.as<int32_t>(), nulls.as<uint8_t>(), column->d_row_base, column->n_chunks, positions,
                                           static_cast<uint32_t>(n), static_cast<uint32_t>(n_source_entries), entry.as<int32_t>());
  profile_end(stream);
  if (st == HY_OK) st = gather_entries(dict, out, entry.as<int32_t>(), d_ranks, nullptr, sc, stream, name, result, result_dict);
  (void)hipStreamSynchronize(stream);   // (the temporaries go back to the pool, the stand-in dies)
  return st;
}

hy_status hy_string_ranks_gather(const hy_string_dictionary* dict, const hy_column* ranks, hy_column** result, hy_string_dictionary** result_dict) {
  const char* name = "hy_string_ranks_gather";
  if (result) *result = nullptr;
  if (result_dict) *result_dict = nullptr;
  if (!result || !result_dict || !dict || !ranks) return fail(HY_ERR_INVALID, "%s: null argument", name);
  HY_TRY(on_this_device(ranks, name));
  if (ranks->is_mvcc || ranks->is_reference || (ranks->data_type != HY_TYPE_INT && ranks->n_chunks)) return fail(HY_ERR_INVALID, "%s: ranks are an int32 data column", name);
  for (const hy_segment& segment : ranks->host_segments)
    if (segment.encoding != HY_ENC_UNENCODED) return fail(HY_ERR_INVALID, "%s: ranks are unencoded segments", name);
  HY_TRY(column_order_check(dict, name));
  if (ranks->rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows (32-bit row ids)", name, static_cast<unsigned long long>(ranks->rows));
  if (!ranks->n_chunks) return empty_string_results(result, result_dict);
  OutChunks out;
  out.n = ranks->rows;
  for (const hy_segment& segment : ranks->host_segments) out.sizes.push_back(segment.size);

  hipStream_t stream = current_stream();
  const uint64_t n = ranks->rows, n_source_entries = dict->entry_offsets[dict->n_chunks];
  DeviceBuffer values, nulls, entry;
  HY_TRY(values.alloc(4 * n + 16));
  HY_TRY(nulls.alloc(n + 16));
  HY_TRY(entry.alloc(4 * n + 16));
  Scratch& sc = scratch();
  HY_TRY(sc.reserve(gather_scratch_bytes(n_source_entries, n, out.sizes.size(), true)));
  HY_TRY(like_dictionary_tables(dict));
  int32_t* d_ranks = nullptr;
  uint32_t* inverse = carve<uint32_t>(sc, n_source_entries);
  if (!inverse) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
  hy_status st = HY_OK;
  if (n_source_entries) {
    d_ranks = carve<int32_t>(sc, n_source_entries);
    if (!d_ranks) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
    uint32_t* d_n_distinct = nullptr;
    st = column_order_launch(dict, sc, d_ranks, &d_n_distinct, stream);
  }
  profile_begin(stream, HY_KERNEL_STRING_RANK);   // (the front end: a bracket of its own)
  if (st == HY_OK && n_source_entries) {
    if (hipMemsetAsync(inverse, 0xFF, 4 * n_source_entries, stream) != hipSuccess) st = fail(HY_ERR_DEVICE, "%s: hipMemsetAsync failed", name);
    else hipLaunchKernelGGL(inverse_ranks, dim3(grid_for(n_source_entries)), dim3(WG), 0, stream, d_ranks, static_cast<uint32_t>(n_source_entries), inverse);
  }
  if (st == HY_OK && n) {
    st = export_column_at(ranks, values.ptr, nulls.as<uint8_t>(), nullptr);
    if (st == HY_OK)
      hipLaunchKernelGGL(entries_of_ranks, dim3(grid_for(n)), dim3(WG), 0, stream, values.as<int32_t>(), nulls.as<uint8_t>(), inverse, static_cast<uint32_t>(n),
                         static_cast<uint32_t>(n_source_entries), entry.as<int32_t>());
  }
  profile_end(stream);
  if (st == HY_OK) st = gather_entries(dict, out, entry.as<int32_t>(), d_ranks, nullptr, sc, stream, name, result, result_dict);
  (void)hipStreamSynchronize(stream);
  return st;
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
  if (dict->device != this_thread_device()) return fail(HY_ERR_INVALID, "%s: the dictionary lives on device %d, the calling thread works on device %d", name, dict->device, this_thread_device());
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
  if (dict->device != this_thread_device()) return fail(HY_ERR_INVALID, "%s: the dictionary lives on device %d, the calling thread works on device %d", name, dict->device, this_thread_device());
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

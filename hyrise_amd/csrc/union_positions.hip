// union_positions.hip -- UnionPositions (operators/union_positions.cpp) on the device: the set union of two reference tables over the same
// data, which is what PredicateSplitUpRule makes of `WHERE p OR q` (two TableScans and a UnionNode).
//
// union_positions.cpp builds one "reference matrix" per input -- a row of n_clusters RowIDs per table row, one per column cluster (:349-372)
// -- sorts both (:128-137) and merges them with std::set_union (:205-230): the output is ascending, and a row that the left input holds m
// times and the right one n times appears max(m, n) times.  Here:
//   union_flatten   per side: the matrix columns as plain RowID arrays (entire-chunk PosLists expanded; a side that already is ONE contiguous
//                   device list is read where it lies) and, in the same pass, whether the side is in order already (a TableScan's output is);
//   sort            only for a side that is not: every cluster gives two 32-bit words, each one stable LSD pass of sort_pairs_u32
//                   (sort_words.hpp, as Sort), constant words skipped, then union_gather_rows applies the permutation;
//   union_partition the merge path: where every tile of TILE merged rows begins in both sides (one binary search per tile);
//   union_merge     a workgroup merges its tile (one cluster: the 64-bit keys go through LDS) -- left rows before equal right rows -- and
//                   decides for every merged row whether it stays: it writes the row's source, or DROPPED, and the tile's count;
//   union_scan_tiles, union_emit   exclusive scan of the tiles' counts, then every tile compacts its sources in LDS and copies the rows out.
//
// Which right rows stay.  In the merged order a run of equal rows is its m left rows followed by its n right rows; the left ones always stay,
// the right row of rank r (0-based among the equal right rows) stays iff r >= m.  When the merge reaches that right row it has consumed
// exactly the left rows <= it, say i of them, so the equal left rows are left[i - m .. i): r < m holds iff left[i - 1 - r] exists and equals
// the row.  That is one more comparison per right row and needs no count of the run, so a run may start anywhere before the tile (one as long
// as the whole input included): r continues from the previous right row, and the rank of a tile's first right row is found with one binary
// search by union_partition -- only where that row equals its predecessor.
#include "hy_device.hpp"
#include "sort_words.hpp"

#include <algorithm>
#include <vector>

namespace hy {

namespace {

constexpr uint32_t MAX_CLUSTERS = 8;
constexpr uint32_t ITEMS = 8;                  // merged rows per thread
constexpr uint32_t TILE = 256 * ITEMS;         // merged rows per workgroup (one cluster: 16 KiB of keys in LDS)
constexpr uint32_t DROPPED = 0xFFFFFFFFu;      // a merged row's source: left row i -> i, right row j -> rows(left) + j (< 2^32 - 1), or this

// A RowID as it lies in memory (chunk_id in the low half of the 64-bit word) -> the number that orders it: chunk_id first.
__host__ __device__ __forceinline__ uint64_t key_of(uint64_t raw) { return (raw << 32) | (raw >> 32); }

// One side's matrix: column c of row i at col[c][i] (RowIDs as they lie in memory).
struct Side {
  const uint64_t* col[MAX_CLUSTERS];
  uint32_t n;
};

// -1 / 0 / +1: row i of x against row j of y, cluster by cluster.
__device__ __forceinline__ int compare_rows(const Side& x, uint32_t i, const Side& y, uint32_t j, uint32_t nc) {
  for (uint32_t c = 0; c < nc; ++c) {
    const uint64_t a = key_of(x.col[c][i]), b = key_of(y.col[c][j]);
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}

// ---- union_flatten ------------------------------------------------------------------------------------------------------------------------
struct FlattenArgs {
  const DevSegment* segments[MAX_CLUSTERS];   // the cluster's reference segments, or ...
  const uint64_t* plain[MAX_CLUSTERS];        // ... the cluster as one contiguous list (then nothing is written for it)
  uint64_t* out[MAX_CLUSTERS];
  const Slice* slices;                        // the side's chunk layout in runs of at most SLICE_ROWS rows; nullptr: every cluster is plain
  const uint64_t* row_base;
  uint32_t n_chunks, nc, n;
  uint32_t* unordered;                        // set to 1 if some row is smaller than its predecessor
};

__device__ __forceinline__ uint64_t flatten_read(const FlattenArgs& a, uint32_t c, uint32_t row, uint32_t chunk, uint32_t offset) {
  if (a.plain[c]) return a.plain[c][row];
  const DevSegment& s = a.segments[c][chunk];
  if (!s.data) return (static_cast<uint64_t>(offset) << 32) | s.ref_chunk_id;   // EntireChunkPosList
  return static_cast<const uint64_t*>(s.data)[offset];
}

// One workgroup per slice.  A lane compares its row with the one the lane before it holds; the first lane of a wave reads its predecessor
// itself, which for the first row of a chunk lies in an earlier chunk (binary search of row_base, as sort_positions).
__global__ __launch_bounds__(256) void union_flatten(FlattenArgs a) {
  uint32_t chunk = 0, begin = 0, count, flat;
  if (a.slices) {
    const Slice s = a.slices[blockIdx.x];
    chunk = s.chunk; begin = s.row_begin; count = s.row_count;
    flat = static_cast<uint32_t>(a.row_base[chunk]) + begin;
  } else {
    flat = blockIdx.x * SLICE_ROWS;
    count = min(SLICE_ROWS, a.n - flat);
  }
  const uint32_t lane = threadIdx.x & 63;
  bool unordered = false;
  for (uint32_t r = threadIdx.x; r < (count + 255) / 256 * 256; r += 256) {   // (whole waves: the shuffles below)
    const bool active = r < count;
    const uint32_t row = flat + r;
    uint32_t before_chunk = chunk, before_offset = begin + r - 1;
    const bool reads_before = active && row > 0 && lane == 0;
    if (reads_before && a.slices && begin + r == 0) {   // the last row of the last chunk before this one that has rows
      uint32_t lo = 0, hi = a.n_chunks;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (a.row_base[mid] <= row - 1) lo = mid; else hi = mid;
      }
      before_chunk = lo;
      before_offset = static_cast<uint32_t>(row - 1 - a.row_base[lo]);
    }
    int order = 0;   // this row against its predecessor, decided by the first cluster that differs
    for (uint32_t c = 0; c < a.nc; ++c) {
      uint64_t raw = 0;
      if (active) {
        raw = flatten_read(a, c, row, chunk, begin + r);
        if (a.out[c]) a.out[c][row] = raw;
      }
      const uint64_t key = key_of(raw);
      uint64_t before = (static_cast<uint64_t>(__shfl_up(static_cast<uint32_t>(key >> 32), 1)) << 32) | __shfl_up(static_cast<uint32_t>(key), 1);
      if (reads_before) before = key_of(flatten_read(a, c, row - 1, before_chunk, before_offset));
      if (order == 0 && key != before) order = key < before ? -1 : 1;
    }
    if (active && row > 0 && order < 0) unordered = true;
  }
  if (unordered) *a.unordered = 1;
}

// ---- the sort of a side that is not in order ----------------------------------------------------------------------------------------------
// stats[2 * c + w]: smallest, stats[16 + 2 * c + w]: largest value of word w (0: chunk_offset, 1: chunk_id) of cluster c (set to ~0 / 0 before).
__global__ __launch_bounds__(256) void union_word_stats(Side side, uint32_t nc, uint32_t* stats) {
  __shared__ uint32_t s_part[4][4];
  for (uint32_t c = 0; c < nc; ++c) {
    uint32_t low[2] = {~0u, ~0u}, high[2] = {0, 0};
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < side.n; i += gridDim.x * 256) {
      const uint64_t raw = side.col[c][i];
      const uint32_t word[2] = {static_cast<uint32_t>(raw >> 32), static_cast<uint32_t>(raw)};
      for (uint32_t w = 0; w < 2; ++w) { low[w] = min(low[w], word[w]); high[w] = max(high[w], word[w]); }
    }
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t w = 0; w < 2; ++w) {
      low[w] = wave_min_u32(low[w]);
      high[w] = wave_max_u32(high[w]);
      if ((threadIdx.x & 63) == 0) { s_part[wave][w] = low[w]; s_part[wave][2 + w] = high[w]; }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      const uint32_t w = threadIdx.x;
      uint32_t lowest = s_part[0][w], highest = s_part[0][2 + w];
      for (uint32_t v = 1; v < 4; ++v) { lowest = min(lowest, s_part[v][w]); highest = max(highest, s_part[v][2 + w]); }
      atomicMin(stats + 2 * c + w, lowest);
      atomicMax(stats + 16 + 2 * c + w, highest);
    }
    __syncthreads();
  }
}

// keys[i] = word (0: chunk_offset, 1: chunk_id) of column[perm[i]] - minimum; perm == nullptr: the identity, which is then written to ids_out.
__global__ __launch_bounds__(256) void union_gather_word(const uint64_t* column, const uint32_t* perm, uint32_t* keys, uint32_t* ids_out, uint32_t n, uint32_t word, uint32_t minimum) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t row = perm ? perm[i] : i;
    const uint64_t raw = column[row];
    keys[i] = static_cast<uint32_t>(word == 0 ? raw >> 32 : raw) - minimum;
    if (!perm) ids_out[i] = row;
  }
}

__global__ __launch_bounds__(256) void union_gather_rows(const uint64_t* column, const uint32_t* perm, uint64_t* out, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = column[perm[i]];
}

// ---- the merge ------------------------------------------------------------------------------------------------------------------------------
// How many of the first `diagonal` merged rows come from the left side: the smallest i with right[diagonal - 1 - i] < left[i].
template <typename Rows>
__device__ __forceinline__ uint32_t merge_path(const Rows& rows, uint32_t diagonal, uint32_t left_begin, uint32_t left_end, uint32_t right_begin, uint32_t right_end) {
  const uint32_t right_rows = right_end - right_begin;
  uint32_t lo = diagonal > right_rows ? diagonal - right_rows : 0, hi = min(diagonal, left_end - left_begin);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (rows.right_before_left(right_begin + diagonal - 1 - mid, left_begin + mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The rows where they lie (any number of clusters).
struct GlobalRows {
  Side left, right;
  uint32_t nc;
  __device__ __forceinline__ bool right_before_left(uint32_t j, uint32_t i) const { return compare_rows(right, j, left, i, nc) < 0; }
  __device__ __forceinline__ bool right_repeats(uint32_t j) const { return compare_rows(right, j, right, j - 1, nc) == 0; }
  __device__ __forceinline__ bool right_less(uint32_t a, uint32_t b) const { return compare_rows(right, a, right, b, nc) < 0; }
  __device__ __forceinline__ bool left_equals_right(uint32_t i, uint32_t j) const { return compare_rows(left, i, right, j, nc) == 0; }
};

// One cluster: a row is one 64-bit key, and a tile's keys [left_begin, left_end) / [right_begin, right_end) lie in LDS.
struct TileKeys {
  const uint64_t* left;        // (global, RowIDs as they lie in memory: the rows before the tile)
  const uint64_t* s_left;      // LDS, keys
  const uint64_t* s_right;
  uint32_t left_begin, right_begin;
  __device__ __forceinline__ bool right_before_left(uint32_t j, uint32_t i) const { return s_right[j - right_begin] < s_left[i - left_begin]; }
  __device__ __forceinline__ bool right_repeats(uint32_t j) const { return s_right[j - right_begin] == s_right[j - 1 - right_begin]; }
  __device__ __forceinline__ bool right_less(uint32_t a, uint32_t b) const { return s_right[a - right_begin] < s_right[b - right_begin]; }
  __device__ __forceinline__ bool left_equals_right(uint32_t i, uint32_t j) const {
    return (i >= left_begin ? s_left[i - left_begin] : key_of(left[i])) == s_right[j - right_begin];
  }
};

// splits[t]: the left rows among the first t * TILE merged rows (t = 0 .. n_tiles); ranks[t]: the rank of tile t's first right row among the
// right rows equal to it that come before the tile.
__global__ __launch_bounds__(256) void union_partition(Side left, Side right, uint32_t nc, uint32_t n_tiles, uint32_t* splits, uint32_t* ranks) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t > n_tiles) return;
  const GlobalRows rows{left, right, nc};
  const uint64_t total = uint64_t{left.n} + right.n;
  const uint32_t diagonal = static_cast<uint32_t>(min(uint64_t{t} * TILE, total));
  const uint32_t split = merge_path(rows, diagonal, 0, left.n, 0, right.n);
  splits[t] = split;
  if (t == n_tiles) return;
  const uint32_t first = diagonal - split;   // the tile's first right row
  uint32_t rank = 0;
  if (first > 0 && first < right.n && rows.right_repeats(first)) {
    uint32_t lo = 0, hi = first - 1;   // the first right row equal to right[first]
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (compare_rows(right, mid, right, first, nc) < 0) lo = mid + 1; else hi = mid;
    }
    rank = first - lo;
  }
  ranks[t] = rank;
}

// The thread's ITEMS merged rows, one after the other: sources[k] = the row's source or DROPPED; -> how many stay.
template <typename Rows>
__device__ __forceinline__ uint32_t merge_items(const Rows& rows, uint32_t i, uint32_t j, uint32_t left_end, uint32_t right_end, uint32_t right_begin, uint32_t tile_rank,
                                               uint32_t left_rows, uint32_t items, uint32_t* sources) {
  uint32_t rank = 0, kept = 0;
  bool rank_known = false;
  for (uint32_t k = 0; k < ITEMS; ++k) {
    uint32_t source = DROPPED;
    if (k < items) {
      if (j >= right_end || (i < left_end && !rows.right_before_left(j, i))) {
        source = i++;
      } else {
        if (!rank_known) {   // the thread's first right row: the equal right rows in front of it, in the tile (binary search) and before it
          uint32_t lo = j;
          if (j > right_begin && rows.right_repeats(j)) {
            lo = right_begin;
            uint32_t hi = j - 1;
            while (lo < hi) {
              const uint32_t mid = (lo + hi) / 2;
              if (rows.right_less(mid, j)) lo = mid + 1; else hi = mid;
            }
          }
          rank = j - lo + (lo == right_begin ? tile_rank : 0);
          rank_known = true;
        } else {
          rank = rows.right_repeats(j) ? rank + 1 : 0;
        }
        const bool twin = i > rank && rows.left_equals_right(i - 1 - rank, j);   // rank < the equal left rows: this one is already there
        if (!twin) source = left_rows + j;
        ++j;
      }
      kept += source != DROPPED;
    }
    sources[k] = source;
  }
  return kept;
}

template <bool SINGLE>
__global__ __launch_bounds__(256) void union_merge(Side left, Side right, uint32_t nc, const uint32_t* splits, const uint32_t* ranks, uint32_t* sources_out, uint32_t* counts) {
  __shared__ uint64_t s_keys[SINGLE ? TILE : 1];
  __shared__ uint32_t s_kept[4];
  const uint32_t tile = blockIdx.x;
  const uint64_t total = uint64_t{left.n} + right.n;
  const uint32_t diagonal = tile * TILE;
  const uint32_t tile_rows = static_cast<uint32_t>(min(uint64_t{TILE}, total - diagonal));
  const uint32_t left_begin = splits[tile], left_end = splits[tile + 1];
  const uint32_t right_begin = diagonal - left_begin, right_end = right_begin + tile_rows - (left_end - left_begin);
  const uint32_t mine = min(threadIdx.x * ITEMS, tile_rows);
  const uint32_t items = min(ITEMS, tile_rows - mine);
  uint32_t sources[ITEMS];
  uint32_t kept;
  // (ranks[tile], the rank of the tile's first right row, counts for every thread whose run of equal right rows reaches back to right_begin)
  if constexpr (SINGLE) {
    const uint32_t left_rows = left_end - left_begin;
    for (uint32_t r = threadIdx.x; r < tile_rows; r += 256)
      s_keys[r] = key_of(r < left_rows ? left.col[0][left_begin + r] : right.col[0][right_begin + r - left_rows]);
    __syncthreads();
    const TileKeys rows{left.col[0], s_keys, s_keys + left_rows, left_begin, right_begin};
    const uint32_t i = left_begin + merge_path(rows, mine, left_begin, left_end, right_begin, right_end);
    kept = merge_items(rows, i, right_begin + mine - (i - left_begin), left_end, right_end, right_begin, ranks[tile], left.n, items, sources);
  } else {
    const GlobalRows rows{left, right, nc};
    const uint32_t i = left_begin + merge_path(rows, mine, left_begin, left_end, right_begin, right_end);
    kept = merge_items(rows, i, right_begin + mine - (i - left_begin), left_end, right_end, right_begin, ranks[tile], left.n, items, sources);
  }
  // sources_out is padded to whole tiles: every thread stores its ITEMS words as two 16-byte vectors
  u32x4_t* out = reinterpret_cast<u32x4_t*>(sources_out + size_t{tile} * TILE + threadIdx.x * ITEMS);
  out[0] = u32x4_t{sources[0], sources[1], sources[2], sources[3]};
  out[1] = u32x4_t{sources[4], sources[5], sources[6], sources[7]};
  for (int offset = 32; offset > 0; offset >>= 1) kept += static_cast<uint32_t>(__shfl_xor(static_cast<int>(kept), offset));
  if ((threadIdx.x & 63) == 0) s_kept[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) counts[tile] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
}

// offsets[t] = the rows that stay in the tiles before t; *total = all of them.  One workgroup: 29 297 tiles for 60 M merged rows.
__global__ __launch_bounds__(1024) void union_scan_tiles(const uint32_t* counts, uint32_t n_tiles, uint32_t* offsets, uint64_t* total) {
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

struct EmitArgs {
  Side left, right;
  uint64_t* out[MAX_CLUSTERS];
  uint32_t nc;
  uint64_t capacity;
};

// A tile's sources that stay, packed in LDS in merged order, then copied out: consecutive lanes write consecutive output rows (8-byte stores,
// 512 bytes per wave and cluster) and read rows that ascend within each side.
__global__ __launch_bounds__(256) void union_emit(EmitArgs a, const uint32_t* sources_in, const uint32_t* offsets) {
  __shared__ uint32_t s_sources[TILE];
  __shared__ uint32_t s_wave[4];
  const uint32_t tile = blockIdx.x;
  const u32x4_t* in = reinterpret_cast<const u32x4_t*>(sources_in + size_t{tile} * TILE + threadIdx.x * ITEMS);
  const u32x4_t lo = in[0], hi = in[1];
  const uint32_t sources[ITEMS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t kept = 0;
  for (uint32_t k = 0; k < ITEMS; ++k) kept += sources[k] != DROPPED;
  uint32_t scan = kept;   // inclusive over the wave
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(scan), step));
    if (lane >= step) scan += up;
  }
  if (lane == 63) s_wave[wave] = scan;
  __syncthreads();
  uint32_t at = scan - kept;
  for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
  const uint32_t count = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  for (uint32_t k = 0; k < ITEMS; ++k)
    if (sources[k] != DROPPED) s_sources[at++] = sources[k];
  __syncthreads();
  const uint64_t base = offsets[tile];
  for (uint32_t k = threadIdx.x; k < count; k += 256) {
    if (base + k >= a.capacity) break;   // (the caller is told: HY_ERR_CAPACITY)
    const uint32_t source = s_sources[k];
    const bool from_left = source < a.left.n;
    const uint32_t row = from_left ? source : source - a.left.n;
    for (uint32_t c = 0; c < a.nc; ++c) a.out[c][base + k] = from_left ? a.left.col[c][row] : a.right.col[c][row];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
hy_status check_side(const hy_column* const* columns, uint32_t n_clusters, const char* name) {
  for (uint32_t c = 0; c < n_clusters; ++c) {
    const hy_column* column = columns[c];
    if (!column) return fail(HY_ERR_INVALID, "hy_union_positions: %s cluster %u: null column", name, c);
    HY_TRY(on_this_device(column, "hy_union_positions"));
    if (column->is_mvcc || (column->n_chunks && !column->is_reference))
      return fail(HY_ERR_INVALID, "hy_union_positions: %s cluster %u is a data column (UnionPositions takes reference tables only)", name, c);
    const hy_column* first = columns[0];
    bool same = column->n_chunks == first->n_chunks && column->rows == first->rows;
    for (uint32_t k = 0; same && k < column->n_chunks; ++k) same = column->host_segments[k].size == first->host_segments[k].size;
    if (!same) return fail(HY_ERR_INVALID, "hy_union_positions: %s cluster %u has %llu rows in %u chunks, cluster 0 %llu in %u (clusters of one table share its chunk layout)", name, c,
                           static_cast<unsigned long long>(column->rows), column->n_chunks, static_cast<unsigned long long>(first->rows), first->n_chunks);
    for (uint32_t k = 0; k < column->n_chunks; ++k)
      if (reinterpret_cast<uintptr_t>(column->host_segments[k].data) % 8 != 0) return fail(HY_ERR_UNSUPPORTED, "hy_union_positions: %s cluster %u chunk %u: PosList not on an 8-byte boundary", name, c, k);
  }
  return HY_OK;
}

// The column's PosLists as ONE device array, if that is how they lie (the dense output of a scan or a join, one pooled block cut into chunks).
const uint64_t* contiguous_list(const hy_column* column) {
  const char* expected = nullptr;
  const uint64_t* first = nullptr;
  for (const hy_segment& s : column->host_segments) {
    if (!s.size) continue;
    if (!s.data || (expected && s.data != expected)) return nullptr;
    if (!first) first = static_cast<const uint64_t*>(s.data);
    expected = static_cast<const char*>(s.data) + size_t{8} * s.size;
  }
  return first;
}

// One input on its way to the merge: `view` is the matrix as the merge reads it.
struct SideState {
  Side view{};
  std::vector<std::unique_ptr<DeviceBuffer>> flat, sorted;
};

hy_status flatten_side(const hy_column* const* columns, uint32_t nc, SideState& side, uint32_t* unordered, hipStream_t stream) {
  const uint32_t n = static_cast<uint32_t>(columns[0]->rows);
  side.view.n = n;
  if (!n) return HY_OK;
  FlattenArgs a{};
  a.nc = nc; a.n = n; a.unordered = unordered;
  a.n_chunks = columns[0]->n_chunks;
  a.row_base = columns[0]->d_row_base;
  bool all_plain = true;
  for (uint32_t c = 0; c < nc; ++c) {
    a.plain[c] = contiguous_list(columns[c]);
    if (a.plain[c]) { side.view.col[c] = a.plain[c]; continue; }
    all_plain = false;
    side.flat.emplace_back(new DeviceBuffer());
    HY_TRY(side.flat.back()->alloc(size_t{8} * n + 16));
    a.segments[c] = columns[c]->d_segments;
    a.out[c] = side.flat.back()->as<uint64_t>();
    side.view.col[c] = a.out[c];
  }
  a.slices = all_plain ? nullptr : columns[0]->d_slices;
  const uint32_t grid = all_plain ? (n + SLICE_ROWS - 1) / SLICE_ROWS : columns[0]->n_slices;
  hipLaunchKernelGGL(union_flatten, dim3(grid), dim3(256), 0, stream, a);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

hy_status sort_side(SideState& side, uint32_t nc, hipStream_t stream) {
  const uint32_t n = side.view.n;
  DeviceBuffer stats_buffer;
  HY_TRY(stats_buffer.alloc(128));
  uint32_t* stats = stats_buffer.as<uint32_t>();
  HY_HIP(hipMemsetAsync(stats, 0xFF, 64, stream));
  HY_HIP(hipMemsetAsync(stats + 16, 0, 64, stream));
  hipLaunchKernelGGL(union_word_stats, dim3(std::min<uint32_t>(grid_for(n / 16), 1024)), dim3(256), 0, stream, side.view, nc, stats);
  HY_HIP(hipGetLastError());
  uint32_t s[32];
  HY_HIP(hipMemcpyAsync(s, stats, sizeof(s), hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));
  WordSort order;
  HY_TRY(order.alloc(n));
  for (uint32_t c = nc; c-- > 0;) {   // the least significant word of the last cluster first
    for (uint32_t word = 0; word < 2; ++word) {
      uint32_t minimum = 0, bits = 0;
      if (!word_range(s[2 * c + word], s[16 + 2 * c + word], &minimum, &bits)) continue;   // the same in every row: nothing to order
      hipLaunchKernelGGL(union_gather_word, dim3(grid_for(n)), dim3(256), 0, stream, side.view.col[c], order.perm, order.key_words(), order.ids(), n, word, minimum);
      HY_HIP(hipGetLastError());
      HY_TRY(order.sort(n, bits, stream));
    }
  }
  if (!order.perm) return HY_OK;   // every row equals every other
  for (uint32_t c = 0; c < nc; ++c) {
    side.sorted.emplace_back(new DeviceBuffer());
    HY_TRY(side.sorted.back()->alloc(size_t{8} * n + 16));
    hipLaunchKernelGGL(union_gather_rows, dim3(grid_for(n)), dim3(256), 0, stream, side.view.col[c], order.perm, side.sorted.back()->as<uint64_t>(), n);
    HY_HIP(hipGetLastError());
    side.view.col[c] = side.sorted.back()->as<uint64_t>();
  }
  return HY_OK;   // (the permutation goes back to the pool, which hands blocks on in stream order)
}

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_union_positions(const hy_column* const* left, const hy_column* const* right, uint32_t n_clusters, uint32_t flags, hy_row_id* const* out, uint64_t capacity,
                             uint64_t* n_out, uint32_t* path) {
  if (!left || !right || !out || !n_out) return fail(HY_ERR_INVALID, "hy_union_positions: null argument");
  *n_out = 0;
  if (path) *path = 0;
  if (!n_clusters) return fail(HY_ERR_INVALID, "hy_union_positions: no column cluster");
  if (n_clusters > MAX_CLUSTERS) return fail(HY_ERR_UNSUPPORTED, "hy_union_positions: %u column clusters (at most %u)", n_clusters, MAX_CLUSTERS);
  if (flags & ~uint32_t{HY_UNION_FORCE_SORT}) return fail(HY_ERR_INVALID, "hy_union_positions: unknown flags %#x", flags);
  HY_TRY(check_side(left, n_clusters, "left"));
  HY_TRY(check_side(right, n_clusters, "right"));
  const uint64_t total = left[0]->rows + right[0]->rows;
  if (total >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "hy_union_positions: %llu input rows (32-bit row ids)", static_cast<unsigned long long>(total));
  if (!total) {
    if (path && (flags & HY_UNION_FORCE_SORT)) *path = 3;
    return HY_OK;
  }
  for (uint32_t c = 0; c < n_clusters; ++c)
    if (!out[c] || reinterpret_cast<uintptr_t>(out[c]) % 8 != 0) return fail(HY_ERR_INVALID, "hy_union_positions: output list %u is null or not on an 8-byte boundary", c);
  hipStream_t stream = current_stream();

  DeviceBuffer words;   // [0], [1]: "this side is not in order"; [2..3]: the output rows
  HY_TRY(words.alloc(64));
  HY_HIP(hipMemsetAsync(words.ptr, 0, 64, stream));
  profile_begin(stream);   // (hy_set_profiling: one event pair around the call's kernels, the host's two reads in between included)
  SideState sides[2];
  HY_TRY(flatten_side(left, n_clusters, sides[0], words.as<uint32_t>(), stream));
  HY_TRY(flatten_side(right, n_clusters, sides[1], words.as<uint32_t>() + 1, stream));
  uint32_t unordered[2] = {1, 1};
  if (!(flags & HY_UNION_FORCE_SORT)) {
    HY_HIP(hipMemcpyAsync(unordered, words.ptr, sizeof(unordered), hipMemcpyDeviceToHost, stream));
    HY_HIP(hipStreamSynchronize(stream));
  }
  uint32_t sorted_sides = 0;
  for (uint32_t s = 0; s < 2; ++s) {
    if (!unordered[s]) continue;
    sorted_sides |= 1u << s;
    if (sides[s].view.n > 1) HY_TRY(sort_side(sides[s], n_clusters, stream));
  }
  if (path) *path = sorted_sides;

  const uint32_t n_tiles = static_cast<uint32_t>((total + TILE - 1) / TILE);
  DeviceBuffer splits, ranks, counts, offsets, sources;
  HY_TRY(splits.alloc(4 * (size_t{n_tiles} + 1)));
  HY_TRY(ranks.alloc(4 * size_t{n_tiles}));
  HY_TRY(counts.alloc(4 * size_t{n_tiles}));
  HY_TRY(offsets.alloc(4 * size_t{n_tiles}));
  HY_TRY(sources.alloc(4 * size_t{n_tiles} * TILE));
  hipLaunchKernelGGL(union_partition, dim3(n_tiles / 256 + 1), dim3(256), 0, stream, sides[0].view, sides[1].view, n_clusters, n_tiles, splits.as<uint32_t>(), ranks.as<uint32_t>());
  HY_HIP(hipGetLastError());
  if (n_clusters == 1) hipLaunchKernelGGL(union_merge<true>, dim3(n_tiles), dim3(256), 0, stream, sides[0].view, sides[1].view, n_clusters, splits.as<uint32_t>(), ranks.as<uint32_t>(), sources.as<uint32_t>(), counts.as<uint32_t>());
  else hipLaunchKernelGGL(union_merge<false>, dim3(n_tiles), dim3(256), 0, stream, sides[0].view, sides[1].view, n_clusters, splits.as<uint32_t>(), ranks.as<uint32_t>(), sources.as<uint32_t>(), counts.as<uint32_t>());
  HY_HIP(hipGetLastError());
  uint64_t* d_total = reinterpret_cast<uint64_t*>(words.as<uint32_t>() + 2);
  hipLaunchKernelGGL(union_scan_tiles, dim3(1), dim3(1024), 0, stream, counts.as<uint32_t>(), n_tiles, offsets.as<uint32_t>(), d_total);
  HY_HIP(hipGetLastError());
  EmitArgs e{};
  e.left = sides[0].view; e.right = sides[1].view; e.nc = n_clusters; e.capacity = capacity;
  for (uint32_t c = 0; c < n_clusters; ++c) e.out[c] = reinterpret_cast<uint64_t*>(out[c]);
  hipLaunchKernelGGL(union_emit, dim3(n_tiles), dim3(256), 0, stream, e, sources.as<uint32_t>(), offsets.as<uint32_t>());
  HY_HIP(hipGetLastError());
  profile_end(stream);
  uint64_t rows = 0;
  HY_HIP(hipMemcpyAsync(&rows, d_total, sizeof(rows), hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool; the caller reads `out` next)
  *n_out = rows;
  if (rows > capacity) return fail(HY_ERR_CAPACITY, "hy_union_positions: %llu output rows, capacity %llu (the lists hold the first %llu)", static_cast<unsigned long long>(rows),
                                   static_cast<unsigned long long>(capacity), static_cast<unsigned long long>(capacity));
  return HY_OK;
}

}  // extern "C"

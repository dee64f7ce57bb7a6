// join_nested_loop.hip -- JoinNestedLoop (operators/join_nested_loop.cpp) on the device: the join the translator ends on where JoinHash and
// JoinSortMerge refuse (lqp_translator.cpp:389-410) -- non-equi predicates under Semi / Anti, secondary predicates beside a non-equi or FULL
// OUTER join, key columns of two types, <> under an outer mode.  Every pair is compared; the output has the reference's order (the header
// states it), so the structure is count -> scan -> emit and no global atomic places a pair:
//   export + nlj_operand   every column a predicate reads, once per side: export_column_at's flat values and null bytes, then one 8-byte word
//                          per row in the predicate's common C++ type (int64, or double -- a float comparison's operands are rounded to float
//                          first, then widened, which compares alike) and one bit per predicate "this operand is NULL";
//   nlj_count              a 256-thread workgroup owns (a tile of 256 consecutive rows of one O chunk, one I chunk).  Wave w holds the
//                          operands of O rows 64 w .. 64 w + 63 in registers, lane = row.  It walks the I chunk in strips of 64 rows (lane = I
//                          row, operands loaded coalesced, once per strip); inside a strip it loops over its O rows: the O operand is read
//                          out of its lane into scalar registers, the comparison's ballot is counted with scalar arithmetic and added to the O
//                          row's counter, which lives in lane i of one register.  count[co][ci][row], outer chunk-major: ONE flat exclusive
//                          scan of it is the output order.  Every (wave, I chunk) ORs the ballot of "row has a partner" into the O side's
//                          bitmap, FULL OUTER every (wave, strip) the ballot of "I row has a partner" into the I side's -- an atomic per
//                          strip at most, never per pair;
//   nlj_flags              one more slot per O row behind the I chunks: "matched nothing" (outer modes), matched ^ invert (Semi / Anti, which
//                          store and scan no pair slots at all), so that the flagged rows of co fall behind co's pairs in the same scan;
//   nlj_scan_segments      the sums of the (tile, I chunk) segments: one workgroup, 64-bit offsets, the total to pinned memory;
//   nlj_unmatched, select_scan_tiles   FULL OUTER: the I rows without a partner as mask words, counted per tile and scanned;
//   -- the host reads the totals here, once: HY_ERR_CAPACITY, or hy_join_nested_loop_count's answer --
//   nlj_emit               the same walk; a match's slot is the segment's offset + the scan of the tile's counts + the row's running count +
//                          the lanes below it in the ballot: consecutive lanes write consecutive pairs of both lists with 8-byte stores, a
//                          strip without a match costs a scalar branch; a segment without pairs returns at once;
//   nlj_emit_flags, smj_outer_emit   the flagged O rows, and the unmatched I rows behind everything.
// Nothing here uses LDS atomics: HY_OPT_LDS_ORDERED_ATOMICS does not matter.
#include "hy_device.hpp"
#include "hy_decode.hpp"
#include "sort_keys.hpp"
#include "join_outer_emit.hpp"

#include <algorithm>

namespace hy {

namespace {

constexpr uint64_t NLJ_MAX_COMPARISONS = HY_NLJ_MAX_COMPARISONS;
constexpr uint32_t NLJ_TILE = 256;                                  // O rows per workgroup: 64 per wave
constexpr uint32_t NLJ_MAX_PREDICATES = 1 + HY_MAX_SECONDARY_PREDICATES;

// One tile of O rows: 256 consecutive rows of one chunk (the last tile of a chunk: fewer).
struct NljTile {
  uint64_t count_base;     // index of count[co][0][the tile's first row]
  uint32_t first;          // flat number of the tile's first row
  uint32_t rows;           // 1 .. NLJ_TILE
  uint32_t chunk;          // co
  uint32_t chunk_first;    // flat number of co's first row
  uint32_t chunk_rows;
  uint32_t segment_first;  // segment of (this tile, I chunk 0); (this tile, ci) is segment_first + ci * segment_stride
  uint32_t segment_stride; // tiles of co
  uint32_t reserved;
};

struct NljArgs {
  const NljTile* tiles;
  const uint64_t* o_operands;   // [n_predicates][o_stride]
  const uint64_t* i_operands;   // [n_predicates][i_stride]
  const uint8_t* o_nulls;       // bit p: predicate p's operand is NULL
  const uint8_t* i_nulls;
  uint64_t o_stride, i_stride;
  const uint64_t* i_row_base;   // [i_chunks + 1]
  uint32_t i_chunks;
  uint32_t slots;               // pair slots per O row: i_chunks, or 0 (Semi / Anti)
  uint32_t null_matches;        // AntiNullAsTrue
  uint32_t track_inner;         // FULL OUTER
  uint32_t condition[NLJ_MAX_PREDICATES];   // O <condition> I
  uint32_t type[NLJ_MAX_PREDICATES];        // HY_TYPE_LONG or HY_TYPE_DOUBLE: what the operand words hold
  uint32_t* counts;
  uint64_t* segment_sums;
  const uint64_t* segment_offsets;
  uint64_t* o_matched;          // [n_tiles][4]
  uint64_t* i_matched;          // bit per flat I row
  uint64_t* o_out;              // nlj_emit
  uint64_t* i_out;
};

__device__ __forceinline__ uint32_t read_lane(uint32_t v, uint32_t lane) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane))); }
__device__ __forceinline__ uint64_t read_lane(uint64_t v, uint32_t lane) {
  return (uint64_t{read_lane(static_cast<uint32_t>(v >> 32), lane)} << 32) | read_lane(static_cast<uint32_t>(v), lane);
}
__device__ __forceinline__ uint64_t shuffle_up(uint64_t v, uint32_t step) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v)), step));
  const uint32_t hi = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v >> 32)), step));
  return (uint64_t{hi} << 32) | lo;
}
__device__ __forceinline__ uint64_t shuffle_xor(uint64_t v, int offset) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), offset));
  const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v >> 32)), offset));
  return (uint64_t{hi} << 32) | lo;
}
__device__ __forceinline__ Value operand_value(uint64_t word) { return Value{false, static_cast<int64_t>(word), __longlong_as_double(static_cast<long long>(word))}; }

// The operands of a wave: its O rows (lane = row) and the walk over an I chunk's strips.  visit(r, mask): the ballot of the I rows of the
// current strip that O row r matches; strip_done(strip, any): after the O rows of a strip, `any` = this lane's I row matched one of them.
template <uint32_t NP>
struct NljWalk {
  uint64_t x[NP];
  uint32_t x_null;
  uint32_t rows;   // of this wave: 0 .. 64

  __device__ __forceinline__ void load_outer(const NljArgs& a, const NljTile& tile, uint32_t wave, uint32_t lane) {
    rows = tile.rows > 64 * wave ? min(64u, tile.rows - 64 * wave) : 0;
    const uint32_t row = tile.first + min(64 * wave + lane, tile.rows - 1);   // (lanes behind the tile read its last row)
#pragma unroll
    for (uint32_t p = 0; p < NP; ++p) x[p] = a.o_operands[p * a.o_stride + row];
    x_null = a.o_nulls[row];
  }

  template <typename Visit, typename StripDone>
  __device__ __forceinline__ void walk(const NljArgs& a, uint32_t ci, uint32_t lane, Visit visit, StripDone strip_done) const {
    const uint64_t i_first = a.i_row_base[ci];
    const uint32_t i_rows = static_cast<uint32_t>(a.i_row_base[ci + 1] - i_first);
    if (!rows || !i_rows) return;
    const bool null_matches = a.null_matches != 0;
    const uint32_t strips = static_cast<uint32_t>((uint64_t{i_rows} + 63) / 64);
    for (uint32_t strip = 0; strip < strips; ++strip) {
      const uint32_t begin = 64 * strip;
      const bool present = begin + lane < i_rows;
      const uint64_t j = i_first + min(begin + lane, i_rows - 1);
      uint64_t y[NP];
#pragma unroll
      for (uint32_t p = 0; p < NP; ++p) y[p] = a.i_operands[p * a.i_stride + j];
      const uint32_t y_null = a.i_nulls[j];
      bool any = false;
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t nulls = read_lane(x_null, r) | y_null;
        bool match = present;
#pragma unroll
        for (uint32_t p = 0; p < NP; ++p) {
          const bool compared = compare_typed(a.condition[p], operand_value(read_lane(x[p], r)), a.type[p], operand_value(y[p]), a.type[p]);
          match = match && ((nulls >> p & 1) ? null_matches : compared);
        }
        any = any || match;
        visit(r, __ballot(match));
      }
      strip_done(begin, any);
    }
  }
};

template <uint32_t NP>
__global__ __launch_bounds__(256) void nlj_count(const NljArgs a) {
  __shared__ uint64_t s_sum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t tile_id = blockIdx.x / a.i_chunks, ci = blockIdx.x % a.i_chunks;
  const NljTile tile = a.tiles[tile_id];
  NljWalk<NP> w;
  w.load_outer(a, tile, wave, lane);
  uint32_t counter = 0;   // lane r: the partners of O row r in this I chunk
  const uint64_t i_first = a.i_row_base[ci];
  w.walk(a, ci, lane,
         [&](uint32_t r, uint64_t mask) {
           const uint32_t found = static_cast<uint32_t>(__popcll(mask));
           if (lane == r) counter += found;
         },
         [&](uint32_t begin, bool any) {
           if (!a.track_inner) return;
           const uint64_t mask = __ballot(any);
           if (mask && lane == 0) {   // the strip's 64 bits lie in two words of the flat bitmap
             const uint64_t bit = i_first + begin;
             const uint32_t shift = static_cast<uint32_t>(bit & 63);
             atomicOr(reinterpret_cast<unsigned long long*>(a.i_matched + (bit >> 6)), static_cast<unsigned long long>(mask << shift));
             if (shift && (mask >> (64 - shift))) atomicOr(reinterpret_cast<unsigned long long*>(a.i_matched + (bit >> 6) + 1), static_cast<unsigned long long>(mask >> (64 - shift)));
           }
         });
  if (lane >= w.rows) counter = 0;
  if (a.slots && lane < w.rows) a.counts[tile.count_base + uint64_t{ci} * tile.chunk_rows + 64 * wave + lane] = counter;
  const uint64_t matched = __ballot(counter != 0);
  if (matched && lane == 0) atomicOr(reinterpret_cast<unsigned long long*>(a.o_matched + 4 * uint64_t{tile_id} + wave), static_cast<unsigned long long>(matched));
  if (!a.slots) return;
  uint64_t sum = counter;
  for (int offset = 32; offset > 0; offset >>= 1) sum += shuffle_xor(sum, offset);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) a.segment_sums[tile.segment_first + ci * tile.segment_stride] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// The slot behind the I chunks: flag = wanted ? (row has a partner) ^ invert : 0, and the segment's sum.
__global__ __launch_bounds__(256) void nlj_flags(const NljTile* tiles, const uint64_t* o_matched, uint32_t slots, uint32_t wanted, uint32_t invert, uint32_t* counts, uint64_t* segment_sums) {
  __shared__ uint32_t s_sum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const NljTile tile = tiles[blockIdx.x];
  const bool present = threadIdx.x < tile.rows;
  const bool matched = (o_matched[4 * uint64_t{blockIdx.x} + wave] >> lane & 1) != 0;
  const bool flag = present && wanted && (matched != (invert != 0));
  if (present) counts[tile.count_base + uint64_t{slots} * tile.chunk_rows + threadIdx.x] = flag ? 1u : 0u;
  const uint64_t mask = __ballot(flag);
  if (lane == 0) s_sum[wave] = static_cast<uint32_t>(__popcll(mask));
  __syncthreads();
  if (threadIdx.x == 0) segment_sums[tile.segment_first + slots * tile.segment_stride] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// offsets[s] = the output rows of the segments before s; *total = all of them (pinned host memory).  smj_scan_tiles' shape.
__global__ __launch_bounds__(1024) void nlj_scan_segments(const uint64_t* sums, uint32_t n, uint64_t* offsets, uint64_t* total) {
  __shared__ uint64_t s_sum[1024];
  const uint32_t per_thread = (n + 1023) / 1024;
  const uint32_t begin = min(n, threadIdx.x * per_thread), end = min(n, begin + per_thread);
  uint64_t sum = 0;
  for (uint32_t s = begin; s < end; ++s) sum += sums[s];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t step = 1; step < 1024; step <<= 1) {   // (inclusive scan of the threads' sums)
    const uint64_t add = threadIdx.x >= step ? s_sum[threadIdx.x - step] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += add;
    __syncthreads();
  }
  uint64_t run = s_sum[threadIdx.x] - sum;
  for (uint32_t s = begin; s < end; ++s) { offsets[s] = run; run += sums[s]; }
  if (threadIdx.x == 1023) *total = s_sum[1023];
}

template <uint32_t NP>
__global__ __launch_bounds__(256) void nlj_emit(const NljArgs a) {
  __shared__ uint64_t s_wave[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t tile_id = blockIdx.x / a.i_chunks, ci = blockIdx.x % a.i_chunks;
  const NljTile tile = a.tiles[tile_id];
  const uint32_t segment = tile.segment_first + ci * tile.segment_stride;
  if (a.segment_sums[segment] == 0) return;   // (uniform: no pair of this tile in this I chunk)
  NljWalk<NP> w;
  w.load_outer(a, tile, wave, lane);
  // where O row r's pairs begin: the segment's offset + the counts of the tile's rows before r
  const uint32_t count = threadIdx.x < tile.rows ? a.counts[tile.count_base + uint64_t{ci} * tile.chunk_rows + threadIdx.x] : 0;
  uint64_t scan = count;   // inclusive over the wave
  for (uint32_t step = 1; step < 64; step <<= 1) {
    const uint64_t up = shuffle_up(scan, step);
    if (lane >= step) scan += up;
  }
  if (lane == 63) s_wave[wave] = scan;
  __syncthreads();
  uint64_t at = a.segment_offsets[segment] + scan - count;   // lane r: the slot of O row r's next pair
  for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
  const uint64_t below = (uint64_t{1} << lane) - 1;
  const uint32_t o_offset = tile.first - tile.chunk_first + 64 * wave;
  uint32_t strip = 0;
  w.walk(a, ci, lane,
         [&](uint32_t r, uint64_t mask) {
           if (!mask) return;   // (scalar branch)
           const uint64_t slot = read_lane(at, r) + static_cast<uint32_t>(__popcll(mask & below));
           if (mask >> lane & 1) {
             a.o_out[slot] = (uint64_t{o_offset + r} << 32) | tile.chunk;
             a.i_out[slot] = (uint64_t{strip + lane} << 32) | ci;
           }
           if (lane == r) at += static_cast<uint32_t>(__popcll(mask));
         },
         [&](uint32_t begin, bool) { strip = begin + 64; });
}

// The flagged O rows of a tile at their slots: own RowID, NULL_ROW_ID on the other side (other_out == nullptr: Semi / Anti).
__global__ __launch_bounds__(256) void nlj_emit_flags(const NljTile* tiles, const uint32_t* counts, const uint64_t* segment_offsets, uint32_t slots, uint64_t* own_out, uint64_t* other_out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const NljTile tile = tiles[blockIdx.x];
  const bool flag = threadIdx.x < tile.rows && counts[tile.count_base + uint64_t{slots} * tile.chunk_rows + threadIdx.x] != 0;
  const uint64_t mask = __ballot(flag);
  if (lane == 0) s_wave[wave] = static_cast<uint32_t>(__popcll(mask));
  __syncthreads();
  uint64_t at = segment_offsets[tile.segment_first + slots * tile.segment_stride] + static_cast<uint32_t>(__popcll(mask & ((uint64_t{1} << lane) - 1)));
  for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
  if (flag) {
    own_out[at] = (uint64_t{tile.first - tile.chunk_first + threadIdx.x} << 32) | tile.chunk;
    if (other_out) other_out[at] = NULL_ROW;
  }
}

// masks[w] = the rows 64 w .. 64 w + 63 of the I side that have no partner (rows behind n: 0); counts[tile] = how many (smj_mark's output).
__global__ __launch_bounds__(256) void nlj_unmatched(const uint64_t* matched, uint32_t n, uint64_t* masks, uint32_t* counts) {
  __shared__ uint32_t s_count[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t count = 0;
  const uint32_t n_words = (n + 63) / 64;
  for (uint32_t step = lane; step < MARK_TILE_WORDS / 4; step += 64) {
    const uint64_t word = uint64_t{blockIdx.x} * MARK_TILE_WORDS + wave * (MARK_TILE_WORDS / 4) + step;
    uint64_t mask = 0;
    if (word < n_words) {
      mask = ~matched[word];
      if (word == n_words - 1 && (n & 63)) mask &= (uint64_t{1} << (n & 63)) - 1;
    }
    masks[word] = mask;
    count += static_cast<uint32_t>(__popcll(mask));
  }
  for (int offset = 32; offset > 0; offset >>= 1) count += static_cast<uint32_t>(__shfl_xor(static_cast<int>(count), offset));
  if (lane == 0) s_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

// One operand column: export_column_at's values (4 or 8 bytes, `from` = its HY_TYPE_*) as 8-byte words of the predicate's common type `to`
// (HY_TYPE_LONG, HY_TYPE_FLOAT -- rounded to float, held as double -- or HY_TYPE_DOUBLE), and bit p of the row's null byte.
__global__ __launch_bounds__(256) void nlj_operand(const void* values, const uint8_t* nulls, uint32_t n, uint32_t from, uint32_t to, uint32_t p, uint64_t* out, uint8_t* null_bits) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    int64_t integer = 0;
    double real = 0.0;
    switch (from) {
      case HY_TYPE_INT: integer = static_cast<const int32_t*>(values)[i]; break;
      case HY_TYPE_LONG: integer = static_cast<const int64_t*>(values)[i]; break;
      case HY_TYPE_FLOAT: real = static_cast<const float*>(values)[i]; break;
      default: real = static_cast<const double*>(values)[i]; break;
    }
    const bool from_real = from == HY_TYPE_FLOAT || from == HY_TYPE_DOUBLE;
    uint64_t word;
    if (to == HY_TYPE_LONG) word = static_cast<uint64_t>(integer);
    else if (to == HY_TYPE_FLOAT) word = static_cast<uint64_t>(__double_as_longlong(static_cast<double>(from_real ? static_cast<float>(real) : static_cast<float>(integer))));
    else word = static_cast<uint64_t>(__double_as_longlong(from_real ? real : static_cast<double>(integer)));
    out[i] = nulls[i] ? 0 : word;
    if (nulls[i]) null_bits[i] |= static_cast<uint8_t>(1u << p);   // (one thread per row, the launches of a side in stream order)
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
uint32_t flip(uint32_t condition) {   // flip_predicate_condition (types.cpp)
  switch (condition) {
    case HY_PRED_LESS_THAN: return HY_PRED_GREATER_THAN;
    case HY_PRED_LESS_THAN_EQUALS: return HY_PRED_GREATER_THAN_EQUALS;
    case HY_PRED_GREATER_THAN: return HY_PRED_LESS_THAN;
    case HY_PRED_GREATER_THAN_EQUALS: return HY_PRED_LESS_THAN_EQUALS;
    default: return condition;
  }
}

uint32_t common_type(uint32_t a, uint32_t b) {   // the usual arithmetic conversions over int32 / int64 / float / double
  if (a == HY_TYPE_DOUBLE || b == HY_TYPE_DOUBLE) return HY_TYPE_DOUBLE;
  if (a == HY_TYPE_FLOAT || b == HY_TYPE_FLOAT) return HY_TYPE_FLOAT;
  return HY_TYPE_LONG;
}

hy_status check_column(const hy_column* column, const char* entry_point) {
  if (!column) return fail(HY_ERR_INVALID, "%s: null column", entry_point);
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_UNSUPPORTED, "%s: MVCC columns are read by hy_validate only", entry_point);
  if (column->data_type < HY_TYPE_INT || column->data_type > HY_TYPE_DOUBLE) return fail(HY_ERR_UNSUPPORTED, "%s: string columns stay on the stock operator", entry_point);
  if (column->has_dictionary_without_values) return fail(HY_ERR_UNSUPPORTED, "%s: the dictionary values are not on the device", entry_point);
  if (column->rows >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "%s: %llu rows on one side (32-bit row ids)", entry_point, static_cast<unsigned long long>(column->rows));
  return HY_OK;
}

// One side's operands: [n_predicates][stride] words and a null byte per row.
struct Operands {
  DeviceBuffer words, nulls;
  uint64_t stride = 0;
};

hy_status load_operands(const hy_column* const* columns, const uint32_t* to, uint32_t n_predicates, uint32_t n, Operands& out, hipStream_t stream) {
  out.stride = (uint64_t{n} + 1) & ~uint64_t{1};
  HY_TRY(out.words.alloc(8 * out.stride * n_predicates + 16));
  HY_TRY(out.nulls.alloc(size_t{n} + 16));
  if (!n) return HY_OK;
  HY_HIP(hipMemsetAsync(out.nulls.ptr, 0, n, stream));
  DeviceBuffer values, nulls;   // export_column_at's output, one column at a time
  HY_TRY(values.alloc(8 * size_t{n} + 16));
  HY_TRY(nulls.alloc(size_t{n} + 16));
  for (uint32_t p = 0; p < n_predicates; ++p) {
    HY_TRY(export_column_at(columns[p], values.ptr, nulls.as<uint8_t>(), nullptr));
    hipLaunchKernelGGL(nlj_operand, dim3(std::min<uint32_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, values.ptr, nulls.as<uint8_t>(), n, columns[p]->data_type, to[p], p,
                       out.words.as<uint64_t>() + p * out.stride, out.nulls.as<uint8_t>());
    HY_HIP(hipGetLastError());
  }
  return HY_OK;
}

template <uint32_t NP>
void launch_walks(bool emit, uint32_t grid, const NljArgs& args, hipStream_t stream) {
  if (emit) hipLaunchKernelGGL(nlj_emit<NP>, dim3(grid), dim3(256), 0, stream, args);
  else hipLaunchKernelGGL(nlj_count<NP>, dim3(grid), dim3(256), 0, stream, args);
}

hy_status launch_walk(bool emit, uint32_t n_predicates, uint32_t grid, const NljArgs& args, hipStream_t stream) {
  switch (n_predicates) {
    case 1: launch_walks<1>(emit, grid, args, stream); break;
    case 2: launch_walks<2>(emit, grid, args, stream); break;
    case 3: launch_walks<3>(emit, grid, args, stream); break;
    case 4: launch_walks<4>(emit, grid, args, stream); break;
    default: launch_walks<5>(emit, grid, args, stream); break;
  }
  HY_HIP(hipGetLastError());
  return HY_OK;
}

// result == nullptr: the counting passes only.
hy_status run_nested_loop(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, const hy_join_predicate* secondary, uint32_t n_secondary,
                          hy_nested_loop_result* result, uint64_t* n_pairs_out, const char* entry_point) {
  if (!left || !right || (n_secondary && !secondary)) return fail(HY_ERR_INVALID, "%s: null argument", entry_point);
  if (mode == HY_JOIN_CROSS || mode > HY_JOIN_ANTI_NULL_AS_FALSE) return fail(HY_ERR_UNSUPPORTED, "%s: join mode %u (Cross is the Product operator)", entry_point, mode);
  if (condition > HY_PRED_GREATER_THAN_EQUALS) return fail(HY_ERR_UNSUPPORTED, "%s: condition %u is no comparison of two columns", entry_point, condition);
  if (n_secondary > HY_MAX_SECONDARY_PREDICATES) return fail(HY_ERR_UNSUPPORTED, "%s: more than %u secondary join predicates stay on the stock operator", entry_point, HY_MAX_SECONDARY_PREDICATES);
  HY_TRY(check_column(left, entry_point));
  HY_TRY(check_column(right, entry_point));
  for (uint32_t p = 0; p < n_secondary; ++p) {
    const hy_join_predicate& predicate = secondary[p];
    if (!predicate.left_column || !predicate.right_column) return fail(HY_ERR_INVALID, "%s: secondary join predicate %u: column missing", entry_point, p);
    if (predicate.condition > HY_PRED_GREATER_THAN_EQUALS) return fail(HY_ERR_INVALID, "%s: secondary join predicate %u: condition %u is no comparison", entry_point, p, predicate.condition);
    HY_TRY(check_column(predicate.left_column, entry_point));
    HY_TRY(check_column(predicate.right_column, entry_point));
    if (predicate.left_column->row_base != left->row_base || predicate.right_column->row_base != right->row_base)
      return fail(HY_ERR_INVALID, "%s: secondary join predicate %u: the columns do not have the chunk layout of the join's input tables", entry_point, p);
  }
  const bool semi_anti = mode == HY_JOIN_SEMI || mode == HY_JOIN_ANTI_NULL_AS_TRUE || mode == HY_JOIN_ANTI_NULL_AS_FALSE;
  if (result) {
    if (result->mem != HY_MEM_HOST && result->mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "%s: result->mem %u", entry_point, result->mem);
    result->n_pairs = 0;
    if (result->capacity && (!result->left_pos || (!semi_anti && !result->right_pos))) return fail(HY_ERR_INVALID, "%s: null output list", entry_point);
    if (reinterpret_cast<uintptr_t>(result->left_pos) % 8 != 0 || (!semi_anti && reinterpret_cast<uintptr_t>(result->right_pos) % 8 != 0))
      return fail(HY_ERR_INVALID, "%s: output list not on an 8-byte boundary", entry_point);
  }
  // O: the side the walk's outer loops run over -- the left input, under Right the right one (join_nested_loop.cpp:130-139)
  const bool swapped = mode == HY_JOIN_RIGHT;
  const hy_column* outer = swapped ? right : left;
  const hy_column* inner = swapped ? left : right;
  const uint32_t n_predicates = 1 + n_secondary;
  const hy_column* o_columns[NLJ_MAX_PREDICATES];
  const hy_column* i_columns[NLJ_MAX_PREDICATES];
  uint32_t conditions[NLJ_MAX_PREDICATES], types[NLJ_MAX_PREDICATES];
  for (uint32_t p = 0; p < n_predicates; ++p) {
    const hy_column* l = p ? secondary[p - 1].left_column : left;
    const hy_column* r = p ? secondary[p - 1].right_column : right;
    const uint32_t c = p ? secondary[p - 1].condition : condition;
    o_columns[p] = swapped ? r : l;
    i_columns[p] = swapped ? l : r;
    conditions[p] = swapped ? flip(c) : c;
    types[p] = common_type(l->data_type, r->data_type);   // (a column without chunks calls itself int and has no row to convert)
  }
  const uint64_t o_rows = outer->rows, i_rows = inner->rows;
  if (o_rows && i_rows > NLJ_MAX_COMPARISONS / o_rows)
    return fail(HY_ERR_UNSUPPORTED, "%s: %llu x %llu rows are more than %llu comparisons", entry_point, static_cast<unsigned long long>(left->rows), static_cast<unsigned long long>(right->rows),
                static_cast<unsigned long long>(NLJ_MAX_COMPARISONS));
  const bool pairs = !semi_anti;
  const bool full = mode == HY_JOIN_FULL_OUTER;
  const bool flags = mode != HY_JOIN_INNER;
  const uint32_t i_chunks = inner->n_chunks;
  const uint32_t slots = pairs ? i_chunks : 0;

  // the tiles of O, and where their counts and segments lie
  std::vector<NljTile> tiles;
  uint64_t n_segments = 0;
  for (uint32_t co = 0; co < outer->n_chunks; ++co) {
    const uint64_t chunk_first = outer->row_base[co];
    const uint32_t chunk_rows = static_cast<uint32_t>(outer->row_base[co + 1] - chunk_first);
    const uint32_t chunk_tiles = (chunk_rows + NLJ_TILE - 1) / NLJ_TILE;
    if (n_segments + uint64_t{chunk_tiles} * (slots + 1) > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "%s: more than 2^31 (tile, chunk) segments", entry_point);
    for (uint32_t t = 0; t < chunk_tiles; ++t) {
      NljTile tile{};
      tile.count_base = chunk_first * (uint64_t{slots} + 1) + uint64_t{t} * NLJ_TILE;
      tile.first = static_cast<uint32_t>(chunk_first + uint64_t{t} * NLJ_TILE);
      tile.rows = std::min<uint32_t>(NLJ_TILE, chunk_rows - t * NLJ_TILE);
      tile.chunk = co;
      tile.chunk_first = static_cast<uint32_t>(chunk_first);
      tile.chunk_rows = chunk_rows;
      tile.segment_first = static_cast<uint32_t>(n_segments) + t;
      tile.segment_stride = chunk_tiles;
      tiles.push_back(tile);
    }
    n_segments += uint64_t{chunk_tiles} * (slots + 1);
  }
  const uint64_t n_tiles = tiles.size();
  const uint64_t walk_grid = n_tiles * i_chunks;
  if (walk_grid > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "%s: %llu (tile, chunk) pairs are more than one launch walks", entry_point, static_cast<unsigned long long>(walk_grid));
  const uint64_t mark_tiles = full ? (i_rows + MARK_TILE - 1) / MARK_TILE : 0;
  const uint64_t temporary_bytes = 8 * n_predicates * (o_rows + i_rows) + 10 * std::max(o_rows, i_rows) + 4 * o_rows * (uint64_t{slots} + 1) + 16 * n_segments + sizeof(NljTile) * n_tiles +
                                   32 * n_tiles + mark_tiles * (8 * MARK_TILE_WORDS + 8) + i_rows / 8;
  if (temporary_bytes > HY_NLJ_MAX_TEMPORARY_BYTES)
    return fail(HY_ERR_UNSUPPORTED, "%s: %llu bytes of temporaries (%llu rows x %u chunks) are more than %llu", entry_point, static_cast<unsigned long long>(temporary_bytes),
                static_cast<unsigned long long>(o_rows), i_chunks, static_cast<unsigned long long>(HY_NLJ_MAX_TEMPORARY_BYTES));

  hipStream_t stream = current_stream();
  uint64_t* totals = nullptr;   // [0] pairs and flagged O rows; 32-bit word [2]: unmatched I rows
  uint64_t* d_totals = nullptr;
  HY_TRY(pinned_staging(64, reinterpret_cast<void**>(&totals), reinterpret_cast<void**>(&d_totals)));
  totals[0] = totals[1] = 0;
  const volatile uint32_t* unmatched_total = reinterpret_cast<const uint32_t*>(totals) + 2;
  profile_begin(stream);   // (hy_set_profiling: one event pair around the call's kernels, the host's read in between included)
  struct ProfileEnd { hipStream_t stream; ~ProfileEnd() { profile_end(stream); } } profile_bracket{stream};

  Operands o, i;
  DeviceBuffer d_tiles, counts, segment_sums, segment_offsets, o_matched, i_matched, masks, mark_counts, mark_offsets;
  NljArgs args{};
  if (n_tiles) {
    HY_TRY(load_operands(o_columns, types, n_predicates, static_cast<uint32_t>(o_rows), o, stream));
    HY_TRY(load_operands(i_columns, types, n_predicates, static_cast<uint32_t>(i_rows), i, stream));
    HY_TRY(d_tiles.alloc(sizeof(NljTile) * n_tiles));
    HY_TRY(counts.alloc(4 * o_rows * (uint64_t{slots} + 1) + 16));
    HY_TRY(segment_sums.alloc(8 * n_segments));
    HY_TRY(segment_offsets.alloc(8 * n_segments));
    HY_TRY(o_matched.alloc(32 * n_tiles));
    HY_HIP(hipMemcpyAsync(d_tiles.ptr, tiles.data(), sizeof(NljTile) * n_tiles, hipMemcpyHostToDevice, stream));   // (pageable memory: copied before the call returns)
    HY_HIP(hipMemsetAsync(o_matched.ptr, 0, 32 * n_tiles, stream));
    args.tiles = d_tiles.as<NljTile>();
    args.o_operands = o.words.as<uint64_t>();
    args.i_operands = i.words.as<uint64_t>();
    args.o_nulls = o.nulls.as<uint8_t>();
    args.i_nulls = i.nulls.as<uint8_t>();
    args.o_stride = o.stride;
    args.i_stride = i.stride;
    args.i_row_base = inner->d_row_base;
    args.i_chunks = i_chunks;
    args.slots = slots;
    args.null_matches = mode == HY_JOIN_ANTI_NULL_AS_TRUE;
    args.track_inner = full;
    for (uint32_t p = 0; p < n_predicates; ++p) {
      args.condition[p] = conditions[p];
      args.type[p] = types[p] == HY_TYPE_LONG ? HY_TYPE_LONG : HY_TYPE_DOUBLE;
    }
    args.counts = counts.as<uint32_t>();
    args.segment_sums = segment_sums.as<uint64_t>();
    args.segment_offsets = segment_offsets.as<uint64_t>();
    args.o_matched = o_matched.as<uint64_t>();
  }
  if (mark_tiles) {
    HY_TRY(i_matched.alloc(8 * mark_tiles * MARK_TILE_WORDS + 16));
    HY_TRY(masks.alloc(8 * mark_tiles * MARK_TILE_WORDS));
    HY_TRY(mark_counts.alloc(4 * mark_tiles));
    HY_TRY(mark_offsets.alloc(4 * mark_tiles));
    HY_HIP(hipMemsetAsync(i_matched.ptr, 0, 8 * mark_tiles * MARK_TILE_WORDS + 16, stream));
    args.i_matched = i_matched.as<uint64_t>();
  }
  if (walk_grid && i_rows) HY_TRY(launch_walk(false, n_predicates, static_cast<uint32_t>(walk_grid), args, stream));
  else if (n_tiles && slots) HY_HIP(hipMemsetAsync(segment_sums.ptr, 0, 8 * n_segments, stream));   // (an I side of empty chunks only: no pair, and nlj_emit does not run)
  if (n_tiles) {
    hipLaunchKernelGGL(nlj_flags, dim3(static_cast<uint32_t>(n_tiles)), dim3(256), 0, stream, args.tiles, args.o_matched, slots, flags ? 1u : 0u,
                       (mode == HY_JOIN_SEMI || mode == HY_JOIN_INNER) ? 0u : 1u, args.counts, args.segment_sums);
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(nlj_scan_segments, dim3(1), dim3(1024), 0, stream, args.segment_sums, static_cast<uint32_t>(n_segments), segment_offsets.as<uint64_t>(), d_totals);
    HY_HIP(hipGetLastError());
  }
  if (mark_tiles) {
    hipLaunchKernelGGL(nlj_unmatched, dim3(static_cast<uint32_t>(mark_tiles)), dim3(256), 0, stream, args.i_matched, static_cast<uint32_t>(i_rows), masks.as<uint64_t>(), mark_counts.as<uint32_t>());
    HY_HIP(hipGetLastError());
    hipLaunchKernelGGL(select_scan_tiles, dim3(1), dim3(1024), 0, stream, mark_counts.as<uint32_t>(), static_cast<uint32_t>(mark_tiles), mark_offsets.as<uint32_t>(), reinterpret_cast<uint32_t*>(d_totals) + 2);
    HY_HIP(hipGetLastError());
  }
  HY_HIP(hipStreamSynchronize(stream));   // the call's one host read before the capacity decision

  const uint64_t n_walked = n_tiles ? totals[0] : 0;   // pairs and flagged O rows, in the walk's order
  const uint64_t n_unmatched = mark_tiles ? *unmatched_total : 0;
  const uint64_t n_pairs = n_walked + n_unmatched;
  if (n_pairs_out) *n_pairs_out = n_pairs;
  if (!result) return HY_OK;
  result->n_pairs = n_pairs;
  if (n_pairs > result->capacity) return fail(HY_ERR_CAPACITY, "%s: %llu rows, capacity %llu", entry_point, static_cast<unsigned long long>(n_pairs), static_cast<unsigned long long>(result->capacity));
  if (!n_pairs) return HY_OK;

  const bool host_result = result->mem == HY_MEM_HOST;
  DeviceBuffer left_list, right_list;   // a host result: the lists in device memory first
  uint64_t* left_out = reinterpret_cast<uint64_t*>(result->left_pos);
  uint64_t* right_out = semi_anti ? nullptr : reinterpret_cast<uint64_t*>(result->right_pos);
  if (host_result) {
    HY_TRY(left_list.alloc(8 * n_pairs));
    left_out = left_list.as<uint64_t>();
    if (!semi_anti) {
      HY_TRY(right_list.alloc(8 * n_pairs));
      right_out = right_list.as<uint64_t>();
    }
  }
  uint64_t* o_out = swapped ? right_out : left_out;
  uint64_t* i_out = swapped ? left_out : right_out;
  if (n_walked) {
    if (pairs && walk_grid && i_rows) {
      args.o_out = o_out;
      args.i_out = i_out;
      HY_TRY(launch_walk(true, n_predicates, static_cast<uint32_t>(walk_grid), args, stream));
    }
    if (flags) {
      hipLaunchKernelGGL(nlj_emit_flags, dim3(static_cast<uint32_t>(n_tiles)), dim3(256), 0, stream, args.tiles, args.counts, args.segment_offsets, slots, o_out, i_out);
      HY_HIP(hipGetLastError());
    }
  }
  if (n_unmatched) {
    hipLaunchKernelGGL(smj_outer_emit, dim3(static_cast<uint32_t>(mark_tiles)), dim3(256), 0, stream, masks.as<uint64_t>(), mark_offsets.as<uint32_t>(), inner->d_row_base, inner->n_chunks, n_walked, i_out, o_out);
    HY_HIP(hipGetLastError());
  }
  if (host_result) {
    HY_HIP(hipMemcpyAsync(result->left_pos, left_out, 8 * n_pairs, hipMemcpyDeviceToHost, stream));
    if (!semi_anti) HY_HIP(hipMemcpyAsync(result->right_pos, right_out, 8 * n_pairs, hipMemcpyDeviceToHost, stream));
  }
  HY_HIP(hipStreamSynchronize(stream));   // (the temporaries go back to the pool; the caller reads the lists next)
  return HY_OK;
}

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_join_nested_loop(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, const hy_join_predicate* secondary, uint32_t n_secondary,
                              hy_nested_loop_result* result) {
  if (!result) return fail(HY_ERR_INVALID, "hy_join_nested_loop: null result");
  return run_nested_loop(left, right, mode, condition, secondary, n_secondary, result, nullptr, "hy_join_nested_loop");
}

hy_status hy_join_nested_loop_count(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, const hy_join_predicate* secondary, uint32_t n_secondary,
                                    uint64_t* n_pairs) {
  if (!n_pairs) return fail(HY_ERR_INVALID, "hy_join_nested_loop_count: null argument");
  *n_pairs = 0;
  return run_nested_loop(left, right, mode, condition, secondary, n_secondary, nullptr, n_pairs, "hy_join_nested_loop_count");
}

}  // extern "C"

// product.hip -- Product (operators/product.cpp) on the device: the cross join the translator emits for every JoinMode::Cross
// (lqp_translator.cpp:362).  Its output is a pure function of the two inputs' chunk sizes and, for reference inputs, their PosLists:
// product.cpp:51-61 runs over the chunk pairs (cl, cr), cl outermost, and :114-128 writes for output row p of a pair the left offset
// p / rows(cr) and the right offset p % rows(cr) -- as RowID {chunk, offset} of a data column, as the input PosList's entry at that offset
// of a reference column.  Both lists are store-only streams of 8 bytes per output row.
//
// product_fill, ONE launch per call: the output is cut into tiles of at most TILE_ROWS rows that never cross a pair's region; the host
// builds the tile table from the chunk sizes (the cuts lie on multiples of TILE_ROWS of the OUTPUT row index, so that with lists on
// 128-byte boundaries only a region's first and last line are shared between two workgroups).  A workgroup owns one tile of ONE list
// (blockIdx.y picks the list: the two lists may lie on different 16-byte parities, and the left list needs p / rows(cr) where the right one
// needs p % rows(cr)).  The tile's record, both segment descriptors and rows(cr) are wave-uniform: scalar loads.  A thread divides once --
// by a multiply-high with the reciprocal the host computed for the right chunk -- and then walks its rows by adding the step's quotient
// and remainder and wrapping.  Lanes write neighbouring 16-byte vectors (two RowIDs at an even slot of the list: 1 KiB per wave and
// instruction); a row whose neighbour in the vector belongs to somebody else (a region that starts or ends on an odd slot) is one
// 8-byte store.  No workgroup waits for another; no atomics, no LDS, no scratch.
// A reference input's left entry is loaded when the left offset changes (once per run of rows(cr) equal rows a thread meets), the right
// list is read cyclically (L2-resident at Hyrise's chunk sizes); NULL_ROW_ID entries pass through like any other.
#include "hy_device.hpp"

#include <algorithm>

namespace hy {

namespace {

constexpr uint32_t TILE_ROWS = 8192;         // output rows per tile: 64 KiB of one list, 16 steps of 256 threads x 2 rows
constexpr uint32_t STEP_ROWS = 2 * 256;      // rows a workgroup writes per step

typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));

// One tile of one pair's region: output rows [out_row, out_row + rows) are the pair's rows [first, first + rows).
struct ProductTile {
  uint64_t out_row;
  uint64_t reciprocal;   // ceil(2^64 / rows(cr)): (p * reciprocal) >> 64 == p / rows(cr) for every p < 2^32 (rows(cr) == 1: unused)
  uint32_t cl, cr;
  uint32_t first;
  uint32_t rows;
};
static_assert(sizeof(ProductTile) == 32, "two 16-byte scalar loads");

struct ProductArgs {
  const ProductTile* tiles;
  const DevSegment* left_segments;
  const DevSegment* right_segments;
  uint64_t* left_out;
  uint64_t* right_out;
  uint32_t left_is_reference, right_is_reference;
  uint32_t first_side;   // 0: blockIdx.y 0 writes the left list; 1: the right one (the only one wanted)
};

__host__ __device__ __forceinline__ uint32_t divide(uint32_t p, uint32_t divisor, uint64_t reciprocal) {
#ifdef __HIP_DEVICE_COMPILE__
  return divisor == 1 ? p : static_cast<uint32_t>(__umul64hi(p, reciprocal));
#else
  return divisor == 1 ? p : static_cast<uint32_t>((static_cast<unsigned __int128>(p) * reciprocal) >> 64);
#endif
}

template <bool NONTEMPORAL>
__global__ __launch_bounds__(256) void product_fill(ProductArgs a) {
  const bool right_side = (a.first_side + blockIdx.y) != 0;
  const ProductTile t = a.tiles[blockIdx.x];
  const uint32_t rc = a.right_segments[t.cr].size;
  const DevSegment& segment = right_side ? a.right_segments[t.cr] : a.left_segments[t.cl];
  const bool is_reference = (right_side ? a.right_is_reference : a.left_is_reference) != 0;
  const uint64_t* list = is_reference ? static_cast<const uint64_t*>(segment.data) : nullptr;   // nullptr: {chunk, offset}
  const uint64_t chunk = is_reference ? segment.ref_chunk_id : (right_side ? t.cr : t.cl);      // (an EntireChunkPosList's chunk)
  uint64_t* out = (right_side ? a.right_out : a.left_out) + t.out_row;
  // slot s of the tile is its row s - parity; slots 2j and 2j + 1 share a 16-byte vector of the list
  const uint32_t parity = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) >> 3) & 1u;
  const uint32_t slots = t.rows + parity;
  const uint32_t step_l = divide(STEP_ROWS, rc, t.reciprocal), step_r = STEP_ROWS - step_l * rc;
  // the thread's second slot is the row that always exists in the pair's arithmetic (the first may be row -1 of the pair)
  const uint32_t p1 = t.first + 2 * threadIdx.x + 1 - parity;
  uint32_t l1 = divide(p1, rc, t.reciprocal), r1 = p1 - l1 * rc;
  uint32_t cached_index = 0xFFFFFFFFu;
  uint64_t cached = 0;
  const auto value_at = [&](uint32_t index) -> uint64_t {
    if (!list) return (static_cast<uint64_t>(index) << 32) | chunk;
    if (index != cached_index) { cached = list[index]; cached_index = index; }
    return cached;
  };
  for (uint32_t slot = 2 * threadIdx.x; slot < slots; slot += STEP_ROWS) {
    const bool valid0 = slot >= parity, valid1 = slot + 1 < slots;
    // the row before (l1, r1)
    const uint32_t l0 = r1 ? l1 : l1 - 1, r0 = r1 ? r1 - 1 : rc - 1;
    uint64_t v0 = 0, v1 = 0;
    if (valid0) v0 = value_at(right_side ? r0 : l0);
    if (valid1) v1 = value_at(right_side ? r1 : l1);
    uint64_t* at = out + slot - parity;   // (slot 0 under parity 1: one RowID in front of the tile, not written)
    if (valid0 && valid1) {
      if constexpr (NONTEMPORAL) __builtin_nontemporal_store(u64x2_t{v0, v1}, reinterpret_cast<u64x2_t*>(at));
      else *reinterpret_cast<u64x2_t*>(at) = u64x2_t{v0, v1};
    } else if (valid0) {
      at[0] = v0;
    } else if (valid1) {
      at[1] = v1;
    }
    const uint32_t r = r1 + step_r;
    l1 += step_l;
    if (r >= rc || r < r1) { r1 = r - rc; ++l1; } else { r1 = r; }
  }
}

hy_status check_input(const hy_column* column, const char* name, const char* entry_point) {
  HY_TRY(on_this_device(column, entry_point));
  if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_UNSUPPORTED, "%s: %s is an MVCC pseudo-column (hy_validate reads those)", entry_point, name);
  if (column->is_reference) {
    for (uint32_t k = 0; k < column->n_chunks; ++k)
      if (reinterpret_cast<uintptr_t>(column->host_segments[k].data) % 8 != 0) return fail(HY_ERR_INVALID, "%s: %s chunk %u: PosList not on an 8-byte boundary", entry_point, name, k);
  }
  return HY_OK;
}

// result == nullptr: the count only.
hy_status run_product(const hy_column* left, const hy_column* right, hy_product_result* result, uint64_t* n_rows_out, const char* entry_point) {
  if (!left || !right) return fail(HY_ERR_INVALID, "%s: null argument", entry_point);
  if (result) {
    result->n_rows = 0;
    if (result->mem != HY_MEM_HOST && result->mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "%s: result->mem %u", entry_point, result->mem);
    if (!result->left_pos && !result->right_pos) return fail(HY_ERR_INVALID, "%s: neither list is wanted (left_pos and right_pos are NULL)", entry_point);
    if (reinterpret_cast<uintptr_t>(result->left_pos) % 8 != 0 || reinterpret_cast<uintptr_t>(result->right_pos) % 8 != 0)
      return fail(HY_ERR_INVALID, "%s: output list not on an 8-byte boundary", entry_point);
  }
  HY_TRY(check_input(left, "left", entry_point));
  HY_TRY(check_input(right, "right", entry_point));
  const uint32_t n_left = left->n_chunks, n_right = right->n_chunks;
  // every pair's rows fit a ChunkOffset (product.cpp:120), the sum fits 64 bits
  uint32_t largest_left = 0, largest_right = 0;
  for (uint32_t cl = 0; cl < n_left; ++cl) largest_left = std::max(largest_left, left->host_segments[cl].size);
  for (uint32_t cr = 0; cr < n_right; ++cr) largest_right = std::max(largest_right, right->host_segments[cr].size);
  if (uint64_t{largest_left} * largest_right >= 0xFFFFFFFFull)
    return fail(HY_ERR_UNSUPPORTED, "%s: a chunk pair of %u x %u rows does not fit a ChunkOffset", entry_point, largest_left, largest_right);
  if (left->rows && right->rows > ~uint64_t{0} / left->rows) return fail(HY_ERR_UNSUPPORTED, "%s: %llu x %llu rows", entry_point, static_cast<unsigned long long>(left->rows),
                                                                         static_cast<unsigned long long>(right->rows));
  const uint64_t n_rows = left->rows * right->rows;
  if (n_rows_out) *n_rows_out = n_rows;
  if (!result) return HY_OK;
  result->n_rows = n_rows;
  if (n_rows > result->capacity) return fail(HY_ERR_CAPACITY, "%s: %llu rows, capacity %llu", entry_point, static_cast<unsigned long long>(n_rows), static_cast<unsigned long long>(result->capacity));

  // the tiles: a pair's region is cut where the output row index passes a multiple of TILE_ROWS
  uint64_t n_tiles = 0;
  if (n_rows) {
    n_tiles = n_rows / TILE_ROWS + 1;
    for (uint32_t cl = 0; cl < n_left; ++cl) if (left->host_segments[cl].size) n_tiles += n_right;   // (an upper bound: a cut and a region's end per tile)
  }
  if (n_tiles > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "%s: more than 2^31 tiles", entry_point);
  ProductTile* tiles = nullptr;
  ProductTile* pinned_device_view = nullptr;
  if (n_tiles) HY_TRY(pinned_staging(sizeof(ProductTile) * n_tiles, reinterpret_cast<void**>(&tiles), reinterpret_cast<void**>(&pinned_device_view)));
  std::vector<uint64_t> reciprocals(n_right, 0);
  for (uint32_t cr = 0; cr < n_right; ++cr) {
    const uint32_t rc = right->host_segments[cr].size;
    if (rc > 1) reciprocals[cr] = ~uint64_t{0} / rc + 1;
  }
  uint64_t* pair_offsets = result->pair_offsets;
  uint64_t out_row = 0;
  uint32_t used = 0;
  for (uint32_t cl = 0; cl < n_left; ++cl) {
    const uint64_t rl = left->host_segments[cl].size;
    for (uint32_t cr = 0; cr < n_right; ++cr) {
      if (pair_offsets) pair_offsets[size_t{cl} * n_right + cr] = out_row;
      const uint64_t pair_rows = rl * right->host_segments[cr].size;
      for (uint64_t first = 0; first < pair_rows;) {
        const uint64_t at = out_row + first;
        const uint64_t rows = std::min(pair_rows - first, TILE_ROWS - at % TILE_ROWS);
        tiles[used++] = ProductTile{at, reciprocals[cr], cl, cr, static_cast<uint32_t>(first), static_cast<uint32_t>(rows)};
        first += rows;
      }
      out_row += pair_rows;
    }
  }
  if (pair_offsets) pair_offsets[size_t{n_left} * n_right] = out_row;
  if (!n_rows) return HY_OK;

  hipStream_t stream = current_stream();
  const bool host_result = result->mem == HY_MEM_HOST;
  DeviceBuffer d_tiles, left_list, right_list;   // a host result: the lists in device memory first
  HY_TRY(d_tiles.alloc(sizeof(ProductTile) * used));
  HY_HIP(hipMemcpyAsync(d_tiles.ptr, tiles, sizeof(ProductTile) * used, hipMemcpyHostToDevice, stream));   // (pinned: the call waits for the stream before it returns)
  ProductArgs args{};
  args.tiles = d_tiles.as<ProductTile>();
  args.left_segments = left->d_segments;
  args.right_segments = right->d_segments;
  args.left_is_reference = left->is_reference;
  args.right_is_reference = right->is_reference;
  args.left_out = reinterpret_cast<uint64_t*>(result->left_pos);
  args.right_out = reinterpret_cast<uint64_t*>(result->right_pos);
  if (host_result) {
    if (result->left_pos) { HY_TRY(left_list.alloc(8 * n_rows)); args.left_out = left_list.as<uint64_t>(); }
    if (result->right_pos) { HY_TRY(right_list.alloc(8 * n_rows)); args.right_out = right_list.as<uint64_t>(); }
  }
  args.first_side = args.left_out ? 0 : 1;
  const dim3 grid(used, args.left_out && args.right_out ? 2 : 1);
  profile_begin(stream);
  if (option(HY_OPT_PRODUCT_NONTEMPORAL)) hipLaunchKernelGGL(product_fill<true>, grid, dim3(256), 0, stream, args);
  else hipLaunchKernelGGL(product_fill<false>, grid, dim3(256), 0, stream, args);
  profile_end(stream);
  HY_HIP(hipGetLastError());
  if (host_result) {
    if (result->left_pos) HY_HIP(hipMemcpyAsync(result->left_pos, args.left_out, 8 * n_rows, hipMemcpyDeviceToHost, stream));
    if (result->right_pos) HY_HIP(hipMemcpyAsync(result->right_pos, args.right_out, 8 * n_rows, hipMemcpyDeviceToHost, stream));
  }
  HY_HIP(hipStreamSynchronize(stream));   // (the tile table goes back to the pool; the caller reads the lists next)
  return HY_OK;
}

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_product(const hy_column* left, const hy_column* right, hy_product_result* result) {
  if (!result) return fail(HY_ERR_INVALID, "hy_product: null result");
  return run_product(left, right, result, nullptr, "hy_product");
}

hy_status hy_product_count(const hy_column* left, const hy_column* right, uint64_t* n_rows) {
  if (!n_rows) return fail(HY_ERR_INVALID, "hy_product_count: null argument");
  *n_rows = 0;
  return run_product(left, right, nullptr, n_rows, "hy_product_count");
}

}  // extern "C"

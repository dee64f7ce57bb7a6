// scan_expression.hip -- TableScan over a predicate expression: the evaluator's scan, one pass, a program in, PosLists out.
//
// What it replaces (reference, CPU):
//   TableScan::create_impl's fallback                                    operators/table_scan.cpp:312-452
//   ExpressionEvaluatorTableScanImpl::scan_chunk                         operators/table_scan/expression_evaluator_table_scan_impl.cpp:21-24
//   ExpressionEvaluator::evaluate_expression_to_pos_list                 expression/evaluation/expression_evaluator.cpp:1129-1311
//
// The reference recurses over the predicate: AND / OR intersect / unite the children's sorted PosLists, every other node is evaluated to a
// result vector and the rows whose value is TRUE (not NULL, not 0) are appended.  That list is { row : the ternary value of the predicate
// is TRUE } (TernaryAnd / TernaryOr are TRUE exactly where both / one of the operands are), so one kernel evaluates the whole program per
// row -- the statements projection_expression_rows compiles (hy_expression_rows.hpp) -- and compacts the TRUE rows into the chunk's region
// of `matches`.  Nothing goes to HBM but the RowIDs: against hy_projection_expression + hy_table_scan(<> 0) it saves the Int column and
// its null bitmap, written and read again (2 x 4 B + 2 bits per row), one launch and one host preparation.
//
// One workgroup owns one chunk and walks it in rounds of PX_ROWS x 256 rows with a running offset into the chunk's region: positions come
// out ascending and no workgroup ever waits for another.
#include "hy_expression.hpp"

#include <cstring>
#include <vector>

namespace hy {

struct ExprScanArgs {
  const DevSegment* columns[PX_COLUMNS];
  ExprTest tests[PX_TESTS];
  const ExprNode* nodes;        // [n_nodes] in device memory: the node loop reads them with scalar loads
  uint32_t n_nodes, n_columns, n_tests, n_chunks;
  const DevSegment* layout;     // the segments of one column of the program: the chunks' sizes
  const uint64_t* row_base;     // [n_chunks + 1] rows in all chunks before chunk c = where its region begins
  const uint8_t* excluded;      // [n_chunks] != 0: the chunk is not scanned; or nullptr
  hy_row_id* matches;           // chunk regions (HY_SCAN_CHUNK_REGIONS): room for every row
  uint64_t* offsets;            // [n_chunks + 1]
  uint32_t* counts;             // [n_chunks] or nullptr
  uint8_t* chunk_state;         // [n_chunks] or nullptr
};

typedef uint32_t row_id_words __attribute__((ext_vector_type(2)));   // a hy_row_id {chunk_id, chunk_offset} as one 8-byte vector store
constexpr uint32_t XS_ROUND_WORDS = PX_ROWS * (WG_THREADS / 64);   // ballot words of a round: 64 consecutive rows each, in row order

// A round: row (i * 256 + thread) of the round's PX_ROWS * 256 rows is lane (thread % 64) of ballot word i * 4 + wave -- the words in
// index order are the rows in row order.  The words' match counts meet in LDS (the round's only barrier; two buffers, so a wave that is a
// round ahead writes the other one), every lane adds up the counts in front of its words, a matching lane stores its RowID at
//   region + matches of the chunk before this round + matches in the words before + matching lanes below it in its word.
// amdgpu_waves_per_eu(2, 2): the occupancy the kernel has anyway (254 registers without it), stated -- with it the allocator keeps 246 VGPRs and
// leaves no stack object behind (without it: two 4-byte spill slots that no instruction uses, 8 bytes of private segment per lane).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void expression_scan_chunks(ExprScanArgs a) {
  __shared__ uint32_t s_counts[2][XS_ROUND_WORDS];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int B = PX_ROWS;
  const uint32_t chunk = blockIdx.x;
  const uint32_t size = a.layout[chunk].size;
  const uint64_t region = a.row_base[chunk];
  const bool excluded = a.excluded && a.excluded[chunk] != 0;
  if (threadIdx.x == 0) {
    a.offsets[chunk] = region;
    if (a.chunk_state) a.chunk_state[chunk] = excluded ? HY_CHUNK_NONE_MATCH : HY_CHUNK_SCANNED;
    if (chunk + 1 == a.n_chunks) a.offsets[a.n_chunks] = region + size;
  }
  uint32_t emitted = 0;   // matches of the chunk before the current round
  Slice slice;            // (what hy_expression_rows.hpp reads: the chunk)
  slice.chunk = chunk;
  const uint32_t rows = excluded ? 0u : size;
#pragma unroll 1
  for (uint32_t begin = 0; begin < rows; begin += B * 256) {
    uint32_t row[B], valid = 0;
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const uint32_t r = begin + i * 256 + threadIdx.x;
      if (r < rows) valid |= 1u << i;
      row[i] = r < rows ? r : 0;
    }
#include "hy_expression_rows.hpp"
    // ---- TRUE rows -> RowIDs ---------------------------------------------------------------------------------------------------------------
    const uint32_t parity = (begin / (B * 256)) & 1;
    uint32_t hit = 0;   // bit i: row i is TRUE
#pragma unroll
    for (int i = 0; i < B; ++i) {
      if (((valid & ~n[0]) >> i) & 1 && s[0][i] != 0) hit |= 1u << i;
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const uint64_t word = __ballot((hit >> i) & 1);
      if (lane == 0) s_counts[parity][i * 4 + wave] = static_cast<uint32_t>(__popcll(word));
    }
    __syncthreads();
    row_id_words* out = reinterpret_cast<row_id_words*>(a.matches + a.row_base[chunk]);
    const uint64_t below = (1ull << lane) - 1;
    uint32_t running = emitted;
#pragma unroll
    for (int i = 0; i < B; ++i) {
      uint32_t before = running;
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) {
        before = w == wave ? running : before;
        running += s_counts[parity][i * 4 + w];
      }
      const uint64_t word = __ballot((hit >> i) & 1);   // (again: cheaper than four words kept across the barrier)
      // (a match is a row of the chunk: its slot is below the chunk's size, inside the chunk's region)
      if ((hit >> i) & 1) out[before + static_cast<uint32_t>(__popcll(word & below))] = row_id_words{chunk, begin + i * 256 + threadIdx.x};
    }
    emitted = running;
  }
  if (threadIdx.x == 0 && a.counts) a.counts[chunk] = emitted;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_table_scan_expression(const hy_projection_program* program, const uint32_t* excluded_chunks, uint32_t n_excluded, hy_scan_result* result) {
  if (!program || !result) return fail(HY_ERR_INVALID, "hy_table_scan_expression: null argument");
  if (n_excluded && !excluded_chunks) return fail(HY_ERR_INVALID, "hy_table_scan_expression: excluded chunk list missing");
  // ---- the result, as hy_table_scan checks it: before anything is launched -----------------------------------------------------------------
  const bool host_result = result->mem == HY_MEM_HOST;
  if (!result->offsets) return fail(HY_ERR_INVALID, "scan result: offsets array missing");
  if (host_result && (!result->counts || !result->chunk_state)) return fail(HY_ERR_INVALID, "scan result: host results need counts and chunk_state");
  if (!host_result && !(result->flags & HY_SCAN_CHUNK_REGIONS)) return fail(HY_ERR_INVALID, "scan result: device results use the chunk-region layout; set HY_SCAN_CHUNK_REGIONS");
  if (result->capacity && !result->matches) return fail(HY_ERR_INVALID, "scan result: matches buffer missing");
  if (!host_result && (reinterpret_cast<uintptr_t>(result->matches) % 16 != 0 || reinterpret_cast<uintptr_t>(result->offsets) % 8 != 0 || reinterpret_cast<uintptr_t>(result->counts) % 4 != 0))
    return fail(HY_ERR_INVALID, "scan result: a device-memory result needs matches on a 16-byte, offsets on an 8-byte and counts on a 4-byte boundary");

  PreparedProgram prepared;
  HY_TRY(check_program(program, "hy_table_scan_expression", true, &prepared));
  const hy_column* shape = prepared.shape;
  const uint32_t n_chunks = shape->n_chunks;
  if (!host_result && result->capacity < shape->rows) return fail(HY_ERR_CAPACITY, "scan result: chunk regions need capacity >= %llu rows", static_cast<unsigned long long>(shape->rows));
  std::vector<uint8_t> excluded(n_excluded ? n_chunks : 0, 0);
  for (uint32_t i = 0; i < n_excluded; ++i) {
    if (excluded_chunks[i] >= n_chunks) return fail(HY_ERR_INVALID, "excluded chunk id %u out of range", excluded_chunks[i]);
    excluded[excluded_chunks[i]] = 1;
  }
  if (n_excluded) {
    bool reference = false;
    for (uint32_t c = 0; c < prepared.n_distinct; ++c) reference |= prepared.distinct[c]->is_reference;
    for (uint32_t t = 0; t < PX_TESTS; ++t) reference |= prepared.tested[t] && prepared.tested[t]->is_reference;
    if (reference) return fail(HY_ERR_INVALID, "excluded chunks apply to data tables only");
  }

  hipStream_t stream = current_stream();
  Scratch& sc = scratch();
  // Scratch: nodes | excluded flags | (host results) the regions, and the dense copy regions_to_host_result takes behind them -- sized by
  // a dry run of the layout
  ExprNode* d_nodes = nullptr;
  uint8_t* d_excluded = nullptr;
  ScanRegions regions{result->matches, result->offsets, result->counts, result->chunk_state};
  auto layout = [&](Carver& carver) {
    d_nodes = carver.take<ExprNode>(HY_MAX_PROJECTION_NODES);
    d_excluded = n_excluded ? carver.take<uint8_t>(n_chunks) : nullptr;
    if (host_result) scan_regions_layout(carver, n_chunks, shape->rows, regions);
  };
  Carver sizing;
  DenseRegions dense;
  layout(sizing);
  if (host_result) dense_regions_layout(sizing, n_chunks, shape->rows, dense);
  HY_TRY(sc.reserve(sizing.used));
  auto drain = [&](hy_status status) { (void)hipStreamSynchronize(stream); return status; };   // (uploads from this call's host arrays may be queued)
  {
    const hy_status status = prepare_program_tests(&prepared);
    if (status != HY_OK) return drain(status);
  }
  Carver carver{&sc};
  layout(carver);
  if (carver.failed) return drain(fail(HY_ERR_DEVICE, "scratch arena exhausted"));
  hy_row_id* d_matches = regions.matches;
  uint64_t* d_offsets = regions.offsets;
  uint32_t* d_counts = regions.counts;
  uint8_t* d_state = regions.state;
  if (hipMemcpyAsync(d_nodes, prepared.nodes, sizeof(prepared.nodes), hipMemcpyHostToDevice, stream) != hipSuccess ||
      (n_excluded && hipMemcpyAsync(d_excluded, excluded.data(), n_chunks, hipMemcpyHostToDevice, stream) != hipSuccess)) {
    return drain(fail(HY_ERR_DEVICE, "hy_table_scan_expression: upload of the program failed"));
  }

  if (n_chunks == 0) {
    if (hipMemsetAsync(d_offsets, 0, 8, stream) != hipSuccess) return drain(fail(HY_ERR_DEVICE, "hy_table_scan_expression: hipMemsetAsync failed"));
  } else {
    ExprScanArgs a{};
    for (uint32_t c = 0; c < prepared.n_distinct; ++c) a.columns[c] = prepared.distinct[c]->d_segments;
    for (uint32_t t = 0; t < PX_TESTS; ++t) a.tests[t] = prepared.tests[t];   // (a test no node uses: segments == nullptr, not evaluated)
    a.nodes = d_nodes;
    a.n_nodes = program->n_nodes;
    a.n_columns = prepared.n_distinct;
    a.n_tests = program->n_tests;
    a.n_chunks = n_chunks;
    a.layout = shape->d_segments;
    a.row_base = shape->d_row_base;
    a.excluded = d_excluded;
    a.matches = d_matches;
    a.offsets = d_offsets;
    a.counts = d_counts;
    a.chunk_state = d_state;
    profile_begin(stream, HY_KERNEL_SCAN);
    hipLaunchKernelGGL(expression_scan_chunks, dim3(n_chunks), dim3(WG_THREADS), 0, stream, a);
    profile_end(stream);
  }
  if (hipGetLastError() != hipSuccess) return drain(fail(HY_ERR_DEVICE, "hy_table_scan_expression: the scan kernel could not be launched"));

  if (host_result) {
    const hy_status status = regions_to_host_result(d_matches, d_offsets, d_counts, d_state, nullptr, n_chunks, true, result);
    if (status != HY_OK) return drain(status);
  } else {
    // the tests' jobs and the program live in this call's temporaries: the kernel has read them when the call returns
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(HY_ERR_DEVICE, "hy_table_scan_expression: the scan kernel failed");
    result->total_matches = 0;
  }
  return HY_OK;
}

}  // extern "C"

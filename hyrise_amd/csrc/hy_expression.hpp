// hy_expression.hpp -- a hy_projection_program evaluated for PX_ROWS rows per lane: the evaluator's cell rules and ternary logic, written
// once.  projection_expression_rows (projection_expression.hip) writes the value as a column, expression_scan_chunks (scan_expression.hip)
// turns its truth value into PosLists.
#pragma once
#include "hy_device.hpp"
#include "hy_decode.hpp"
#include "hy_arithmetic.hpp"
#include "hy_scan_job.hpp"

namespace hy {

constexpr int PX_DEPTH = HY_MAX_PROJECTION_DEPTH, PX_COLUMNS = HY_MAX_PROJECTION_COLUMNS, PX_TESTS = HY_MAX_PROJECTION_TESTS;
constexpr int PX_ROWS = 4;   // rows a lane evaluates side by side: row (block * PX_ROWS + i) * 256 + thread of the slice

struct ExprNode {     // a node with everything the host resolved: the type it computes in and its operands' types
  uint8_t kind;       // HY_PROJ_*
  uint8_t op;         // HY_ARITH_* | HY_PRED_*
  uint8_t type;       // HY_TYPE_* of the value it pushes
  uint8_t at, bt;     // types of the operands: binary nodes left / right; CASE then / otherwise; UNARY_MINUS at
  uint8_t index;      // COLUMN: distinct column; COLUMN_TEST: test
  uint16_t reserved;
  uint64_t literal;   // LITERAL: the value as the stack holds it
};

struct ExprTest {
  const DevSegment* segments;   // the tested column (data or reference segments)
  const ScanJob* jobs;          // per DATA chunk (prepare_scan_jobs)
  uint32_t null_test;           // 0: a comparison / LIKE / IN; 1: IS NULL; 2: IS NOT NULL
  uint32_t reserved;
};


// A value on the stack: int64 (Int / Long) or the bits of a double (Float widened, Double) -- decode_rows' convention.
__device__ __forceinline__ uint64_t value_bits(const Value& v, uint32_t type) {
  return is_float_type(type) ? static_cast<uint64_t>(__double_as_longlong(v.f)) : static_cast<uint64_t>(v.i);
}

// One cell of a data segment against its chunk's job.  The evaluator's rule, not the scan's: *is_null where the cell is NULL, except for
// the NULL tests themselves.
__device__ __forceinline__ bool test_cell(const DevSegment& s, const ScanJob& job, uint32_t row, uint32_t null_test, bool* is_null) {
  uint32_t vid = 0;
  bool cell_null;
  if (s.encoding == HY_ENC_DICTIONARY) {
    vid = aload_compressed(s.data, s.width, row);
    cell_null = vid >= s.aux_size;
  } else {
    cell_null = s.nulls ? ((s.nulls[row >> 6] >> (row & 63)) & 1) != 0 : false;
  }
  if (null_test) {   // expression_evaluator.cpp:382-402
    *is_null = false;
    return cell_null == (null_test == 1);
  }
  *is_null = cell_null;
  if (cell_null) return false;
  if (job.mode == JOB_ALL) return true;
  if (job.mode == JOB_NONE || (job.flags & JF_NEVER)) return false;
  const bool invert = job.flags & JF_INVERT;
  bool in;
  if (s.encoding == HY_ENC_DICTIONARY) {
    if (job.kind == KIND_VALUE_ID_SET) return ((reinterpret_cast<const uint64_t*>(job.lo)[vid >> 6] >> (vid & 63)) & 1) != 0;
    in = (vid - static_cast<uint32_t>(job.lo)) <= static_cast<uint32_t>(job.span);
  } else if (s.encoding == HY_ENC_FRAME_OF_REFERENCE) {
    const uint32_t x = aload_compressed(s.data, s.width, row) + static_cast<uint32_t>(static_cast<const int32_t*>(s.aux)[row / HY_FOR_BLOCK_SIZE]);
    in = (x - static_cast<uint32_t>(job.lo)) <= static_cast<uint32_t>(job.span);
  } else if (job.kind == KIND_U32) {
    in = (static_cast<const uint32_t*>(s.data)[row] - static_cast<uint32_t>(job.lo)) <= static_cast<uint32_t>(job.span);
  } else if (job.kind == KIND_I64) {
    in = (static_cast<const uint64_t*>(s.data)[row] - job.lo) <= job.span;
  } else if (job.kind == KIND_F32) {
    const float x = static_cast<const float*>(s.data)[row];
    const float lower = __uint_as_float(static_cast<uint32_t>(job.lo)), upper = __uint_as_float(static_cast<uint32_t>(job.span));
    in = ((job.flags & JF_LOWER_INCL) ? x >= lower : x > lower) && ((job.flags & JF_UPPER_INCL) ? x <= upper : x < upper);
  } else {
    const double x = static_cast<const double*>(s.data)[row];
    const double lower = __longlong_as_double(static_cast<long long>(job.lo)), upper = __longlong_as_double(static_cast<long long>(job.span));
    in = ((job.flags & JF_LOWER_INCL) ? x >= lower : x > lower) && ((job.flags & JF_UPPER_INCL) ? x <= upper : x < upper);
  }
  return in != invert;
}

// PX_ROWS rows of a tested column: bit i of *value = the test holds, of *nulls = it is NULL.
__device__ __forceinline__ void test_rows(const ExprTest& t, uint32_t chunk, const uint32_t (&row)[PX_ROWS], uint32_t valid, uint32_t* value, uint32_t* nulls) {
  *value = 0;
  *nulls = 0;
  const DevSegment seg = t.segments[chunk];
  if (seg.encoding != HY_ENC_REFERENCE) {   // (uniform: descriptor and job stay in scalar registers)
    const ScanJob job = t.jobs[chunk];
#pragma unroll
    for (int i = 0; i < PX_ROWS; ++i) {
      if (!((valid >> i) & 1)) continue;
      bool is_null;
      if (test_cell(seg, job, row[i], t.null_test, &is_null)) *value |= 1u << i;
      if (is_null) *nulls |= 1u << i;
    }
    return;
  }
#pragma unroll 1
  for (int i = 0; i < PX_ROWS; ++i) {   // behind a PosList: the RowID's chunk picks the job
    if (!((valid >> i) & 1)) continue;
    uint32_t row_i = row[0];   // (row i selected by comparisons: an index would put the rows into scratch memory)
#pragma unroll
    for (int j = 1; j < PX_ROWS; ++j) row_i = i == j ? row[j] : row_i;
    hy_row_id r;
    if (seg.data) r = static_cast<const hy_row_id*>(seg.data)[row_i];
    else { r.chunk_id = seg.ref_chunk_id; r.chunk_offset = row_i; }
    bool is_null = true, holds = false;
    if (r.chunk_offset == 0xFFFFFFFFu) {   // a NULL RowID is a NULL cell
      if (t.null_test) { is_null = false; holds = t.null_test == 1; }
    } else {
      holds = test_cell(seg.ref[r.chunk_id], t.jobs[r.chunk_id], r.chunk_offset, t.null_test, &is_null);
    }
    if (holds) *value |= 1u << i;
    if (is_null) *nulls |= 1u << i;
  }
}

// PX_ROWS rows of a column as (bits, NULL mask): projection.hip's operand_rows for a column.
__device__ __forceinline__ void column_rows(const DevSegment* segments, uint32_t chunk, const uint32_t (&row)[PX_ROWS], uint32_t valid, uint64_t (&bits)[PX_ROWS], uint32_t* nulls) {
  const uint32_t* pos_words;
  const DevSegment segment = resolve_segment(segments[chunk], &pos_words);
  uint32_t operand_row[PX_ROWS];
#pragma unroll
  for (int i = 0; i < PX_ROWS; ++i) operand_row[i] = row[i];
  const uint32_t null_rows = pos_words ? dereference_rows<PX_ROWS>(pos_words, operand_row) : 0u;
  if (segment.encoding == HY_ENC_REFERENCE) {   // a PosList over several chunks: RowID by RowID -- unrolled here (decode_rows walks these rows
                                                // with an index, which would put the caller's column registers into scratch memory)
    *nulls = 0;
    const bool is_float = is_float_type(segment.data_type);
#pragma unroll
    for (int i = 0; i < PX_ROWS; ++i) {
      bits[i] = 0;
      if (!((valid >> i) & 1)) continue;
      const Value v = column_value(segments, chunk, operand_row[i]);
      if (v.is_null) *nulls |= 1u << i;
      else bits[i] = is_float ? static_cast<uint64_t>(__double_as_longlong(v.f)) : static_cast<uint64_t>(v.i);
    }
  } else {
    decode_rows<PX_ROWS>(segment, segments, chunk, operand_row, valid, bits, nulls);
  }
  *nulls |= null_rows;
}

// ---- host side (projection_expression.hip): a hy_projection_program as the kernels take it --------------------------------------------
struct PreparedProgram {
  ExprNode nodes[HY_MAX_PROJECTION_NODES];
  const hy_column* distinct[PX_COLUMNS] = {};   // the decoded twins (plain_column) of the columns the program reads, each once
  uint32_t n_distinct = 0;
  uint32_t result_type = HY_TYPE_NULL;
  const hy_column* shape = nullptr;             // a column of the program: the chunk layout all of them share
  const hy_column* tested[PX_TESTS] = {};       // per test that a node uses: its column, the data column behind it, its predicate
  const hy_column* tested_data[PX_TESTS] = {};
  hy_predicate predicates[PX_TESTS];
  std::vector<uint64_t> list_words[PX_TESTS], list_offsets[PX_TESTS];   // (an IN list's bitmaps: what its predicate points to)
  ExprTest tests[PX_TESTS] = {};                // prepare_program_tests: what the kernel reads
  DeviceBuffer temporary;                       // ... and the jobs it points to
};
hy_status check_program(const hy_projection_program* program, const char* entry, bool scan, PreparedProgram* prepared);
hy_status prepare_program_tests(PreparedProgram* prepared);

}  // namespace hy

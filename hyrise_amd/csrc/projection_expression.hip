// projection_expression.hip -- a Projection's whole expression tree per output column, in one pass.
//
// What it replaces (reference, CPU):
//   Projection::_on_execute -> ExpressionEvaluator::evaluate_expression_to_segment     operators/projection.cpp
//   _evaluate_arithmetic / _predicate / _logical / _case / _is_null / _unary_minus      expression/evaluation/expression_evaluator.cpp
//   the cell functors                                                                   expression/evaluation/expression_functors.hpp
//
// The reference materialises one ExpressionResult vector per node of the tree; hy_projection_arithmetic (projection.hip) one device
// column per arithmetic node.  Here one kernel evaluates a postfix program -- arithmetic, comparisons, AND / OR, IS NULL, unary minus,
// CASE WHEN, and a column tested against a scan's predicate -- for every row and writes ONE column: the program's distinct columns are
// decoded once per row (the loads of all of them in flight together), the operand stack lives in registers with static indices (push
// and pop move the slots), the node loop is uniform across the wave.  HBM-bound on data tables: bytes in (the distinct columns'
// widths) + bytes out (the result's width) per row, no intermediate column.
#include "hy_device.hpp"
#include "hy_decode.hpp"
#include "hy_arithmetic.hpp"
#include "hy_scan_job.hpp"

#include <cstring>
#include <vector>

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

struct ExprArgs {
  const DevSegment* columns[PX_COLUMNS];
  ExprTest tests[PX_TESTS];
  const ExprNode* nodes;        // [n_nodes] in device memory: the node loop reads them with scalar loads
  uint32_t n_nodes, n_columns, n_tests, result_type;
  const Slice* slices;
  void* values;                 // result values, chunk c at value_base[c] (projection.hip's layout)
  const uint64_t* value_base;
  uint64_t* nulls;
  const uint64_t* null_base;
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

// One workgroup per 8192-row slice; a thread owns rows k * 256 + tid, PX_ROWS of them at a time.  Row r of a wave's round lands in bit
// (r % 64) of one bitmap word: a null word is one ballot.  Values are written a lane per row: consecutive lanes, consecutive cells.
__global__ __launch_bounds__(256) void projection_expression_rows(ExprArgs a) {
  // projection_rows' mapping: of every 64 consecutive slices XCD x takes eight consecutive ones -- one chunk -- so that a chunk's dictionary
  // and the segments a PosList points into are fetched into ONE L2.
  uint32_t slice_index = blockIdx.x;
  if ((blockIdx.x | 63u) < gridDim.x) slice_index = (blockIdx.x & ~63u) | ((blockIdx.x & 7u) << 3) | ((blockIdx.x >> 3) & 7u);
  const Slice slice = a.slices[slice_index];
  const uint32_t lane = threadIdx.x & 63;
  char* values = static_cast<char*>(a.values) + a.value_base[slice.chunk];
  uint64_t* null_words = a.nulls + a.null_base[slice.chunk];
  const uint32_t rt = a.result_type;
  constexpr int B = PX_ROWS;
#pragma unroll 1
  for (uint32_t block = 0; block < SLICE_ROWS / 256 / B; ++block) {
    if (block * B * 256 >= ((slice.row_count + 63) & ~63u)) break;
    uint32_t row[B], valid = 0;
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const uint32_t r = (block * B + i) * 256 + threadIdx.x;
      if (r < slice.row_count) valid |= 1u << i;
      row[i] = slice.row_begin + (r < slice.row_count ? r : 0);
    }
    // ---- every distinct column once, every test once ----------------------------------------------------------------------------
    uint64_t column[PX_COLUMNS][B];
    uint32_t column_nulls[PX_COLUMNS], test_value[PX_TESTS], test_nulls[PX_TESTS];
#pragma unroll
    for (int c = 0; c < PX_COLUMNS; ++c) {
      column_nulls[c] = 0;
#pragma unroll
      for (int i = 0; i < B; ++i) column[c][i] = 0;
      if (static_cast<uint32_t>(c) < a.n_columns) column_rows(a.columns[c], slice.chunk, row, valid, column[c], &column_nulls[c]);
    }
#pragma unroll
    for (int t = 0; t < PX_TESTS; ++t) {
      test_value[t] = test_nulls[t] = 0;
      if (static_cast<uint32_t>(t) < a.n_tests && a.tests[t].segments) test_rows(a.tests[t], slice.chunk, row, valid, &test_value[t], &test_nulls[t]);
    }
    // ---- the program: slot 0 = top of the stack ------------------------------------------------------------------------------------
    uint64_t s[PX_DEPTH][B];
    uint32_t n[PX_DEPTH];
#pragma unroll
    for (int d = 0; d < PX_DEPTH; ++d) {
      n[d] = 0;
#pragma unroll
      for (int i = 0; i < B; ++i) s[d][i] = 0;
    }
#pragma unroll 1
    for (uint32_t k = 0; k < a.n_nodes; ++k) {
      const ExprNode node = a.nodes[k];
      const uint32_t kind = node.kind, op = node.op, type = node.type, at = node.at, bt = node.bt;
      if (kind == HY_PROJ_COLUMN || kind == HY_PROJ_LITERAL || kind == HY_PROJ_COLUMN_TEST) {   // push
#pragma unroll
        for (int d = PX_DEPTH - 1; d > 0; --d) {
          n[d] = n[d - 1];
#pragma unroll
          for (int i = 0; i < B; ++i) s[d][i] = s[d - 1][i];
        }
        if (kind == HY_PROJ_COLUMN) {
#pragma unroll
          for (int c = 0; c < PX_COLUMNS; ++c) {
            if (node.index != c) continue;
#pragma unroll
            for (int i = 0; i < B; ++i) s[0][i] = column[c][i];
            n[0] = column_nulls[c];
          }
        } else if (kind == HY_PROJ_LITERAL) {
#pragma unroll
          for (int i = 0; i < B; ++i) s[0][i] = node.literal;
          n[0] = type == HY_TYPE_NULL ? 0xFFFFFFFFu : 0u;
        } else {
#pragma unroll
          for (int t = 0; t < PX_TESTS; ++t) {
            if (node.index != t) continue;
#pragma unroll
            for (int i = 0; i < B; ++i) s[0][i] = (test_value[t] >> i) & 1u;
            n[0] = test_nulls[t];
          }
        }
        continue;
      }
      if (kind == HY_PROJ_IS_NULL || kind == HY_PROJ_IS_NOT_NULL) {   // expression_evaluator.cpp:382-402: never NULL
        const uint32_t is = kind == HY_PROJ_IS_NULL ? n[0] : ~n[0];
#pragma unroll
        for (int i = 0; i < B; ++i) s[0][i] = (is >> i) & 1u;
        n[0] = 0;
        continue;
      }
      if (kind == HY_PROJ_UNARY_MINUS) {   // :965-988; the NULL flags stay
#pragma unroll
        for (int i = 0; i < B; ++i) {
          if (is_float_type(type)) s[0][i] ^= 0x8000000000000000ull;
          else if (type == HY_TYPE_INT) s[0][i] = static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(0u - static_cast<uint32_t>(s[0][i]))));
          else s[0][i] = 0ull - s[0][i];
        }
        continue;
      }
      if (kind == HY_PROJ_CASE) {   // :726-759 -- when = slot 2, then = slot 1, otherwise = slot 0
        uint32_t nulls = 0;
#pragma unroll
        for (int i = 0; i < B; ++i) {
          const bool take = !((n[2] >> i) & 1) && s[2][i] != 0;
          const Value chosen = take ? convert(as_value(s[1][i], at), at, type) : convert(as_value(s[0][i], bt), bt, type);
          const bool is_null = ((take ? n[1] : n[0]) >> i) & 1;
          s[0][i] = is_null ? 0 : value_bits(chosen, type);
          if (is_null) nulls |= 1u << i;
        }
        n[0] = nulls;
#pragma unroll
        for (int d = 1; d + 2 < PX_DEPTH; ++d) {
          n[d] = n[d + 2];
#pragma unroll
          for (int i = 0; i < B; ++i) s[d][i] = s[d + 2][i];
        }
        continue;
      }
      // ---- binary nodes: slot 1 <op> slot 0 -> slot 0, the slots below move up -------------------------------------------------------
      uint32_t nulls = n[1] | n[0];
      if (kind == HY_PROJ_ARITHMETIC) {
        if (op <= HY_ARITH_MUL) {
#pragma unroll
          for (int i = 0; i < B; ++i) {
            Value result{false, 0, 0.0};
            if (((valid & ~nulls) >> i) & 1) arithmetic_cell(op, at, bt, type, as_value(s[1][i], at), as_value(s[0][i], bt), &result);
            s[0][i] = value_bits(result, type);
          }
        } else {   // / and %: long instruction sequences -- one instance, the rows one after the other, row i selected by comparisons
                   // (an index would put the stack into scratch memory)
#pragma unroll 1
          for (int i = 0; i < B; ++i) {
            uint64_t x = s[1][0], y = s[0][0];
#pragma unroll
            for (int j = 1; j < B; ++j) { x = i == j ? s[1][j] : x; y = i == j ? s[0][j] : y; }
            Value result{false, 0, 0.0};
            bool is_null = true;
            if (((valid & ~nulls) >> i) & 1) is_null = arithmetic_cell(op, at, bt, type, as_value(x, at), as_value(y, bt), &result);   // NULL: division / modulo by zero
            if (is_null) nulls |= 1u << i;
            const uint64_t bits = is_null ? 0 : value_bits(result, type);
#pragma unroll
            for (int j = 0; j < B; ++j) s[0][j] = i == j ? bits : s[0][j];
          }
        }
      } else if (kind == HY_PROJ_COMPARISON) {   // expression_functors.hpp:90-116; > and >= are the swapped < and <= (expression_evaluator.cpp:73-90)
        const bool swapped = op == HY_PRED_GREATER_THAN || op == HY_PRED_GREATER_THAN_EQUALS;
        const uint32_t condition = op == HY_PRED_GREATER_THAN ? HY_PRED_LESS_THAN : op == HY_PRED_GREATER_THAN_EQUALS ? HY_PRED_LESS_THAN_EQUALS : op;
#pragma unroll
        for (int i = 0; i < B; ++i) {
          const Value x = as_value(s[1][i], at), y = as_value(s[0][i], bt);
          const bool holds = swapped ? compare_typed(condition, y, bt, x, at) : compare_typed(condition, x, at, y, bt);
          s[0][i] = (holds && !((nulls >> i) & 1)) ? 1u : 0u;
        }
      } else {   // AND / OR: expression_functors.hpp:41-84
        uint32_t a_true = 0, b_true = 0;
#pragma unroll
        for (int i = 0; i < B; ++i) {
          if (s[1][i] != 0) a_true |= 1u << i;
          if (s[0][i] != 0) b_true |= 1u << i;
        }
        a_true &= ~n[1];
        b_true &= ~n[0];
        uint32_t holds;
        if (kind == HY_PROJ_AND) {
          holds = a_true & b_true;
          nulls = (n[1] & n[0]) | (a_true & n[0]) | (b_true & n[1]);
        } else {
          holds = a_true | b_true;
          nulls = (n[1] | n[0]) & ~holds;
        }
#pragma unroll
        for (int i = 0; i < B; ++i) s[0][i] = (holds >> i) & 1u;
      }
      n[0] = nulls;
#pragma unroll
      for (int d = 1; d + 1 < PX_DEPTH; ++d) {
        n[d] = n[d + 1];
#pragma unroll
        for (int i = 0; i < B; ++i) s[d][i] = s[d + 1][i];
      }
    }
    // ---- the result: a lane per cell, a ballot per null word ---------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const bool in = (valid >> i) & 1;
      const bool is_null = (n[0] >> i) & 1;
      const uint64_t bits = is_null ? 0 : s[0][i];   // NULL cells hold T{} (value_segment.hpp)
      if (in) {
        switch (rt) {
          case HY_TYPE_INT: reinterpret_cast<int32_t*>(values)[row[i]] = static_cast<int32_t>(static_cast<int64_t>(bits)); break;
          case HY_TYPE_LONG: reinterpret_cast<uint64_t*>(values)[row[i]] = bits; break;
          case HY_TYPE_FLOAT: reinterpret_cast<float*>(values)[row[i]] = static_cast<float>(__longlong_as_double(static_cast<long long>(bits))); break;
          default: reinterpret_cast<uint64_t*>(values)[row[i]] = bits; break;
        }
      }
      const uint32_t r = (block * B + i) * 256 + threadIdx.x;
      const uint64_t null_lanes = __ballot(in && is_null);   // slices start at multiples of 8192: 64 consecutive rows = one word
      if (lane == 0 && r < ((slice.row_count + 63) & ~63u)) null_words[(slice.row_begin + r) >> 6] = null_lanes;
    }
  }
}

static bool px_numeric(uint32_t t) { return t >= HY_TYPE_INT && t <= HY_TYPE_DOUBLE; }

static uint64_t literal_bits(uint32_t type, const hy_value& v) {
  double d = 0.0;
  switch (type) {
    case HY_TYPE_INT: return static_cast<uint64_t>(static_cast<int64_t>(v.i32));
    case HY_TYPE_LONG: return static_cast<uint64_t>(v.i64);
    case HY_TYPE_FLOAT: d = static_cast<double>(v.f32); break;
    case HY_TYPE_DOUBLE: d = v.f64; break;
    default: return 0;
  }
  uint64_t bits;
  std::memcpy(&bits, &d, 8);
  return bits;
}

// column IN (...) over a dictionary string column as the value-id bitmaps a LIKE predicate carries (bit v of data chunk c: value id v is
// one of the elements -- or, NOT IN, is none of them): the same KIND_VALUE_ID_SET jobs, the NULL value id matches neither.
static hy_status in_list_as_bitmaps(const hy_column* data_column, const hy_in_list* list, std::vector<uint64_t>* words, std::vector<uint64_t>* offsets, hy_predicate* predicate) {
  if (list->n_values == 0) return fail(HY_ERR_INVALID, "hy_projection_expression: an empty IN list has a constant result; the caller answers it");
  if (list->n_values > HY_MAX_IN_LIST) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: %u IN elements, at most %u are evaluated here", list->n_values, HY_MAX_IN_LIST);
  if (list->negated > 1) return fail(HY_ERR_INVALID, "hy_projection_expression: hy_in_list.negated is 0 or 1");
  if (list->value_type != HY_TYPE_STRING || data_column->data_type != HY_TYPE_STRING)
    return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: an IN list is tested over dictionary string columns (numeric lists: OR of comparisons)");
  if (!list->per_chunk_value_ids) return fail(HY_ERR_INVALID, "string column IN list needs per-chunk value ids (hy_in_list.per_chunk_value_ids)");
  offsets->assign(size_t{data_column->n_chunks} + 1, 0);
  for (uint32_t c = 0; c < data_column->n_chunks; ++c) (*offsets)[c + 1] = (*offsets)[c] + (uint64_t{data_column->host_segments[c].aux_size} + 63) / 64;
  words->assign(offsets->back() ? offsets->back() : 1, 0);
  for (uint32_t c = 0; c < data_column->n_chunks; ++c) {
    const uint32_t d = data_column->host_segments[c].aux_size;
    uint64_t* chunk_words = words->data() + (*offsets)[c];
    for (uint32_t i = 0; i < list->n_values; ++i) {
      const uint32_t vid = list->per_chunk_value_ids[size_t{c} * list->n_values + i];
      if (vid < d) chunk_words[vid >> 6] |= 1ull << (vid & 63);
    }
    if (list->negated) {
      for (uint32_t v = 0; v < d; v += 64) chunk_words[v >> 6] = ~chunk_words[v >> 6] & (d - v >= 64 ? ~0ull : (1ull << (d - v)) - 1);
    }
  }
  std::memset(predicate, 0, sizeof(*predicate));
  predicate->condition = HY_PRED_LIKE;   // (the matcher's bitmaps: what is set matches)
  predicate->value_type = HY_TYPE_STRING;
  predicate->column_is_nullable = list->column_is_nullable;
  predicate->match_words = words->data();
  predicate->match_word_offsets = offsets->data();
  return HY_OK;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_projection_expression(const hy_projection_program* program, hy_column** out) {
  if (!program || !out) return fail(HY_ERR_INVALID, "hy_projection_expression: null argument");
  *out = nullptr;
  if (program->n_nodes == 0) return fail(HY_ERR_INVALID, "hy_projection_expression: an empty program");
  if (program->n_nodes > HY_MAX_PROJECTION_NODES) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: %u nodes, at most %u are evaluated here", program->n_nodes, HY_MAX_PROJECTION_NODES);
  if (program->n_columns > HY_MAX_PROJECTION_COLUMNS) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: %u columns, at most %u", program->n_columns, HY_MAX_PROJECTION_COLUMNS);
  if (program->n_tests > HY_MAX_PROJECTION_TESTS) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: %u column tests, at most %u", program->n_tests, HY_MAX_PROJECTION_TESTS);

  // ---- the program, checked: a stack of types (operand types are resolved here, the kernel's nodes carry them) ------------------------
  ExprArgs a{};
  ExprNode nodes[HY_MAX_PROJECTION_NODES];
  std::memset(nodes, 0, sizeof(nodes));
  const hy_column* distinct[PX_COLUMNS] = {};   // the decoded twins (plain_column) of the columns the program reads, each once
  uint32_t n_distinct = 0;
  const hy_column* shape = nullptr;
  uint32_t stack[PX_DEPTH];
  uint32_t depth = 0;
  bool test_used[PX_TESTS] = {};
  for (uint32_t k = 0; k < program->n_nodes; ++k) {
    const hy_projection_node& in = program->nodes[k];
    ExprNode& node = nodes[k];
    if (in.kind >= HY_PROJ_BETWEEN && in.kind <= HY_PROJ_PARAMETER) {
      static const char* const names[] = {"Between", "Cast", "Extract", "function", "subquery", "parameter"};
      return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: %s expressions are not evaluated on the device", names[in.kind - HY_PROJ_BETWEEN]);
    }
    if (in.kind > HY_PROJ_PARAMETER) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u has unknown kind %u", k, in.kind);
    node.kind = static_cast<uint8_t>(in.kind);
    const bool pushes = in.kind == HY_PROJ_COLUMN || in.kind == HY_PROJ_LITERAL || in.kind == HY_PROJ_COLUMN_TEST;
    const uint32_t operands = pushes ? 0 : in.kind == HY_PROJ_CASE ? 3 : (in.kind == HY_PROJ_IS_NULL || in.kind == HY_PROJ_IS_NOT_NULL || in.kind == HY_PROJ_UNARY_MINUS) ? 1 : 2;
    if (depth < operands) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u pops %u operands, the stack holds %u", k, operands, depth);
    if (pushes && depth == PX_DEPTH) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: the program needs more than %u stack entries", PX_DEPTH);
    uint32_t type = HY_TYPE_INT;
    switch (in.kind) {
      case HY_PROJ_COLUMN: {
        if (in.index >= program->n_columns || !program->columns[in.index]) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u names column %u", k, in.index);
        const hy_column* column = program->columns[in.index];
        HY_TRY(on_this_device(column, "hy_projection_expression"));
        if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_UNSUPPORTED, "MVCC columns are read by hy_validate only");
        if (!px_numeric(column->data_type)) return fail(HY_ERR_UNSUPPORTED, "string expressions stay on the CPU path (a string column is read by a column test only)");
        HY_TRY(plain_column(column, &column));
        uint32_t c = 0;
        while (c < n_distinct && distinct[c] != column) ++c;
        if (c == n_distinct) distinct[n_distinct++] = column;
        if (!shape) shape = column;
        node.index = static_cast<uint8_t>(c);
        type = column->data_type;
        break;
      }
      case HY_PROJ_LITERAL:
        if (in.literal_type == HY_TYPE_STRING) return fail(HY_ERR_UNSUPPORTED, "string expressions stay on the CPU path");
        if (in.literal_type > HY_TYPE_DOUBLE) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u has literal type %u", k, in.literal_type);
        type = in.literal_type;
        node.literal = literal_bits(type, in.literal);
        break;
      case HY_PROJ_COLUMN_TEST:
        if (in.index >= program->n_tests || !program->tests[in.index].column) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u names column test %u", k, in.index);
        test_used[in.index] = true;
        node.index = static_cast<uint8_t>(in.index);
        break;
      case HY_PROJ_ARITHMETIC:
        if (in.op > HY_ARITH_MOD) return fail(HY_ERR_INVALID, "unknown arithmetic operator %u", in.op);
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        if (node.at == HY_TYPE_NULL && node.bt == HY_TYPE_NULL) return fail(HY_ERR_INVALID, "Cannot deduce common type if both sides are NULL.");
        type = expression_common_type(node.at, node.bt);
        break;
      case HY_PROJ_COMPARISON:
        if (in.op >= HY_PRED_BETWEEN_INCLUSIVE && in.op <= HY_PRED_BETWEEN_EXCLUSIVE) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: Between expressions are not evaluated on the device");
        if (in.op > HY_PRED_GREATER_THAN_EQUALS) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u compares with condition %u", k, in.op);
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        break;
      case HY_PROJ_AND:
      case HY_PROJ_OR:
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        for (uint32_t t : {uint32_t{node.at}, uint32_t{node.bt}}) {
          if (t != HY_TYPE_INT && t != HY_TYPE_NULL) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u: AND / OR take Int operands (a predicate's result)", k);
        }
        break;
      case HY_PROJ_UNARY_MINUS:
        node.at = static_cast<uint8_t>(stack[depth - 1]);
        if (!px_numeric(node.at)) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u negates a NULL literal", k);
        type = node.at;
        break;
      case HY_PROJ_CASE:
        if (stack[depth - 3] != HY_TYPE_INT && stack[depth - 3] != HY_TYPE_NULL) return fail(HY_ERR_INVALID, "hy_projection_expression: node %u: CASE takes an Int `when` (a predicate's result)", k);
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        if (node.at == HY_TYPE_NULL && node.bt == HY_TYPE_NULL) return fail(HY_ERR_INVALID, "Cannot deduce common type if both sides are NULL.");
        type = expression_common_type(node.at, node.bt);
        break;
      default: break;   // IS_NULL / IS_NOT_NULL: Int
    }
    node.op = static_cast<uint8_t>(in.op);
    node.type = static_cast<uint8_t>(type);
    depth = depth - operands + 1;
    stack[depth - 1] = type;
  }
  if (depth != 1) return fail(HY_ERR_INVALID, "hy_projection_expression: the program leaves %u values, not one", depth);
  const uint32_t result_type = stack[0];
  if (!px_numeric(result_type)) return fail(HY_ERR_INVALID, "hy_projection_expression: the result's type cannot be deduced (a NULL literal)");

  // ---- the tests' columns -----------------------------------------------------------------------------------------------------------
  const hy_column* tested[PX_TESTS] = {};
  const hy_column* tested_data[PX_TESTS] = {};
  hy_predicate predicates[PX_TESTS];
  std::vector<uint64_t> list_words[PX_TESTS], list_offsets[PX_TESTS];
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (!test_used[t]) continue;
    const hy_projection_test& test = program->tests[t];
    const hy_column* column = test.column;
    HY_TRY(on_this_device(column, "hy_projection_expression"));
    if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_UNSUPPORTED, "MVCC columns are read by hy_validate only");
    HY_TRY(plain_column(column, &column));
    const hy_column* data_column = column->is_reference ? column->ref : column;
    if (!data_column) return fail(HY_ERR_INVALID, "hy_projection_expression: column test %u over a reference column without a referenced column", t);
    HY_TRY(plain_column(data_column, &data_column));
    if (column->data_type == HY_TYPE_STRING) {
      for (uint32_t c = 0; c < data_column->n_chunks; ++c) {
        if (data_column->host_segments[c].encoding != HY_ENC_DICTIONARY) return fail(HY_ERR_UNSUPPORTED, "column tests on unencoded string segments stay on the CPU path");
      }
    } else if (!px_numeric(column->data_type)) {
      return fail(HY_ERR_INVALID, "hy_projection_expression: column test %u over a column of type %u", t, column->data_type);
    }
    if (test.in_list) {
      HY_TRY(in_list_as_bitmaps(data_column, test.in_list, &list_words[t], &list_offsets[t], &predicates[t]));
    } else {
      predicates[t] = test.predicate;
      const uint32_t condition = predicates[t].condition;
      if (condition >= HY_PRED_BETWEEN_INCLUSIVE && condition <= HY_PRED_BETWEEN_EXCLUSIVE) return fail(HY_ERR_UNSUPPORTED, "hy_projection_expression: Between expressions are not evaluated on the device");
      if (condition == HY_PRED_IN || condition == HY_PRED_NOT_IN) return fail(HY_ERR_INVALID, "hy_projection_expression: an IN list is passed as hy_projection_test.in_list");
    }
    tested[t] = column;
    tested_data[t] = data_column;
    if (!shape) shape = column;
  }
  if (!shape) return fail(HY_ERR_INVALID, "hy_projection_expression: at least one operand must be a column");
  auto same_layout = [&](const hy_column* column) -> hy_status {
    if (column->n_chunks != shape->n_chunks) return fail(HY_ERR_INVALID, "operand columns do not belong to one table (chunk counts differ)");
    for (uint32_t c = 0; c < shape->n_chunks; ++c) {
      if (column->host_segments[c].size != shape->host_segments[c].size) return fail(HY_ERR_INVALID, "operand columns do not belong to one table (chunk %u)", c);
    }
    return HY_OK;
  };
  for (uint32_t c = 0; c < n_distinct; ++c) HY_TRY(same_layout(distinct[c]));
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (tested[t]) HY_TRY(same_layout(tested[t]));
  }

  const uint32_t width = (result_type == HY_TYPE_INT || result_type == HY_TYPE_FLOAT) ? 4 : 8;
  hipStream_t stream = current_stream();

  // ---- the tests' per-chunk jobs, in a block that lives until the kernel has run ----------------------------------------------------------
  size_t jobs_at[PX_TESTS + 1] = {}, staging_at[PX_TESTS + 1] = {};
  size_t temporary_bytes = 0;
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (!tested[t]) continue;
    jobs_at[t] = temporary_bytes;
    temporary_bytes += align_up(sizeof(ScanJob) * (size_t{tested_data[t]->n_chunks} + 1), 256);
    staging_at[t] = temporary_bytes;
    temporary_bytes += align_up(scan_jobs_staging_bytes(tested_data[t], &predicates[t]) + 256, 256);
  }
  DeviceBuffer temporary;
  if (temporary_bytes) HY_TRY(temporary.alloc(temporary_bytes));
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (!tested[t]) continue;
    ScanJob* jobs = reinterpret_cast<ScanJob*>(temporary.as<char>() + jobs_at[t]);
    const hy_status status = prepare_scan_jobs(tested_data[t], &predicates[t], jobs, temporary.as<char>() + staging_at[t]);
    if (status != HY_OK) {
      (void)hipStreamSynchronize(stream);   // (uploads from this call's host arrays may be queued)
      return status;
    }
    const uint32_t condition = predicates[t].condition;
    a.tests[t] = ExprTest{tested[t]->d_segments, jobs, condition == HY_PRED_IS_NULL ? 1u : condition == HY_PRED_IS_NOT_NULL ? 2u : 0u, 0};
  }

  // ---- result buffers: hy_projection_arithmetic's layout -- one allocation, chunk c's values at value_base[c] (256-byte aligned), then all bitmaps
  const uint32_t n_chunks = shape->n_chunks;
  std::vector<uint64_t> value_base(n_chunks + 1, 0), null_base(n_chunks + 1, 0);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint64_t rows = shape->host_segments[c].size;
    value_base[c + 1] = value_base[c] + ((rows * width + 16 + 255) & ~uint64_t{255});
    null_base[c + 1] = null_base[c] + ((rows + 63) / 64 + 31) / 32 * 32;
  }
  const uint64_t values_bytes = value_base[n_chunks], null_words = null_base[n_chunks];
  const uint64_t tables_bytes = 16 * (uint64_t{n_chunks} + 1) + sizeof(nodes);
  char* arena = nullptr;
  size_t arena_capacity = 0;
  auto drain = [&](hy_status status) { (void)hipStreamSynchronize(stream); return status; };
  const hy_status acquired = pool_acquire(values_bytes + 8 * null_words + tables_bytes + 256, reinterpret_cast<void**>(&arena), &arena_capacity);
  if (acquired != HY_OK) return drain(acquired);
  uint64_t* d_nulls = reinterpret_cast<uint64_t*>(arena + values_bytes);
  uint64_t* d_value_base = reinterpret_cast<uint64_t*>(arena + values_bytes + 8 * null_words);
  uint64_t* d_null_base = d_value_base + n_chunks + 1;
  auto release = [&](hy_status status) { (void)hipStreamSynchronize(stream); pool_release(arena, arena_capacity); return status; };
  if (hipMemcpyAsync(d_value_base, value_base.data(), 8 * (size_t{n_chunks} + 1), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(d_null_base, null_base.data(), 8 * (size_t{n_chunks} + 1), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(d_null_base + n_chunks + 1, nodes, sizeof(nodes), hipMemcpyHostToDevice, stream) != hipSuccess) {
    return release(fail(HY_ERR_DEVICE, "projection: upload of the chunk tables failed"));
  }
  for (uint32_t c = 0; c < n_distinct; ++c) a.columns[c] = distinct[c]->d_segments;
  a.nodes = reinterpret_cast<const ExprNode*>(d_null_base + n_chunks + 1);
  a.n_nodes = program->n_nodes;
  a.n_columns = n_distinct;
  a.n_tests = program->n_tests;
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (!tested[t]) a.tests[t] = ExprTest{nullptr, nullptr, 0, 0};
  }
  a.result_type = result_type;
  a.slices = shape->d_slices;
  a.values = arena;
  a.value_base = d_value_base;
  a.nulls = d_nulls;
  a.null_base = d_null_base;
  if (shape->n_slices && shape->rows) {
    profile_begin(stream, HY_KERNEL_PROJECTION);
    hipLaunchKernelGGL(projection_expression_rows, dim3(shape->n_slices), dim3(256), 0, stream, a);
    profile_end(stream);
  }
  if (hipStreamSynchronize(stream) != hipSuccess || hipGetLastError() != hipSuccess) return release(fail(HY_ERR_DEVICE, "projection expression kernel failed"));

  // the result as a column over the device buffers (HY_MEM_DEVICE: nothing is copied), which then owns them
  std::vector<hy_segment> segments(n_chunks ? n_chunks : 1);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    hy_segment& s = segments[c];
    std::memset(&s, 0, sizeof(s));
    s.encoding = HY_ENC_UNENCODED;
    s.data_type = result_type;
    s.size = shape->host_segments[c].size;
    s.width = width;
    s.data = arena + value_base[c];
    s.nulls = d_nulls + null_base[c];
    s.ref_chunk_id = 0xFFFFFFFFu;
  }
  hy_column* column = nullptr;
  const hy_status status = hy_column_create(segments.data(), n_chunks, HY_MEM_DEVICE, &column);
  if (status != HY_OK) return release(status);
  column->pooled.emplace_back(arena_capacity, arena);
  *out = column;
  return HY_OK;
}

}  // extern "C"

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
#include "hy_expression.hpp"

#include <cstring>
#include <vector>

namespace hy {

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
#include "hy_expression_rows.hpp"
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

// The program, checked on the host -- nothing is launched: the kernel's nodes (operand types resolved), the distinct columns, the tests'
// predicates.  `scan`: the program is a TableScan's predicate (hy_table_scan_expression).
hy_status check_program(const hy_projection_program* program, const char* entry, bool scan, PreparedProgram* p) {
  if (program->n_nodes == 0) return fail(HY_ERR_INVALID, "%s: an empty program", entry);
  if (program->n_nodes > HY_MAX_PROJECTION_NODES) return fail(HY_ERR_UNSUPPORTED, "%s: %u nodes, at most %u are evaluated here", entry, program->n_nodes, HY_MAX_PROJECTION_NODES);
  if (program->n_columns > HY_MAX_PROJECTION_COLUMNS) return fail(HY_ERR_UNSUPPORTED, "%s: %u columns, at most %u", entry, program->n_columns, HY_MAX_PROJECTION_COLUMNS);
  if (program->n_tests > HY_MAX_PROJECTION_TESTS) return fail(HY_ERR_UNSUPPORTED, "%s: %u column tests, at most %u", entry, program->n_tests, HY_MAX_PROJECTION_TESTS);

  // ---- the program, checked: a stack of types (operand types are resolved here, the kernel's nodes carry them) ------------------------
  ExprNode (&nodes)[HY_MAX_PROJECTION_NODES] = p->nodes;
  std::memset(nodes, 0, sizeof(nodes));
  const hy_column* (&distinct)[PX_COLUMNS] = p->distinct;   // the decoded twins (plain_column) of the columns the program reads, each once
  uint32_t& n_distinct = p->n_distinct;
  const hy_column*& shape = p->shape;
  uint32_t first[HY_MAX_PROJECTION_NODES];   // where node k's subtree begins (its operands are what lies between)
  uint32_t begins[PX_DEPTH];
  uint32_t stack[PX_DEPTH];
  uint32_t depth = 0;
  bool test_used[PX_TESTS] = {};
  for (uint32_t k = 0; k < program->n_nodes; ++k) {
    const hy_projection_node& in = program->nodes[k];
    ExprNode& node = nodes[k];
    if (in.kind >= HY_PROJ_BETWEEN && in.kind <= HY_PROJ_PARAMETER) {
      static const char* const names[] = {"Between", "Cast", "Extract", "function", "subquery", "parameter"};
      return fail(HY_ERR_UNSUPPORTED, "%s: %s expressions are not evaluated on the device", entry, names[in.kind - HY_PROJ_BETWEEN]);
    }
    if (in.kind > HY_PROJ_PARAMETER) return fail(HY_ERR_INVALID, "%s: node %u has unknown kind %u", entry, k, in.kind);
    node.kind = static_cast<uint8_t>(in.kind);
    const bool pushes = in.kind == HY_PROJ_COLUMN || in.kind == HY_PROJ_LITERAL || in.kind == HY_PROJ_COLUMN_TEST;
    const uint32_t operands = pushes ? 0 : in.kind == HY_PROJ_CASE ? 3 : (in.kind == HY_PROJ_IS_NULL || in.kind == HY_PROJ_IS_NOT_NULL || in.kind == HY_PROJ_UNARY_MINUS) ? 1 : 2;
    if (depth < operands) return fail(HY_ERR_INVALID, "%s: node %u pops %u operands, the stack holds %u", entry, k, operands, depth);
    if (pushes && depth == PX_DEPTH) return fail(HY_ERR_UNSUPPORTED, "%s: the program needs more than %u stack entries", entry, PX_DEPTH);
    uint32_t type = HY_TYPE_INT;
    switch (in.kind) {
      case HY_PROJ_COLUMN: {
        if (in.index >= program->n_columns || !program->columns[in.index]) return fail(HY_ERR_INVALID, "%s: node %u names column %u", entry, k, in.index);
        const hy_column* column = program->columns[in.index];
        HY_TRY(on_this_device(column, entry));
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
        if (in.literal_type > HY_TYPE_DOUBLE) return fail(HY_ERR_INVALID, "%s: node %u has literal type %u", entry, k, in.literal_type);
        type = in.literal_type;
        node.literal = literal_bits(type, in.literal);
        break;
      case HY_PROJ_COLUMN_TEST:
        if (in.index >= program->n_tests || !program->tests[in.index].column) return fail(HY_ERR_INVALID, "%s: node %u names column test %u", entry, k, in.index);
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
        if (in.op >= HY_PRED_BETWEEN_INCLUSIVE && in.op <= HY_PRED_BETWEEN_EXCLUSIVE) return fail(HY_ERR_UNSUPPORTED, "%s: Between expressions are not evaluated on the device", entry);
        if (in.op > HY_PRED_GREATER_THAN_EQUALS) return fail(HY_ERR_INVALID, "%s: node %u compares with condition %u", entry, k, in.op);
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        break;
      case HY_PROJ_AND:
      case HY_PROJ_OR:
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        for (uint32_t t : {uint32_t{node.at}, uint32_t{node.bt}}) {
          if (t != HY_TYPE_INT && t != HY_TYPE_NULL) return fail(HY_ERR_INVALID, "%s: node %u: AND / OR take Int operands (a predicate's result)", entry, k);
        }
        break;
      case HY_PROJ_UNARY_MINUS:
        node.at = static_cast<uint8_t>(stack[depth - 1]);
        if (!px_numeric(node.at)) return fail(HY_ERR_INVALID, "%s: node %u negates a NULL literal", entry, k);
        type = node.at;
        break;
      case HY_PROJ_CASE:
        if (stack[depth - 3] != HY_TYPE_INT && stack[depth - 3] != HY_TYPE_NULL) return fail(HY_ERR_INVALID, "%s: node %u: CASE takes an Int `when` (a predicate's result)", entry, k);
        node.at = static_cast<uint8_t>(stack[depth - 2]);
        node.bt = static_cast<uint8_t>(stack[depth - 1]);
        if (node.at == HY_TYPE_NULL && node.bt == HY_TYPE_NULL) return fail(HY_ERR_INVALID, "Cannot deduce common type if both sides are NULL.");
        type = expression_common_type(node.at, node.bt);
        break;
      default: break;   // IS_NULL / IS_NOT_NULL: Int
    }
    node.op = static_cast<uint8_t>(in.op);
    node.type = static_cast<uint8_t>(type);
    first[k] = operands ? begins[depth - operands] : k;
    depth = depth - operands + 1;
    stack[depth - 1] = type;
    begins[depth - 1] = first[k];
  }
  if (depth != 1) return fail(HY_ERR_INVALID, "%s: the program leaves %u values, not one", entry, depth);
  const uint32_t result_type = p->result_type = stack[0];
  if (!px_numeric(result_type)) return fail(HY_ERR_INVALID, "%s: the result's type cannot be deduced (a NULL literal)", entry);
  // ---- a scan's predicate: a boolean root; on the spine -- the root and every node all of whose ancestors are AND / OR -- FALSE and NULL
  // both drop the row, so a column test there may carry a Between condition (test_cell evaluates the range job; below the spine
  // _evaluate_between_expression's FALSE-for-NULL, expression_evaluator.cpp:590-656, could be seen: refused as in a projection)
  bool between_refused[PX_TESTS] = {};
  {
    bool spine[HY_MAX_PROJECTION_NODES] = {};
    const uint32_t root = program->n_nodes - 1;
    if (scan) {
      const uint32_t kind = nodes[root].kind;
      if (kind != HY_PROJ_COMPARISON && kind != HY_PROJ_COLUMN_TEST && kind != HY_PROJ_IS_NULL && kind != HY_PROJ_IS_NOT_NULL && kind != HY_PROJ_AND && kind != HY_PROJ_OR)
        return fail(HY_ERR_INVALID, "%s: Expression type cannot be evaluated to PosList (the root is a comparison, a column test, IS [NOT] NULL, AND or OR)", entry);
      spine[root] = true;
    }
    for (uint32_t k = program->n_nodes; k-- > 0;) {   // a node's operands lie in front of it: parents first
      if (spine[k] && (nodes[k].kind == HY_PROJ_AND || nodes[k].kind == HY_PROJ_OR)) spine[k - 1] = spine[first[k - 1] - 1] = true;
      if (nodes[k].kind == HY_PROJ_COLUMN_TEST && !spine[k]) between_refused[nodes[k].index] = true;
    }
  }

  // ---- the tests' columns -----------------------------------------------------------------------------------------------------------
  const hy_column* (&tested)[PX_TESTS] = p->tested;
  const hy_column* (&tested_data)[PX_TESTS] = p->tested_data;
  hy_predicate (&predicates)[PX_TESTS] = p->predicates;
  for (uint32_t t = 0; t < program->n_tests; ++t) {
    if (!test_used[t]) continue;
    const hy_projection_test& test = program->tests[t];
    const hy_column* column = test.column;
    HY_TRY(on_this_device(column, entry));
    if (column->is_mvcc || (column->ref && column->ref->is_mvcc)) return fail(HY_ERR_UNSUPPORTED, "MVCC columns are read by hy_validate only");
    HY_TRY(plain_column(column, &column));
    const hy_column* data_column = column->is_reference ? column->ref : column;
    if (!data_column) return fail(HY_ERR_INVALID, "%s: column test %u over a reference column without a referenced column", entry, t);
    HY_TRY(plain_column(data_column, &data_column));
    if (column->data_type == HY_TYPE_STRING) {
      for (uint32_t c = 0; c < data_column->n_chunks; ++c) {
        if (data_column->host_segments[c].encoding != HY_ENC_DICTIONARY) return fail(HY_ERR_UNSUPPORTED, "column tests on unencoded string segments stay on the CPU path");
      }
    } else if (!px_numeric(column->data_type)) {
      return fail(HY_ERR_INVALID, "%s: column test %u over a column of type %u", entry, t, column->data_type);
    }
    if (test.in_list) {
      HY_TRY(in_list_as_bitmaps(data_column, test.in_list, &p->list_words[t], &p->list_offsets[t], &predicates[t]));
    } else {
      predicates[t] = test.predicate;
      const uint32_t condition = predicates[t].condition;
      if (between_refused[t] && condition >= HY_PRED_BETWEEN_INCLUSIVE && condition <= HY_PRED_BETWEEN_EXCLUSIVE)
        return fail(HY_ERR_UNSUPPORTED, "%s: Between expressions are not evaluated on the device%s", entry, scan ? " below the AND / OR spine of the predicate" : "");
      if (condition == HY_PRED_IN || condition == HY_PRED_NOT_IN) return fail(HY_ERR_INVALID, "%s: an IN list is passed as hy_projection_test.in_list", entry);
    }
    tested[t] = column;
    tested_data[t] = data_column;
    if (!shape) shape = column;
  }
  if (!shape) return fail(HY_ERR_INVALID, "%s: at least one operand must be a column", entry);
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
  return HY_OK;
}

// The tests' per-chunk jobs (prepare_jobs, queued on the current stream), in a block that lives as long as `p`: until the kernel has run.
hy_status prepare_program_tests(PreparedProgram* p) {
  hipStream_t stream = current_stream();
  // ---- the tests' per-chunk jobs, in a block that lives until the kernel has run ----------------------------------------------------------
  size_t jobs_at[PX_TESTS + 1] = {}, staging_at[PX_TESTS + 1] = {};
  size_t temporary_bytes = 0;
  for (uint32_t t = 0; t < PX_TESTS; ++t) {
    if (!p->tested[t]) continue;
    jobs_at[t] = temporary_bytes;
    temporary_bytes += align_up(sizeof(ScanJob) * (size_t{p->tested_data[t]->n_chunks} + 1), 256);
    staging_at[t] = temporary_bytes;
    temporary_bytes += align_up(scan_jobs_staging_bytes(p->tested_data[t], &p->predicates[t]) + 256, 256);
  }
  if (temporary_bytes) HY_TRY(p->temporary.alloc(temporary_bytes));
  for (uint32_t t = 0; t < PX_TESTS; ++t) {
    if (!p->tested[t]) continue;
    ScanJob* jobs = reinterpret_cast<ScanJob*>(p->temporary.as<char>() + jobs_at[t]);
    const hy_status status = prepare_scan_jobs(p->tested_data[t], &p->predicates[t], jobs, p->temporary.as<char>() + staging_at[t]);
    if (status != HY_OK) {
      (void)hipStreamSynchronize(stream);   // (uploads from this call's host arrays may be queued)
      return status;
    }
    const uint32_t condition = p->predicates[t].condition;
    p->tests[t] = ExprTest{p->tested[t]->d_segments, jobs, condition == HY_PRED_IS_NULL ? 1u : condition == HY_PRED_IS_NOT_NULL ? 2u : 0u, 0};
  }
  return HY_OK;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_projection_expression(const hy_projection_program* program, hy_column** out) {
  if (!program || !out) return fail(HY_ERR_INVALID, "hy_projection_expression: null argument");
  *out = nullptr;
  PreparedProgram prepared;
  HY_TRY(check_program(program, "hy_projection_expression", false, &prepared));
  HY_TRY(prepare_program_tests(&prepared));
  ExprArgs a{};
  const ExprNode (&nodes)[HY_MAX_PROJECTION_NODES] = prepared.nodes;
  const hy_column* const shape = prepared.shape;
  const hy_column* const (&distinct)[PX_COLUMNS] = prepared.distinct;
  const hy_column* const (&tested)[PX_TESTS] = prepared.tested;
  const uint32_t n_distinct = prepared.n_distinct, result_type = prepared.result_type;
  for (uint32_t t = 0; t < PX_TESTS; ++t) a.tests[t] = prepared.tests[t];
  const uint32_t width = (result_type == HY_TYPE_INT || result_type == HY_TYPE_FLOAT) ? 4 : 8;
  hipStream_t stream = current_stream();

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

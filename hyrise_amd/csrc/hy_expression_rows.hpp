// hy_expression_rows.hpp -- the evaluation of a hy_projection_program for PX_ROWS rows per lane, as program text: included INSIDE the row
// loop of the two kernels that evaluate a program (projection_expression_rows, projection_expression.hip: the value becomes a cell;
// expression_scan_chunks, scan_expression.hip: its truth value a RowID), so that both compile the same statements and neither pays for
// a function boundary (as a __forceinline__ function the same statements leave projection_expression_rows another register allocation).
// In scope where it is included:  a  (columns, tests, nodes and their counts: ExprArgs / ExprScanArgs),  slice  (.chunk),
// row[B], valid  (the lane's rows and which of them exist),  constexpr int B = PX_ROWS.
// Afterwards:  s[0][i] = the bits of row i's result (value_bits), bit i of n[0] = it is NULL.
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

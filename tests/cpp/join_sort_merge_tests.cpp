// join_sort_merge_tests.cpp -- the C++ mirror's JoinSortMerge (hyrise_amd/host/hyrise_host.hpp), which joins on the device through
// hy_join_sort_merge, over the reference's JoinTestRunner input tables (tests/golden/tbl/join_test_runner):
//   the output's rows as a multiset against a nested loop (the reference's JoinVerification contract; join_test_runner.cpp compares
//   unordered), over data inputs and over a TableScan's reference output, with device-resident and host results;
//   the chunk boundaries (matched pairs | unmatched left rows | unmatched right rows, Chunk::DEFAULT_SIZE pairs inside a part), and the
//   sorted / clustered flags of an Inner equi-join (join_sort_merge.cpp:940-958);
//   JoinSortMerge::supports' truth table (join_sort_merge.cpp:43-47).
// Usage: join_sort_merge_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>

#include "../../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;

static std::string g_tbl;
static int g_failures = 0;

#define EXPECT_TRUE(cond)                                                                      \
  do {                                                                                         \
    if (!(cond)) { std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } \
  } while (0)

static std::shared_ptr<TableWrapper> wrap(std::shared_ptr<const Table> table) {
  auto wrapper = std::make_shared<TableWrapper>(std::move(table));
  wrapper->execute();
  return wrapper;
}

static void run(const std::string& name, const std::function<void()>& test) {
  const int before = g_failures;
  try { test(); } catch (const std::exception& e) { std::printf("  EXCEPTION: %s\n", e.what()); ++g_failures; }
  std::printf("[%s] %s\n", g_failures == before ? "  OK  " : "FAILED", name.c_str());
}

static double as_double(const AllTypeVariant& v) {
  switch (v.index()) { case 1: return static_cast<double>(std::get<int32_t>(v)); case 2: return static_cast<double>(std::get<int64_t>(v));
                       case 3: return static_cast<double>(std::get<float>(v)); default: return std::get<double>(v); }
}

static bool satisfies(PredicateCondition condition, double l, double r) {
  switch (condition) {
    case PredicateCondition::Equals: return l == r;
    case PredicateCondition::NotEquals: return l != r;
    case PredicateCondition::LessThan: return l < r;
    case PredicateCondition::LessThanEquals: return l <= r;
    case PredicateCondition::GreaterThan: return l > r;
    default: return l >= r;
  }
}

// A row as text (NULL cells as "null"): rows compare as strings, tables as sorted vectors of them.
static std::string row_text(const std::vector<AllTypeVariant>& row) {
  std::string text;
  for (const auto& cell : row) {
    if (variant_is_null(cell)) text += "null|";
    else if (cell.index() == 5) text += std::get<std::string>(cell) + "|";
    else text += std::to_string(as_double(cell)) + "|";
  }
  return text;
}

static std::vector<std::string> nested_loop(const Table& left, const Table& right, JoinMode mode, ColumnIDPair ids, PredicateCondition condition) {
  const auto l = left.get_rows(), r = right.get_rows();
  const std::vector<AllTypeVariant> left_nulls(left.column_count(), AllTypeVariant{}), right_nulls(right.column_count(), AllTypeVariant{});
  const auto joined = [](std::vector<AllTypeVariant> a, const std::vector<AllTypeVariant>& b) { a.insert(a.end(), b.begin(), b.end()); return row_text(a); };
  std::vector<std::string> rows;
  std::vector<bool> right_matched(r.size(), false);
  for (const auto& a : l) {
    bool matched = false;
    for (size_t j = 0; j < r.size(); ++j) {
      if (variant_is_null(a[ids.first]) || variant_is_null(r[j][ids.second]) || !satisfies(condition, as_double(a[ids.first]), as_double(r[j][ids.second]))) continue;
      matched = right_matched[j] = true;
      rows.push_back(joined(a, r[j]));
    }
    if (!matched && (mode == JoinMode::Left || mode == JoinMode::FullOuter)) rows.push_back(joined(a, right_nulls));
  }
  if (mode == JoinMode::Right || mode == JoinMode::FullOuter)
    for (size_t j = 0; j < r.size(); ++j)
      if (!right_matched[j]) rows.push_back(joined(left_nulls, r[j]));
  std::sort(rows.begin(), rows.end());
  return rows;
}

static std::vector<std::string> sorted_rows(const Table& table) {
  std::vector<std::string> rows;
  for (const auto& row : table.get_rows()) rows.push_back(row_text(row));
  std::sort(rows.begin(), rows.end());
  return rows;
}

static const std::vector<std::pair<JoinMode, PredicateCondition>>& accepted() {
  static std::vector<std::pair<JoinMode, PredicateCondition>> all;
  if (all.empty()) {
    for (const auto condition : {PredicateCondition::Equals, PredicateCondition::NotEquals, PredicateCondition::LessThan, PredicateCondition::LessThanEquals,
                                 PredicateCondition::GreaterThan, PredicateCondition::GreaterThanEquals})
      for (const auto mode : {JoinMode::Inner, JoinMode::Left, JoinMode::Right, JoinMode::FullOuter})
        if (condition != PredicateCondition::NotEquals || mode == JoinMode::Inner) all.emplace_back(mode, condition);
  }
  return all;
}

// The output's parts begin new chunks; the flags of an Inner equi-join.
static void check_shape(const JoinSortMerge& join, const Table& out, JoinMode mode, PredicateCondition condition, const Table& left, ColumnIDPair ids) {
  EXPECT_TRUE(out.type() == TableType::References);
  const uint64_t ends[3] = {join.n_matched, join.n_matched + join.n_left_outer, out.row_count()};
  uint64_t at = 0;
  size_t part = 0;
  for (ChunkID k = 0; k < out.chunk_count(); ++k) {
    while (part < 3 && at == ends[part]) ++part;
    EXPECT_TRUE(part < 3);
    if (part >= 3) break;
    const uint64_t size = out.get_chunk(k)->size();
    EXPECT_TRUE(size > 0 && at + size <= ends[part]);                                   // no chunk spans two parts
    EXPECT_TRUE(size == Chunk::DEFAULT_SIZE || at + size == ends[part]);                // only a part's last chunk is short
    at += size;
  }
  EXPECT_TRUE(at == out.row_count());
  const bool sorted_output = mode == JoinMode::Inner && condition == PredicateCondition::Equals;
  const ColumnID right_key = static_cast<ColumnID>(left.column_count() + ids.second);
  for (ChunkID k = 0; k < out.chunk_count(); ++k) {
    const auto& chunk = out.get_chunk(k);
    EXPECT_TRUE(chunk->is_mutable() == !sorted_output);
    const auto& sorted_by = chunk->individually_sorted_by();
    if (!sorted_output) { EXPECT_TRUE(sorted_by.empty()); continue; }
    EXPECT_TRUE(sorted_by.size() == 2 && sorted_by[0].column == ids.first && sorted_by[1].column == right_key && sorted_by[0].sort_mode == SortMode::AscendingNullsFirst &&
                sorted_by[1].sort_mode == SortMode::AscendingNullsFirst);
    for (ChunkOffset r = 1; r < chunk->size(); ++r) {   // ... and they are
      EXPECT_TRUE(as_double((*chunk->get_segment(ids.first))[r - 1]) <= as_double((*chunk->get_segment(ids.first))[r]));
      EXPECT_TRUE(as_double((*chunk->get_segment(right_key))[r - 1]) <= as_double((*chunk->get_segment(right_key))[r]));
    }
  }
  if (sorted_output && out.chunk_count() <= 1) EXPECT_TRUE((out.value_clustered_by() == std::vector<ColumnID>{ids.first, right_key}));
  else EXPECT_TRUE(out.value_clustered_by().empty());
}

static void test_inputs(const std::shared_ptr<const AbstractOperator>& left, const std::shared_ptr<const AbstractOperator>& right) {
  const auto left_table = left->get_output(), right_table = right->get_output();
  for (ColumnID a = 0; a < left_table->column_count(); ++a) {
    for (ColumnID b = 0; b < right_table->column_count(); ++b) {
      if (left_table->column_data_type(a) != right_table->column_data_type(b) || left_table->column_data_type(a) == DataType::String) continue;
      for (const auto& [mode, condition] : accepted()) {
        JoinSortMerge join(left, right, mode, OperatorJoinPredicate{{a, b}, condition});
        join.execute();
        const auto out = join.get_output();
        const auto want = nested_loop(*left_table, *right_table, mode, {a, b}, condition);
        if (sorted_rows(*out) != want) {
          std::printf("  columns %u x %u mode %u condition %u: %zu rows, the nested loop has %zu (or they differ)\n", a, b, static_cast<unsigned>(mode), static_cast<unsigned>(condition),
                      static_cast<size_t>(out->row_count()), want.size());
          ++g_failures;
        }
        check_shape(join, *out, mode, condition, *left_table, {a, b});
        for (ColumnID c = 0; c < out->column_count(); ++c) {
          const bool from_left = c < left_table->column_count();
          const bool input_nullable = from_left ? left_table->column_is_nullable(c) : right_table->column_is_nullable(c - left_table->column_count());
          const bool outer = from_left ? (mode == JoinMode::Right || mode == JoinMode::FullOuter) : (mode == JoinMode::Left || mode == JoinMode::FullOuter);
          EXPECT_TRUE(out->column_is_nullable(c) == (input_nullable || outer));
        }
      }
    }
  }
}

static std::shared_ptr<const AbstractOperator> scanned(const std::shared_ptr<TableWrapper>& input) {   // every row with a non-NULL first column <= 1338: a reference table
  auto scan = std::make_shared<TableScan>(input, ColumnID{0}, PredicateCondition::LessThanEquals, AllTypeVariant{int32_t{1338}});
  scan->execute();
  return scan;
}

static void test_many_pairs() {   // 400 x 400 rows of 2 keys: 80 000 matched pairs cut into two chunks, no clustering claimed
  TableColumnDefinitions definitions{{"k", DataType::Int, false}, {"v", DataType::Int, false}};
  auto left = std::make_shared<Table>(definitions, TableType::Data, ChunkOffset{150}), right = std::make_shared<Table>(definitions, TableType::Data, ChunkOffset{97});
  for (int32_t i = 0; i < 400; ++i) {
    left->append({AllTypeVariant{int32_t{i % 2}}, AllTypeVariant{i}});
    right->append({AllTypeVariant{int32_t{(i / 3) % 2}}, AllTypeVariant{i}});
  }
  left->finalize();
  right->finalize();
  const auto l = wrap(left), r = wrap(right);
  for (const auto mode : {JoinMode::Inner, JoinMode::FullOuter}) {
    JoinSortMerge join(l, r, mode, OperatorJoinPredicate{{ColumnID{0}, ColumnID{0}}, PredicateCondition::Equals});
    join.execute();
    const auto out = join.get_output();
    EXPECT_TRUE(out->row_count() == 80000 && join.n_matched == 80000 && out->chunk_count() == 2 && out->get_chunk(0)->size() == Chunk::DEFAULT_SIZE);
    check_shape(join, *out, mode, PredicateCondition::Equals, *left, {ColumnID{0}, ColumnID{0}});
    EXPECT_TRUE(sorted_rows(*out) == nested_loop(*left, *right, mode, {ColumnID{0}, ColumnID{0}}, PredicateCondition::Equals));
  }
}

static void test_supports() {
  const DataType types[] = {DataType::Int, DataType::Long, DataType::Float, DataType::Double, DataType::String};
  for (int m = 0; m <= static_cast<int>(JoinMode::AntiNullAsFalse); ++m) {
    for (int c = 0; c <= static_cast<int>(PredicateCondition::GreaterThanEquals); ++c) {
      for (const auto l : types) {
        for (const auto r : types) {
          const auto mode = static_cast<JoinMode>(m);
          const auto condition = static_cast<PredicateCondition>(c);
          const bool want = (condition != PredicateCondition::NotEquals || mode == JoinMode::Inner) && l == r && mode != JoinMode::Semi && mode != JoinMode::AntiNullAsTrue &&
                            mode != JoinMode::AntiNullAsFalse;
          EXPECT_TRUE(JoinSortMerge::supports(JoinConfiguration{mode, condition, l, r, false}) == want);
        }
      }
    }
  }
  EXPECT_TRUE(JoinSortMerge::supports(JoinConfiguration{JoinMode::FullOuter, PredicateCondition::Equals, DataType::Int, DataType::Int, true}));
  EXPECT_TRUE(!JoinSortMerge::supports(JoinConfiguration{JoinMode::Left, PredicateCondition::NotEquals, DataType::Int, DataType::Int, false}));
}

static void test_refusals() {   // what the library refuses arrives as JoinHash's refusals do: a logic_error with the library's message
  const auto left = wrap(load_table(g_tbl + "/join_test_runner/input_table_left_10.tbl", ChunkOffset{4})), right = wrap(load_table(g_tbl + "/join_test_runner/input_table_right_10.tbl", ChunkOffset{3}));
  const auto refused = [&](JoinMode mode, ColumnIDPair ids, PredicateCondition condition, std::vector<OperatorJoinPredicate> secondary = {}) {
    bool threw = false;
    try {
      JoinSortMerge join(left, right, mode, OperatorJoinPredicate{ids, condition}, std::move(secondary));
      join.execute();
    } catch (const std::logic_error&) {
      threw = true;
    }
    return threw;
  };
  EXPECT_TRUE(refused(JoinMode::Semi, {ColumnID{0}, ColumnID{0}}, PredicateCondition::Equals));
  EXPECT_TRUE(refused(JoinMode::Left, {ColumnID{0}, ColumnID{0}}, PredicateCondition::NotEquals));
  EXPECT_TRUE(refused(JoinMode::Inner, {ColumnID{0}, ColumnID{6}}, PredicateCondition::Equals));    // int x long
  EXPECT_TRUE(refused(JoinMode::Inner, {ColumnID{8}, ColumnID{8}}, PredicateCondition::Equals));    // strings
  EXPECT_TRUE(refused(JoinMode::Inner, {ColumnID{0}, ColumnID{0}}, PredicateCondition::Equals, {OperatorJoinPredicate{{ColumnID{2}, ColumnID{2}}, PredicateCondition::LessThan}}));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: join_sort_merge_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  for (const bool resident : {true, false}) {
    device_resident_results() = resident;
    const std::string where = resident ? " (results in HBM)" : " (host results)";
    for (const int left_size : {0, 10, 15}) {
      for (const int right_size : {0, 10, 15}) {
        if (!resident && left_size != right_size) continue;
        const auto left = wrap(load_table(g_tbl + "/join_test_runner/input_table_left_" + std::to_string(left_size) + ".tbl", ChunkOffset{4}));
        const auto right = wrap(load_table(g_tbl + "/join_test_runner/input_table_right_" + std::to_string(right_size) + ".tbl", ChunkOffset{7}));
        const std::string sizes = std::to_string(left_size) + " x " + std::to_string(right_size);
        run("JoinSortMerge data inputs " + sizes + where, [&] { test_inputs(left, right); });
        if (left_size && right_size) run("JoinSortMerge reference inputs " + sizes + where, [&] { test_inputs(scanned(left), scanned(right)); });
      }
    }
    run("JoinSortMerge chunks of 65 535 pairs" + where, test_many_pairs);
  }
  device_resident_results() = true;
  run("JoinSortMerge::supports", test_supports);
  run("JoinSortMerge refusals", test_refusals);
  hy_shutdown();
  std::printf("%s\n", g_failures ? "JOIN SORT MERGE TESTS FAILED" : "JOIN SORT MERGE TESTS PASSED");
  return g_failures ? 1 : 0;
}

// projection_tests.cpp -- the C++ mirror's Projection (hyrise_amd/host/hyrise_host.hpp) over hy_projection_expression:
//   the series of expression_evaluator_to_values_test.cpp over input_a.tbl / input_bools.tbl against their recorded answers
//   a projection that only forwards (data and reference input): the input's table type, the segments shared
//   forwarded and computed columns side by side over a scan's output, a string column among them
//   TableScan -> Projection (CASE over a string column test) -> AggregateHash: no DeviceValueSegment fetches its chunk, and the rows equal
//   those of the same chain with host results
// Usage: projection_tests <tests/golden/tbl directory> <tests/golden/expression directory>.  One line per test, non-zero exit if one failed.
#include <cstdio>
#include <functional>
#include <string>

#include "../../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;

static std::string g_tbl, g_expression;
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

struct ResidentResults {   // device_resident_results() for a scope
  explicit ResidentResults(bool enabled) : before(device_resident_results()) { device_resident_results() = enabled; }
  ~ResidentResults() { device_resident_results() = before; }
  bool before;
};

static std::vector<AllTypeVariant> column_cells(const std::shared_ptr<const Table>& table, ColumnID column) {
  std::vector<AllTypeVariant> cells;
  for (ChunkID k = 0; k < table->chunk_count(); ++k) {
    const auto segment = table->get_chunk(k)->get_segment(column);
    for (ChunkOffset r = 0; r < segment->size(); ++r) cells.push_back((*segment)[r]);
  }
  return cells;
}

static bool identical(const AllTypeVariant& a, const AllTypeVariant& b) {
  if (a.index() != b.index()) return false;
  switch (a.index()) {
    case 0: return true;
    case 1: return std::get<int32_t>(a) == std::get<int32_t>(b);
    case 2: return std::get<int64_t>(a) == std::get<int64_t>(b);
    case 3: return std::get<float>(a) == std::get<float>(b);
    case 4: return std::get<double>(a) == std::get<double>(b);
    default: return std::get<std::string>(a) == std::get<std::string>(b);
  }
}
static bool same(const std::vector<AllTypeVariant>& a, const std::vector<AllTypeVariant>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (!identical(a[i], b[i])) return false;
  return true;
}

static std::shared_ptr<const Table> project(const std::shared_ptr<const AbstractOperator>& in, std::vector<ExpressionPtr> expressions) {
  auto projection = std::make_shared<Projection>(in, std::move(expressions));
  projection->execute();
  return projection->get_output();
}

static const AllTypeVariant N = NullValue{};
static std::vector<AllTypeVariant> ints(std::initializer_list<AllTypeVariant> cells) { return cells; }

static void test_recorded_answers() {   // expression_evaluator_to_values_test.cpp, the line of every case beside it
  const auto a = column_(0), b = column_(1), c = column_(2), f = column_(8);   // input_a.tbl: a|b|c|d|s1|s2|s3|e|f
  const auto mul_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Multiplication, std::move(l), std::move(r)); };
  const auto add_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Addition, std::move(l), std::move(r)); };
  const auto mod_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Modulo, std::move(l), std::move(r)); };
  const auto cmp_ = [](PredicateCondition condition, ExpressionPtr l, ExpressionPtr r) { return predicate_(condition, {std::move(l), std::move(r)}); };
  struct Case { int line; ExpressionPtr expression; std::vector<AllTypeVariant> expected; };
  const auto a2 = mul_(a, value_(int32_t{2}));
  const std::vector<Case> over_a = {
      {247, mul_(a, b), ints({2, 6, 12, 20})}, {248, mod_(b, a), ints({0, 1, 1, 1})}, {249, mod_(a, c), ints({1, N, 3, N})}, {250, add_(a, add_(b, c)), ints({36, N, 41, N})},
      {251, add_(a, null_()), ints({N, N, N, N})}, {252, add_(a, add_(b, null_())), ints({N, N, N, N})},
      {336, cmp_(PredicateCondition::GreaterThan, b, a), ints({1, 1, 1, 1})}, {338, cmp_(PredicateCondition::GreaterThan, b, null_()), ints({N, N, N, N})},
      {340, cmp_(PredicateCondition::GreaterThan, c, a), ints({1, N, 1, N})}, {341, cmp_(PredicateCondition::GreaterThanEquals, b, a2), ints({1, 0, 0, 0})},
      {342, cmp_(PredicateCondition::Equals, b, a2), ints({1, 0, 0, 0})}, {343, cmp_(PredicateCondition::NotEquals, b, a2), ints({0, 1, 1, 1})},
      {344, cmp_(PredicateCondition::LessThan, b, a2), ints({0, 1, 1, 1})}, {345, cmp_(PredicateCondition::LessThanEquals, b, a2), ints({1, 1, 1, 1})},
      {346, cmp_(PredicateCondition::LessThanEquals, c, f), ints({1, N, 0, N})},
      {390, case_(cmp_(PredicateCondition::GreaterThan, c, a), b, value_(int32_t{1337})), ints({2, 1337, 4, 1337})},
      {391, case_(cmp_(PredicateCondition::GreaterThan, c, value_(int32_t{0})), null_(), c), ints({N, N, N, N})}, {392, case_(value_(int32_t{1}), c, a), ints({33, N, 34, N})},
      {411, is_null_(add_(c, a)), ints({0, 1, 0, 1})}, {412, is_not_null_(add_(c, a)), ints({1, 0, 1, 0})},
      {422, unary_minus_(a), ints({-1, -2, -3, -4})}, {423, unary_minus_(c), ints({-33, N, -34, N})}, {424, unary_minus_(unary_minus_(c)), ints({33, N, 34, N})},
  };
  const std::vector<Case> over_bools = {
      {190, or_(a, b), ints({0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1})}, {191, or_(a, c), ints({0, 1, N, 0, 1, N, 1, 1, 1, 1, 1, 1})},
      {212, and_(a, b), ints({0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1})}, {213, and_(a, c), ints({0, 0, 0, 0, 0, 0, 0, 1, N, 0, 1, N})},
  };
  for (const auto encoding : {EncodingType::Unencoded, EncodingType::Dictionary}) {
    for (const bool bools : {false, true}) {
      auto table = load_table(bools ? g_expression + "/input_bools.tbl" : g_tbl + "/expression_evaluator/input_a.tbl", 3);
      if (encoding == EncodingType::Dictionary) ChunkEncoder::encode_all_chunks(table, encoding);
      else if (!bools) continue;   // (input_a.tbl holds unencoded strings otherwise; its numeric columns are read unencoded in the Python tests)
      const auto in = wrap(table);
      for (const auto& test : bools ? over_bools : over_a) {
        const auto out = project(in, {test.expression});
        const auto cells = column_cells(out, 0);
        bool same = cells.size() == test.expected.size() && out->type() == TableType::Data && out->column_data_type(0) == DataType::Int && out->chunk_count() == table->chunk_count();
        for (size_t r = 0; same && r < cells.size(); ++r) same = identical(cells[r], test.expected[r]);
        if (!same) std::printf("  line %d (%s)\n", test.line, bools ? "input_bools" : "input_a");
        EXPECT_TRUE(same);
      }
    }
  }
}

static std::shared_ptr<Table> encoded_input_a() {
  auto table = load_table(g_tbl + "/expression_evaluator/input_a.tbl", 3);
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

static void test_forwarding_only() {
  const auto table = encoded_input_a();
  const auto out = project(wrap(table), {column_(4), column_(0)});
  EXPECT_TRUE(out->type() == TableType::Data && out->column_count() == 2 && out->column_name(0) == "s1" && out->column_data_type(1) == DataType::Int);
  for (ChunkID k = 0; k < table->chunk_count(); ++k) {
    EXPECT_TRUE(out->get_chunk(k)->get_segment(0) == table->get_chunk(k)->get_segment(4));   // shared, not copied
    EXPECT_TRUE(out->get_chunk(k)->get_segment(1) == table->get_chunk(k)->get_segment(0));
  }
  auto scan = std::make_shared<TableScan>(wrap(table), ColumnID{0}, PredicateCondition::GreaterThan, int32_t{1});
  scan->execute();
  const auto referenced = project(scan, {column_(1), column_(5)});
  EXPECT_TRUE(referenced->type() == TableType::References && referenced->row_count() == 3);
  for (ChunkID k = 0; k < referenced->chunk_count(); ++k) {
    EXPECT_TRUE(referenced->get_chunk(k)->get_segment(0) == scan->get_output()->get_chunk(k)->get_segment(1));
    EXPECT_TRUE(dynamic_cast<const ReferenceSegment*>(referenced->get_chunk(k)->get_segment(1).get()) != nullptr);
  }
  EXPECT_TRUE(same(column_cells(referenced, 0), ints({3, 4, 5})));
}

static void test_forward_and_compute() {
  const auto table = encoded_input_a();
  auto scan = std::make_shared<TableScan>(wrap(table), ColumnID{0}, PredicateCondition::GreaterThan, int32_t{1});   // rows 2, 3, 4 of a
  scan->execute();
  const auto s1_is_what = predicate_(PredicateCondition::Equals, {column_(4), value_(std::string("what"))});
  const auto s3_like = predicate_(PredicateCondition::Like, {column_(6), value_(std::string("%z%"))});
  const auto s1_in = predicate_(PredicateCondition::In, {column_(4), value_(std::string("Same")), value_(std::string("Hello")), value_(std::string("absent"))});
  const auto out = project(scan, {column_(4), column_(2), arithmetic_(ArithmeticOperator::Multiplication, column_(0), column_(8)),
                                  case_(s1_is_what, column_(1), value_(int32_t{0})), s3_like, s1_in, is_null_(column_(6))});
  EXPECT_TRUE(out->type() == TableType::Data && out->column_count() == 7 && out->row_count() == 3);
  EXPECT_TRUE(out->column_data_type(0) == DataType::String && out->column_data_type(2) == DataType::Double && out->column_data_type(3) == DataType::Int);
  EXPECT_TRUE(same(column_cells(out, 0), (std::vector<AllTypeVariant>{std::string("Hello"), std::string("what"), std::string("Same")})));
  EXPECT_TRUE(same(column_cells(out, 1), ints({N, 34, N})));
  EXPECT_TRUE(same(column_cells(out, 2), (std::vector<AllTypeVariant>{2 * 2.2, 3 * 13.8, 4 * 15.9})));
  EXPECT_TRUE(same(column_cells(out, 3), ints({0, 4, 0})));
  EXPECT_TRUE(same(column_cells(out, 4), ints({0, 1, N})));   // s3: abcd, xyzlol, NULL -- NULL where the cell is NULL
  EXPECT_TRUE(same(column_cells(out, 5), ints({1, 0, 1})));
  EXPECT_TRUE(same(column_cells(out, 6), ints({0, 0, 1})));
  for (ChunkID k = 0; k < out->chunk_count(); ++k) EXPECT_TRUE(dynamic_cast<const ReferenceSegment*>(out->get_chunk(k)->get_segment(1).get()) == nullptr);
  bool refused = false;   // Between is refused by the library: a Fail, the mirror has no CPU operators
  try { project(scan, {predicate_(PredicateCondition::BetweenInclusive, {column_(1), column_(0), column_(3)})}); } catch (const std::logic_error&) { refused = true; }
  EXPECT_TRUE(refused);
}

// Q12's shape: SELECT priority_group, SUM(CASE WHEN priority = '1-URGENT' OR priority = '2-HIGH' THEN amount ELSE 0 END) ... WHERE amount > :x
static std::shared_ptr<Table> orders_table(size_t rows) {
  static const char* const priorities[] = {"1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"};
  auto table = std::make_shared<Table>(TableColumnDefinitions{{"group", DataType::Int, false}, {"amount", DataType::Int, false}, {"priority", DataType::String, true}}, TableType::Data,
                                       ChunkOffset{4096});
  for (size_t r = 0; r < rows; ++r) {
    const size_t k = (r * 2654435761u) >> 7;
    table->append({static_cast<int32_t>(r % 7), static_cast<int32_t>(k % 1000), r % 13 == 0 ? AllTypeVariant{NullValue{}} : AllTypeVariant{std::string(priorities[k % 5])}});
  }
  table->finalize();
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

static std::shared_ptr<const Table> chain(const std::shared_ptr<Table>& table) {
  auto scan = std::make_shared<TableScan>(wrap(table), ColumnID{1}, PredicateCondition::GreaterThan, int32_t{100});
  scan->execute();
  const auto urgent = predicate_(PredicateCondition::Equals, {column_(2), value_(std::string("1-URGENT"))});
  const auto high = predicate_(PredicateCondition::Equals, {column_(2), value_(std::string("2-HIGH"))});
  auto projection = std::make_shared<Projection>(scan, std::vector<ExpressionPtr>{column_(0), case_(or_(urgent, high), column_(1), value_(int32_t{0}))});
  projection->execute();
  auto aggregate = std::make_shared<AggregateHash>(projection, std::vector<AggregateDefinition>{{1, WindowFunction::Sum}, {INVALID_COLUMN_ID, WindowFunction::Count}}, std::vector<ColumnID>{0});
  aggregate->execute();
  return aggregate->get_output();
}

static void test_chain_stays_in_hbm() {
  const auto table = orders_table(20000);
  const uint64_t fetches_before = device_value_segment_fetches().load();
  std::shared_ptr<const Table> resident;
  { const ResidentResults scope(true); resident = chain(table); }
  EXPECT_TRUE(device_value_segment_fetches().load() == fetches_before);   // neither the projection's nor the aggregate's columns came to the host
  std::shared_ptr<const Table> host;
  { const ResidentResults scope(false); host = chain(table); }
  // the expected rows, from the table itself
  std::map<int32_t, std::pair<int64_t, int64_t>> expected;
  for (ChunkID k = 0; k < table->chunk_count(); ++k) {
    const auto chunk = table->get_chunk(k);
    for (ChunkOffset r = 0; r < chunk->size(); ++r) {
      const auto amount = std::get<int32_t>((*chunk->get_segment(1))[r]);
      if (amount <= 100) continue;
      const auto priority = (*chunk->get_segment(2))[r];
      const bool counts = !variant_is_null(priority) && (std::get<std::string>(priority) == "1-URGENT" || std::get<std::string>(priority) == "2-HIGH");
      auto& group = expected[std::get<int32_t>((*chunk->get_segment(0))[r])];
      group.first += counts ? amount : 0;
      group.second += 1;
    }
  }
  for (const auto& out : {resident, host}) {
    std::map<int32_t, std::pair<int64_t, int64_t>> got;
    const auto keys = column_cells(out, 0), sums = column_cells(out, 1), counts = column_cells(out, 2);
    for (size_t r = 0; r < keys.size(); ++r) got[std::get<int32_t>(keys[r])] = {std::get<int64_t>(sums[r]), std::get<int64_t>(counts[r])};
    EXPECT_TRUE(got == expected && keys.size() == 7);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: projection_tests <tests/golden/tbl> <tests/golden/expression>\n"); return 2; }
  g_tbl = argv[1];
  g_expression = argv[2];
  check_status(hy_init(0));
  run("recorded answers of the evaluator's series", test_recorded_answers);
  run("forwarding only", test_forwarding_only);
  run("forwarded and computed columns", test_forward_and_compute);
  run("TableScan -> Projection -> AggregateHash stays in HBM", test_chain_stays_in_hbm);
  hy_shutdown();
  std::printf(g_failures ? "PROJECTION TESTS FAILED\n" : "PROJECTION TESTS PASSED\n");
  return g_failures ? 1 : 0;
}

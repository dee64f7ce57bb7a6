// expression_scan_tests.cpp -- the C++ mirror's TableScan over a predicate expression (hyrise_amd/host/hyrise_host.hpp) through
// hy_table_scan_expression, over a small table of three chunks:
//   predicates the other scan implementations do not take, against a row-by-row evaluation on the host (ternary logic, NULL drops the row),
//   over the data table and over the output of another scan; device-resident and host results
//   BETWEEN lowered on the spine (numeric: two comparisons; string column: one column test), refused below it
//   a Value root and the NULL literal, answered on the host
//   TableScan(expression) -> Projection -> AggregateHash without a PosList or a column leaving HBM
// Usage: expression_scan_tests.  One line per test, non-zero exit if one failed.
#include <cstdio>
#include <functional>
#include <optional>
#include <string>

#include "../../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;

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

using Row = std::vector<AllTypeVariant>;   // a | b | s | g
using Truth = std::optional<bool>;         // nullopt: NULL

static std::vector<Row> rows_of(const std::shared_ptr<const Table>& table) {
  std::vector<Row> rows;
  for (ChunkID k = 0; k < table->chunk_count(); ++k) {
    const auto chunk = table->get_chunk(k);
    for (ChunkOffset r = 0; r < chunk->size(); ++r) {
      Row row;
      for (ColumnID c = 0; c < table->column_count(); ++c) row.push_back((*chunk->get_segment(c))[r]);
      rows.push_back(std::move(row));
    }
  }
  return rows;
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

static bool same_rows(const std::vector<Row>& a, const std::vector<Row>& b) {
  if (a.size() != b.size()) return false;
  for (size_t r = 0; r < a.size(); ++r) {
    if (a[r].size() != b[r].size()) return false;
    for (size_t c = 0; c < a[r].size(); ++c) if (!identical(a[r][c], b[r][c])) return false;
  }
  return true;
}

// 130 rows in chunks of 50, 50 and 30: a Int, b Double, s String (all nullable), g Int
static std::shared_ptr<Table> small_table() {
  static const char* const words[] = {"apple", "banana", "cherry", "date", "elder"};
  auto table = std::make_shared<Table>(TableColumnDefinitions{{"a", DataType::Int, true}, {"b", DataType::Double, true}, {"s", DataType::String, true}, {"g", DataType::Int, false}},
                                       TableType::Data, ChunkOffset{50});
  for (size_t r = 0; r < 130; ++r) {
    const size_t k = (r * 2654435761u) >> 9;
    table->append({r % 7 == 3 ? AllTypeVariant{NullValue{}} : AllTypeVariant{static_cast<int32_t>(k % 11) - 3}, r % 5 == 1 ? AllTypeVariant{NullValue{}} : AllTypeVariant{static_cast<double>(k % 9) * 0.5},
                   r % 6 == 2 ? AllTypeVariant{NullValue{}} : AllTypeVariant{std::string(words[k % 5])}, static_cast<int32_t>(r % 4)});
  }
  table->finalize();
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

static Truth and3(Truth x, Truth y) {
  if ((x && !*x) || (y && !*y)) return false;
  if (!x || !y) return std::nullopt;
  return true;
}
static Truth or3(Truth x, Truth y) {
  if ((x && *x) || (y && *y)) return true;
  if (!x || !y) return std::nullopt;
  return false;
}
static bool is_null(const AllTypeVariant& v) { return variant_is_null(v); }
static int32_t a_of(const Row& row) { return std::get<int32_t>(row[0]); }
static double b_of(const Row& row) { return std::get<double>(row[1]); }
static const std::string& s_of(const Row& row) { return std::get<std::string>(row[2]); }

struct Case {
  const char* name;
  ExpressionPtr predicate;
  std::function<Truth(const Row&)> holds;
};

static ExpressionPtr cmp_(PredicateCondition condition, ExpressionPtr l, ExpressionPtr r) { return predicate_(condition, {std::move(l), std::move(r)}); }

static std::vector<Case> cases() {
  const auto a = column_(0), b = column_(1), s = column_(2);
  const auto mul_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Multiplication, std::move(l), std::move(r)); };
  const auto sub_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Subtraction, std::move(l), std::move(r)); };
  const auto add_ = [](ExpressionPtr l, ExpressionPtr r) { return arithmetic_(ArithmeticOperator::Addition, std::move(l), std::move(r)); };
  const auto a_is = [](const Row& row, const std::function<bool(int32_t)>& f) -> Truth { return is_null(row[0]) ? Truth{} : Truth{f(a_of(row))}; };
  const auto s_is = [](const Row& row, const std::function<bool(const std::string&)>& f) -> Truth { return is_null(row[2]) ? Truth{} : Truth{f(s_of(row))}; };
  return {
      {"a * (1 - b) > 1.5", cmp_(PredicateCondition::GreaterThan, mul_(a, sub_(value_(int32_t{1}), b)), value_(1.5)),
       [](const Row& row) -> Truth { return is_null(row[0]) || is_null(row[1]) ? Truth{} : Truth{a_of(row) * (1 - b_of(row)) > 1.5}; }},
      {"a < b + 1", cmp_(PredicateCondition::LessThan, a, add_(b, value_(int32_t{1}))),
       [](const Row& row) -> Truth { return is_null(row[0]) || is_null(row[1]) ? Truth{} : Truth{a_of(row) < b_of(row) + 1}; }},
      {"a <> 2.5 AND a < 3.5 (literals without a lossless cast)", and_(cmp_(PredicateCondition::NotEquals, a, value_(2.5)), cmp_(PredicateCondition::LessThan, a, value_(3.5))),
       [=](const Row& row) { return a_is(row, [](int32_t x) { return x != 2.5 && x < 3.5; }); }},
      {"a = 1 OR b IS NULL", or_(cmp_(PredicateCondition::Equals, a, value_(int32_t{1})), is_null_(b)),
       [=](const Row& row) { return or3(a_is(row, [](int32_t x) { return x == 1; }), Truth{is_null(row[1])}); }},
      {"CASE WHEN a > 0 THEN a ELSE g END = 1", cmp_(PredicateCondition::Equals, case_(cmp_(PredicateCondition::GreaterThan, a, value_(int32_t{0})), a, column_(3)), value_(int32_t{1})),
       [](const Row& row) -> Truth { return Truth{(!is_null(row[0]) && a_of(row) > 0 ? a_of(row) : std::get<int32_t>(row[3])) == 1}; }},
      {"a BETWEEN 0 AND 4 AND s = 'cherry'", and_(predicate_(PredicateCondition::BetweenInclusive, {a, value_(int32_t{0}), value_(int32_t{4})}), cmp_(PredicateCondition::Equals, s, value_(std::string("cherry")))),
       [=](const Row& row) { return and3(a_is(row, [](int32_t x) { return x >= 0 && x <= 4; }), s_is(row, [](const std::string& x) { return x == "cherry"; })); }},
      {"s BETWEEN 'b' AND 'd' OR a < -1", or_(predicate_(PredicateCondition::BetweenUpperExclusive, {s, value_(std::string("b")), value_(std::string("d"))}), cmp_(PredicateCondition::LessThan, a, value_(int32_t{-1}))),
       [=](const Row& row) { return or3(s_is(row, [](const std::string& x) { return x >= "b" && x < "d"; }), a_is(row, [](int32_t x) { return x < -1; })); }},
      {"s LIKE '%an%' AND (s IN ('banana', 'fig') OR b > 3)",
       and_(cmp_(PredicateCondition::Like, s, value_(std::string("%an%"))),
            or_(predicate_(PredicateCondition::In, {s, value_(std::string("banana")), value_(std::string("fig"))}), cmp_(PredicateCondition::GreaterThan, b, value_(int32_t{3})))),
       [=](const Row& row) {
         return and3(s_is(row, [](const std::string& x) { return x.find("an") != std::string::npos; }),
                     or3(s_is(row, [](const std::string& x) { return x == "banana" || x == "fig"; }), is_null(row[1]) ? Truth{} : Truth{b_of(row) > 3}));
       }},
  };
}

static std::shared_ptr<const Table> scan(const std::shared_ptr<const AbstractOperator>& in, ExpressionPtr predicate) {
  auto op = std::make_shared<TableScan>(in, std::move(predicate));
  op->execute();
  return op->get_output();
}

static void check_cases(const std::shared_ptr<const AbstractOperator>& in) {
  const auto input = rows_of(in->get_output());
  for (const auto& test : cases()) {
    std::vector<Row> expected;
    for (const auto& row : input) { const Truth t = test.holds(row); if (t && *t) expected.push_back(row); }
    for (const bool resident : {true, false}) {
      const ResidentResults scope(resident);
      const auto out = scan(in, test.predicate);
      const bool ok = out->type() == TableType::References && same_rows(rows_of(out), expected) && !expected.empty() && expected.size() < input.size();
      if (!ok) std::printf("  %s (%s results): %zu rows, expected %zu of %zu\n", test.name, resident ? "device" : "host", size_t{out->row_count()}, expected.size(), input.size());
      EXPECT_TRUE(ok);
    }
  }
}

static void test_over_a_data_table() { check_cases(wrap(small_table())); }

static void test_over_the_output_of_another_scan() {
  auto first = std::make_shared<TableScan>(wrap(small_table()), ColumnID{3}, PredicateCondition::NotEquals, int32_t{2});   // partial chunks: PosLists
  first->execute();
  EXPECT_TRUE(first->get_output()->type() == TableType::References && first->get_output()->row_count() > 80);
  check_cases(first);
}

static void test_constant_roots_and_refusals() {
  const auto table = small_table();
  const auto in = wrap(table);
  for (const bool resident : {true, false}) {
    const ResidentResults scope(resident);
    EXPECT_TRUE(same_rows(rows_of(scan(in, value_(int32_t{7}))), rows_of(table)));
    EXPECT_TRUE(scan(in, value_(int32_t{0}))->row_count() == 0);
    EXPECT_TRUE(scan(in, null_())->row_count() == 0);
  }
  const auto between = predicate_(PredicateCondition::BetweenInclusive, {column_(0), value_(int32_t{0}), value_(int32_t{4})});
  for (const auto& refused : {is_null_(between), cmp_(PredicateCondition::Equals, case_(between, column_(0), column_(3)), value_(int32_t{1})),
                              arithmetic_(ArithmeticOperator::Addition, column_(0), column_(3)), ExpressionPtr{column_(0)}}) {
    bool failed = false;
    try { scan(in, refused); } catch (const std::logic_error&) { failed = true; }
    EXPECT_TRUE(failed);
  }
}

// SELECT g, SUM(a * 2), COUNT(*) WHERE a * (1 - b) > 1.5 OR s = 'date' GROUP BY g
static std::shared_ptr<const Table> chain(const std::shared_ptr<Table>& table, std::shared_ptr<const Table>* scanned = nullptr) {
  const auto predicate = or_(cmp_(PredicateCondition::GreaterThan, arithmetic_(ArithmeticOperator::Multiplication, column_(0), arithmetic_(ArithmeticOperator::Subtraction, value_(int32_t{1}), column_(1))), value_(1.5)),
                             cmp_(PredicateCondition::Equals, column_(2), value_(std::string("date"))));
  auto filtered = std::make_shared<TableScan>(wrap(table), predicate);
  filtered->execute();
  if (scanned) *scanned = filtered->get_output();
  auto projection = std::make_shared<Projection>(filtered, std::vector<ExpressionPtr>{column_(3), arithmetic_(ArithmeticOperator::Multiplication, column_(0), value_(int32_t{2}))});
  projection->execute();
  auto aggregate = std::make_shared<AggregateHash>(projection, std::vector<AggregateDefinition>{{1, WindowFunction::Sum}, {INVALID_COLUMN_ID, WindowFunction::Count}}, std::vector<ColumnID>{0});
  aggregate->execute();
  return aggregate->get_output();
}

static void test_chain_stays_in_hbm() {
  const auto table = small_table();
  const uint64_t fetches_before = device_value_segment_fetches().load();
  std::shared_ptr<const Table> resident, scanned;
  { const ResidentResults scope(true); resident = chain(table, &scanned); }
  EXPECT_TRUE(device_value_segment_fetches().load() == fetches_before);
  size_t device_lists = 0;
  for (ChunkID k = 0; k < scanned->chunk_count(); ++k) {   // the scan's PosLists are DevicePosLists of which no row has crossed the link
    const auto list = std::dynamic_pointer_cast<const DevicePosList>(std::static_pointer_cast<ReferenceSegment>(scanned->get_chunk(k)->get_segment(0))->pos_list());
    if (list && !list->on_host()) ++device_lists;
  }
  EXPECT_TRUE(scanned->chunk_count() == 3 && device_lists == 3);
  std::shared_ptr<const Table> host;
  { const ResidentResults scope(false); host = chain(table); }
  std::map<int32_t, std::pair<int64_t, int64_t>> expected;
  for (const auto& row : rows_of(table)) {
    const Truth first = is_null(row[0]) || is_null(row[1]) ? Truth{} : Truth{a_of(row) * (1 - b_of(row)) > 1.5};
    const Truth second = is_null(row[2]) ? Truth{} : Truth{s_of(row) == "date"};
    const Truth keep = or3(first, second);
    if (!keep || !*keep) continue;
    auto& group = expected[std::get<int32_t>(row[3])];
    group.first += is_null(row[0]) ? 0 : 2 * a_of(row);
    group.second += 1;
  }
  for (const auto& out : {resident, host}) {
    std::map<int32_t, std::pair<int64_t, int64_t>> got;
    for (const auto& row : rows_of(out)) got[std::get<int32_t>(row[0])] = {is_null(row[1]) ? 0 : std::get<int64_t>(row[1]), std::get<int64_t>(row[2])};
    EXPECT_TRUE(got == expected && expected.size() == 4);
  }
}

int main() {
  check_status(hy_init(0));
  run("predicate expressions over a data table", test_over_a_data_table);
  run("predicate expressions over the output of another scan", test_over_the_output_of_another_scan);
  run("a Value root, the NULL literal, and what is refused", test_constant_roots_and_refusals);
  run("TableScan(expression) -> Projection -> AggregateHash stays in HBM", test_chain_stays_in_hbm);
  hy_shutdown();
  std::printf(g_failures ? "EXPRESSION SCAN TESTS FAILED\n" : "EXPRESSION SCAN TESTS PASSED\n");
  return g_failures ? 1 : 0;
}

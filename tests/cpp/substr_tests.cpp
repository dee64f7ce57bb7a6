// substr_tests.cpp -- SUBSTR through the C++ mirror (hyrise_amd/host/hyrise_host.hpp): Projection(SUBSTR(l_shipdate, 1, 4)) and (6, 2) made in
// HBM (device_string_results(): one hy_string_column_substr, DeviceStringDictionarySegments) against the host path (the switch off) cell for
// cell, both against substr_of row by row, over a data table and a TableScan's output; the Q9-shaped chain TableScan -> Projection ->
// AggregateHash -> Sort without a segment fetch before the final read; and a column with a ValueSegment<pmr_string> chunk on the host path.
// Usage: substr_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
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

template <typename Op, typename... Args>
static std::shared_ptr<Op> executed(Args&&... args) {
  auto op = std::make_shared<Op>(std::forward<Args>(args)...);
  op->execute();
  return op;
}

static void run(const std::string& name, const std::function<void()>& test) {
  const int before = g_failures;
  try { test(); } catch (const std::exception& e) { std::printf("  EXCEPTION: %s\n", e.what()); ++g_failures; }
  std::printf("[%s] %s\n", g_failures == before ? "  OK  " : "FAILED", name.c_str());
}

using Row = std::vector<AllTypeVariant>;
using Rows = std::vector<Row>;

// ORDERKEY int, EXTENDEDPRICE float, DISCOUNT float, SHIPDATE string (NULL in every seventh row or so)
static const ColumnID ORDERKEY{0}, EXTENDEDPRICE{1}, DISCOUNT{2}, SHIPDATE{3};

static Rows lineitem_rows() {
  const auto table = load_table(g_tbl + "/tpch/sf-0.001/lineitem.tbl", ChunkOffset{65535});
  Rows rows;
  for (const auto& row : table->get_rows()) {
    const int32_t orderkey = std::get<int32_t>(row[0]), linenumber = std::get<int32_t>(row[3]);
    rows.push_back(Row{orderkey, row[5], row[6], (orderkey + linenumber) % 7 == 0 ? AllTypeVariant{NullValue{}} : row[10]});
  }
  return rows;
}

static std::shared_ptr<Table> make_table(const Rows& rows, ChunkOffset chunk_size, bool keep_a_value_segment = false) {
  const TableColumnDefinitions definitions{{"orderkey", DataType::Int, false}, {"extendedprice", DataType::Float, false}, {"discount", DataType::Float, false}, {"shipdate", DataType::String, true}};
  auto table = std::make_shared<Table>(definitions, TableType::Data, chunk_size);
  for (const auto& row : rows) table->append(row);
  table->finalize();
  const auto unencoded = table->chunk_count() > 1 ? table->get_chunk(ChunkID{1})->get_segment(SHIPDATE) : nullptr;
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  if (keep_a_value_segment && unencoded) table->get_chunk(ChunkID{1})->replace_segment(SHIPDATE, unencoded);
  return table;
}

static std::string cell(const AllTypeVariant& value) {
  return std::visit([](const auto& v) -> std::string {
    using T = std::decay_t<decltype(v)>;
    if constexpr (std::is_same_v<T, NullValue>) return "NULL";
    else if constexpr (std::is_same_v<T, std::string>) return "s" + v;
    else return std::to_string(v);
  }, value);
}

static bool same_rows(const Rows& got, const Rows& want) {
  if (got.size() != want.size()) return false;
  for (size_t r = 0; r < got.size(); ++r) {
    if (got[r].size() != want[r].size()) return false;
    for (size_t c = 0; c < got[r].size(); ++c) if (cell(got[r][c]) != cell(want[r][c])) return false;
  }
  return true;
}

static size_t device_string_segments(const std::shared_ptr<const Table>& table, ColumnID column) {
  size_t n = 0;
  for (ChunkID c = 0; c < table->chunk_count(); ++c) n += dynamic_cast<const DeviceStringDictionarySegment*>(table->get_chunk(c)->get_segment(column).get()) != nullptr;
  return n;
}

static AllTypeVariant substr_cell(const AllTypeVariant& value, int32_t start, int32_t length) {
  if (variant_is_null(value)) return value;
  return substr_of(std::get<std::string>(value), start, length);
}

// Projection(orderkey, SUBSTR(shipdate, start, length)) with the switch on and off, against substr_of over the rows
static void check_projection(const std::shared_ptr<const AbstractOperator>& input, const Rows& input_rows, int32_t start, int32_t length, bool device_expected) {
  const std::vector<ExpressionPtr> expressions{column_(ORDERKEY), substr_(column_(SHIPDATE), start, length)};
  device_string_results() = true;
  const auto on = executed<Projection>(input, expressions)->get_output();
  EXPECT_TRUE(on->chunk_count() > 0 && device_string_segments(on, ColumnID{1}) == (device_expected ? on->chunk_count() : 0));
  device_string_results() = false;
  std::shared_ptr<const Table> off;
  try { off = executed<Projection>(input, expressions)->get_output(); } catch (...) { device_string_results() = true; throw; }
  device_string_results() = true;
  EXPECT_TRUE(device_string_segments(off, ColumnID{1}) == 0);
  Rows want;
  for (const auto& row : input_rows) want.push_back(Row{row[ORDERKEY], substr_cell(row[SHIPDATE], start, length)});
  EXPECT_TRUE(on->column_data_type(ColumnID{1}) == DataType::String && on->chunk_count() == off->chunk_count());
  EXPECT_TRUE(same_rows(on->get_rows(), off->get_rows()));
  EXPECT_TRUE(same_rows(on->get_rows(), want));
}

static double as_double(const AllTypeVariant& value) {
  return std::visit([](const auto& v) -> double {
    using T = std::decay_t<decltype(v)>;
    if constexpr (std::is_arithmetic_v<T>) return static_cast<double>(v);
    else return std::nan("");
  }, value);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: substr_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const Rows rows = lineitem_rows();

  run("Substr.HostFormula", [&] {
    EXPECT_TRUE(substr_of("HELLO", 0, 2) == "H" && substr_of("HELLO", -1, 2) == "O" && substr_of("HELLO", -8, 1).empty() && substr_of("HELLO", -8, 5) == "HE");
    EXPECT_TRUE(substr_of("HELLO", 1, 2147483647) == "HELLO" && substr_of("HELLO", 2, 2147483647) == "ELLO" && substr_of("HELLO", 2147483647, 2147483647).empty());
    EXPECT_TRUE(substr_of("HELLO", -2147483647 - 1, 2147483647) == "HELL" && substr_of("HELLO", 3, 0).empty() && substr_of("", 1, 4).empty());   // (s = 5 - 2^31, e = 4)
  });
  run("Substr.ProjectionOverADataTable", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1000}, ChunkOffset{65535}}) {
      const auto input = wrap(make_table(rows, chunk_size));
      check_projection(input, rows, 1, 4, true);
      check_projection(input, rows, 6, 2, true);
    }
  });
  run("Substr.ProjectionOverATableScansOutput", [&] {
    const auto scan = executed<TableScan>(wrap(make_table(rows, ChunkOffset{700})), ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    Rows kept;
    for (const auto& row : rows) if (std::get<int32_t>(row[ORDERKEY]) > 3000) kept.push_back(row);
    EXPECT_TRUE(!kept.empty() && kept.size() < rows.size());
    check_projection(scan, kept, 1, 4, true);
    check_projection(scan, kept, 6, 2, true);
  });
  run("Substr.AValueSegmentChunkTakesTheHostPath", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{1000}, true));
    EXPECT_TRUE(dynamic_cast<const ValueSegment<std::string>*>(input->get_output()->get_chunk(ChunkID{1})->get_segment(SHIPDATE).get()) != nullptr);
    check_projection(input, rows, 1, 4, false);
    check_projection(input, rows, -5, 2, false);
  });
  run("Substr.OverAnythingButAColumnFails", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{1000}));
    const auto fails = [&](std::vector<ExpressionPtr> expressions) {
      try { executed<Projection>(input, std::move(expressions)); } catch (const std::exception&) { return true; }
      return false;
    };
    EXPECT_TRUE(fails({substr_(value_(std::string{"HELLO"}), 1, 2)}));
    EXPECT_TRUE(fails({substr_(column_(ORDERKEY), 1, 2)}));
    EXPECT_TRUE(fails({substr_(substr_(column_(SHIPDATE), 1, 4), 1, 2)}));
    EXPECT_TRUE(fails({is_null_(substr_(column_(SHIPDATE), 1, 4))}));
  });
  run("SubstrChain.ScanProjectAggregateSortWithoutAFetch", [&] {   // Q9's shape: SUM(l_extendedprice * (1 - l_discount)) GROUP BY SUBSTR(l_shipdate, 1, 4)
    const auto input = wrap(make_table(rows, ChunkOffset{1000}));
    const uint64_t string_fetches = device_string_segment_fetches().load(), value_fetches = device_value_segment_fetches().load();
    const auto scan = executed<TableScan>(input, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{1500}});
    const auto amount = arithmetic_(ArithmeticOperator::Multiplication, column_(EXTENDEDPRICE), arithmetic_(ArithmeticOperator::Subtraction, value_(1.0f), column_(DISCOUNT)));
    const auto projection = executed<Projection>(scan, std::vector<ExpressionPtr>{substr_(column_(SHIPDATE), 1, 4), amount});
    EXPECT_TRUE(device_string_segments(projection->get_output(), ColumnID{0}) == projection->get_output()->chunk_count());
    const auto aggregate = executed<AggregateHash>(projection, std::vector<AggregateDefinition>{AggregateDefinition{ColumnID{1}, WindowFunction::Sum}}, std::vector<ColumnID>{ColumnID{0}});
    const auto sort = executed<Sort>(aggregate, std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}});
    EXPECT_TRUE(device_string_segment_fetches().load() == string_fetches && device_value_segment_fetches().load() == value_fetches);
    const auto got = sort->get_output()->get_rows();
    EXPECT_TRUE(device_string_segment_fetches().load() > string_fetches);
    // row by row: the products in float as the column's type has them, summed in double; "NULL" orders first in the map as NULLS FIRST asks
    std::map<std::string, double> sums;
    for (const auto& row : rows) {
      if (std::get<int32_t>(row[ORDERKEY]) <= 1500) continue;
      const float product = std::get<float>(row[EXTENDEDPRICE]) * (1.0f - std::get<float>(row[DISCOUNT]));
      sums[cell(substr_cell(row[SHIPDATE], 1, 4))] += static_cast<double>(product);
    }
    EXPECT_TRUE(sums.size() == 8 && got.size() == sums.size());   // 1992 .. 1998 and NULL
    size_t r = 0;
    for (const auto& [year, sum] : sums) {
      if (r >= got.size()) break;
      EXPECT_TRUE(cell(got[r][0]) == year);
      // a double sum of a few thousand float products in another order: relative error below n * 2^-53 < 1e-12; 1e-9 leaves three digits of room
      EXPECT_TRUE(std::abs(as_double(got[r][1]) - sum) <= 1e-9 * std::abs(sum));
      ++r;
    }
  });

  std::printf(g_failures ? "SUBSTR TESTS FAILED: %d\n" : "SUBSTR TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

// string_forward_tests.cpp -- string columns behind PosLists through the C++ mirror (hyrise_amd/host/hyrise_host.hpp): a Projection that
// forwards a string column beside a computed one over a TableScan's output (device_string_results(): one hy_string_column_materialize,
// DeviceStringDictionarySegments) against the host loop (the switch off) cell for cell, both against the rows; the chain TableScan ->
// Projection -> AggregateHash (GROUP BY the forwarded string) -> Sort without a segment fetch before the final read; Sort with
// ForceMaterialization::Yes and a row limit of 20 over a table with a string payload column (hy_string_column_gather at the sorted positions);
// and a column with a ValueSegment<pmr_string> chunk on the host path.
// Usage: string_forward_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

static ExpressionPtr amount_() {
  return arithmetic_(ArithmeticOperator::Multiplication, column_(EXTENDEDPRICE), arithmetic_(ArithmeticOperator::Subtraction, value_(1.0f), column_(DISCOUNT)));
}

static double as_double(const AllTypeVariant& value) {
  return std::visit([](const auto& v) -> double {
    using T = std::decay_t<decltype(v)>;
    if constexpr (std::is_arithmetic_v<T>) return static_cast<double>(v);
    else return std::nan("");
  }, value);
}

// Projection(shipdate, extendedprice * (1 - discount)) over `input` with the switch on and off, against the rows
static void check_projection(const std::shared_ptr<const AbstractOperator>& input, const Rows& input_rows, bool device_expected) {
  const std::vector<ExpressionPtr> expressions{column_(SHIPDATE), amount_()};
  device_string_results() = true;
  const auto on = executed<Projection>(input, expressions)->get_output();
  EXPECT_TRUE(on->chunk_count() > 0 && device_string_segments(on, ColumnID{0}) == (device_expected ? on->chunk_count() : 0));
  device_string_results() = false;
  std::shared_ptr<const Table> off;
  try { off = executed<Projection>(input, expressions)->get_output(); } catch (...) { device_string_results() = true; throw; }
  device_string_results() = true;
  EXPECT_TRUE(device_string_segments(off, ColumnID{0}) == 0);
  EXPECT_TRUE(on->type() == TableType::Data && on->column_data_type(ColumnID{0}) == DataType::String && on->chunk_count() == off->chunk_count());
  EXPECT_TRUE(on->column_is_nullable(ColumnID{0}) && off->column_is_nullable(ColumnID{0}));
  const auto got = on->get_rows();
  EXPECT_TRUE(same_rows(got, off->get_rows()));
  EXPECT_TRUE(got.size() == input_rows.size());
  for (size_t r = 0; r < got.size() && r < input_rows.size(); ++r) {
    if (cell(got[r][0]) != cell(input_rows[r][SHIPDATE])) { EXPECT_TRUE(cell(got[r][0]) == cell(input_rows[r][SHIPDATE])); break; }
    const float product = std::get<float>(input_rows[r][EXTENDEDPRICE]) * (1.0f - std::get<float>(input_rows[r][DISCOUNT]));
    if (as_double(got[r][1]) != static_cast<double>(product)) { EXPECT_TRUE(as_double(got[r][1]) == static_cast<double>(product)); break; }   // (one float product: exact)
  }
}

// Sort by orderkey descending (ties: shipdate, then price, so that the order is total over the rows that matter), materialised, the first 20 rows
static void check_sort(const std::shared_ptr<const AbstractOperator>& input, Rows input_rows, bool device_expected) {
  const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{ORDERKEY, SortMode::DescendingNullsFirst}, SortColumnDefinition{EXTENDEDPRICE, SortMode::AscendingNullsFirst}};
  device_string_results() = true;
  const auto on = executed<Sort>(input, definitions, ChunkOffset{7}, Sort::ForceMaterialization::Yes, std::optional<uint64_t>{20})->get_output();
  EXPECT_TRUE(on->row_count() == 20 && on->chunk_count() == 3 && on->type() == TableType::Data);
  EXPECT_TRUE(device_string_segments(on, SHIPDATE) == (device_expected ? on->chunk_count() : 0));
  device_string_results() = false;
  std::shared_ptr<const Table> off;
  try { off = executed<Sort>(input, definitions, ChunkOffset{7}, Sort::ForceMaterialization::Yes, std::optional<uint64_t>{20})->get_output(); } catch (...) { device_string_results() = true; throw; }
  device_string_results() = true;
  EXPECT_TRUE(device_string_segments(off, SHIPDATE) == 0);
  EXPECT_TRUE(same_rows(on->get_rows(), off->get_rows()));
  std::stable_sort(input_rows.begin(), input_rows.end(), [](const Row& a, const Row& b) {
    if (std::get<int32_t>(a[ORDERKEY]) != std::get<int32_t>(b[ORDERKEY])) return std::get<int32_t>(a[ORDERKEY]) > std::get<int32_t>(b[ORDERKEY]);
    return std::get<float>(a[EXTENDEDPRICE]) < std::get<float>(b[EXTENDEDPRICE]);
  });
  input_rows.resize(std::min<size_t>(input_rows.size(), 20));
  EXPECT_TRUE(same_rows(on->get_rows(), input_rows));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: string_forward_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const Rows rows = lineitem_rows();
  Rows kept;
  for (const auto& row : rows) if (std::get<int32_t>(row[ORDERKEY]) > 3000) kept.push_back(row);

  run("Forward.ProjectionOverATableScansOutput", [&] {
    EXPECT_TRUE(!kept.empty() && kept.size() < rows.size());
    for (const ChunkOffset chunk_size : {ChunkOffset{700}, ChunkOffset{65535}}) {
      const auto scan = executed<TableScan>(wrap(make_table(rows, chunk_size)), ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
      check_projection(scan, kept, true);
    }
  });
  run("Forward.AValueSegmentChunkTakesTheHostPath", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{1000}, true));
    EXPECT_TRUE(dynamic_cast<const ValueSegment<std::string>*>(input->get_output()->get_chunk(ChunkID{1})->get_segment(SHIPDATE).get()) != nullptr);
    const auto scan = executed<TableScan>(input, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    check_projection(scan, kept, false);
    check_sort(input, rows, false);
  });
  run("Forward.SortMaterializesAStringPayloadAtTwentyRows", [&] {
    check_sort(wrap(make_table(rows, ChunkOffset{1000})), rows, true);
    const auto scan = executed<TableScan>(wrap(make_table(rows, ChunkOffset{700})), ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    check_sort(scan, kept, true);
  });
  run("ForwardChain.ScanProjectAggregateSortWithoutAFetch", [&] {   // Q1's shape: SUM(l_extendedprice * (1 - l_discount)) GROUP BY a forwarded string column
    const auto input = wrap(make_table(rows, ChunkOffset{1000}));
    const uint64_t string_fetches = device_string_segment_fetches().load(), value_fetches = device_value_segment_fetches().load();
    const auto scan = executed<TableScan>(input, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{1500}});
    const auto projection = executed<Projection>(scan, std::vector<ExpressionPtr>{column_(SHIPDATE), amount_()});
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
      sums[cell(row[SHIPDATE])] += static_cast<double>(product);
    }
    EXPECT_TRUE(sums.size() > 100 && got.size() == sums.size());   // (days, and NULL)
    size_t r = 0;
    for (const auto& [day, sum] : sums) {
      if (r >= got.size()) break;
      if (cell(got[r][0]) != day) { EXPECT_TRUE(cell(got[r][0]) == day); break; }
      // a double sum of at most a few thousand float products in another order: relative error below n * 2^-53 < 1e-12; 1e-9 leaves three digits of room
      if (!(std::abs(as_double(got[r][1]) - sum) <= 1e-9 * std::abs(sum))) { EXPECT_TRUE(std::abs(as_double(got[r][1]) - sum) <= 1e-9 * std::abs(sum)); break; }
      ++r;
    }
  });

  std::printf(g_failures ? "STRING FORWARD TESTS FAILED: %d\n" : "STRING FORWARD TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

// string_gather_tests.cpp -- AggregateHash's string outputs through the C++ mirror (hyrise_amd/host/hyrise_host.hpp): string GROUP BY columns
// and MIN / MAX / ANY over a string column, made in HBM (device_string_results(): hy_string_column_gather at the representative rows,
// hy_string_ranks_gather over the MIN / MAX of the rank stand-in) against the host path (the switch off) cell for cell, both against a
// row-by-row evaluation with std::string comparisons; and AggregateHash -> TableScan (LIKE) -> Sort without a DeviceStringDictionarySegment
// fetch before the final read.
// Usage: string_gather_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
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

// ORDERKEY int, LINENUMBER int, SHIPMODE string (7 distinct, NULL in every fifth row or so), COMMENT string (nearly every row its own)
static const ColumnID ORDERKEY{0}, LINENUMBER{1}, SHIPMODE{2}, COMMENT{3};

static Rows lineitem_rows() {
  const auto table = load_table(g_tbl + "/tpch/sf-0.001/lineitem.tbl", ChunkOffset{65535});
  Rows rows;
  for (const auto& row : table->get_rows()) {
    const int32_t orderkey = std::get<int32_t>(row[0]), linenumber = std::get<int32_t>(row[3]);
    rows.push_back(Row{orderkey, linenumber, (orderkey + linenumber) % 5 == 0 ? AllTypeVariant{NullValue{}} : row[14], row[15]});
  }
  return rows;
}

static std::shared_ptr<Table> make_table(const Rows& rows, ChunkOffset chunk_size) {
  const TableColumnDefinitions definitions{{"orderkey", DataType::Int, false}, {"linenumber", DataType::Int, false}, {"shipmode", DataType::String, true}, {"comment", DataType::String, false}};
  auto table = std::make_shared<Table>(definitions, TableType::Data, chunk_size);
  for (const auto& row : rows) table->append(row);
  table->finalize();
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
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

static std::vector<std::string> cells_of(const Row& row) {
  std::vector<std::string> out;
  for (const auto& value : row) out.push_back(cell(value));
  return out;
}

static bool same_rows(const Rows& got, const Rows& want) {
  if (got.size() != want.size()) return false;
  for (size_t r = 0; r < got.size(); ++r) if (cells_of(got[r]) != cells_of(want[r])) return false;
  return true;
}

static bool same_rows_in_any_order(const Rows& got, const Rows& want) {
  std::vector<std::vector<std::string>> a, b;
  for (const auto& row : got) a.push_back(cells_of(row));
  for (const auto& row : want) b.push_back(cells_of(row));
  std::sort(a.begin(), a.end());
  std::sort(b.begin(), b.end());
  return a == b;
}

// GROUP BY `groupby` with MIN / MAX / ANY / COUNT(*) aggregates, row by row: strings compared as std::string, NULLs skipped (a group without a
// value: NULL); ANY is only asked of a column that the group determines
static Rows evaluated(const Rows& rows, const std::vector<ColumnID>& groupby, const std::vector<AggregateDefinition>& aggregates) {
  std::map<std::vector<std::string>, Row> groups;
  std::vector<std::vector<std::string>> order;
  for (const auto& row : rows) {
    std::vector<std::string> key;
    for (const auto id : groupby) key.push_back(cell(row[id]));
    auto found = groups.find(key);
    if (found == groups.end()) {
      Row fresh;
      for (const auto id : groupby) fresh.push_back(row[id]);
      for (const auto& aggregate : aggregates) fresh.push_back(aggregate.function == WindowFunction::Count ? AllTypeVariant{int64_t{0}} : AllTypeVariant{NullValue{}});
      found = groups.emplace(key, std::move(fresh)).first;
      order.push_back(key);
    }
    for (size_t a = 0; a < aggregates.size(); ++a) {
      AllTypeVariant& slot = found->second[groupby.size() + a];
      if (aggregates[a].function == WindowFunction::Count) { slot = std::get<int64_t>(slot) + 1; continue; }
      const AllTypeVariant& value = row[aggregates[a].column_id];
      if (variant_is_null(value)) continue;
      if (variant_is_null(slot) || aggregates[a].function == WindowFunction::Any) { if (variant_is_null(slot)) slot = value; continue; }
      bool smaller = false;
      if (const auto* s = std::get_if<std::string>(&value)) smaller = *s < std::get<std::string>(slot);
      else smaller = std::get<int32_t>(value) < std::get<int32_t>(slot);
      const bool larger = !smaller && cell(value) != cell(slot);
      if (aggregates[a].function == WindowFunction::Min ? smaller : larger) slot = value;
    }
  }
  Rows out;
  for (const auto& key : order) out.push_back(groups[key]);
  return out;
}

// how many of a table's segments of `column` are DeviceStringDictionarySegments
static size_t device_string_segments(const std::shared_ptr<const Table>& table, ColumnID column) {
  size_t n = 0;
  for (ChunkID c = 0; c < table->chunk_count(); ++c) n += dynamic_cast<const DeviceStringDictionarySegment*>(table->get_chunk(c)->get_segment(column).get()) != nullptr;
  return n;
}

struct Case {
  std::vector<ColumnID> groupby;
  std::vector<AggregateDefinition> aggregates;
  std::vector<ColumnID> string_outputs;   // output columns that hold strings
};

static std::vector<Case> cases() {
  const auto agg = [](ColumnID column, WindowFunction function) { return AggregateDefinition{column, function}; };
  return {
      {{SHIPMODE}, {agg(COMMENT, WindowFunction::Min), agg(COMMENT, WindowFunction::Max), agg(SHIPMODE, WindowFunction::Any), agg(INVALID_COLUMN_ID, WindowFunction::Count)}, {0, 1, 2}},
      {{COMMENT}, {agg(SHIPMODE, WindowFunction::Min), agg(SHIPMODE, WindowFunction::Max), agg(COMMENT, WindowFunction::Any), agg(ORDERKEY, WindowFunction::Min)}, {0, 1, 2, 3}},
      {{SHIPMODE, LINENUMBER}, {agg(COMMENT, WindowFunction::Max), agg(ORDERKEY, WindowFunction::Max)}, {0, 2}},
      {{ORDERKEY}, {agg(COMMENT, WindowFunction::Min), agg(SHIPMODE, WindowFunction::Max)}, {1, 2}},
      {{}, {agg(COMMENT, WindowFunction::Min), agg(SHIPMODE, WindowFunction::Max)}, {0, 1}},
  };
}

static void check_case(const std::shared_ptr<const AbstractOperator>& input, const Rows& input_rows, const Case& c) {
  const auto want = evaluated(input_rows, c.groupby, c.aggregates);
  device_string_results() = true;
  const auto on = executed<AggregateHash>(input, c.aggregates, c.groupby)->get_output();
  for (const auto column : c.string_outputs) EXPECT_TRUE(on->chunk_count() > 0 && device_string_segments(on, column) == on->chunk_count());
  device_string_results() = false;
  std::shared_ptr<const Table> off;
  try { off = executed<AggregateHash>(input, c.aggregates, c.groupby)->get_output(); } catch (...) { device_string_results() = true; throw; }
  device_string_results() = true;
  for (const auto column : c.string_outputs) EXPECT_TRUE(device_string_segments(off, column) == 0);
  const auto on_rows = on->get_rows(), off_rows = off->get_rows();
  EXPECT_TRUE(on->column_count() == off->column_count() && same_rows(on_rows, off_rows));   // cell for cell, the groups in the same order
  EXPECT_TRUE(same_rows_in_any_order(on_rows, want));
  EXPECT_TRUE(same_rows_in_any_order(off_rows, want));
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: string_gather_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const Rows rows = lineitem_rows();

  run("StringGather.AggregateOverADataTable", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1000}, ChunkOffset{65535}}) {
      for (const auto& c : cases()) check_case(wrap(make_table(rows, chunk_size)), rows, c);
    }
  });
  run("StringGather.AggregateOverATableScansOutput", [&] {
    const auto scan = executed<TableScan>(wrap(make_table(rows, ChunkOffset{700})), ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    Rows kept;
    for (const auto& row : rows) if (std::get<int32_t>(row[ORDERKEY]) > 3000) kept.push_back(row);
    EXPECT_TRUE(!kept.empty() && kept.size() < rows.size());
    for (const auto& c : cases()) check_case(scan, kept, c);
  });
  run("StringGather.HostRanksKeepTheHostPath", [&] {   // device_string_ranking() off: int64 ranks, which hy_string_ranks_gather does not take
    device_string_ranking() = false;
    try {
      const auto c = cases()[3];
      const auto input = wrap(make_table(rows, ChunkOffset{1000}));
      const auto got = executed<AggregateHash>(input, c.aggregates, c.groupby)->get_output();
      EXPECT_TRUE(device_string_segments(got, ColumnID{1}) == 0 && same_rows_in_any_order(got->get_rows(), evaluated(rows, c.groupby, c.aggregates)));
    } catch (...) { device_string_ranking() = true; throw; }
    device_string_ranking() = true;
  });
  run("StringGatherChain.AggregateLikeScanSortWithoutAFetch", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{1000}));
    const std::vector<AggregateDefinition> aggregates{AggregateDefinition{SHIPMODE, WindowFunction::Min}, AggregateDefinition{INVALID_COLUMN_ID, WindowFunction::Count}};
    const uint64_t string_fetches = device_string_segment_fetches().load(), value_fetches = device_value_segment_fetches().load();
    const auto aggregate = executed<AggregateHash>(input, aggregates, std::vector<ColumnID>{COMMENT});
    const auto scan = executed<TableScan>(aggregate, ColumnID{0}, PredicateCondition::Like, AllTypeVariant{std::string{"%the%"}});
    const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{ColumnID{0}, SortMode::DescendingNullsFirst}};
    const auto sort = executed<Sort>(scan, definitions);
    EXPECT_TRUE(device_string_segment_fetches().load() == string_fetches && device_value_segment_fetches().load() == value_fetches);
    const auto got = sort->get_output()->get_rows();
    EXPECT_TRUE(device_string_segment_fetches().load() > string_fetches);
    Rows want;
    for (const auto& row : evaluated(rows, {COMMENT}, aggregates)) if (std::get<std::string>(row[0]).find("the") != std::string::npos) want.push_back(row);
    std::stable_sort(want.begin(), want.end(), [](const Row& a, const Row& b) { return std::get<std::string>(a[0]) > std::get<std::string>(b[0]); });
    EXPECT_TRUE(want.size() > 10 && same_rows(got, want));   // (one group per comment: no ties)
  });

  std::printf(g_failures ? "STRING GATHER TESTS FAILED: %d\n" : "STRING GATHER TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

// aggregate_columns_tests.cpp -- the C++ mirror's AggregateHash with its output table in HBM (hy_aggregate_hash_columns, DeviceValueSegment;
// hyrise_amd/host/hyrise_host.hpp) against the same operator with device_resident_results(false):
//   the aggregate_test.cpp fixture pairs of tests/golden/tbl/aggregateoperator: equal cell by cell, column definitions and chunk sizes included
//   TableScan -> JoinHash -> AggregateHash -> TableScan (HAVING) -> Sort with a row limit over generated tables: the same ten rows, and no
//   DeviceValueSegment fetches its chunk to the host before the test reads them
//   device_column_of_chunks over a part of the aggregate's output chunks: the fallback through the chunks' host copies
// Usage: aggregate_columns_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
//        aggregate_columns_tests --chain-bench STEPS [ORDERS]: timing only (tools/aggregate_columns_bench.py, case B)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
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

static bool cells_identical(const AllTypeVariant& a, const AllTypeVariant& b) {
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

// the device-resident result against the host result of the same build: the same kernels computed both, so cells are compared exactly
static bool tables_identical(const std::shared_ptr<const Table>& got, const std::shared_ptr<const Table>& want) {
  if (got->column_count() != want->column_count() || got->type() != want->type()) { std::printf("  column counts or table types differ\n"); return false; }
  for (ColumnID c = 0; c < got->column_count(); ++c) {
    if (got->column_name(c) != want->column_name(c) || got->column_data_type(c) != want->column_data_type(c) || got->column_is_nullable(c) != want->column_is_nullable(c)) {
      std::printf("  column %u: definitions differ\n", c);
      return false;
    }
  }
  if (got->chunk_count() != want->chunk_count()) { std::printf("  chunk counts differ: %u vs %u\n", got->chunk_count(), want->chunk_count()); return false; }
  for (ChunkID k = 0; k < got->chunk_count(); ++k) {
    if (got->get_chunk(k)->size() != want->get_chunk(k)->size()) { std::printf("  chunk %u: sizes differ\n", k); return false; }
    for (ColumnID c = 0; c < got->column_count(); ++c) {
      for (ChunkOffset r = 0; r < got->get_chunk(k)->size(); ++r) {
        if (!cells_identical((*got->get_chunk(k)->get_segment(c))[r], (*want->get_chunk(k)->get_segment(c))[r])) { std::printf("  chunk %u column %u row %u differs\n", k, c, r); return false; }
      }
    }
  }
  return true;
}

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

static void test_fixtures_resident_against_host() {   // aggregate_test.cpp: test_output<>(input, aggregates, group by, expected)
  struct Case { std::string input; std::vector<AggregateDefinition> aggregates; std::vector<ColumnID> groupby; };
  const std::string d1 = "aggregateoperator/groupby_int_1gb_1agg/", d2 = "aggregateoperator/groupby_int_1gb_2agg/", d21 = "aggregateoperator/groupby_int_2gb_1agg/",
                    s = "aggregateoperator/groupby_string_1gb_1agg/";
  const std::vector<Case> cases = {
      {d1 + "input.tbl", {{1, WindowFunction::Max}}, {0}}, {d1 + "input.tbl", {{1, WindowFunction::Min}}, {0}}, {d1 + "input.tbl", {{1, WindowFunction::Sum}}, {0}},
      {d1 + "input.tbl", {{1, WindowFunction::Avg}}, {0}}, {d1 + "input.tbl", {{1, WindowFunction::Count}}, {0}}, {d1 + "input_null.tbl", {{1, WindowFunction::Sum}}, {0}},
      {d1 + "input_null.tbl", {{1, WindowFunction::Avg}}, {0}}, {d1 + "input_null.tbl", {{INVALID_COLUMN_ID, WindowFunction::Count}}, {0}},
      {d1 + "input.tbl", {{1, WindowFunction::StandardDeviationSample}, {1, WindowFunction::CountDistinct}, {1, WindowFunction::Any}}, {0}},
      {d1 + "input.tbl", {{1, WindowFunction::Sum}, {INVALID_COLUMN_ID, WindowFunction::Count}}, {}}, {d1 + "input.tbl", {{INVALID_COLUMN_ID, WindowFunction::Count}}, {}},
      {d2 + "input.tbl", {{1, WindowFunction::Max}, {2, WindowFunction::Avg}}, {0}}, {d2 + "input.tbl", {{1, WindowFunction::Sum}, {2, WindowFunction::Sum}}, {0}},
      {d21 + "input.tbl", {{2, WindowFunction::Max}}, {0, 1}}, {d21 + "input.tbl", {{2, WindowFunction::Sum}}, {0, 1}}, {d21 + "input.tbl", {}, {0, 1}},
      {s + "input.tbl", {{1, WindowFunction::Sum}}, {0}}, {s + "input.tbl", {{1, WindowFunction::Avg}}, {0}}, {s + "input.tbl", {{1, WindowFunction::Min}}, {0, 1}},
  };
  for (const auto encoding : {EncodingType::Unencoded, EncodingType::Dictionary}) {
    for (const auto& c : cases) {
      if (encoding == EncodingType::Unencoded && c.input.find("string") != std::string::npos) continue;   // unencoded strings: CPU path
      std::shared_ptr<const Table> tables[2];
      for (const bool resident : {true, false}) {
        const ResidentResults scope(resident);
        auto table = load_table(g_tbl + "/" + c.input, 2);
        ChunkEncoder::encode_all_chunks(table, encoding);
        auto aggregate = std::make_shared<AggregateHash>(wrap(table), c.aggregates, c.groupby);
        aggregate->execute();
        tables[resident ? 0 : 1] = aggregate->get_output();
      }
      const bool ok = tables_identical(tables[0], tables[1]);
      if (!ok) std::printf("  case %s, %zu aggregates, %zu GROUP BY columns\n", c.input.c_str(), c.aggregates.size(), c.groupby.size());
      EXPECT_TRUE(ok);
      EXPECT_TRUE(tables[0]->row_count() > 0);
    }
  }
}

// 200 000 fact rows over 50 000 keys in chunks of 4 096 rows: several chunks everywhere, and an aggregate finished on the device
static std::shared_ptr<Table> generated_table(size_t rows, const std::function<int32_t(size_t)>& first, const std::function<int32_t(size_t)>& second, const char* second_name) {
  auto table = std::make_shared<Table>(TableColumnDefinitions{{"key", DataType::Int, false}, {second_name, DataType::Int, false}}, TableType::Data, ChunkOffset{4096});
  for (size_t begin = 0; begin < rows; begin += 4096) {
    const size_t size = std::min<size_t>(4096, rows - begin);
    std::vector<int32_t> a(size), b(size);
    for (size_t i = 0; i < size; ++i) { a[i] = first(begin + i); b[i] = second(begin + i); }
    table->append_chunk({std::make_shared<ValueSegment<int32_t>>(std::move(a), std::nullopt), std::make_shared<ValueSegment<int32_t>>(std::move(b), std::nullopt)});
  }
  return table;
}
static std::shared_ptr<Table> fact_table() {
  return generated_table(200'000, [](size_t i) { return static_cast<int32_t>((i * 7919) % 50'000); }, [](size_t i) { return static_cast<int32_t>((i * 31) % 1000); }, "value");
}
static std::shared_ptr<Table> key_table() {
  return generated_table(50'000, [](size_t i) { return static_cast<int32_t>(i); }, [](size_t i) { return static_cast<int32_t>(i % 3); }, "flag");
}

struct Chain {
  std::shared_ptr<const Table> aggregated, result;
};
// TableScan -> JoinHash -> AggregateHash (GROUP BY key, SUM(value), COUNT(*)) -> TableScan (SUM > 1500) -> Sort (SUM DESC, key) with row_limit 10
static Chain run_chain() {
  auto scan = std::make_shared<TableScan>(wrap(fact_table()), ColumnID{1}, PredicateCondition::GreaterThanEquals, AllTypeVariant{int32_t{100}});
  scan->execute();
  auto join = std::make_shared<JoinHash>(scan, wrap(key_table()), JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
  join->execute();
  auto aggregate = std::make_shared<AggregateHash>(join, std::vector<AggregateDefinition>{{ColumnID{1}, WindowFunction::Sum}, {INVALID_COLUMN_ID, WindowFunction::Count}}, std::vector<ColumnID>{ColumnID{0}});
  aggregate->execute();
  auto having = std::make_shared<TableScan>(aggregate, ColumnID{1}, PredicateCondition::GreaterThan, AllTypeVariant{int64_t{1500}});
  having->execute();
  auto sort = std::make_shared<Sort>(having, std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst}, SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}}, Chunk::DEFAULT_SIZE,
                                     Sort::ForceMaterialization::No, uint64_t{10});
  sort->execute();
  return Chain{aggregate->get_output(), sort->get_output()};
}

static void test_chain_stays_in_hbm() {
  const uint64_t fetches_before = device_value_segment_fetches().load();
  Chain resident;
  {
    const ResidentResults scope(true);
    resident = run_chain();
  }
  EXPECT_TRUE(device_value_segment_fetches().load() == fetches_before);   // nothing of the aggregate's columns has crossed to the host
  EXPECT_TRUE(resident.aggregated->row_count() > 4096);                     // (more than STAGED_GROUPS groups: the device finish)
  EXPECT_TRUE(dynamic_cast<const DeviceValueSegment<int64_t>*>(resident.aggregated->get_chunk(0)->get_segment(1).get()) != nullptr);
  EXPECT_TRUE(dynamic_cast<const DeviceValueSegment<int32_t>*>(resident.aggregated->get_chunk(0)->get_segment(0).get()) != nullptr);
  Chain host;
  {
    const ResidentResults scope(false);
    host = run_chain();
  }
  EXPECT_TRUE(resident.result->row_count() == 10 && host.result->row_count() == 10);
  const auto got = resident.result->get_rows(), want = host.result->get_rows();   // (the final ten rows: read through the DeviceValueSegments)
  for (size_t r = 0; r < got.size() && r < want.size(); ++r) {
    EXPECT_TRUE(got[r].size() == want[r].size());
    for (size_t c = 0; c < got[r].size() && c < want[r].size(); ++c) EXPECT_TRUE(cells_identical(got[r][c], want[r][c]));
  }
  EXPECT_TRUE(device_value_segment_fetches().load() > fetches_before);
  EXPECT_TRUE(tables_identical(resident.aggregated, host.aggregated));
}

static void test_partial_chunk_range() {
  // 70 000 groups: two output chunks (65 535 + 4 465); a column made of the second chunk alone is no whole hy_column and goes through the
  // chunk's host copy
  const ResidentResults scope(true);
  auto table = generated_table(140'000, [](size_t i) { return static_cast<int32_t>(i % 70'000); }, [](size_t i) { return static_cast<int32_t>(i % 977); }, "value");
  auto aggregate = std::make_shared<AggregateHash>(wrap(table), std::vector<AggregateDefinition>{{ColumnID{1}, WindowFunction::Sum}}, std::vector<ColumnID>{ColumnID{0}});
  aggregate->execute();
  const auto output = aggregate->get_output();
  EXPECT_TRUE(output->chunk_count() == 2 && output->get_chunk(1)->size() == 70'000 - 65'535);
  const auto whole = device_column_of_chunks(output, ColumnID{1}, StringKeys::None, 0, 2);
  EXPECT_TRUE(whole->resident != nullptr);
  const uint64_t fetches_before = device_value_segment_fetches().load();
  const auto part = device_column_of_chunks(output, ColumnID{1}, StringKeys::None, 1, 2);
  EXPECT_TRUE(part->resident == nullptr && device_value_segment_fetches().load() == fetches_before + 1);
  hy_predicate predicate{};
  predicate.condition = HY_PRED_GREATER_THAN;
  predicate.value_type = HY_TYPE_LONG;
  predicate.value.i64 = 1000;
  const uint32_t rows = output->get_chunk(1)->size();
  std::vector<hy_row_id> matches(rows);
  uint64_t offsets[2] = {0, 0};
  uint32_t counts[1] = {0};
  uint8_t states[1] = {0};
  hy_scan_result result{};
  result.mem = HY_MEM_HOST;
  result.matches = matches.data();
  result.capacity = rows;
  result.offsets = offsets;
  result.counts = counts;
  result.chunk_state = states;
  check_status(hy_table_scan(part->handle, &predicate, nullptr, 0, &result));
  std::vector<uint32_t> want;
  for (ChunkOffset r = 0; r < rows; ++r) {
    const auto cell = (*output->get_chunk(1)->get_segment(1))[r];
    if (!variant_is_null(cell) && std::get<int64_t>(cell) > 1000) want.push_back(r);
  }
  EXPECT_TRUE(offsets[1] == want.size() && !want.empty() && want.size() < rows);
  for (size_t i = 0; i < want.size() && i < offsets[1]; ++i) EXPECT_TRUE(matches[i].chunk_id == 0 && matches[i].chunk_offset == want[i]);
}

// ---- --chain-bench STEPS [ORDERS]: case B of tools/aggregate_columns_bench.py -----------------------------------------------------------
// AggregateHash (GROUP BY l_orderkey, SUM(l_quantity), COUNT(*)) -> TableScan (HAVING SUM > 300) -> Sort (SUM DESC, l_orderkey) with row_limit
// 100 over an SF10-shaped lineitem (one to seven lines per order, quantities 1 .. 50), device-resident results against
// device_resident_results(false) in alternating pairs; one line per pair and a summary.  The inputs' device columns are cached by the table.
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int chain_bench(int steps, uint64_t n_orders) {
  auto lineitem = std::make_shared<Table>(TableColumnDefinitions{{"l_orderkey", DataType::Int, false}, {"l_quantity", DataType::Int, false}}, TableType::Data, Chunk::DEFAULT_SIZE);
  std::vector<int32_t> keys, quantities;
  uint64_t state = 42, rows = 0;
  const auto next = [&] { state = state * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(state >> 33); };
  const auto flush = [&] {
    if (keys.empty()) return;
    lineitem->append_chunk({std::make_shared<ValueSegment<int32_t>>(std::move(keys), std::nullopt), std::make_shared<ValueSegment<int32_t>>(std::move(quantities), std::nullopt)});
    keys.clear(); quantities.clear();
  };
  for (uint64_t o = 0; o < n_orders; ++o) {
    const uint32_t lines = 1 + next() % 7;
    for (uint32_t l = 0; l < lines; ++l, ++rows) {
      keys.push_back(static_cast<int32_t>((o / 8) * 32 + o % 8 + 1));   // dbgen's sparse order keys
      quantities.push_back(static_cast<int32_t>(1 + next() % 50));
      if (keys.size() == Chunk::DEFAULT_SIZE) flush();
    }
  }
  flush();
  const auto input = wrap(lineitem);
  const auto chain = [&](bool resident) {
    const ResidentResults scope(resident);
    const double t0 = now_ms();
    auto aggregate = std::make_shared<AggregateHash>(input, std::vector<AggregateDefinition>{{ColumnID{1}, WindowFunction::Sum}, {INVALID_COLUMN_ID, WindowFunction::Count}}, std::vector<ColumnID>{ColumnID{0}});
    aggregate->execute();
    const double t1 = now_ms();
    auto having = std::make_shared<TableScan>(aggregate, ColumnID{1}, PredicateCondition::GreaterThan, AllTypeVariant{int64_t{300}});
    having->execute();
    auto sort = std::make_shared<Sort>(having, std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst}, SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}},
                                       Chunk::DEFAULT_SIZE, Sort::ForceMaterialization::No, uint64_t{100});
    sort->execute();
    const auto rows_out = sort->get_output()->get_rows();   // (the hundred rows are read: the device-resident form fetches their chunks here)
    const double t2 = now_ms();
    return std::make_tuple(t2 - t0, t1 - t0, aggregate->get_output()->row_count(), rows_out);
  };
  const auto warm_resident = chain(true), warm_host = chain(false);
  bool same = std::get<3>(warm_resident).size() == std::get<3>(warm_host).size();
  for (size_t r = 0; same && r < std::get<3>(warm_host).size(); ++r)
    for (size_t c = 0; same && c < std::get<3>(warm_host)[r].size(); ++c) same = cells_identical(std::get<3>(warm_resident)[r][c], std::get<3>(warm_host)[r][c]);
  std::printf("case B: %llu rows, %llu groups, %zu result rows, device-resident == host-result: %s\n", static_cast<unsigned long long>(rows),
              static_cast<unsigned long long>(std::get<2>(warm_host)), std::get<3>(warm_host).size(), same ? "yes" : "NO");
  std::vector<double> resident_ms, host_ms, resident_aggregate_ms, host_aggregate_ms;
  int faster = 0;
  for (int step = 0; step < steps; ++step) {
    const bool resident_first = step % 2 == 0;
    const auto first = chain(resident_first), second = chain(!resident_first);
    const auto& r = resident_first ? first : second;
    const auto& h = resident_first ? second : first;
    resident_ms.push_back(std::get<0>(r)); host_ms.push_back(std::get<0>(h));
    resident_aggregate_ms.push_back(std::get<1>(r)); host_aggregate_ms.push_back(std::get<1>(h));
    faster += std::get<0>(r) < std::get<0>(h);
    std::printf("  pair %d: device-resident %9.2f ms (AggregateHash %9.2f)   host results %9.2f ms (AggregateHash %9.2f)\n", step, std::get<0>(r), std::get<1>(r), std::get<0>(h), std::get<1>(h));
    std::fflush(stdout);
  }
  const auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; };
  std::printf("  median of %d: device-resident %.2f ms (AggregateHash %.2f), host results %.2f ms (AggregateHash %.2f): %.2f x; device-resident faster in %d/%d pairs\n", steps,
              median(resident_ms), median(resident_aggregate_ms), median(host_ms), median(host_aggregate_ms), median(host_ms) / std::max(1e-9, median(resident_ms)), faster, steps);
  return same ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc >= 3 && std::string(argv[1]) == "--chain-bench") {
    check_status(hy_init(0));
    const int rc = chain_bench(std::atoi(argv[2]), argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 15'000'000ull);
    hy_shutdown();
    return rc;
  }
  if (argc < 2) { std::printf("usage: aggregate_columns_tests <tests/golden/tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  run("AggregateHash: device-resident output == host output (aggregate_test.cpp fixtures)", test_fixtures_resident_against_host);
  run("scan -> join -> aggregate -> scan -> sort/limit stays in HBM", test_chain_stays_in_hbm);
  run("device_column_of_chunks over a partial chunk range", test_partial_chunk_range);
  hy_shutdown();
  std::printf(g_failures == 0 ? "AGGREGATE COLUMNS TESTS PASSED\n" : "AGGREGATE COLUMNS TESTS FAILED (%d)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}

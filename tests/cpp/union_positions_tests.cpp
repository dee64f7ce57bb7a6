// union_positions_tests.cpp -- the reference's UnionPositions tests (src/test/lib/operators/union_positions_test.cpp), re-stated against the
// C++ mirror's UnionPositions (hyrise_amd/host/hyrise_host.hpp), which unions on the device through hy_union_positions: the nine cases
// (GetTable becomes TableWrapper; the JoinNestedLoop of MultipleReferencedTables becomes JoinHash, the comparison is unordered), the PosList
// sharing check, both early results and both error cases -- plus UnionAll, and a chain TableScan u TableScan -> AggregateHash / -> Sort
// whose PosLists stay in HBM against the same chain with host PosLists.
// Usage: union_positions_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
#include <cmath>
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

static double as_double(const AllTypeVariant& v) {
  switch (v.index()) { case 1: return static_cast<double>(std::get<int32_t>(v)); case 2: return static_cast<double>(std::get<int64_t>(v));
                       case 3: return static_cast<double>(std::get<float>(v)); default: return std::get<double>(v); }
}

// EXPECT_TABLE_EQ_UNORDERED (check_table_equal.cpp): the same column definitions and the same multiset of rows
static bool tables_equal_unordered(const std::shared_ptr<const Table>& got, const std::shared_ptr<const Table>& want) {
  if (!same_column_definitions(*got, *want)) { std::printf("  column definitions differ\n"); return false; }
  const auto key = [](const std::vector<AllTypeVariant>& row) {
    std::vector<double> k;
    for (const auto& cell : row) k.push_back(variant_is_null(cell) ? -1e300 : as_double(cell));
    return k;
  };
  std::vector<std::vector<double>> a, b;
  for (const auto& row : got->get_rows()) a.push_back(key(row));
  for (const auto& row : want->get_rows()) b.push_back(key(row));
  if (a.size() != b.size()) { std::printf("  row counts differ: %zu vs %zu\n", a.size(), b.size()); return false; }
  std::sort(a.begin(), a.end());
  std::sort(b.begin(), b.end());
  for (size_t r = 0; r < a.size(); ++r)
    for (size_t c = 0; c < a[r].size(); ++c)
      if (std::fabs(a[r][c] - b[r][c]) > 1e-4 * std::max(1.0, std::fabs(b[r][c]))) { std::printf("  sorted row %zu column %zu differs: %f vs %f\n", r, c, a[r][c], b[r][c]); return false; }
  return true;
}

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

static bool throws_logic_error(const std::function<void()>& f) {
  try { f(); } catch (const std::logic_error&) { return true; }
  return false;
}

static void run(const std::string& name, const std::function<void()>& test) {
  const int before = g_failures;
  try { test(); } catch (const std::exception& e) { std::printf("  EXCEPTION: %s\n", e.what()); ++g_failures; }
  std::printf("[%s] %s\n", g_failures == before ? "  OK  " : "FAILED", name.c_str());
}

static std::shared_ptr<Table> g_10_ints, g_int_float4, g_int_int;   // SetUp (:26-39): chunks of 3, 3 and 2 rows
static const auto LT = PredicateCondition::LessThan;
static const auto GT = PredicateCondition::GreaterThan;

static std::shared_ptr<const AbstractPosList> pos_list_of(const std::shared_ptr<const Table>& table, ColumnID column_id) {
  return std::dynamic_pointer_cast<const ReferenceSegment>(table->get_chunk(0)->get_segment(column_id))->pos_list();
}

static std::shared_ptr<RowIDPosList> rows(std::vector<RowID> init) { return std::make_shared<RowIDPosList>(std::move(init)); }

static void multiple_shuffled_pos_list() {   // :228-316: two clusters (a, b | c), two chunks per side, no order, duplicates
  const auto l00 = rows({{1, 2}, {0, 1}, {1, 2}}), l10 = rows({{2, 0}, {0, 1}});
  const auto l01 = rows({{2, 0}, {1, 1}, {1, 1}}), l11 = rows({{1, 0}, {2, 0}});
  const auto r00 = rows({{2, 0}, {2, 0}, {1, 2}, {1, 0}}), r10 = rows({{0, 0}, {2, 0}});
  const auto r01 = rows({{1, 0}, {1, 0}, {2, 0}, {0, 0}}), r11 = rows({{1, 0}, {1, 0}});
  const TableColumnDefinitions definitions{{"a", DataType::Int, false}, {"b", DataType::Float, false}, {"c", DataType::Int, false}};
  const auto table_of = [&](const std::vector<std::pair<std::shared_ptr<RowIDPosList>, std::shared_ptr<RowIDPosList>>>& chunks) {
    auto table = std::make_shared<Table>(definitions, TableType::References);
    for (const auto& [ab, c] : chunks)
      table->append_chunk(Segments{std::make_shared<ReferenceSegment>(g_int_float4, 0, ab), std::make_shared<ReferenceSegment>(g_int_float4, 1, ab), std::make_shared<ReferenceSegment>(g_10_ints, 0, c)});
    return table;
  };
  const auto left = wrap(table_of({{l00, l01}, {l10, l11}})), right = wrap(table_of({{r00, r01}, {r10, r11}}));
  const auto set_union = executed<UnionPositions>(left, right);
  EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), load_table(g_tbl + "/union_positions/union_positions_multiple_shuffled_pos_list.tbl")));
  EXPECT_TRUE(set_union->path() == 3);
  const auto output = set_union->get_output();
  EXPECT_TRUE(pos_list_of(output, 0) == pos_list_of(output, 1));
  EXPECT_TRUE(pos_list_of(output, 0) != pos_list_of(output, 2));
}

// WHERE a > 20 OR a < 100 over a table of `n` rows in chunks of 1 000, then COUNT(*) / SUM(a) GROUP BY b and ORDER BY a
static void chain(bool on_device, std::vector<std::vector<AllTypeVariant>>& aggregated, std::vector<std::vector<AllTypeVariant>>& sorted, uint32_t& path) {
  device_resident_results() = on_device;
  auto table = std::make_shared<Table>(TableColumnDefinitions{{"a", DataType::Int, false}, {"b", DataType::Int, false}}, TableType::Data, ChunkOffset{1000});
  uint32_t state = 12345;
  for (int r = 0; r < 150000; ++r) {
    state = state * 1664525u + 1013904223u;
    table->append({int32_t(state >> 8) % 100000, int32_t(r % 7)});
  }
  table->finalize();
  const auto input = wrap(table);
  const auto p = executed<TableScan>(input, ColumnID{0}, GT, AllTypeVariant{int32_t{60000}});
  const auto q = executed<TableScan>(input, ColumnID{0}, LT, AllTypeVariant{int32_t{70000}});
  const auto set_union = executed<UnionPositions>(p, q);
  path = set_union->path();
  EXPECT_TRUE(set_union->get_output()->row_count() == 150000);
  const bool lists_on_device = dynamic_cast<const DevicePosList*>(pos_list_of(set_union->get_output(), 0).get()) != nullptr;
  EXPECT_TRUE(lists_on_device == on_device);
  const auto aggregate = executed<AggregateHash>(set_union, std::vector<AggregateDefinition>{{INVALID_COLUMN_ID, WindowFunction::Count}, {ColumnID{0}, WindowFunction::Sum}}, std::vector<ColumnID>{ColumnID{1}});
  aggregated = aggregate->get_output()->get_rows();
  const auto narrow = executed<TableScan>(set_union, ColumnID{0}, LT, AllTypeVariant{int32_t{500}});
  const auto sort = executed<Sort>(narrow, std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}, SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst}});
  sorted = sort->get_output()->get_rows();
  device_resident_results() = true;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: union_positions_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  g_10_ints = load_table(g_tbl + "/union_positions/10_ints.tbl", ChunkOffset{3});
  g_int_float4 = load_table(g_tbl + "/int_float4.tbl", ChunkOffset{3});
  g_int_int = load_table(g_tbl + "/union_positions/int_int.tbl", ChunkOffset{2});
  const auto ints = wrap(g_10_ints), int_float4 = wrap(g_int_float4), int_int = wrap(g_int_int);
  const auto int32 = [](int32_t v) { return AllTypeVariant{v}; };

  run("UnionPositionsTest.SelfUnionSimple", [&] {   // :46-70
    const auto a = executed<TableScan>(ints, ColumnID{0}, GT, int32(24)), b = executed<TableScan>(ints, ColumnID{0}, GT, int32(24));
    EXPECT_TRUE(a->get_output()->row_count() == 4 && b->get_output()->row_count() == 4);
    const auto set_union = executed<UnionPositions>(a, b);
    EXPECT_TRUE(tables_equal_unordered(a->get_output(), set_union->get_output()));
    EXPECT_TRUE(set_union->path() == 0);   // two scans of a data table arrive in order
  });
  run("UnionPositionsTest.SelfUnionExlusiveRanges", [&] {   // :72-90
    const auto set_union = executed<UnionPositions>(executed<TableScan>(ints, ColumnID{0}, LT, int32(10)), executed<TableScan>(ints, ColumnID{0}, GT, int32(200)));
    EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), load_table(g_tbl + "/union_positions/10_ints_exclusive_ranges.tbl")));
  });
  run("UnionPositionsTest.SelfUnionOverlappingRanges", [&] {   // :92-110
    const auto set_union = executed<UnionPositions>(executed<TableScan>(ints, ColumnID{0}, GT, int32(20)), executed<TableScan>(ints, ColumnID{0}, LT, int32(100)));
    EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), g_10_ints));
  });
  run("UnionPositionsTest.EarlyResultLeft", [&] {   // :112-133
    const auto a = executed<TableScan>(int_float4, ColumnID{0}, LT, int32(12346)), b = executed<TableScan>(int_float4, ColumnID{0}, LT, int32(0));
    const auto set_union = executed<UnionPositions>(a, b);
    EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), load_table(g_tbl + "/int_float2.tbl")));
    EXPECT_TRUE(a->get_output() == set_union->get_output());   // the same table object
  });
  run("UnionPositionsTest.EarlyResultRight", [&] {   // :135-154
    const auto a = executed<TableScan>(int_float4, ColumnID{0}, LT, int32(0)), b = executed<TableScan>(int_float4, ColumnID{0}, LT, int32(12346));
    const auto set_union = executed<UnionPositions>(a, b);
    EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), load_table(g_tbl + "/int_float2.tbl")));
    EXPECT_TRUE(b->get_output() == set_union->get_output());
  });
  run("UnionPositionsTest.SelfUnionOverlappingRangesMultipleSegments", [&] {   // :156-173
    const auto set_union = executed<UnionPositions>(executed<TableScan>(int_float4, ColumnID{0}, GT, int32(12345)), executed<TableScan>(int_float4, ColumnID{1}, LT, AllTypeVariant{400.0f}));
    EXPECT_TRUE(tables_equal_unordered(set_union->get_output(), load_table(g_tbl + "/union_positions/int_float4_overlapping_ranges.tbl")));
    EXPECT_TRUE(pos_list_of(set_union->get_output(), 0) == pos_list_of(set_union->get_output(), 1));
  });
  run("UnionPositionsTest.MultipleReferencedTables", [&] {   // :175-226
    const auto join = executed<JoinHash>(int_float4, int_int, JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
    const auto a = executed<TableScan>(join, ColumnID{3}, PredicateCondition::GreaterThanEquals, int32(2));
    const auto b = executed<TableScan>(join, ColumnID{1}, LT, AllTypeVariant{457.0f});
    const auto set_union = executed<UnionPositions>(a, b);
    const auto output = set_union->get_output();
    EXPECT_TRUE(tables_equal_unordered(output, load_table(g_tbl + "/union_positions/int_float4_int_int_union_positions.tbl")));
    EXPECT_TRUE(pos_list_of(output, 0) == pos_list_of(output, 1));   // no redundant PosLists: one per cluster
    EXPECT_TRUE(pos_list_of(output, 2) == pos_list_of(output, 3));
    EXPECT_TRUE(pos_list_of(output, 0) != pos_list_of(output, 2));
  });
  run("UnionPositionsTest.MultipleShuffledPosList", multiple_shuffled_pos_list);
  run("UnionPositionsTest.DifferentTables", [&] {   // :318-330
    auto set_union = std::make_shared<UnionPositions>(ints, int_float4);
    EXPECT_TRUE(throws_logic_error([&] { set_union->execute(); }));
  });
  run("UnionPositionsTest.SameColumnsDifferentTables", [&] {   // :332-351 (a debug check there, always made here)
    auto data_tables = std::make_shared<UnionPositions>(ints, wrap(load_table(g_tbl + "/union_positions/10_ints.tbl", ChunkOffset{3})));
    EXPECT_TRUE(throws_logic_error([&] { data_tables->execute(); }));
    // ... and two reference tables with equal column definitions over different data tables
    const auto copy = wrap(load_table(g_tbl + "/union_positions/10_ints.tbl", ChunkOffset{3}));
    auto different = std::make_shared<UnionPositions>(executed<TableScan>(ints, ColumnID{0}, GT, int32(20)), executed<TableScan>(copy, ColumnID{0}, LT, int32(100)));
    EXPECT_TRUE(throws_logic_error([&] { different->execute(); }));
  });
  run("UnionAllTest.UnionOfTwoScansSharesTheirChunks", [&] {
    const auto a = executed<TableScan>(ints, ColumnID{0}, LT, int32(10)), b = executed<TableScan>(ints, ColumnID{0}, GT, int32(200));
    const auto all = executed<UnionAll>(a, b);
    const auto output = all->get_output();
    EXPECT_TRUE(tables_equal_unordered(output, load_table(g_tbl + "/union_positions/10_ints_exclusive_ranges.tbl")));
    EXPECT_TRUE(output->chunk_count() == a->get_output()->chunk_count() + b->get_output()->chunk_count());
    EXPECT_TRUE(output->type() == TableType::References);
    if (output->chunk_count()) EXPECT_TRUE(output->get_chunk(0)->get_segment(0) == a->get_output()->get_chunk(0)->get_segment(0));   // shared, not copied
    auto mismatched = std::make_shared<UnionAll>(ints, int_float4);
    EXPECT_TRUE(throws_logic_error([&] { mismatched->execute(); }));
  });
  run("UnionPositionsChain.DeviceListsEqualHostLists", [&] {
    std::vector<std::vector<AllTypeVariant>> aggregated[2], sorted[2];
    uint32_t path[2] = {9, 9};
    chain(true, aggregated[0], sorted[0], path[0]);
    chain(false, aggregated[1], sorted[1], path[1]);
    EXPECT_TRUE(path[0] == 0 && path[1] == 0);
    EXPECT_TRUE(aggregated[0].size() == 7 && !sorted[0].empty());
    const auto same = [](const std::vector<std::vector<AllTypeVariant>>& a, const std::vector<std::vector<AllTypeVariant>>& b) {
      if (a.size() != b.size()) return false;
      for (size_t r = 0; r < a.size(); ++r)
        for (size_t c = 0; c < a[r].size(); ++c)
          if (variant_is_null(a[r][c]) != variant_is_null(b[r][c]) || (!variant_is_null(a[r][c]) && as_double(a[r][c]) != as_double(b[r][c]))) return false;
      return true;
    };
    EXPECT_TRUE(same(aggregated[0], aggregated[1]));
    EXPECT_TRUE(same(sorted[0], sorted[1]));
    for (size_t r = 1; r < sorted[0].size(); ++r) EXPECT_TRUE(as_double(sorted[0][r - 1][0]) <= as_double(sorted[0][r][0]));
  });

  std::printf(g_failures ? "UNION POSITIONS TESTS FAILED: %d\n" : "UNION POSITIONS TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

// sort_tests.cpp -- the reference's Sort tests (src/test/lib/operators/sort_test.cpp), re-stated against the C++ mirror's Sort
// (hyrise_amd/host/hyrise_host.hpp), which sorts on the device through hy_sort / hy_column_gather:
//   SortTest.Sort and SortTest.UnchangedNullability over the 14 Variations (:151-176): ordered equality with the expected .tbl, output
//   chunk sizes, table type, nullability of the ValueSegments
//   SortTest.JoinProducesReferences (:181-194), InputReferencesDifferentTables (:196-225), InputReferencesDifferentColumns (:227-254)
// plus string sort keys (ranks of a dictionary column, and of value segments read on the host) against std::stable_sort.
// Usage: sort_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

static bool cells_equal(const AllTypeVariant& a, const AllTypeVariant& b) {   // check_table_equal.cpp:34,109-115
  if (variant_is_null(a) || variant_is_null(b)) return variant_is_null(a) && variant_is_null(b);
  if (a.index() == 5 || b.index() == 5) return a.index() == b.index() && std::get<std::string>(a) == std::get<std::string>(b);
  const auto as_double = [](const AllTypeVariant& v) {
    switch (v.index()) { case 1: return static_cast<double>(std::get<int32_t>(v)); case 2: return static_cast<double>(std::get<int64_t>(v));
                         case 3: return static_cast<double>(std::get<float>(v)); default: return std::get<double>(v); }
  };
  return std::fabs(as_double(a) - as_double(b)) < 1e-6;
}

// EXPECT_TABLE_EQ_ORDERED (check_table_equal.cpp): same column count, names, types, nullability, and the same rows in the same order
static bool tables_equal_ordered(const std::shared_ptr<const Table>& got, const std::shared_ptr<const Table>& want) {
  if (got->column_count() != want->column_count()) { std::printf("  column counts differ\n"); return false; }
  for (ColumnID c = 0; c < got->column_count(); ++c) {
    if (got->column_name(c) != want->column_name(c) || got->column_data_type(c) != want->column_data_type(c) || got->column_is_nullable(c) != want->column_is_nullable(c)) {
      std::printf("  column %u: definitions differ\n", c);
      return false;
    }
  }
  const auto a = got->get_rows(), b = want->get_rows();
  if (a.size() != b.size()) { std::printf("  row counts differ: %zu vs %zu\n", a.size(), b.size()); return false; }
  for (size_t r = 0; r < a.size(); ++r) {
    for (size_t c = 0; c < a[r].size(); ++c) {
      if (!cells_equal(a[r][c], b[r][c])) { std::printf("  row %zu column %zu differs\n", r, c); return false; }
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

struct SortTestParam {   // sort_test.cpp:26-35
  std::vector<SortColumnDefinition> sort_columns;
  bool input_is_empty;
  bool input_is_reference;
  ChunkOffset output_chunk_size;
  Sort::ForceMaterialization force_materialization;
  std::string expected_filename;
};

static std::shared_ptr<Table> g_input_table;   // SetUpTestCase: input.tbl in chunks of 20 rows
static std::shared_ptr<TableWrapper> g_input_wrapper;

static std::shared_ptr<const AbstractOperator> input_of(const SortTestParam& param) {
  if (param.input_is_empty) {
    if (param.input_is_reference) {   // an empty reference table: a scan that matches nothing
      auto scan = std::make_shared<TableScan>(g_input_wrapper, ColumnID{0}, PredicateCondition::Equals, AllTypeVariant{int32_t{-12345}});
      scan->execute();
      return scan;
    }
    return wrap(std::make_shared<Table>(g_input_table->column_definitions(), TableType::Data));   // Table::create_dummy_table
  }
  if (param.input_is_reference) {   // (the reference test sorts the data table here; a scan's output -- PosLists in HBM -- is the stronger case)
    auto scan = std::make_shared<TableScan>(g_input_wrapper, ColumnID{0}, PredicateCondition::GreaterThanEquals, AllTypeVariant{int32_t{0}});
    scan->execute();
    return scan;
  }
  return g_input_wrapper;
}

static void test_sort(const SortTestParam& param) {   // SortTest.Sort (:50-89)
  auto sort = Sort{input_of(param), param.sort_columns, param.output_chunk_size, param.force_materialization};
  sort.execute();
  const auto expected = load_table(g_tbl + "/sort/" + param.expected_filename);
  const auto result = sort.get_output();
  EXPECT_TRUE(tables_equal_ordered(result, expected));
  if (param.force_materialization == Sort::ForceMaterialization::Yes || (param.input_is_empty && !param.input_is_reference)) {
    EXPECT_TRUE(result->type() == TableType::Data);
  } else {
    EXPECT_TRUE(result->type() == TableType::References);
  }
  for (ChunkID k = 0; k + 1 < result->chunk_count(); ++k) EXPECT_TRUE(result->get_chunk(k)->size() == param.output_chunk_size);
  if (!param.input_is_empty) {
    for (ChunkID k = 0; k < result->chunk_count(); ++k) {   // :381-389
      EXPECT_TRUE(!result->get_chunk(k)->is_mutable());
      const auto& sorted_by = result->get_chunk(k)->individually_sorted_by();
      EXPECT_TRUE(sorted_by.size() == 1 && sorted_by[0].column == param.sort_columns[0].column && sorted_by[0].sort_mode == param.sort_columns[0].sort_mode);
    }
  }
}

static bool segment_nullability_implies_column_nullability(const std::shared_ptr<const Table>& table) {   // :94-114
  for (ChunkID k = 0; k < table->chunk_count(); ++k) {
    for (ColumnID c = 0; c < table->column_count(); ++c) {
      const auto* segment = table->get_chunk(k)->get_segment(c).get();
      bool nullable = false;
      if (const auto* s = dynamic_cast<const ValueSegment<int32_t>*>(segment)) nullable = s->is_nullable();
      else if (const auto* s = dynamic_cast<const ValueSegment<int64_t>*>(segment)) nullable = s->is_nullable();
      else if (const auto* s = dynamic_cast<const ValueSegment<float>*>(segment)) nullable = s->is_nullable();
      else if (const auto* s = dynamic_cast<const ValueSegment<double>*>(segment)) nullable = s->is_nullable();
      else if (const auto* s = dynamic_cast<const ValueSegment<std::string>*>(segment)) nullable = s->is_nullable();
      if (nullable && !table->column_is_nullable(c)) return false;
    }
  }
  return true;
}

static void test_unchanged_nullability(const SortTestParam& param) {   // SortTest.UnchangedNullability (:91-125)
  EXPECT_TRUE(segment_nullability_implies_column_nullability(g_input_table));
  auto sort = Sort{g_input_wrapper, param.sort_columns, param.output_chunk_size, param.force_materialization};
  sort.execute();
  EXPECT_TRUE(segment_nullability_implies_column_nullability(sort.get_output()));
  if (param.force_materialization == Sort::ForceMaterialization::Yes) {   // (materialised: a ValueSegment is nullable iff its column is)
    const auto output = sort.get_output();
    for (ChunkID k = 0; k < output->chunk_count(); ++k) {
      for (ColumnID c = 0; c < output->column_count(); ++c) {
        const auto* segment = output->get_chunk(k)->get_segment(c).get();
        if (const auto* s = dynamic_cast<const ValueSegment<int32_t>*>(segment)) EXPECT_TRUE(s->is_nullable() == output->column_is_nullable(c));
        if (const auto* s = dynamic_cast<const ValueSegment<std::string>*>(segment)) EXPECT_TRUE(s->is_nullable() == output->column_is_nullable(c));
      }
    }
  }
}

static void test_join_produces_references() {   // :181-194
  const auto right = wrap(load_table(g_tbl + "/int3.tbl"));
  auto join = std::make_shared<JoinHash>(g_input_wrapper, right, JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
  join->execute();
  auto sort = Sort{join, {SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst}}};
  sort.execute();
  const auto output = sort.get_output();
  EXPECT_TRUE(output->type() == TableType::References);
  // (and the order: b descending, NULLs first, ties in the join output's order)
  auto want = join->get_output()->get_rows();
  std::stable_sort(want.begin(), want.end(), [](const auto& x, const auto& y) {
    if (variant_is_null(y[1])) return false;
    if (variant_is_null(x[1])) return true;
    return std::get<int32_t>(x[1]) > std::get<int32_t>(y[1]);
  });
  const auto got = output->get_rows();
  EXPECT_TRUE(got.size() == want.size());
  for (size_t r = 0; r < std::min(got.size(), want.size()); ++r)
    for (size_t c = 0; c < got[r].size(); ++c) EXPECT_TRUE(cells_equal(got[r][c], want[r][c]));
}

static std::shared_ptr<Table> union_like_table(const std::shared_ptr<const Table>& first, ColumnID first_column, const std::shared_ptr<const Table>& second,
                                               ColumnID second_column) {
  auto table = std::make_shared<Table>(TableColumnDefinitions{TableColumnDefinition{"a", DataType::Int, true}}, TableType::References);
  const auto pos_list = std::make_shared<RowIDPosList>(std::vector<RowID>{RowID{0, 0}, RowID{0, 1}, RowID{1, 0}});
  table->append_chunk(Segments{std::make_shared<ReferenceSegment>(first, first_column, pos_list)});
  table->append_chunk(Segments{std::make_shared<ReferenceSegment>(second, second_column, pos_list)});
  return table;
}

static void expect_descending_ints(const std::shared_ptr<const Table>& output, std::vector<AllTypeVariant> want) {
  std::stable_sort(want.begin(), want.end(), [](const auto& x, const auto& y) {
    if (variant_is_null(y)) return false;
    if (variant_is_null(x)) return true;
    return std::get<int32_t>(x) > std::get<int32_t>(y);
  });
  const auto got = output->get_rows();
  EXPECT_TRUE(got.size() == want.size());
  for (size_t r = 0; r < std::min(got.size(), want.size()); ++r) EXPECT_TRUE(cells_equal(got[r][0], want[r]));
}

static void test_input_references_different_tables() {   // :196-225
  const auto second_table = load_table(g_tbl + "/sort/a_asc.tbl", ChunkOffset{10});
  const auto table = union_like_table(g_input_table, ColumnID{0}, second_table, ColumnID{0});
  auto sort = Sort{wrap(table), {SortColumnDefinition{ColumnID{0}, SortMode::DescendingNullsFirst}}};
  sort.execute();
  EXPECT_TRUE(sort.get_output()->type() == TableType::Data);
  expect_descending_ints(sort.get_output(), {g_input_table->get_value(0, 0), g_input_table->get_value(0, 1), g_input_table->get_value(0, 20),
                                             second_table->get_value(0, 0), second_table->get_value(0, 1), second_table->get_value(0, 10)});
}

static void test_input_references_different_columns() {   // :227-254
  const auto table = union_like_table(g_input_table, ColumnID{0}, g_input_table, ColumnID{1});
  auto sort = Sort{wrap(table), {SortColumnDefinition{ColumnID{0}, SortMode::DescendingNullsFirst}}};
  sort.execute();
  EXPECT_TRUE(sort.get_output()->type() == TableType::Data);
  expect_descending_ints(sort.get_output(), {g_input_table->get_value(0, 0), g_input_table->get_value(0, 1), g_input_table->get_value(0, 20),
                                             g_input_table->get_value(1, 0), g_input_table->get_value(1, 1), g_input_table->get_value(1, 20)});
}

static void test_string_keys(EncodingType encoding, SortMode mode) {   // ORDER BY c (string), then a: byte order, NULLs first, stable
  auto table = load_table(g_tbl + "/sort/input.tbl", ChunkOffset{7});
  if (encoding != EncodingType::Unencoded) ChunkEncoder::encode_all_chunks(table, encoding);
  const auto wrapper = wrap(table);
  auto scan = std::make_shared<TableScan>(wrapper, ColumnID{0}, PredicateCondition::GreaterThanEquals, AllTypeVariant{int32_t{2}});
  scan->execute();
  for (const std::shared_ptr<const AbstractOperator>& input : {std::static_pointer_cast<const AbstractOperator>(wrapper), std::static_pointer_cast<const AbstractOperator>(scan)}) {
    auto sort = Sort{input, {SortColumnDefinition{ColumnID{2}, mode}, SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}}, ChunkOffset{9}};
    sort.execute();
    auto want = input->get_output()->get_rows();
    std::stable_sort(want.begin(), want.end(), [](const auto& x, const auto& y) { return std::get<int32_t>(x[0]) < std::get<int32_t>(y[0]); });
    std::stable_sort(want.begin(), want.end(), [&](const auto& x, const auto& y) {
      return mode == SortMode::AscendingNullsFirst ? std::get<std::string>(x[2]) < std::get<std::string>(y[2]) : std::get<std::string>(x[2]) > std::get<std::string>(y[2]);
    });
    const auto got = sort.get_output()->get_rows();
    EXPECT_TRUE(got.size() == want.size());
    for (size_t r = 0; r < std::min(got.size(), want.size()); ++r)
      for (size_t c = 0; c < got[r].size(); ++c) EXPECT_TRUE(cells_equal(got[r][c], want[r][c]));
  }
}

static void test_nulls_last_is_refused() {   // sort.cpp:294-296
  for (const auto mode : {SortMode::AscendingNullsLast, SortMode::DescendingNullsLast}) {
    bool threw = false;
    try {
      auto sort = Sort{g_input_wrapper, {SortColumnDefinition{ColumnID{0}, mode}}};
      sort.execute();
    } catch (const std::logic_error&) {
      threw = true;
    }
    EXPECT_TRUE(threw);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: sort_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  g_input_table = load_table(g_tbl + "/sort/input.tbl", ChunkOffset{20});
  g_input_wrapper = wrap(g_input_table);
  using FM = Sort::ForceMaterialization;
  const auto a_asc = SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}, a_desc = SortColumnDefinition{ColumnID{0}, SortMode::DescendingNullsFirst};
  const auto b_asc = SortColumnDefinition{ColumnID{1}, SortMode::AscendingNullsFirst}, b_desc = SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst};
  const ChunkOffset DEFAULT = Chunk::DEFAULT_SIZE;
  const std::vector<SortTestParam> variations = {   // sort_test.cpp:151-176
      {{a_asc}, false, false, DEFAULT, FM::No, "a_asc.tbl"},
      {{a_desc}, false, false, DEFAULT, FM::No, "a_desc.tbl"},
      {{a_asc, b_desc}, false, false, DEFAULT, FM::No, "a_asc_b_desc.tbl"},
      {{a_desc, b_asc}, false, false, DEFAULT, FM::No, "a_desc_b_asc.tbl"},
      {{a_asc, b_desc}, false, false, ChunkOffset{40}, FM::No, "a_asc_b_desc.tbl"},
      {{a_asc, b_desc}, false, true, ChunkOffset{40}, FM::No, "a_asc_b_desc.tbl"},
      {{a_asc}, true, false, DEFAULT, FM::No, "empty.tbl"},
      {{a_asc}, true, true, DEFAULT, FM::No, "empty.tbl"},
      {{a_asc, b_desc}, false, false, DEFAULT, FM::Yes, "a_asc_b_desc.tbl"},
      {{a_asc, b_desc}, false, false, ChunkOffset{33}, FM::Yes, "a_asc_b_desc.tbl"},
      {{a_asc, b_desc}, false, true, DEFAULT, FM::Yes, "a_asc_b_desc.tbl"},
      {{a_asc, b_desc}, false, true, ChunkOffset{33}, FM::Yes, "a_asc_b_desc.tbl"},
      {{a_asc}, true, false, DEFAULT, FM::Yes, "empty.tbl"},
      {{a_asc}, true, true, DEFAULT, FM::Yes, "empty.tbl"},
  };
  for (size_t i = 0; i < variations.size(); ++i) {
    const auto& p = variations[i];
    const std::string name = "Variations/" + std::to_string(i) + " " + p.expected_filename + (p.input_is_empty ? " empty" : "") + (p.input_is_reference ? " reference" : " data") +
                             " chunk " + std::to_string(p.output_chunk_size) + (p.force_materialization == FM::Yes ? " materialized" : "");
    run("SortTest.Sort " + name, [&] { test_sort(p); });
    run("SortTest.UnchangedNullability " + name, [&] { test_unchanged_nullability(p); });
  }
  run("SortTest.JoinProducesReferences", test_join_produces_references);
  run("SortTest.InputReferencesDifferentTables", test_input_references_different_tables);
  run("SortTest.InputReferencesDifferentColumns", test_input_references_different_columns);
  for (const auto encoding : {EncodingType::Unencoded, EncodingType::Dictionary}) {
    for (const auto mode : {SortMode::AscendingNullsFirst, SortMode::DescendingNullsFirst}) {
      run(std::string("Sort by a string column (") + (encoding == EncodingType::Dictionary ? "dictionary" : "value") + " segments, " +
              (mode == SortMode::AscendingNullsFirst ? "ascending" : "descending") + ")",
          [&] { test_string_keys(encoding, mode); });
    }
  }
  run("Sort refuses NULLS LAST", test_nulls_last_is_refused);
  g_input_wrapper.reset();
  g_input_table.reset();
  hy_shutdown();
  std::printf("%s\n", g_failures ? "SORT TESTS FAILED" : "SORT TESTS PASSED");
  return g_failures ? 1 : 0;
}

// limit_tests.cpp -- the reference's Limit tests (src/test/lib/operators/limit_test.cpp), re-stated against the C++ mirror's Limit
// (hyrise_amd/host/hyrise_host.hpp): Limit1 / 2 / 4 / 10 over value and reference segments, ForwardSortedByFlag, Name.  OnlyIntegralTypes is
// the adapter's: the mirror has no expression classes, its Limit takes the evaluated row count.
// Plus what only the mirror has:
//   Limit over a TableScan's device-resident output: DevicePosList views of the same pooled block, and no row crosses to the host
//   Limit(Sort(x), k) against Sort(x, row_limit = k) (hy_sort_limit): the same rows in the same order, chunk sizes and individually_sorted_by,
//   for a data input, a reference input and ForceMaterialization::Yes (the fused form's table type is Sort's own)
//   string sort keys (ranks) with a row limit, and the same tables with device_resident_results(false)
// Usage: limit_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

static std::shared_ptr<TableWrapper> g_table_wrapper;   // SetUp: int_int3.tbl in chunks of 3 rows

static std::shared_ptr<const AbstractOperator> scan_accepting_all_rows(const std::shared_ptr<const AbstractOperator>& input) {   // limit_test.cpp:76-79
  auto scan = std::make_shared<TableScan>(input, ColumnID{0}, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{-1}});
  scan->execute();
  return scan;
}

// A scan that keeps a part of every chunk of sort/input.tbl (a chunk whose rows all match would be forwarded as an EntireChunkPosList): with
// device-resident results its PosLists are DevicePosLists.
static std::shared_ptr<const AbstractOperator> scan_keeping_part_of_every_chunk(const std::shared_ptr<const AbstractOperator>& input) {
  auto scan = std::make_shared<TableScan>(input, ColumnID{0}, PredicateCondition::GreaterThanEquals, AllTypeVariant{int32_t{3}});
  scan->execute();
  return scan;
}

static void test_limit(const std::shared_ptr<const AbstractOperator>& input, uint64_t row_count, const std::string& expected_filename) {   // :28-64
  auto limit = std::make_shared<Limit>(input, row_count);
  limit->execute();
  const auto expected = load_table(g_tbl + "/" + expected_filename, ChunkOffset{3});
  EXPECT_TRUE(tables_equal_ordered(limit->get_output(), expected));
  EXPECT_TRUE(limit->get_output()->type() == TableType::References);
  for (ChunkID k = 0; k < limit->get_output()->chunk_count(); ++k) EXPECT_TRUE(!limit->get_output()->get_chunk(k)->is_mutable());
}

static bool same_sorted_by(const std::vector<SortColumnDefinition>& a, const std::vector<SortColumnDefinition>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (a[i].column != b[i].column || a[i].sort_mode != b[i].sort_mode) return false;
  return true;
}

static void test_forward_sorted_by_flag() {   // :122-148
  auto limit = std::make_shared<Limit>(g_table_wrapper, 4);
  limit->execute();
  for (ChunkID k = 0; k < limit->get_output()->chunk_count(); ++k) EXPECT_TRUE(limit->get_output()->get_chunk(k)->individually_sorted_by().empty());
  const auto sort_definition = std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}};
  auto sort = std::make_shared<Sort>(g_table_wrapper, sort_definition);
  sort->execute();
  auto limit_sorted = std::make_shared<Limit>(sort, 4);
  limit_sorted->execute();
  EXPECT_TRUE(limit_sorted->get_output()->chunk_count() > 0);
  for (ChunkID k = 0; k < limit_sorted->get_output()->chunk_count(); ++k)
    EXPECT_TRUE(same_sorted_by(limit_sorted->get_output()->get_chunk(k)->individually_sorted_by(), sort_definition));
}

static void test_name() {   // :158-161
  EXPECT_TRUE(std::make_shared<Limit>(g_table_wrapper, 2)->name() == "Limit");
}

static const DevicePosList* device_list_of(const std::shared_ptr<const Table>& table, ChunkID chunk, ColumnID column) {
  const auto segment = std::dynamic_pointer_cast<const ReferenceSegment>(table->get_chunk(chunk)->get_segment(column));
  return segment ? dynamic_cast<const DevicePosList*>(segment->pos_list().get()) : nullptr;
}

// A scan's PosLists lie in one pooled block of HBM: Limit cuts them as views of that block, and nothing is read back for it.
static void test_limit_keeps_device_pos_lists() {
  const auto table = load_table(g_tbl + "/sort/input.tbl", ChunkOffset{20});
  const auto scan = scan_keeping_part_of_every_chunk(wrap(table));
  const auto scanned = scan->get_output();
  EXPECT_TRUE(scanned->chunk_count() > 2 && device_list_of(scanned, 0, ColumnID{0}) != nullptr);
  if (!device_list_of(scanned, 0, ColumnID{0})) return;
  const uint64_t row_count = scanned->get_chunk(0)->size() + scanned->get_chunk(1)->size() / 2;   // one whole chunk and half of the next
  auto limit = std::make_shared<Limit>(scan, row_count);
  limit->execute();
  const auto output = limit->get_output();
  EXPECT_TRUE(output->chunk_count() == 2 && output->row_count() == row_count);
  for (ChunkID k = 0; k < output->chunk_count(); ++k) {
    for (ColumnID c = 0; c < output->column_count(); ++c) {
      const auto* before = device_list_of(scanned, k, c);
      const auto* after = device_list_of(output, k, c);
      EXPECT_TRUE(before && after);
      if (!before || !after) continue;
      EXPECT_TRUE(after->block() == before->block() && after->device_data() == before->device_data());
      EXPECT_TRUE(after->size() == (k == 0 ? before->size() : before->size() / 2));
      EXPECT_TRUE(!after->on_host() && !before->on_host());
      EXPECT_TRUE(after == device_list_of(output, k, ColumnID{0}));   // (the columns still share one PosList)
    }
  }
  auto rows = scanned->get_rows();   // (now the lists are read: the cut ones index the same rows)
  rows.resize(row_count);
  const auto got = output->get_rows();
  EXPECT_TRUE(got.size() == rows.size());
  for (size_t r = 0; r < std::min(got.size(), rows.size()); ++r)
    for (size_t c = 0; c < got[r].size(); ++c) EXPECT_TRUE(cells_equal(got[r][c], rows[r][c]));
}

static std::vector<ChunkOffset> chunk_sizes_of(const std::shared_ptr<const Table>& table) {
  std::vector<ChunkOffset> sizes;
  for (ChunkID k = 0; k < table->chunk_count(); ++k) sizes.push_back(table->get_chunk(k)->size());
  return sizes;
}

// Limit(Sort(x), k) against Sort(x, row_limit = k)
static void expect_fused_equals_chain(const std::shared_ptr<const AbstractOperator>& input, const std::vector<SortColumnDefinition>& definitions, ChunkOffset chunk_size,
                                      Sort::ForceMaterialization force, uint64_t k) {
  auto sort = std::make_shared<Sort>(input, definitions, chunk_size, force);
  sort->execute();
  auto limit = std::make_shared<Limit>(sort, k);
  limit->execute();
  auto fused = std::make_shared<Sort>(input, definitions, chunk_size, force, k);
  fused->execute();
  const auto want = limit->get_output(), got = fused->get_output();
  EXPECT_TRUE(tables_equal_ordered(got, want));
  EXPECT_TRUE(got->row_count() == std::min<uint64_t>(k, input->get_output()->row_count()));
  EXPECT_TRUE(chunk_sizes_of(got) == chunk_sizes_of(want));
  EXPECT_TRUE(got->type() == sort->get_output()->type());
  for (ChunkID c = 0; c < std::min(got->chunk_count(), want->chunk_count()); ++c) {
    EXPECT_TRUE(!got->get_chunk(c)->is_mutable());
    EXPECT_TRUE(same_sorted_by(got->get_chunk(c)->individually_sorted_by(), want->get_chunk(c)->individually_sorted_by()));
    EXPECT_TRUE(same_sorted_by(got->get_chunk(c)->individually_sorted_by(), {definitions[0]}));
  }
}

static void test_fused_sort_limit(bool reference_input, Sort::ForceMaterialization force) {
  const auto wrapper = wrap(load_table(g_tbl + "/sort/input.tbl", ChunkOffset{20}));
  const std::shared_ptr<const AbstractOperator> input = reference_input ? scan_keeping_part_of_every_chunk(wrapper) : std::static_pointer_cast<const AbstractOperator>(wrapper);
  const uint64_t rows = input->get_output()->row_count();
  const auto a_asc = SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}, a_desc = SortColumnDefinition{ColumnID{0}, SortMode::DescendingNullsFirst};
  const auto b_asc = SortColumnDefinition{ColumnID{1}, SortMode::AscendingNullsFirst}, b_desc = SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst};
  for (const auto& definitions : {std::vector<SortColumnDefinition>{a_asc}, std::vector<SortColumnDefinition>{a_desc, b_asc}, std::vector<SortColumnDefinition>{b_desc, a_asc}}) {
    for (const ChunkOffset chunk_size : {ChunkOffset{9}, Chunk::DEFAULT_SIZE}) {
      for (const uint64_t k : {uint64_t{0}, uint64_t{1}, uint64_t{9}, uint64_t{10}, uint64_t{25}, rows - 1, rows, rows + 5})
        expect_fused_equals_chain(input, definitions, chunk_size, force, k);
    }
  }
}

static void test_string_keys_with_a_row_limit(EncodingType encoding) {   // ORDER BY c (string, as ranks), then a
  auto table = load_table(g_tbl + "/sort/input.tbl", ChunkOffset{7});
  if (encoding != EncodingType::Unencoded) ChunkEncoder::encode_all_chunks(table, encoding);
  const auto wrapper = wrap(table);
  for (const auto mode : {SortMode::AscendingNullsFirst, SortMode::DescendingNullsFirst}) {
    for (const std::shared_ptr<const AbstractOperator>& input : {std::static_pointer_cast<const AbstractOperator>(wrapper), scan_keeping_part_of_every_chunk(wrapper)}) {
      for (const uint64_t k : {uint64_t{1}, uint64_t{12}, uint64_t{1000}})
        expect_fused_equals_chain(input, {SortColumnDefinition{ColumnID{2}, mode}, SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}}, ChunkOffset{9}, Sort::ForceMaterialization::No, k);
    }
  }
}

static void test_host_resident_results_give_the_same_tables() {
  const auto wrapper = wrap(load_table(g_tbl + "/sort/input.tbl", ChunkOffset{20}));
  const auto definitions = std::vector<SortColumnDefinition>{SortColumnDefinition{ColumnID{1}, SortMode::DescendingNullsFirst}, SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}};
  std::shared_ptr<const Table> tables[2][2];
  for (const bool on_device : {true, false}) {
    device_resident_results() = on_device;
    const auto scan = scan_keeping_part_of_every_chunk(wrapper);
    EXPECT_TRUE((device_list_of(scan->get_output(), 0, ColumnID{0}) != nullptr) == on_device);
    auto limit = std::make_shared<Limit>(scan, 25);
    limit->execute();
    auto fused = std::make_shared<Sort>(scan, definitions, ChunkOffset{9}, Sort::ForceMaterialization::No, 25);
    fused->execute();
    tables[on_device][0] = limit->get_output();
    tables[on_device][1] = fused->get_output();
    expect_fused_equals_chain(scan, definitions, ChunkOffset{9}, Sort::ForceMaterialization::No, 25);
  }
  device_resident_results() = true;
  for (int t = 0; t < 2; ++t) {
    EXPECT_TRUE(tables_equal_ordered(tables[0][t], tables[1][t]));
    EXPECT_TRUE(chunk_sizes_of(tables[0][t]) == chunk_sizes_of(tables[1][t]));
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: limit_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  g_table_wrapper = wrap(load_table(g_tbl + "/int_int3.tbl", ChunkOffset{3}));
  const std::pair<uint64_t, std::string> limits[] = {{1, "limit/int_int3_limit_1.tbl"}, {2, "limit/int_int3_limit_2.tbl"}, {4, "limit/int_int3_limit_4.tbl"}, {10, "int_int3.tbl"}};
  for (const auto& [row_count, expected] : limits) {
    run("OperatorsLimitTest.Limit" + std::to_string(row_count) + "ValueSegment", [&] { test_limit(g_table_wrapper, row_count, expected); });
    run("OperatorsLimitTest.Limit" + std::to_string(row_count) + "ReferenceSegment", [&] { test_limit(scan_accepting_all_rows(g_table_wrapper), row_count, expected); });
  }
  run("OperatorsLimitTest.ForwardSortedByFlag", test_forward_sorted_by_flag);
  run("OperatorsLimitTest.Name", test_name);
  run("Limit over a scan's device-resident output: views of the same block, nothing fetched", test_limit_keeps_device_pos_lists);
  using FM = Sort::ForceMaterialization;
  run("Limit(Sort(x), k) == Sort(x, row_limit = k), data input", [] { test_fused_sort_limit(false, FM::No); });
  run("Limit(Sort(x), k) == Sort(x, row_limit = k), reference input", [] { test_fused_sort_limit(true, FM::No); });
  run("Limit(Sort(x), k) == Sort(x, row_limit = k), data input, materialized", [] { test_fused_sort_limit(false, FM::Yes); });
  run("Limit(Sort(x), k) == Sort(x, row_limit = k), reference input, materialized", [] { test_fused_sort_limit(true, FM::Yes); });
  run("String sort keys with a row limit (value segments)", [] { test_string_keys_with_a_row_limit(EncodingType::Unencoded); });
  run("String sort keys with a row limit (dictionary segments)", [] { test_string_keys_with_a_row_limit(EncodingType::Dictionary); });
  run("device_resident_results(false) gives the same tables", test_host_resident_results_give_the_same_tables);
  g_table_wrapper.reset();
  hy_shutdown();
  std::printf("%s\n", g_failures ? "LIMIT TESTS FAILED" : "LIMIT TESTS PASSED");
  return g_failures ? 1 : 0;
}

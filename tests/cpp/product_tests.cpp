// product_tests.cpp -- the reference's OperatorsProductTest (src/test/lib/operators/product_test.cpp) against the C++ mirror's Product
// (hyrise_amd/host/hyrise_host.hpp), which writes its PosLists on the device through hy_product, and the mirror's own:
//   the three reference tests, row multisets against the expected .tbl (tests/golden/tbl/product), with device-resident and with host results;
//   both kinds of output equal list by list, chunk by chunk; one output chunk per pair of input chunks with rows(cl) * rows(cr) rows;
//   columns that shared an input PosList share the output PosList, and every segment references the data table;
//   TableScan -> Product -> TableScan (ColumnVsValue over a right-side column) with no DevicePosList read back before the final read;
//   Product -> TableScan ColumnVsColumn (left.a < right.b) against JoinNestedLoop Inner on the same predicate, as multisets.
// Usage: product_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <string>
#include <type_traits>

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

static std::string row_text(const std::vector<AllTypeVariant>& row) {
  std::string text;
  for (const auto& cell : row) {
    if (variant_is_null(cell)) text += "null|";
    else if (cell.index() == 5) text += std::get<std::string>(cell) + "|";
    else text += std::visit([](const auto& v) -> std::string { if constexpr (std::is_arithmetic_v<std::decay_t<decltype(v)>>) return std::to_string(static_cast<double>(v)); else return ""; }, cell) + "|";
  }
  return text;
}

static std::vector<std::string> sorted_rows(const Table& table) {   // EXPECT_TABLE_EQ_UNORDERED: the rows as a multiset
  std::vector<std::string> rows;
  for (const auto& row : table.get_rows()) rows.push_back(row_text(row));
  std::sort(rows.begin(), rows.end());
  return rows;
}

static bool same_definitions(const Table& got, const Table& want) {
  if (got.column_count() != want.column_count()) return false;
  for (ColumnID c = 0; c < got.column_count(); ++c)
    if (got.column_name(c) != want.column_name(c) || got.column_data_type(c) != want.column_data_type(c) || got.column_is_nullable(c) != want.column_is_nullable(c)) return false;
  return true;
}

static std::shared_ptr<const AbstractPosList> list_of(const Table& table, ChunkID chunk, ColumnID column) {
  const auto segment = std::dynamic_pointer_cast<const ReferenceSegment>(table.get_chunk(chunk)->get_segment(column));
  return segment ? segment->pos_list() : nullptr;
}

// Has any DevicePosList of the table been read back?  (-> how many lists of the table lie in HBM)
static size_t device_lists_untouched(const Table& table, bool* any_on_host) {
  size_t lists = 0;
  for (ChunkID k = 0; k < table.chunk_count(); ++k) {
    for (ColumnID c = 0; c < table.column_count(); ++c) {
      const auto* list = dynamic_cast<const DevicePosList*>(list_of(table, k, c).get());
      if (!list) continue;
      ++lists;
      if (list->on_host()) *any_on_host = true;
    }
  }
  return lists;
}

// The output's shape (product.cpp:33-61, 99-136) against the inputs.
static void expect_shape(const Table& out, const Table& left, const Table& right) {
  EXPECT_TRUE(out.type() == TableType::References);
  EXPECT_TRUE(out.column_count() == left.column_count() + right.column_count());
  for (ColumnID c = 0; c < out.column_count(); ++c) {
    const Table& from = c < left.column_count() ? left : right;
    const ColumnID at = c < left.column_count() ? c : static_cast<ColumnID>(c - left.column_count());
    EXPECT_TRUE(out.column_name(c) == from.column_name(at) && out.column_data_type(c) == from.column_data_type(at) && out.column_is_nullable(c) == from.column_is_nullable(at));
  }
  EXPECT_TRUE(out.chunk_count() == left.chunk_count() * right.chunk_count());
  if (out.chunk_count() != left.chunk_count() * right.chunk_count()) return;
  for (ChunkID cl = 0; cl < left.chunk_count(); ++cl) {
    for (ChunkID cr = 0; cr < right.chunk_count(); ++cr) {
      const ChunkID k = cl * right.chunk_count() + cr;
      EXPECT_TRUE(out.get_chunk(k)->size() == left.get_chunk(cl)->size() * right.get_chunk(cr)->size());
      for (ColumnID c = 0; c < out.column_count(); ++c) {
        const bool from_left = c < left.column_count();
        const Table& from = from_left ? left : right;
        const ColumnID at = from_left ? c : static_cast<ColumnID>(c - left.column_count());
        const auto segment = std::dynamic_pointer_cast<const ReferenceSegment>(out.get_chunk(k)->get_segment(c));
        EXPECT_TRUE(segment != nullptr);
        if (!segment) continue;
        const auto in = std::dynamic_pointer_cast<const ReferenceSegment>(from.get_chunk(from_left ? cl : cr)->get_segment(at));
        EXPECT_TRUE(segment->referenced_table()->type() == TableType::Data);
        if (in) {
          EXPECT_TRUE(segment->referenced_table() == in->referenced_table() && segment->referenced_column_id() == in->referenced_column_id());
        } else {
          EXPECT_TRUE(segment->referenced_table().get() == &from && segment->referenced_column_id() == at);
        }
        // columns that shared an input list (a data input: all of them) share the output list
        const ColumnID first = from_left ? ColumnID{0} : left.column_count();
        const auto in_first = std::dynamic_pointer_cast<const ReferenceSegment>(from.get_chunk(from_left ? cl : cr)->get_segment(0));
        if (!in || in->pos_list() == in_first->pos_list()) EXPECT_TRUE(segment->pos_list() == list_of(out, k, first));
      }
    }
  }
  EXPECT_TRUE(list_of(out, 0, 0) != list_of(out, 0, left.column_count()));
}

// Both tables list by list: the same RowIDs in every chunk and column, and the same sharing.
static void expect_same_lists(const Table& a, const Table& b) {
  EXPECT_TRUE(a.chunk_count() == b.chunk_count() && a.column_count() == b.column_count());
  if (a.chunk_count() != b.chunk_count() || a.column_count() != b.column_count()) return;
  for (ChunkID k = 0; k < a.chunk_count(); ++k) {
    for (ColumnID c = 0; c < a.column_count(); ++c) {
      const auto x = list_of(a, k, c), y = list_of(b, k, c);
      EXPECT_TRUE(x && y && x->size() == y->size());
      if (!x || !y || x->size() != y->size()) continue;
      bool same = x->references_single_chunk() == y->references_single_chunk();
      for (size_t i = 0; i < x->size() && same; ++i) same = (*x)[i] == (*y)[i];
      EXPECT_TRUE(same);
      EXPECT_TRUE((x == list_of(a, k, 0)) == (y == list_of(b, k, 0)));
    }
  }
}

// One reference test: Product(left, right) with device-resident and with host results.
static void test_product(const std::function<std::shared_ptr<const AbstractOperator>()>& left, const std::function<std::shared_ptr<const AbstractOperator>()>& right,
                         const std::string& expected_file, ChunkOffset expected_chunk_size) {
  const auto expected = load_table(g_tbl + "/product/" + expected_file, expected_chunk_size);
  std::shared_ptr<const Table> outputs[2];
  for (const bool resident : {true, false}) {
    device_resident_results() = resident;
    const auto l = left(), r = right();
    auto product = std::make_shared<Product>(l, r);
    product->execute();
    const auto out = product->get_output();
    outputs[resident] = out;
    expect_shape(*out, *l->get_output(), *r->get_output());
    bool on_host = false;
    EXPECT_TRUE((device_lists_untouched(*out, &on_host) > 0) == resident && !on_host);
    EXPECT_TRUE(same_definitions(*out, *expected));
    EXPECT_TRUE(sorted_rows(*out) == sorted_rows(*expected));
  }
  device_resident_results() = true;
  expect_same_lists(*outputs[1], *outputs[0]);
}

static std::shared_ptr<const AbstractOperator> table_a() { return wrap(load_table(g_tbl + "/int.tbl", ChunkOffset{5})); }
static std::shared_ptr<const AbstractOperator> table_b() { return wrap(load_table(g_tbl + "/product/float.tbl", ChunkOffset{2})); }

static void test_name() {
  EXPECT_TRUE(std::make_shared<Product>(table_a(), table_b())->name() == "Product");
}

// An input whose columns sit behind TWO PosLists (a join's output): each side's list is shared by that side's columns only.
static void test_two_lists_per_side() {
  const auto left = wrap(load_table(g_tbl + "/product/int_int.tbl", ChunkOffset{2})), right = wrap(load_table(g_tbl + "/product/float.tbl", ChunkOffset{2}));
  auto join = std::make_shared<JoinNestedLoop>(left, left, JoinMode::Left, OperatorJoinPredicate{{ColumnID{1}, ColumnID{1}}, PredicateCondition::LessThan});
  join->execute();
  std::shared_ptr<const Table> outputs[2];
  for (const bool resident : {true, false}) {
    device_resident_results() = resident;
    auto product = std::make_shared<Product>(join, right);
    product->execute();
    const auto out = product->get_output();
    outputs[resident] = out;
    expect_shape(*out, *join->get_output(), *right->get_output());
    EXPECT_TRUE(out->column_count() == 5 && out->chunk_count() == 2);
    EXPECT_TRUE(list_of(*out, 0, 0) == list_of(*out, 0, 1) && list_of(*out, 0, 2) == list_of(*out, 0, 3) && list_of(*out, 0, 0) != list_of(*out, 0, 2));
    // the rows: every row of the join next to every row of float.tbl (the join's unmatched left row carries NULLs through)
    std::vector<std::string> want;
    for (const auto& a : join->get_output()->get_rows())
      for (const auto& b : right->get_output()->get_rows()) { auto row = a; row.insert(row.end(), b.begin(), b.end()); want.push_back(row_text(row)); }
    std::sort(want.begin(), want.end());
    EXPECT_TRUE(sorted_rows(*out) == want);
  }
  device_resident_results() = true;
  expect_same_lists(*outputs[1], *outputs[0]);
}

static std::shared_ptr<const Table> run_chain(const std::shared_ptr<TableWrapper>& left, const std::shared_ptr<TableWrapper>& right, bool expect_lists_in_hbm) {
  auto first = std::make_shared<TableScan>(left, ColumnID{0}, PredicateCondition::LessThanEquals, AllTypeVariant{int32_t{1338}});   // keeps a part of every chunk but one
  first->execute();
  auto product = std::make_shared<Product>(first, right);
  product->execute();
  const ColumnID right_int = left->get_output()->column_count();   // r_int
  auto last = std::make_shared<TableScan>(product, right_int, PredicateCondition::LessThan, AllTypeVariant{int32_t{1338}});
  last->execute();
  bool on_host = false;
  size_t lists = 0;
  for (const auto& table : {first->get_output(), product->get_output(), last->get_output()}) lists += device_lists_untouched(*table, &on_host);
  EXPECT_TRUE(!on_host);   // nothing has crossed to the host until the rows are read below
  EXPECT_TRUE((lists > 0) == expect_lists_in_hbm);
  if (expect_lists_in_hbm) {
    bool unused = false;
    EXPECT_TRUE(device_lists_untouched(*product->get_output(), &unused) == size_t{product->get_output()->chunk_count()} * product->get_output()->column_count());
    EXPECT_TRUE(device_lists_untouched(*last->get_output(), &unused) == size_t{last->get_output()->chunk_count()} * last->get_output()->column_count());
  }
  return last->get_output();
}

static void test_chain() {
  const auto left_table = load_table(g_tbl + "/join_test_runner/input_table_left_15.tbl", ChunkOffset{4}), right_table = load_table(g_tbl + "/join_test_runner/input_table_right_15.tbl", ChunkOffset{7});
  const auto left = wrap(left_table), right = wrap(right_table);
  device_resident_results() = true;
  const auto resident = run_chain(left, right, true);
  device_resident_results() = false;
  const auto on_host = run_chain(left, right, false);
  device_resident_results() = true;
  const auto got = sorted_rows(*resident);
  EXPECT_TRUE(got == sorted_rows(*on_host));
  EXPECT_TRUE(resident->chunk_count() == on_host->chunk_count());
  std::vector<std::string> want;   // the same query on the host: l_int <= 1338 AND r_int < 1338 over all pairs
  for (const auto& a : left_table->get_rows()) {
    for (const auto& b : right_table->get_rows()) {
      if (std::get<int32_t>(a[0]) > 1338 || std::get<int32_t>(b[0]) >= 1338) continue;
      auto row = a;
      row.insert(row.end(), b.begin(), b.end());
      want.push_back(row_text(row));
    }
  }
  std::sort(want.begin(), want.end());
  EXPECT_TRUE(!want.empty() && got == want);
}

// Product -> TableScan(left.a < right.b) is JoinNestedLoop Inner on the same predicate.
static void test_product_then_scan_is_a_join(bool reference_inputs) {
  const auto left_data = wrap(load_table(g_tbl + "/join_test_runner/input_table_left_15.tbl", ChunkOffset{4})), right_data = wrap(load_table(g_tbl + "/join_test_runner/input_table_right_15.tbl", ChunkOffset{7}));
  std::shared_ptr<const AbstractOperator> left = left_data, right = right_data;
  if (reference_inputs) {
    auto l = std::make_shared<TableScan>(left_data, ColumnID{0}, PredicateCondition::LessThanEquals, AllTypeVariant{int32_t{1338}});
    auto r = std::make_shared<TableScan>(right_data, ColumnID{0}, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{976}});
    l->execute();
    r->execute();
    left = l;
    right = r;
  }
  const ColumnID a{0}, b{0};   // l_int < r_int
  auto product = std::make_shared<Product>(left, right);
  product->execute();
  const ColumnID right_column = static_cast<ColumnID>(left->get_output()->column_count() + b);
  std::vector<std::string> got;
  try {
    auto scan = std::make_shared<TableScan>(product, a, PredicateCondition::LessThan, right_column, true);
    scan->execute();
    got = sorted_rows(*scan->get_output());
  } catch (const std::logic_error& e) {   // the library refuses this scan shape: the stock operator's comparison over the product's rows
    std::printf("  (ColumnVsColumn over the product stays with the host: %s)\n", e.what());
    for (const auto& row : product->get_output()->get_rows())
      if (std::get<int32_t>(row[a]) < std::get<int32_t>(row[right_column])) got.push_back(row_text(row));
    std::sort(got.begin(), got.end());
  }
  auto join = std::make_shared<JoinNestedLoop>(left, right, JoinMode::Inner, OperatorJoinPredicate{{a, b}, PredicateCondition::LessThan});
  join->execute();
  const auto want = sorted_rows(*join->get_output());
  EXPECT_TRUE(!want.empty() && got == want);
}

// tools/product_timing.py's second half: Product -> TableScan over left_rows x right_rows (one int column each, Hyrise chunks), device-resident
// results against host results in alternating pairs; host clock around the two execute() calls (every operator synchronises before it returns).
static int chain_timing(uint64_t left_rows, uint64_t right_rows, int pairs) {
  const auto make = [](uint64_t rows, const std::string& name) {
    auto table = std::make_shared<Table>(TableColumnDefinitions{{name, DataType::Int, false}}, TableType::Data);
    for (uint64_t r = 0; r < rows; ++r) table->append({AllTypeVariant{static_cast<int32_t>(r % 1000)}});
    table->finalize();
    return wrap(table);
  };
  const auto left = make(left_rows, "a"), right = make(right_rows, "b");
  const auto once = [&](bool resident, uint64_t* rows_out) {
    device_resident_results() = resident;
    const auto begin = std::chrono::steady_clock::now();
    auto product = std::make_shared<Product>(left, right);
    product->execute();
    auto scan = std::make_shared<TableScan>(product, ColumnID{1}, PredicateCondition::LessThan, AllTypeVariant{int32_t{10}});
    scan->execute();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
    *rows_out = scan->get_output()->row_count();
    return ms;
  };
  uint64_t rows = 0;
  (void)once(true, &rows);   // warm-up: code objects, pools, the inputs' residency
  int slower = 0;
  for (int p = 0; p < pairs; ++p) {
    uint64_t device_rows = 0, host_rows = 0;
    const double on_device = once(true, &device_rows), on_host = once(false, &host_rows);
    std::printf("pair %d: Product -> TableScan over %llu x %llu rows: device-resident %.2f ms, host results %.2f ms (%llu rows out%s)\n", p, static_cast<unsigned long long>(left_rows),
                static_cast<unsigned long long>(right_rows), on_device, on_host, static_cast<unsigned long long>(device_rows), device_rows == host_rows ? "" : ", ROW COUNTS DIFFER");
    if (on_device >= on_host || device_rows != host_rows) ++slower;
  }
  device_resident_results() = true;
  std::printf("%s\n", slower ? "CHAIN TIMING: device-resident results were not faster in every pair" : "CHAIN TIMING: device-resident results faster in every pair");
  return slower ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: product_tests <tbl directory> | product_tests --chain-timing <left rows> <right rows> <pairs>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  if (g_tbl == "--chain-timing" && argc == 5) {
    const int status = chain_timing(std::stoull(argv[2]), std::stoull(argv[3]), std::stoi(argv[4]));
    hy_shutdown();
    return status;
  }
  run("OperatorsProductTest.ValueSegments", [] { test_product(table_a, table_b, "int_float_product.tbl", ChunkOffset{3}); });
  run("OperatorsProductTest.ReferenceAndValueSegments", [] {
    test_product([] {
      auto scan = std::make_shared<TableScan>(table_a(), ColumnID{0}, PredicateCondition::GreaterThanEquals, AllTypeVariant{int32_t{1234}});
      scan->execute();
      return std::static_pointer_cast<const AbstractOperator>(scan);
    }, table_b, "int_filtered_float_product.tbl", ChunkOffset{3});
  });
  run("OperatorsProductTest.SelfProduct", [] {
    const auto c = wrap(load_table(g_tbl + "/product/int_int.tbl", ChunkOffset{2}));
    test_product([&] { return c; }, [&] { return c; }, "int_int_self_product.tbl", Chunk::DEFAULT_SIZE);
  });
  run("Product name", test_name);
  run("Product over an input behind two PosLists", test_two_lists_per_side);
  run("TableScan -> Product -> TableScan: PosLists stay in HBM, same rows as with host results", test_chain);
  run("Product -> TableScan(left.a < right.b) == JoinNestedLoop Inner, data inputs", [] { test_product_then_scan_is_a_join(false); });
  run("Product -> TableScan(left.a < right.b) == JoinNestedLoop Inner, reference inputs", [] { test_product_then_scan_is_a_join(true); });
  hy_shutdown();
  std::printf("%s\n", g_failures ? "PRODUCT TESTS FAILED" : "PRODUCT TESTS PASSED");
  return g_failures ? 1 : 0;
}

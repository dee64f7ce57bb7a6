// in_list_tests.cpp -- TableScan with PredicateCondition::In / NotIn over a literal list through the C++ mirror (hyrise_amd/host/
// hyrise_host.hpp), which scans on the device through hy_table_scan_in_list: every numeric column of the reference's JoinTestRunner tables
// in every encoding against a row-by-row evaluation of expression_evaluator.cpp:404-506's rule (not NULL and == some element / no element),
// string dictionaries, reference inputs, the constants the mirror answers on the host (empty list, NULL element, a list that is empty after
// hy_in_list_cast), and the chain TableScan(In) -> JoinHash -> AggregateHash with its PosLists in HBM against the same chain over the union
// of the elements' Equals scans.  That comparison side is the mirror's own Equals scans joined by its UnionPositions, not the CPU oracle:
// what pins the scans to an independent statement is expected_rows (row by row on the host), which the chain's scan is checked against too.
// Usage: in_list_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

static const auto IN = PredicateCondition::In;
static const auto NOT_IN = PredicateCondition::NotIn;
using List = std::vector<AllTypeVariant>;
using Rows = std::vector<std::vector<AllTypeVariant>>;

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

// operator== of two non-NULL variants as C++ compares the two types (integers exactly, anything else as double; strings with strings only)
static bool equal_cells(const AllTypeVariant& a, const AllTypeVariant& b) {
  const bool a_string = a.index() == 5, b_string = b.index() == 5;
  if (a_string || b_string) return a_string && b_string && std::get<std::string>(a) == std::get<std::string>(b);
  const auto integral = [](const AllTypeVariant& v) { return v.index() == 1 || v.index() == 2; };
  const auto as_long = [](const AllTypeVariant& v) { return v.index() == 1 ? static_cast<int64_t>(std::get<int32_t>(v)) : std::get<int64_t>(v); };
  const auto as_double = [&](const AllTypeVariant& v) { return integral(v) ? static_cast<double>(as_long(v)) : v.index() == 3 ? static_cast<double>(std::get<float>(v)) : std::get<double>(v); };
  if (integral(a) && integral(b)) return as_long(a) == as_long(b);
  return as_double(a) == as_double(b);
}

static bool same_rows(const Rows& a, const Rows& b) {
  if (a.size() != b.size()) { std::printf("  row counts differ: %zu vs %zu\n", a.size(), b.size()); return false; }
  for (size_t r = 0; r < a.size(); ++r)
    for (size_t c = 0; c < a[r].size(); ++c) {
      if (variant_is_null(a[r][c]) != variant_is_null(b[r][c])) { std::printf("  row %zu column %zu: NULL on one side\n", r, c); return false; }
      if (!variant_is_null(a[r][c]) && !equal_cells(a[r][c], b[r][c])) { std::printf("  row %zu column %zu differs\n", r, c); return false; }
    }
  return true;
}

// the rows of `table`, in order, that `column [NOT] IN (list)` keeps
static Rows expected_rows(const std::shared_ptr<const Table>& table, ColumnID column, const List& list, bool negated) {
  Rows out;
  bool has_null = false;
  for (const auto& element : list) has_null = has_null || variant_is_null(element);
  for (const auto& row : table->get_rows()) {
    if (list.empty()) { if (negated) out.push_back(row); continue; }   // x IN () is false, x NOT IN () true (expression_evaluator.cpp:415-419)
    if (variant_is_null(row[column])) continue;
    bool hit = false;
    for (const auto& element : list) hit = hit || (!variant_is_null(element) && equal_cells(row[column], element));
    if (negated ? (!hit && !has_null) : hit) out.push_back(row);
  }
  return out;
}

// every PosList of `table` lies in HBM (or names an entire chunk and holds no RowIDs at all)
static bool all_lists_on_device(const std::shared_ptr<const Table>& table) {
  for (ChunkID c = 0; c < table->chunk_count(); ++c)
    for (ColumnID col = 0; col < table->column_count(); ++col) {
      const auto ref = std::dynamic_pointer_cast<const ReferenceSegment>(table->get_chunk(c)->get_segment(col));
      if (!ref || !(dynamic_cast<const DevicePosList*>(ref->pos_list().get()) || dynamic_cast<const EntireChunkPosList*>(ref->pos_list().get()))) return false;   // (a chunk that matches entirely: table_scan.cpp:201-205)
    }
  return true;
}

static bool some_list_on_device(const std::shared_ptr<const Table>& table) {
  for (ChunkID c = 0; c < table->chunk_count(); ++c) {
    const auto ref = std::dynamic_pointer_cast<const ReferenceSegment>(table->get_chunk(c)->get_segment(0));
    if (ref && dynamic_cast<const DevicePosList*>(ref->pos_list().get())) return true;
  }
  return false;
}

static std::shared_ptr<Table> load(const std::string& name, ChunkOffset chunk_size, int encoding) {   // 0: unencoded, 1: dictionary, 2: FrameOfReference where it applies
  auto table = load_table(g_tbl + "/join_test_runner/" + name, chunk_size);
  if (encoding == 1) ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  if (encoding == 2) ChunkEncoder::encode_all_chunks(table, EncodingType::FrameOfReference);
  return table;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: in_list_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const auto i32 = [](int32_t v) { return AllTypeVariant{v}; };
  const auto i64 = [](int64_t v) { return AllTypeVariant{v}; };
  const auto f32 = [](float v) { return AllTypeVariant{v}; };
  const auto f64 = [](double v) { return AllTypeVariant{v}; };
  const AllTypeVariant null{NullValue{}};
  // lists per numeric column of input_table_left_*: present and absent values, duplicates, unsorted
  const std::vector<std::pair<ColumnID, List>> lists = {
      {ColumnID{0}, {i32(1337), i32(7331), i32(5), i32(1337)}},          {ColumnID{1}, {i32(724), i32(1338), i32(-3), i32(99999), i32(724)}},
      {ColumnID{2}, {f32(1337.0f), f32(724.3f), f32(0.5f), f32(1337.7f)}}, {ColumnID{3}, {f32(1338.0f), f32(1337.2f), f32(1.0f), f32(1338.0f)}},
      {ColumnID{4}, {f64(4294968633.0), f64(1337.7), f64(2.0), f64(7331.6)}}, {ColumnID{5}, {f64(724.3), f64(1338.0), f64(1337.2), f64(9.0)}},
      {ColumnID{6}, {i64(1337), i64(724), i64(4294968633), i64(-1)}},   {ColumnID{7}, {i64(1338), i64(7331), i64(12), i64(1338)}}};

  run("InListTest.EveryNumericColumnAndEncoding", [&] {
    for (const char* name : {"input_table_left_15.tbl", "input_table_left_10.tbl", "input_table_left_0.tbl"})
      for (const ChunkOffset chunk_size : {ChunkOffset{1}, ChunkOffset{4}, ChunkOffset{100}})
        for (int encoding = 0; encoding < 3; ++encoding) {
          const auto table = load(name, chunk_size, encoding);
          const auto input = wrap(table);
          for (const auto& [column, list] : lists)
            for (const auto condition : {IN, NOT_IN}) {
              const auto scan = executed<TableScan>(input, column, condition, list);
              EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), expected_rows(table, column, list, condition == NOT_IN)));
              EXPECT_TRUE(all_lists_on_device(scan->get_output()));
            }
        }
  });
  run("InListTest.MixedTypesNullsAndConstants", [&] {
    const auto table = load("input_table_left_15.tbl", ChunkOffset{4}, 1);
    const auto input = wrap(table);
    const std::vector<std::pair<ColumnID, List>> cases = {
        {ColumnID{0}, {i32(1337), f64(1338.0), f64(1337.5), i64(int64_t{1} << 40), null}},   // int column: 2.0-like doubles are kept, 2.5-like and 2^40 dropped
        {ColumnID{0}, {i32(1337), f64(7331.0)}},
        {ColumnID{1}, {null, i32(1338)}},
        {ColumnID{1}, {null}},
        {ColumnID{1}, {}},
        {ColumnID{0}, {}},
        {ColumnID{1}, {f64(0.5), AllTypeVariant{std::string{"1338"}}}},                      // nothing left after the cast
        {ColumnID{2}, {f64(0.1), f64(1337.0), f64(724.3)}},                                   // float column: no float equals the double 724.3
        {ColumnID{6}, {i32(1337), i32(724), f32(1338.0f)}},                                   // long column, int and float elements
        {ColumnID{7}, {i32(1338), null, i32(7331)}}};
    for (const auto& [column, list] : cases)
      for (const auto condition : {IN, NOT_IN}) {
        const auto scan = executed<TableScan>(input, column, condition, list);
        EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), expected_rows(table, column, list, condition == NOT_IN)));
      }
  });
  run("InListTest.StringDictionaries", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{3}, ChunkOffset{100}}) {
      const auto table = load("input_table_left_15.tbl", chunk_size, 1);
      const auto input = wrap(table);
      const auto s = [](const char* v) { return AllTypeVariant{std::string{v}}; };
      for (const ColumnID column : {ColumnID{8}, ColumnID{9}})
        for (const List& list : {List{s("o"), s("d"), s("zz"), s("o")}, List{s("a")}, List{s("nothing")}, List{s("r"), null}, List{s("d"), i32(5)}})
          for (const auto condition : {IN, NOT_IN}) {
            const auto scan = executed<TableScan>(input, column, condition, list);
            EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), expected_rows(table, column, list, condition == NOT_IN)));
          }
    }
  });
  run("InListTest.ReferenceInputs", [&] {
    for (int encoding = 0; encoding < 3; ++encoding) {
      const auto table = load("input_table_left_15.tbl", ChunkOffset{4}, encoding);
      const auto input = wrap(table);
      const auto first = executed<TableScan>(input, ColumnID{0}, PredicateCondition::GreaterThan, i32(1000));
      const auto kept = first->get_output();
      for (const auto& [column, list] : lists)
        for (const auto condition : {IN, NOT_IN}) {
          const auto scan = executed<TableScan>(first, column, condition, list);
          EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), expected_rows(kept, column, list, condition == NOT_IN)));
        }
    }
  });
  run("InListChain.ScanJoinAggregateStaysInHbm", [&] {
    // TableScan(l_int IN (...)) -> JoinHash(l_int = r_int) -> AggregateHash(COUNT(*), SUM(r_long) GROUP BY l_int), PosLists in HBM, against
    // the same chain over UnionPositions of the elements' Equals scans
    const auto left_table = load("input_table_left_15.tbl", ChunkOffset{4}, 1), right_table = load("input_table_right_15.tbl", ChunkOffset{4}, 1);
    const auto left = wrap(left_table), right = wrap(right_table);
    const List list = {i32(1338), i32(1337), i32(9331), i32(42)};
    const auto scan = executed<TableScan>(left, ColumnID{0}, IN, list);
    EXPECT_TRUE(scan->get_output()->row_count() > 0 && scan->get_output()->row_count() < left_table->row_count());
    EXPECT_TRUE(all_lists_on_device(scan->get_output()));
    EXPECT_TRUE(some_list_on_device(scan->get_output()));
    const auto join = executed<JoinHash>(scan, right, JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
    EXPECT_TRUE(join->get_output()->row_count() > 0);
    EXPECT_TRUE(all_lists_on_device(join->get_output()));
    EXPECT_TRUE(some_list_on_device(join->get_output()));
    const std::vector<AggregateDefinition> aggregates{{INVALID_COLUMN_ID, WindowFunction::Count}, {ColumnID{16}, WindowFunction::Sum}};
    const auto aggregate = executed<AggregateHash>(join, aggregates, std::vector<ColumnID>{ColumnID{0}});

    std::shared_ptr<const AbstractOperator> united = executed<TableScan>(left, ColumnID{0}, PredicateCondition::Equals, list[0]);
    for (size_t e = 1; e < list.size(); ++e) united = executed<UnionPositions>(united, executed<TableScan>(left, ColumnID{0}, PredicateCondition::Equals, list[e]));
    EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), united->get_output()->get_rows()));
    EXPECT_TRUE(same_rows(scan->get_output()->get_rows(), expected_rows(left_table, ColumnID{0}, list, false)));
    const auto want_join = executed<JoinHash>(united, right, JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
    const auto want = executed<AggregateHash>(want_join, aggregates, std::vector<ColumnID>{ColumnID{0}});
    auto got_rows = aggregate->get_output()->get_rows(), want_rows = want->get_output()->get_rows();
    const auto by_key = [](const std::vector<AllTypeVariant>& a, const std::vector<AllTypeVariant>& b) { return std::get<int32_t>(a[0]) < std::get<int32_t>(b[0]); };
    std::sort(got_rows.begin(), got_rows.end(), by_key);
    std::sort(want_rows.begin(), want_rows.end(), by_key);
    EXPECT_TRUE(!got_rows.empty() && same_rows(got_rows, want_rows));
  });

  std::printf(g_failures ? "IN LIST TESTS FAILED: %d\n" : "IN LIST TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

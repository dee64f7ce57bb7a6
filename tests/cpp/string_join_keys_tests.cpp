// string_join_keys_tests.cpp -- JoinHash and JoinSortMerge on string keys through the C++ mirror (hyrise_amd/host/hyrise_host.hpp): the keys
// of both columns are made on the device for the pair (device_string_join_key_columns -> hy_column_string_join_keys) and no string is hashed
// or compared on the host.  JoinHash: the output table with device_string_join_keys() on is the table with it off (ids from string_join_id),
// cell for cell and chunk for chunk -- data tables, a TableScan's output, four modes, a secondary predicate.  JoinSortMerge: against a
// nested loop over the strings, unordered.  A ValueSegment<pmr_string> chunk keeps JoinHash on its host route and JoinSortMerge refusing.
// And the chains TableScan (LIKE) -> JoinHash on strings -> AggregateHash, over base tables and over a string column an AggregateHash left in
// HBM, whose strings never come to the host.  Every run on the device route is counted (device_string_join_key_pairs).
// Usage: string_join_keys_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

static std::string cell(const AllTypeVariant& value) {
  return std::visit([](const auto& v) -> std::string {
    using T = std::decay_t<decltype(v)>;
    if constexpr (std::is_same_v<T, NullValue>) return "NULL";
    else if constexpr (std::is_same_v<T, std::string>) return "s" + v;
    else return std::to_string(v);
  }, value);
}

static std::string line(const Row& row) {
  std::string out;
  for (const auto& value : row) out += cell(value) + "|";
  return out;
}

// the same table: chunk for chunk, row for row, cell for cell
static bool same_tables(const std::shared_ptr<const Table>& a, const std::shared_ptr<const Table>& b) {
  if (a->chunk_count() != b->chunk_count() || a->column_count() != b->column_count()) return false;
  for (ChunkID k{0}; k < a->chunk_count(); ++k) if (a->get_chunk(k)->size() != b->get_chunk(k)->size()) return false;
  const auto rows_a = a->get_rows(), rows_b = b->get_rows();
  if (rows_a.size() != rows_b.size()) return false;
  for (size_t r = 0; r < rows_a.size(); ++r) if (line(rows_a[r]) != line(rows_b[r])) return false;
  return true;
}

static std::map<std::string, size_t> multiset(const Rows& rows) {
  std::map<std::string, size_t> out;
  for (const auto& row : rows) ++out[line(row)];
  return out;
}

// LEFT: ORDERKEY int, LINENUMBER int, SHIPMODE string (7 distinct, NULL in every fifth row or so), COMMENT string
static const ColumnID ORDERKEY{0}, LINENUMBER{1}, SHIPMODE{2}, COMMENT{3};
// RIGHT: ID int, MODE string (shipmodes twice or three times, two strings no lineitem has, NULLs), WEIGHT int
static const ColumnID ID{0}, MODE{1}, WEIGHT{2};

static Rows lineitem_rows() {
  const auto table = load_table(g_tbl + "/tpch/sf-0.001/lineitem.tbl", ChunkOffset{65535});
  Rows rows;
  for (const auto& row : table->get_rows()) {
    const int32_t orderkey = std::get<int32_t>(row[0]), linenumber = std::get<int32_t>(row[3]);
    rows.push_back(Row{orderkey, linenumber, (orderkey + linenumber) % 5 == 0 ? AllTypeVariant{NullValue{}} : row[14], row[15]});
  }
  return rows;
}

static Rows mode_rows() {
  const char* modes[] = {"AIR", "MAIL", "SHIP", "TRUCK", "REG AIR", "RAIL", "FOB", "AIR", "PIGEON", "MAIL", "", "AIR", "RAIL", "REG AIR ", "TRUCK"};
  Rows rows;
  int32_t id = 0;
  for (const char* mode : modes) {
    rows.push_back(Row{id, id % 6 == 4 ? AllTypeVariant{NullValue{}} : AllTypeVariant{std::string(mode)}, int32_t{3 + id % 4}});
    ++id;
  }
  return rows;
}

// `unencoded_tail`: the last chunk stays a chunk of ValueSegments
static std::shared_ptr<Table> make_table(const TableColumnDefinitions& definitions, const Rows& rows, ChunkOffset chunk_size, size_t unencoded_tail = 0) {
  auto table = std::make_shared<Table>(definitions, TableType::Data, chunk_size);
  const size_t tail = std::min(rows.size(), unencoded_tail);
  for (size_t r = 0; r + tail < rows.size(); ++r) table->append(rows[r]);
  table->finalize();
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  for (size_t r = rows.size() - tail; r < rows.size(); ++r) table->append(rows[r]);
  table->finalize();
  return table;
}

static const TableColumnDefinitions LEFT_DEFINITIONS{{"orderkey", DataType::Int, false}, {"linenumber", DataType::Int, false}, {"shipmode", DataType::String, true}, {"comment", DataType::String, false}};
static const TableColumnDefinitions RIGHT_DEFINITIONS{{"id", DataType::Int, false}, {"mode", DataType::String, true}, {"weight", DataType::Int, false}};

// the operator with its keys made on the device: exactly one pair of stand-ins came from hy_column_string_join_keys
template <typename Op, typename... Args>
static std::shared_ptr<const Table> on_the_device(Args&&... args) {
  const uint64_t pairs = device_string_join_key_pairs().load();
  const auto out = executed<Op>(std::forward<Args>(args)...)->get_output();
  EXPECT_TRUE(device_string_join_key_pairs().load() == pairs + 1);
  return out;
}

// the same operator with the keys made on the host: none did
template <typename Op, typename... Args>
static std::shared_ptr<const Table> on_the_host(Args&&... args) {
  const uint64_t pairs = device_string_join_key_pairs().load();
  device_string_join_keys() = false;
  std::shared_ptr<const Table> out;
  try { out = executed<Op>(std::forward<Args>(args)...)->get_output(); } catch (...) { device_string_join_keys() = true; throw; }
  device_string_join_keys() = true;
  EXPECT_TRUE(device_string_join_key_pairs().load() == pairs);
  return out;
}

static bool strings_match(const AllTypeVariant& a, const AllTypeVariant& b, PredicateCondition condition) {
  if (variant_is_null(a) || variant_is_null(b)) return false;
  const auto& x = std::get<std::string>(a);
  const auto& y = std::get<std::string>(b);
  switch (condition) {
    case PredicateCondition::Equals: return x == y;
    case PredicateCondition::NotEquals: return x != y;
    case PredicateCondition::LessThan: return x < y;
    case PredicateCondition::LessThanEquals: return x <= y;
    case PredicateCondition::GreaterThan: return x > y;
    default: return x >= y;
  }
}

static Row joined(const Row* l, const Row* r, size_t left_columns, size_t right_columns) {
  Row out;
  for (size_t c = 0; c < left_columns; ++c) out.push_back(l ? (*l)[c] : AllTypeVariant{NullValue{}});
  for (size_t c = 0; c < right_columns; ++c) out.push_back(r ? (*r)[c] : AllTypeVariant{NullValue{}});
  return out;
}

// the join row by row; Left / FullOuter add the unmatched rows, Semi / Anti keep left rows
static Rows nested_loop(const Rows& left, ColumnID left_key, const Rows& right, ColumnID right_key, JoinMode mode, PredicateCondition condition,
                        const std::function<bool(const Row&, const Row&)>& secondary = nullptr) {
  Rows out;
  std::vector<bool> right_matched(right.size(), false);
  for (const auto& l : left) {
    bool any = false;
    for (size_t j = 0; j < right.size(); ++j) {
      if (!strings_match(l[left_key], right[j][right_key], condition) || (secondary && !secondary(l, right[j]))) continue;
      any = true;
      right_matched[j] = true;
      if (mode == JoinMode::Inner || mode == JoinMode::Left || mode == JoinMode::FullOuter) out.push_back(joined(&l, &right[j], l.size(), right[j].size()));
    }
    if (!any && (mode == JoinMode::Left || mode == JoinMode::FullOuter)) out.push_back(joined(&l, nullptr, l.size(), right.empty() ? 0 : right[0].size()));
    if (mode == JoinMode::Semi ? any : ((mode == JoinMode::AntiNullAsTrue && !any && !variant_is_null(l[left_key])) || (mode == JoinMode::AntiNullAsFalse && !any))) out.push_back(l);
  }
  if (mode == JoinMode::FullOuter)
    for (size_t j = 0; j < right.size(); ++j) if (!right_matched[j]) out.push_back(joined(nullptr, &right[j], left.empty() ? 0 : left[0].size(), right[j].size()));
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: string_join_keys_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const Rows left_rows = lineitem_rows(), right_rows = mode_rows();
  const JoinMode hash_modes[] = {JoinMode::Inner, JoinMode::Left, JoinMode::Semi, JoinMode::AntiNullAsTrue};

  run("StringJoinKeys.JoinHashOnAndOffDataTables", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1000}, ChunkOffset{257}}) {
      const auto left = wrap(make_table(LEFT_DEFINITIONS, left_rows, chunk_size)), right = wrap(make_table(RIGHT_DEFINITIONS, right_rows, ChunkOffset{4}));
      for (const JoinMode mode : hash_modes) {
        for (const std::optional<size_t> radix_bits : {std::optional<size_t>{}, std::optional<size_t>{3}}) {
          const auto on = on_the_device<JoinHash>(left, right, mode, ColumnIDPair{SHIPMODE, MODE}, radix_bits);
          const auto off = on_the_host<JoinHash>(left, right, mode, ColumnIDPair{SHIPMODE, MODE}, radix_bits);
          // (the right keys hold NULLs: NOT IN over them keeps no row, with either kind of keys; the runner tables below have a column without)
          EXPECT_TRUE((on->row_count() > 0 || mode == JoinMode::AntiNullAsTrue) && same_tables(on, off));
          if (mode != JoinMode::AntiNullAsTrue) EXPECT_TRUE(multiset(on->get_rows()) == multiset(nested_loop(left_rows, SHIPMODE, right_rows, MODE, mode, PredicateCondition::Equals)));
        }
      }
      // both ways round: the small table builds either way, the key columns change sides
      const auto on = on_the_device<JoinHash>(right, left, JoinMode::Inner, ColumnIDPair{MODE, SHIPMODE});
      EXPECT_TRUE(same_tables(on, on_the_host<JoinHash>(right, left, JoinMode::Inner, ColumnIDPair{MODE, SHIPMODE})));
      EXPECT_TRUE(multiset(on->get_rows()) == multiset(nested_loop(right_rows, MODE, left_rows, SHIPMODE, JoinMode::Inner, PredicateCondition::Equals)));
    }
  });
  run("StringJoinKeys.JoinHashOnAndOffRunnerTables", [&] {   // the fixtures of the mirror's first string join test
    for (const auto chunk : {ChunkOffset{4}, ChunkOffset{10}}) {
      auto left_table = load_table(g_tbl + "/join_test_runner/input_table_left_15.tbl", chunk), right_table = load_table(g_tbl + "/join_test_runner/input_table_right_10.tbl", ChunkOffset{3});
      ChunkEncoder::encode_all_chunks(left_table, EncodingType::Dictionary);
      ChunkEncoder::encode_all_chunks(right_table, EncodingType::Dictionary);
      const auto left = wrap(left_table), right = wrap(right_table);
      for (const ColumnID column : {ColumnID{8}, ColumnID{9}}) {   // string, string_null
        for (const JoinMode mode : hash_modes) {
          const auto on = on_the_device<JoinHash>(left, right, mode, ColumnIDPair{column, column}, 3);
          EXPECT_TRUE(same_tables(on, on_the_host<JoinHash>(left, right, mode, ColumnIDPair{column, column}, 3)));
        }
      }
    }
  });
  run("StringJoinKeys.JoinHashOverATableScansOutputAndASecondaryPredicate", [&] {
    const auto left = wrap(make_table(LEFT_DEFINITIONS, left_rows, ChunkOffset{700})), right = wrap(make_table(RIGHT_DEFINITIONS, right_rows, ChunkOffset{4}));
    const auto scan = executed<TableScan>(left, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    Rows kept;
    for (const auto& row : left_rows) if (std::get<int32_t>(row[ORDERKEY]) > 3000) kept.push_back(row);
    EXPECT_TRUE(!kept.empty() && kept.size() < left_rows.size());
    for (const JoinMode mode : hash_modes) {
      const auto on = on_the_device<JoinHash>(scan, right, mode, ColumnIDPair{SHIPMODE, MODE});
      EXPECT_TRUE((on->row_count() > 0 || mode == JoinMode::AntiNullAsTrue) && same_tables(on, on_the_host<JoinHash>(scan, right, mode, ColumnIDPair{SHIPMODE, MODE})));
      if (mode != JoinMode::AntiNullAsTrue) EXPECT_TRUE(multiset(on->get_rows()) == multiset(nested_loop(kept, SHIPMODE, right_rows, MODE, mode, PredicateCondition::Equals)));
    }
    const std::vector<OperatorJoinPredicate> secondary{OperatorJoinPredicate{ColumnIDPair{LINENUMBER, WEIGHT}, PredicateCondition::LessThan}};
    const auto holds = [](const Row& l, const Row& r) { return std::get<int32_t>(l[LINENUMBER]) < std::get<int32_t>(r[WEIGHT]); };
    for (const JoinMode mode : {JoinMode::Inner, JoinMode::Left, JoinMode::Semi}) {
      const auto on = on_the_device<JoinHash>(scan, right, mode, ColumnIDPair{SHIPMODE, MODE}, std::nullopt, secondary);
      EXPECT_TRUE(on->row_count() > 0 && same_tables(on, on_the_host<JoinHash>(scan, right, mode, ColumnIDPair{SHIPMODE, MODE}, std::nullopt, secondary)));
      EXPECT_TRUE(multiset(on->get_rows()) == multiset(nested_loop(kept, SHIPMODE, right_rows, MODE, mode, PredicateCondition::Equals, holds)));
    }
  });
  run("StringJoinKeys.JoinSortMergeAgainstANestedLoop", [&] {
    const auto left = wrap(make_table(LEFT_DEFINITIONS, left_rows, ChunkOffset{1000})), right = wrap(make_table(RIGHT_DEFINITIONS, right_rows, ChunkOffset{4}));
    const auto scan = executed<TableScan>(left, ORDERKEY, PredicateCondition::LessThan, AllTypeVariant{int32_t{600}});
    Rows kept;
    for (const auto& row : left_rows) if (std::get<int32_t>(row[ORDERKEY]) < 600) kept.push_back(row);
    const OperatorJoinPredicate equals{ColumnIDPair{SHIPMODE, MODE}, PredicateCondition::Equals};
    for (const JoinMode mode : {JoinMode::Inner, JoinMode::Left, JoinMode::FullOuter}) {
      const auto got = on_the_device<JoinSortMerge>(left, right, mode, equals)->get_rows();
      EXPECT_TRUE(!got.empty() && multiset(got) == multiset(nested_loop(left_rows, SHIPMODE, right_rows, MODE, mode, PredicateCondition::Equals)));
    }
    for (const auto condition : {PredicateCondition::LessThan, PredicateCondition::GreaterThanEquals, PredicateCondition::NotEquals}) {   // (over the scan's output: fewer pairs)
      const auto got = on_the_device<JoinSortMerge>(scan, right, JoinMode::Inner, OperatorJoinPredicate{ColumnIDPair{SHIPMODE, MODE}, condition})->get_rows();
      EXPECT_TRUE(!got.empty() && multiset(got) == multiset(nested_loop(kept, SHIPMODE, right_rows, MODE, JoinMode::Inner, condition)));
    }
    bool refused = false;   // the switch off: as before
    try { on_the_host<JoinSortMerge>(left, right, JoinMode::Inner, equals); } catch (const std::logic_error&) { refused = true; }
    EXPECT_TRUE(refused);
  });
  run("StringJoinKeys.AValueSegmentChunkKeepsTheHostRoute", [&] {
    // the last 300 rows stay a chunk of ValueSegments, NULL keys among them; the right keys without NULLs, so that NOT IN keeps rows
    const auto left_table = make_table(LEFT_DEFINITIONS, left_rows, ChunkOffset{1000}, 300);
    const auto* tail = dynamic_cast<const ValueSegment<std::string>*>(left_table->get_chunk(ChunkID{left_table->chunk_count() - 1})->get_segment(SHIPMODE).get());
    EXPECT_TRUE(tail != nullptr);
    size_t tail_nulls = 0;
    for (ChunkOffset row = 0; tail && row < tail->size(); ++row) tail_nulls += tail->is_null(row);
    EXPECT_TRUE(tail_nulls > 10);
    Rows present_modes;
    for (const auto& row : right_rows) if (!variant_is_null(row[MODE])) present_modes.push_back(row);
    const auto left = wrap(left_table), right = wrap(make_table(RIGHT_DEFINITIONS, present_modes, ChunkOffset{4}));
    const uint64_t pairs = device_string_join_key_pairs().load();
    for (const JoinMode mode : {JoinMode::Inner, JoinMode::Semi, JoinMode::Left, JoinMode::AntiNullAsTrue, JoinMode::AntiNullAsFalse}) {
      const auto on = executed<JoinHash>(left, right, mode, ColumnIDPair{SHIPMODE, MODE})->get_output();
      EXPECT_TRUE(left_table->device_columns && left_table->device_columns->columns.count({SHIPMODE, StringKeys::JoinIds}) == 1);   // (ids from string_join_id)
      EXPECT_TRUE(on->row_count() > 0 && multiset(on->get_rows()) == multiset(nested_loop(left_rows, SHIPMODE, present_modes, MODE, mode, PredicateCondition::Equals)));
    }
    // the unencoded chunk, NULL keys and all, on the right of a Left join
    const auto flipped = executed<JoinHash>(right, left, JoinMode::Left, ColumnIDPair{MODE, SHIPMODE})->get_output();
    EXPECT_TRUE(multiset(flipped->get_rows()) == multiset(nested_loop(present_modes, MODE, left_rows, SHIPMODE, JoinMode::Left, PredicateCondition::Equals)));
    EXPECT_TRUE(device_string_join_key_pairs().load() == pairs);
    bool refused = false;
    try { executed<JoinSortMerge>(left, right, JoinMode::Inner, OperatorJoinPredicate{ColumnIDPair{SHIPMODE, MODE}, PredicateCondition::Equals}); } catch (const std::logic_error&) { refused = true; }
    EXPECT_TRUE(refused);
  });
  run("StringJoinKeysChain.ScanJoinAggregateWithoutAFetch", [&] {
    const auto left_table = make_table(LEFT_DEFINITIONS, left_rows, ChunkOffset{1000});
    const auto left = wrap(left_table), right = wrap(make_table(RIGHT_DEFINITIONS, right_rows, ChunkOffset{4}));
    const uint64_t string_fetches = device_string_segment_fetches().load(), value_fetches = device_value_segment_fetches().load();
    const auto scan = executed<TableScan>(left, COMMENT, PredicateCondition::Like, AllTypeVariant{std::string("%the%")});
    const auto join = executed<JoinHash>(scan, right, JoinMode::Inner, ColumnIDPair{SHIPMODE, MODE});
    const ColumnID weight = static_cast<ColumnID>(LEFT_DEFINITIONS.size() + WEIGHT);
    const auto aggregate = executed<AggregateHash>(join, std::vector<AggregateDefinition>{AggregateDefinition{LINENUMBER, WindowFunction::Sum}}, std::vector<ColumnID>{weight});
    EXPECT_TRUE(device_string_segment_fetches().load() == string_fetches && device_value_segment_fetches().load() == value_fetches);
    // the join's keys came from the device: no host-made ids were cached for either column
    EXPECT_TRUE(!left_table->device_columns || left_table->device_columns->columns.count({SHIPMODE, StringKeys::JoinIds}) == 0);
    std::map<int32_t, int64_t> sums;
    for (const auto& l : left_rows) {
      if (std::get<std::string>(l[COMMENT]).find("the") == std::string::npos) continue;
      for (const auto& r : right_rows) if (strings_match(l[SHIPMODE], r[MODE], PredicateCondition::Equals)) sums[std::get<int32_t>(r[WEIGHT])] += std::get<int32_t>(l[LINENUMBER]);
    }
    const auto got = aggregate->get_output()->get_rows();
    EXPECT_TRUE(sums.size() == 4 && got.size() == sums.size());
    for (const auto& row : got) EXPECT_TRUE(sums.count(std::get<int32_t>(row[0])) && sums[std::get<int32_t>(row[0])] == std::get<int64_t>(row[1]));
  });

  run("StringJoinKeysChain.AStringColumnMadeInHBMJoinsWithoutAFetch", [&] {
    // AggregateHash leaves its GROUP BY column -- the ship modes -- in HBM; a LIKE scan over it, the join on it and the aggregate behind the
    // join read it there: a key made on the host would have to fetch the segment's dictionary first
    const auto left = wrap(make_table(LEFT_DEFINITIONS, left_rows, ChunkOffset{1000})), right = wrap(make_table(RIGHT_DEFINITIONS, right_rows, ChunkOffset{4}));
    const uint64_t string_fetches = device_string_segment_fetches().load(), value_fetches = device_value_segment_fetches().load();
    const auto modes = executed<AggregateHash>(left, std::vector<AggregateDefinition>{AggregateDefinition{INVALID_COLUMN_ID, WindowFunction::Count}}, std::vector<ColumnID>{SHIPMODE});
    const auto scan = executed<TableScan>(modes, ColumnID{0}, PredicateCondition::Like, AllTypeVariant{std::string("%A%")});
    const auto join = on_the_device<JoinHash>(scan, right, JoinMode::Inner, ColumnIDPair{ColumnID{0}, MODE});
    const ColumnID weight = static_cast<ColumnID>(2 + WEIGHT);
    const auto aggregate = executed<AggregateHash>(wrap(join), std::vector<AggregateDefinition>{AggregateDefinition{ColumnID{1}, WindowFunction::Sum}}, std::vector<ColumnID>{weight});
    EXPECT_TRUE(device_string_segment_fetches().load() == string_fetches && device_value_segment_fetches().load() == value_fetches);
    const auto got = aggregate->get_output()->get_rows();
    EXPECT_TRUE(device_string_segment_fetches().load() == string_fetches && device_value_segment_fetches().load() > value_fetches);   // (the sums came; no string ever did)
    std::map<std::string, int64_t> count_of;
    for (const auto& l : left_rows) if (!variant_is_null(l[SHIPMODE])) ++count_of[std::get<std::string>(l[SHIPMODE])];
    std::map<int32_t, int64_t> sums;
    for (const auto& [mode, count] : count_of) {
      if (mode.find('A') == std::string::npos) continue;
      for (const auto& r : right_rows) if (!variant_is_null(r[MODE]) && std::get<std::string>(r[MODE]) == mode) sums[std::get<int32_t>(r[WEIGHT])] += count;
    }
    EXPECT_TRUE(sums.size() >= 3 && got.size() == sums.size());
    for (const auto& row : got) EXPECT_TRUE(sums.count(std::get<int32_t>(row[0])) && sums[std::get<int32_t>(row[0])] == std::get<int64_t>(row[1]));
  });

  std::printf(g_failures ? "STRING JOIN KEYS TESTS FAILED: %d\n" : "STRING JOIN KEYS TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

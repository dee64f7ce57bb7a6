// string_order_tests.cpp -- Sort by a string column through the C++ mirror (hyrise_amd/host/hyrise_host.hpp): the key column's ranks are made
// on the device (device_string_rank_column: the residency cache's device_string_dictionary, then hy_column_string_ranks) and no string is
// copied or compared on the host.  Checked against std::stable_sort over the strings row by row: over a data table and over a TableScan's
// output, ascending and descending, with NULLs, two keys, a row limit, a materialised output; the forced host ranking gives the identical
// table; a ValueSegment<pmr_string> chunk still sorts (host_key_table); and the chain TableScan -> Sort -> Limit.
// Usage: string_order_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>
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

// `unencoded_tail`: the last chunk stays a chunk of ValueSegments
static std::shared_ptr<Table> make_table(const Rows& rows, ChunkOffset chunk_size, bool unencoded_tail = false) {
  const TableColumnDefinitions definitions{{"orderkey", DataType::Int, false}, {"linenumber", DataType::Int, false}, {"shipmode", DataType::String, true}, {"comment", DataType::String, false}};
  auto table = std::make_shared<Table>(definitions, TableType::Data, chunk_size);
  const size_t tail = unencoded_tail ? std::min<size_t>(rows.size(), 300) : 0;
  for (size_t r = 0; r + tail < rows.size(); ++r) table->append(rows[r]);
  table->finalize();
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  for (size_t r = rows.size() - tail; r < rows.size(); ++r) table->append(rows[r]);
  table->finalize();
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
    for (size_t c = 0; c < got[r].size(); ++c)
      if (cell(got[r][c]) != cell(want[r][c])) return false;
  }
  return true;
}

// Sort's contract on the host: one std::stable_sort per definition, from the last to the first; NULLs first in both directions
static Rows stable_sorted(Rows rows, const std::vector<SortColumnDefinition>& definitions) {
  for (size_t d = definitions.size(); d-- > 0;) {
    const ColumnID column = definitions[d].column;
    const bool descending = definitions[d].sort_mode == SortMode::DescendingNullsFirst;
    std::stable_sort(rows.begin(), rows.end(), [&](const Row& a, const Row& b) {
      const bool a_null = variant_is_null(a[column]), b_null = variant_is_null(b[column]);
      if (a_null || b_null) return a_null && !b_null;
      if (const auto* s = std::get_if<std::string>(&a[column])) return descending ? *s > std::get<std::string>(b[column]) : *s < std::get<std::string>(b[column]);
      return descending ? std::get<int32_t>(a[column]) > std::get<int32_t>(b[column]) : std::get<int32_t>(a[column]) < std::get<int32_t>(b[column]);
    });
  }
  return rows;
}

// how the cached sort key of (table, column) was made: on the device (an int32 stand-in, no key names) or on the host (int64 ranks)
static bool ranked_on_device(const std::shared_ptr<const Table>& table, ColumnID column) {
  if (!table->device_columns) return false;
  const auto found = table->device_columns->columns.find({column, StringKeys::Ranks});
  if (found == table->device_columns->columns.end() || !found->second) return false;
  return found->second->key_names.empty() && hy_column_data_type(found->second->handle) == HY_TYPE_INT;
}
static bool ranked_on_host(const std::shared_ptr<const Table>& table, ColumnID column) {
  if (!table->device_columns) return false;
  const auto found = table->device_columns->columns.find({column, StringKeys::Ranks});
  if (found == table->device_columns->columns.end() || !found->second) return false;
  return !found->second->key_names.empty() && hy_column_data_type(found->second->handle) == HY_TYPE_LONG;
}

// the same Sort with the host ranking forced: the identical table
template <typename... Args>
static Rows host_ranked(const std::shared_ptr<const AbstractOperator>& in, const std::shared_ptr<const Table>& table, ColumnID column, Args&&... args) {
  device_string_ranking() = false;
  Rows rows;
  try {
    rows = executed<Sort>(in, std::forward<Args>(args)...)->get_output()->get_rows();
    EXPECT_TRUE(ranked_on_host(table, column));
  } catch (...) { device_string_ranking() = true; throw; }
  device_string_ranking() = true;
  return rows;
}

static const SortMode ASC = SortMode::AscendingNullsFirst, DESC = SortMode::DescendingNullsFirst;

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: string_order_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const Rows rows = lineitem_rows();

  run("StringOrder.DataTableAgainstStableSort", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1000}, ChunkOffset{257}, ChunkOffset{65535}}) {
      for (const ColumnID column : {SHIPMODE, COMMENT}) {
        for (const SortMode mode : {ASC, DESC}) {
          const auto table = make_table(rows, chunk_size);   // (a table of its own: the first Sort builds the cache)
          const auto input = wrap(table);
          const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{column, mode}};
          const auto got = executed<Sort>(input, definitions)->get_output()->get_rows();
          EXPECT_TRUE(ranked_on_device(table, column));
          EXPECT_TRUE(same_rows(got, stable_sorted(rows, definitions)));
          EXPECT_TRUE(same_rows(host_ranked(input, table, column, definitions), got));
          EXPECT_TRUE(same_rows(executed<Sort>(input, definitions)->get_output()->get_rows(), got) && ranked_on_device(table, column));   // (and back)
        }
      }
    }
  });
  run("StringOrder.OverATableScansOutput", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{700}));
    const auto scan = executed<TableScan>(input, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    Rows kept;
    for (const auto& row : rows) if (std::get<int32_t>(row[ORDERKEY]) > 3000) kept.push_back(row);
    EXPECT_TRUE(!kept.empty() && kept.size() < rows.size());
    for (const ColumnID column : {SHIPMODE, COMMENT}) {
      for (const SortMode mode : {ASC, DESC}) {
        const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{column, mode}};
        const auto got = executed<Sort>(scan, definitions)->get_output()->get_rows();
        EXPECT_TRUE(ranked_on_device(scan->get_output(), column));
        EXPECT_TRUE(same_rows(got, stable_sorted(kept, definitions)));
        EXPECT_TRUE(same_rows(host_ranked(scan, scan->get_output(), column, definitions), got));
      }
    }
  });
  run("StringOrder.TwoKeysRowLimitAndMaterialization", [&] {
    const auto table = make_table(rows, ChunkOffset{1000});
    const auto input = wrap(table);
    for (const auto& definitions : {std::vector<SortColumnDefinition>{SortColumnDefinition{SHIPMODE, DESC}, SortColumnDefinition{LINENUMBER, ASC}},
                                    std::vector<SortColumnDefinition>{SortColumnDefinition{LINENUMBER, DESC}, SortColumnDefinition{SHIPMODE, ASC}},
                                    std::vector<SortColumnDefinition>{SortColumnDefinition{SHIPMODE, ASC}, SortColumnDefinition{COMMENT, DESC}}}) {
      const auto want = stable_sorted(rows, definitions);
      const auto got = executed<Sort>(input, definitions)->get_output()->get_rows();
      EXPECT_TRUE(same_rows(got, want) && ranked_on_device(table, SHIPMODE));
      EXPECT_TRUE(same_rows(host_ranked(input, table, SHIPMODE, definitions), got));
      for (const uint64_t limit : {uint64_t{1}, uint64_t{10}, uint64_t{rows.size() + 1}}) {
        const auto limited = executed<Sort>(input, definitions, Chunk::DEFAULT_SIZE, Sort::ForceMaterialization::No, limit)->get_output()->get_rows();
        EXPECT_TRUE(same_rows(limited, Rows(want.begin(), want.begin() + std::min<uint64_t>(limit, want.size()))));
      }
      const auto materialized = executed<Sort>(input, definitions, ChunkOffset{333}, Sort::ForceMaterialization::Yes)->get_output();
      EXPECT_TRUE(materialized->type() == TableType::Data && same_rows(materialized->get_rows(), want));
    }
  });
  run("StringOrder.AValueSegmentChunkSortsThroughTheHostKeyTable", [&] {
    const auto table = make_table(rows, ChunkOffset{1000}, true);
    const auto input = wrap(table);
    for (const SortMode mode : {ASC, DESC}) {
      const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{SHIPMODE, mode}};
      EXPECT_TRUE(same_rows(executed<Sort>(input, definitions)->get_output()->get_rows(), stable_sorted(rows, definitions)));
      EXPECT_TRUE(!ranked_on_device(table, SHIPMODE));
    }
  });
  run("StringOrderChain.ScanSortLimit", [&] {
    const auto input = wrap(make_table(rows, ChunkOffset{1000}));
    const auto scan = executed<TableScan>(input, LINENUMBER, PredicateCondition::LessThanEquals, AllTypeVariant{int32_t{3}});
    const std::vector<SortColumnDefinition> definitions{SortColumnDefinition{COMMENT, DESC}};
    const auto sort = executed<Sort>(scan, definitions);
    const auto limit = executed<Limit>(sort, uint64_t{25});
    Rows kept;
    for (const auto& row : rows) if (std::get<int32_t>(row[LINENUMBER]) <= 3) kept.push_back(row);
    const auto want = stable_sorted(kept, definitions);
    EXPECT_TRUE(ranked_on_device(scan->get_output(), COMMENT));
    EXPECT_TRUE(want.size() > 25 && same_rows(limit->get_output()->get_rows(), Rows(want.begin(), want.begin() + 25)));
  });

  std::printf(g_failures ? "STRING ORDER TESTS FAILED: %d\n" : "STRING ORDER TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

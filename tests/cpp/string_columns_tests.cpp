// string_columns_tests.cpp -- TableScan(in, left, condition, right) on two string columns through the C++ mirror (hyrise_amd/host/
// hyrise_host.hpp): the dictionaries of both columns come from the residency cache's device_string_dictionary, the scan is
// hy_table_scan_columns_strings.  Checked against a row-by-row comparison of the std::strings on the host: over the data table (several
// chunk sizes, all six conditions), over another scan's output, a string column against a number (a Fail, as in the reference), and the
// chain TableScan(strings) -> AggregateHash with the PosLists in HBM and no row of them fetched.
// Usage: string_columns_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

// the RowIDs of an output table's first column, chunk after chunk (fetches device lists: for comparisons only)
static std::vector<uint64_t> rows_of(const std::shared_ptr<const Table>& table) {
  std::vector<uint64_t> rows;
  for (ChunkID c = 0; c < table->chunk_count(); ++c) {
    const auto ref = std::static_pointer_cast<const ReferenceSegment>(table->get_chunk(c)->get_segment(ColumnID{0}));
    for (size_t i = 0; i < ref->pos_list()->size(); ++i) {
      const RowID row = (*ref->pos_list())[i];
      rows.push_back(uint64_t{row.chunk_id} << 32 | row.chunk_offset);
    }
  }
  return rows;
}

// every PosList lies in HBM or names an entire chunk, and no row of a device list has crossed the link
static bool lists_stayed_in_hbm(const std::shared_ptr<const Table>& table) {
  for (ChunkID c = 0; c < table->chunk_count(); ++c)
    for (ColumnID col = 0; col < table->column_count(); ++col) {
      const auto ref = std::dynamic_pointer_cast<const ReferenceSegment>(table->get_chunk(c)->get_segment(col));
      if (!ref) return false;
      if (dynamic_cast<const EntireChunkPosList*>(ref->pos_list().get())) continue;
      const auto* on_device = dynamic_cast<const DevicePosList*>(ref->pos_list().get());
      if (!on_device || on_device->on_host()) return false;
    }
  return true;
}

static bool holds(PredicateCondition condition, const std::string& l, const std::string& r) {
  switch (condition) {
    case PredicateCondition::Equals: return l == r;
    case PredicateCondition::NotEquals: return l != r;
    case PredicateCondition::LessThan: return l < r;
    case PredicateCondition::LessThanEquals: return l <= r;
    case PredicateCondition::GreaterThan: return l > r;
    default: return l >= r;
  }
}

static const std::vector<PredicateCondition> CONDITIONS = {PredicateCondition::Equals,      PredicateCondition::NotEquals,         PredicateCondition::LessThan,
                                                           PredicateCondition::LessThanEquals, PredicateCondition::GreaterThan, PredicateCondition::GreaterThanEquals};
// lineitem.tbl: l_orderkey 0, l_linenumber 3, l_shipdate 10, l_commitdate 11, l_receiptdate 12, l_shipinstruct 13, l_shipmode 14
static const ColumnID ORDERKEY{0}, LINENUMBER{3}, SHIPDATE{10}, COMMITDATE{11}, RECEIPTDATE{12}, SHIPINSTRUCT{13}, SHIPMODE{14};

static std::shared_ptr<Table> load(ChunkOffset chunk_size) {
  auto table = load_table(g_tbl + "/tpch/sf-0.001/lineitem.tbl", chunk_size);
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: string_columns_tests <tbl directory>\n"); return 2; }
  g_tbl = argv[1];
  check_status(hy_init(0));

  run("StringColumns.DataTableAgainstTheStrings", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1000}, ChunkOffset{257}, ChunkOffset{65535}}) {
      const auto table = load(chunk_size);
      const auto rows = table->get_rows();
      const auto input = wrap(table);
      for (const auto& [left, right] : {std::pair{COMMITDATE, RECEIPTDATE}, std::pair{SHIPDATE, COMMITDATE}, std::pair{SHIPINSTRUCT, SHIPMODE}, std::pair{SHIPDATE, SHIPDATE}}) {
        for (const auto condition : CONDITIONS) {
          const auto scan = executed<TableScan>(input, left, condition, right, true);
          std::vector<uint64_t> want;
          for (size_t r = 0; r < rows.size(); ++r)
            if (holds(condition, std::get<std::string>(rows[r][left]), std::get<std::string>(rows[r][right]))) want.push_back(uint64_t{r / chunk_size} << 32 | r % chunk_size);
          EXPECT_TRUE(rows_of(scan->get_output()) == want);
        }
      }
      EXPECT_TRUE(table->device_columns && table->device_columns->string_dictionaries.size() == 5);   // packed once per column for all scans
    }
  });
  run("StringColumns.OverAnotherScansOutput", [&] {
    const ChunkOffset chunk_size{700};
    const auto table = load(chunk_size);
    const auto rows = table->get_rows();
    const auto input = wrap(table);
    const auto first = executed<TableScan>(input, ORDERKEY, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{3000}});
    EXPECT_TRUE(first->get_output()->row_count() > 0 && first->get_output()->row_count() < table->row_count());
    for (const auto condition : CONDITIONS) {
      const auto scan = executed<TableScan>(first, COMMITDATE, condition, RECEIPTDATE, true);
      std::vector<uint64_t> want;
      for (size_t r = 0; r < rows.size(); ++r)
        if (std::get<int32_t>(rows[r][ORDERKEY]) > 3000 && holds(condition, std::get<std::string>(rows[r][COMMITDATE]), std::get<std::string>(rows[r][RECEIPTDATE])))
          want.push_back(uint64_t{r / chunk_size} << 32 | r % chunk_size);
      EXPECT_TRUE(lists_stayed_in_hbm(scan->get_output()));   // (before rows_of fetches them for the comparison)
      EXPECT_TRUE(rows_of(scan->get_output()) == want);
    }
  });
  run("StringColumns.StringsAgainstNonStringsFail", [&] {
    const auto input = wrap(load(ChunkOffset{1000}));
    bool failed = false;
    try { executed<TableScan>(input, COMMITDATE, PredicateCondition::LessThan, ORDERKEY, true); } catch (const std::logic_error& e) {
      failed = std::string(e.what()).find("strings and non-strings") != std::string::npos;
    }
    EXPECT_TRUE(failed);
  });
  run("StringColumnsChain.ScanAggregateStaysInHbm", [&] {
    const auto table = load(ChunkOffset{1000});
    const auto rows = table->get_rows();
    const auto input = wrap(table);
    const auto scan = executed<TableScan>(input, COMMITDATE, PredicateCondition::LessThan, RECEIPTDATE, true);
    EXPECT_TRUE(scan->get_output()->row_count() > 0 && scan->get_output()->row_count() < table->row_count());
    EXPECT_TRUE(lists_stayed_in_hbm(scan->get_output()));
    const std::vector<AggregateDefinition> aggregates{{INVALID_COLUMN_ID, WindowFunction::Count}};
    const auto aggregate = executed<AggregateHash>(scan, aggregates, std::vector<ColumnID>{LINENUMBER});
    EXPECT_TRUE(lists_stayed_in_hbm(scan->get_output()));
    std::map<int32_t, int64_t> want, got;
    for (const auto& row : rows)
      if (std::get<std::string>(row[COMMITDATE]) < std::get<std::string>(row[RECEIPTDATE])) ++want[std::get<int32_t>(row[LINENUMBER])];
    for (const auto& row : aggregate->get_output()->get_rows()) got[std::get<int32_t>(row[0])] = std::get<int64_t>(row[1]);
    EXPECT_TRUE(!got.empty() && got == want);
  });

  std::printf(g_failures ? "STRING COLUMNS TESTS FAILED: %d\n" : "STRING COLUMNS TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

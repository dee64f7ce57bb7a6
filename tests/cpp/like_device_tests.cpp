// like_device_tests.cpp -- TableScan with the LIKE family through the C++ mirror (hyrise_amd/host/hyrise_host.hpp) with the dictionaries
// matched on the device (hy_table_scan_like over the residency cache's device_string_dictionary) against the same scan with the host
// matcher's bitmaps (device_like_matching() = false: find_matches_in_dictionaries + hy_table_scan): PosLists equal entry by entry, over the
// data table and over another scan's output; a pattern beyond HY_MAX_LIKE_PATTERN, which the library refuses and the host matcher keeps;
// and the chain TableScan(LIKE) -> JoinHash -> AggregateHash with its PosLists in HBM and no row of them fetched.
// Usage: like_device_tests <tests/golden/tbl directory>.  Prints one line per test, exits non-zero if one failed.
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

struct LikeOnDevice {   // the process-wide switch for a scope
  explicit LikeOnDevice(bool enabled) : before(device_like_matching()) { device_like_matching() = enabled; }
  ~LikeOnDevice() { device_like_matching() = before; }
  bool before;
};

// every PosList of every chunk and column, RowID by RowID (fetches device lists: for comparisons only)
static std::vector<std::vector<uint64_t>> lists_of(const std::shared_ptr<const Table>& table) {
  std::vector<std::vector<uint64_t>> out;
  for (ChunkID c = 0; c < table->chunk_count(); ++c)
    for (ColumnID col = 0; col < table->column_count(); ++col) {
      const auto ref = std::static_pointer_cast<const ReferenceSegment>(table->get_chunk(c)->get_segment(col));
      std::vector<uint64_t> rows;
      for (size_t i = 0; i < ref->pos_list()->size(); ++i) {
        const RowID row = (*ref->pos_list())[i];
        rows.push_back(uint64_t{row.chunk_id} << 32 | row.chunk_offset);
      }
      out.push_back(std::move(rows));
    }
  return out;
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

static std::shared_ptr<Table> load(const std::string& name, ChunkOffset chunk_size) {
  auto table = load_table(g_tbl + "/" + name, chunk_size);
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

static const std::vector<std::pair<PredicateCondition, std::string>> CASES = {
    {PredicateCondition::Like, "%"}, {PredicateCondition::Like, "%D%_m_f%"}, {PredicateCondition::Like, "Dampf%"}, {PredicateCondition::Like, "%gesellschaft"},
    {PredicateCondition::Like, "Schiff%schaft"}, {PredicateCondition::Like, "%schifffahrtsgesellschaft%"}, {PredicateCondition::Like, "%not_there%"},
    {PredicateCondition::NotLike, "%"}, {PredicateCondition::NotLike, "%foo%"}, {PredicateCondition::NotLike, "D_m_f%"}, {PredicateCondition::Like, ""},
    {PredicateCondition::LikeInsensitive, "dAMPF%"}, {PredicateCondition::NotLikeInsensitive, "d_M_f%"}, {PredicateCondition::Like, "____"}};

// ---- --timing <chunks> <rounds>: tools/like_dictionary_time.py ------------------------------------------------------------------------------
// A column shaped like o_comment: `chunks` chunks of 65 535 rows, each with 65 535 distinct strings of 19 - 78 bytes (lower-case words, a few
// of them "special", "requests", "forest", "green").  Per pattern, alternating in one process: (a) the mirror's TableScan with the host
// matcher (find_matches_in_dictionaries + hy_table_scan), (b) the same TableScan over hy_table_scan_like, (c) the matcher launch alone by
// the library's event pairs (HY_KERNEL_LIKE).  Host clock around execute(), which ends in a transfer that waits for the stream.
static double milliseconds_of(const std::function<void()>& call) {
  const auto begin = std::chrono::steady_clock::now();
  call();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
}

static void print_times(const char* label, std::vector<double> times) {
  std::sort(times.begin(), times.end());
  std::printf("  %-58s median %10.3f ms  (min %.3f, max %.3f, n = %zu)\n", label, times[times.size() / 2], times.front(), times.back(), times.size());
}

static int timing(uint32_t chunk_count, uint32_t rounds) {
  static const char* const WORDS[] = {"special", "requests", "forest", "green", "carefully", "final", "deposits", "accounts", "quickly", "ironic", "packages", "regular",
                                      "pending", "furiously", "express", "bold", "even", "slyly", "blithely", "theodolites", "asymptotes", "foxes"};
  uint64_t state = 88172645463325252ull;
  const auto next = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
  std::vector<std::shared_ptr<Chunk>> chunks;
  uint64_t char_bytes = 0, entries = 0;
  for (uint32_t c = 0; c < chunk_count; ++c) {
    std::vector<std::string> dictionary;
    for (uint32_t i = 0; i < 65535; ++i) {
      const size_t length = 19 + next() % 60;
      char id[16];
      std::snprintf(id, sizeof(id), " %05x%03x", i, c);   // distinct within the chunk
      std::string s;
      while (s.size() < length - 9) { s += WORDS[next() % 22]; s += ' '; }
      s.resize(length - 9);
      s += id;
      dictionary.push_back(std::move(s));
    }
    std::sort(dictionary.begin(), dictionary.end());
    for (const auto& s : dictionary) char_bytes += s.size();
    entries += dictionary.size();
    std::vector<uint32_t> value_ids(65535);
    for (uint32_t i = 0; i < 65535; ++i) value_ids[i] = static_cast<uint32_t>((uint64_t{i} * 40503u) % 65535u);   // (a permutation: 40503 and 65535 are coprime)
    Segments segments{std::make_shared<DictionarySegment<std::string>>(std::move(dictionary), CompressedVector::compress(value_ids, 65535), 65535)};
    chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
  }
  const auto table = std::make_shared<Table>(TableColumnDefinitions{{"o_comment", DataType::String, false}}, TableType::Data, std::move(chunks));
  const auto input = wrap(table);
  const uint64_t matcher_bytes = char_bytes + 4 * (entries + chunk_count);
  std::printf("column: %u chunks x 65535 rows, %llu distinct strings of 19 - 78 bytes, %.1f MB of chars + offsets\n", chunk_count, static_cast<unsigned long long>(entries),
              matcher_bytes / 1e6);
  const std::vector<std::pair<PredicateCondition, std::string>> patterns = {
      {PredicateCondition::NotLike, "%special%requests%"}, {PredicateCondition::Like, "forest%"}, {PredicateCondition::Like, "%green%"}};
  const auto scan = [&](bool on_device, PredicateCondition condition, const std::string& pattern, uint64_t* rows) {
    LikeOnDevice mode(on_device);
    return milliseconds_of([&] { *rows = executed<TableScan>(input, ColumnID{0}, condition, AllTypeVariant{pattern})->get_output()->row_count(); });
  };
  uint64_t rows_host = 0, rows_device = 0;
  (void)scan(true, PredicateCondition::Like, "%warm%up%", &rows_device);   // uploads the column and the dictionary, loads the code objects
  (void)scan(false, PredicateCondition::Like, "%warm%up%", &rows_host);
  const auto dictionary = device_string_dictionary(table, ColumnID{0});
  std::vector<uint64_t> word_offsets(chunk_count + 1);
  check_status(hy_string_dictionary_match_layout(dictionary->handle, word_offsets.data()));
  void* d_words = nullptr;
  check_status(hy_device_malloc(&d_words, 8 * word_offsets[chunk_count] + 16));
  int status = 0;
  for (const auto& [condition, pattern] : patterns) {
    std::vector<double> host_times, device_times;
    for (uint32_t r = 0; r < rounds; ++r) {
      if (r % 2 == 0) { host_times.push_back(scan(false, condition, pattern, &rows_host)); device_times.push_back(scan(true, condition, pattern, &rows_device)); }
      else { device_times.push_back(scan(true, condition, pattern, &rows_device)); host_times.push_back(scan(false, condition, pattern, &rows_host)); }
      if (rows_host != rows_device) { std::printf("  FAILED: %llu rows on the host path, %llu on the device path\n", static_cast<unsigned long long>(rows_host), static_cast<unsigned long long>(rows_device)); status = 1; }
    }
    check_status(hy_like_matches(dictionary->handle, pattern.data(), static_cast<uint32_t>(pattern.size()), static_cast<uint32_t>(condition), HY_MEM_DEVICE, static_cast<uint64_t*>(d_words)));
    check_status(hy_synchronize());
    check_status(hy_set_profiling(1));
    std::vector<double> kernel_times;
    for (uint32_t r = 0; r < rounds; ++r) {
      check_status(hy_like_matches(dictionary->handle, pattern.data(), static_cast<uint32_t>(pattern.size()), static_cast<uint32_t>(condition), HY_MEM_DEVICE, static_cast<uint64_t*>(d_words)));
      float ms = 0;
      uint32_t launches = 0;
      check_status(hy_profile_read_kernel(HY_KERNEL_LIKE, &ms, &launches));
      float total = 0;
      check_status(hy_profile_read(&total, &launches));   // (clears the session: one launch per reading)
      kernel_times.push_back(ms);
    }
    check_status(hy_set_profiling(0));
    std::printf("%s '%s': %llu of %llu rows\n", condition == PredicateCondition::NotLike ? "NOT LIKE" : "LIKE", pattern.c_str(), static_cast<unsigned long long>(rows_device),
                static_cast<unsigned long long>(table->row_count()));
    print_times("(a) TableScan, host matcher + hy_table_scan", host_times);
    print_times("(b) TableScan, hy_table_scan_like", device_times);
    print_times("(c) like_match alone (event pair)", kernel_times);
    std::sort(kernel_times.begin(), kernel_times.end());
    const double median = kernel_times[kernel_times.size() / 2];
    std::printf("      (c) reads %.1f MB: %.3f TB/s, %.3f of 8 TB/s\n", matcher_bytes / 1e6, matcher_bytes / median / 1e9, matcher_bytes / median / 1e9 / 8.0);
  }
  check_status(hy_device_free(d_words));
  return status;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: like_device_tests <tbl directory> | --timing <chunks> <rounds>\n"); return 2; }
  if (std::string(argv[1]) == "--timing") {
    check_status(hy_init(0));
    const int status = timing(argc > 2 ? static_cast<uint32_t>(std::atoi(argv[2])) : 229, argc > 3 ? static_cast<uint32_t>(std::atoi(argv[3])) : 7);
    hy_shutdown();
    return status;
  }
  g_tbl = argv[1];
  check_status(hy_init(0));
  const AllTypeVariant zero{int32_t{0}};

  run("LikeDevice.DataTableAgainstHostBitmaps", [&] {
    for (const ChunkOffset chunk_size : {ChunkOffset{1}, ChunkOffset{5}, ChunkOffset{100}}) {
      const auto table = load("int_string_like.tbl", chunk_size);
      const auto input = wrap(table);
      for (const auto& [condition, pattern] : CASES) {
        const auto on_device = executed<TableScan>(input, ColumnID{1}, condition, AllTypeVariant{pattern});
        std::shared_ptr<TableScan> on_host;
        { LikeOnDevice off(false); on_host = executed<TableScan>(input, ColumnID{1}, condition, AllTypeVariant{pattern}); }
        EXPECT_TRUE(lists_of(on_device->get_output()) == lists_of(on_host->get_output()));
        EXPECT_TRUE(on_device->num_chunks_with_early_out == on_host->num_chunks_with_early_out);
        EXPECT_TRUE(on_device->num_chunks_with_all_rows_matching == on_host->num_chunks_with_all_rows_matching);
      }
      EXPECT_TRUE(table->device_columns && table->device_columns->string_dictionaries.size() == 1);   // packed once for all patterns
    }
  });
  run("LikeDevice.SpecialCharacters", [&] {
    const auto table = load("int_string_like_special_chars.tbl", ChunkOffset{2});
    const auto input = wrap(table);
    for (const char* pattern : {"%2^2%", "%$%$%", "%(%)%", "%la\\.^$+?)({}.*__bl%"}) {
      const auto on_device = executed<TableScan>(input, ColumnID{1}, PredicateCondition::Like, AllTypeVariant{std::string{pattern}});
      std::shared_ptr<TableScan> on_host;
      { LikeOnDevice off(false); on_host = executed<TableScan>(input, ColumnID{1}, PredicateCondition::Like, AllTypeVariant{std::string{pattern}}); }
      EXPECT_TRUE(on_device->get_output()->row_count() > 0);
      EXPECT_TRUE(lists_of(on_device->get_output()) == lists_of(on_host->get_output()));
    }
  });
  run("LikeDevice.OverAnotherScansOutput", [&] {
    const auto table = load("int_string_like.tbl", ChunkOffset{5});
    const auto input = wrap(table);
    const auto first = executed<TableScan>(input, ColumnID{0}, PredicateCondition::GreaterThan, AllTypeVariant{int32_t{1000}});
    EXPECT_TRUE(first->get_output()->row_count() > 0 && first->get_output()->row_count() < table->row_count());
    for (const auto& [condition, pattern] : CASES) {
      const auto on_device = executed<TableScan>(first, ColumnID{1}, condition, AllTypeVariant{pattern});
      std::shared_ptr<TableScan> on_host;
      { LikeOnDevice off(false); on_host = executed<TableScan>(first, ColumnID{1}, condition, AllTypeVariant{pattern}); }
      EXPECT_TRUE(lists_of(on_device->get_output()) == lists_of(on_host->get_output()));
    }
  });
  run("LikeDevice.PatternTooLongFallsBackToTheHostMatcher", [&] {
    const auto table = load("int_string_like.tbl", ChunkOffset{5});
    const auto input = wrap(table);
    const std::string long_pattern = std::string(HY_MAX_LIKE_PATTERN, '%') + "Dampf%";   // the same language as %Dampf%, 262 bytes
    const auto fallen_back = executed<TableScan>(input, ColumnID{1}, PredicateCondition::Like, AllTypeVariant{long_pattern});
    const auto on_device = executed<TableScan>(input, ColumnID{1}, PredicateCondition::Like, AllTypeVariant{std::string{"%Dampf%"}});
    EXPECT_TRUE(fallen_back->get_output()->row_count() > 0);
    EXPECT_TRUE(lists_of(fallen_back->get_output()) == lists_of(on_device->get_output()));
  });
  run("LikeDeviceChain.ScanJoinAggregateStaysInHbm", [&] {
    const auto left_table = load("int_string_like.tbl", ChunkOffset{3}), right_table = load("int_string_like.tbl", ChunkOffset{4});
    const auto left = wrap(left_table), right = wrap(right_table);
    const std::vector<AggregateDefinition> aggregates{{INVALID_COLUMN_ID, WindowFunction::Count}};
    const auto chain = [&](bool check_residency) {
      const auto scan = executed<TableScan>(left, ColumnID{1}, PredicateCondition::Like, AllTypeVariant{std::string{"%schiff%"}});
      EXPECT_TRUE(scan->get_output()->row_count() > 0 && scan->get_output()->row_count() < left_table->row_count());
      const auto join = executed<JoinHash>(scan, right, JoinMode::Inner, ColumnIDPair{ColumnID{0}, ColumnID{0}});
      EXPECT_TRUE(join->get_output()->row_count() > 0);
      const auto aggregate = executed<AggregateHash>(join, aggregates, std::vector<ColumnID>{ColumnID{0}});
      if (check_residency) {
        EXPECT_TRUE(lists_stayed_in_hbm(scan->get_output()));
        EXPECT_TRUE(lists_stayed_in_hbm(join->get_output()));
      }
      auto rows = aggregate->get_output()->get_rows();
      std::sort(rows.begin(), rows.end(), [](const auto& a, const auto& b) { return std::get<int32_t>(a[0]) < std::get<int32_t>(b[0]); });
      return rows;
    };
    const auto got = chain(true);
    LikeOnDevice off(false);
    const auto want = chain(false);
    EXPECT_TRUE(!got.empty() && got.size() == want.size());
    for (size_t r = 0; r < got.size() && r < want.size(); ++r) {
      EXPECT_TRUE(std::get<int32_t>(got[r][0]) == std::get<int32_t>(want[r][0]));
      EXPECT_TRUE(std::get<int64_t>(got[r][1]) == std::get<int64_t>(want[r][1]));
    }
  });

  std::printf(g_failures ? "LIKE DEVICE TESTS FAILED: %d\n" : "LIKE DEVICE TESTS PASSED\n", g_failures);
  hy_shutdown();
  return g_failures ? 1 : 0;
}

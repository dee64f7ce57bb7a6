// string_order_time.cpp -- what a string sort key costs before the first sort kernel runs, device ranking against host ranking, through the
// C++ mirror (hyrise_amd/host/hyrise_host.hpp).  Built and run by tools/string_order_time.py; prints the table of profiles/string_order.txt.
//   (a) hy_string_dictionary_order over dictionaries shaped like l_shipmode, s_name, c_name and a high-cardinality column: HIP events
//       (HY_KERNEL_STRING_RANK: the whole launch sequence, bracketed on the stream) and host wall clock around the call, median of RUNS --
//       against the host ranking of the same strings: the mirror's device_column_of_chunks(StringKeys::Ranks) with the device path switched
//       off, wall clock, minus the same column made without ranks (the upload both paths share).
//   (b) Sort by one string key on the c_name shape, end to end (wall clock around execute()), device path against host path: the first call
//       on a fresh table (packs and uploads the dictionaries, ranks, builds the cache) and a second call on the same table (cache hit).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;
using Clock = std::chrono::steady_clock;

static constexpr int RUNS = 7;

static double ms_since(Clock::time_point begin) { return std::chrono::duration<double, std::milli>(Clock::now() - begin).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

// one string column whose chunk c holds entries[c], each once, in a shuffled order: the chunk's dictionary is exactly entries[c]
static std::shared_ptr<Table> table_of(const std::vector<std::vector<std::string>>& entries, std::mt19937& rng) {
  auto table = std::make_shared<Table>(TableColumnDefinitions{{"s", DataType::String, false}}, TableType::Data);
  for (auto chunk : entries) {
    std::shuffle(chunk.begin(), chunk.end(), rng);
    table->append_chunk(Segments{std::make_shared<ValueSegment<std::string>>(std::move(chunk), std::nullopt)});
  }
  ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
  return table;
}

static std::string numbered(const char* prefix, uint64_t i) {
  char buffer[64];
  std::snprintf(buffer, sizeof(buffer), "%s#%09llu", prefix, static_cast<unsigned long long>(i));
  return buffer;
}

struct Shape {
  std::string name;
  std::vector<std::vector<std::string>> entries;
};

static std::vector<Shape> shapes() {
  std::vector<Shape> out;
  const std::vector<std::string> modes{"AIR", "FOB", "MAIL", "RAIL", "REG AIR", "SHIP", "TRUCK"};
  out.push_back({"l_shipmode 916 x 7", std::vector<std::vector<std::string>>(916, modes)});
  Shape s_name{"s_name 2 x 50 000", {}};
  for (uint64_t c = 0; c < 2; ++c) {   // dealt alternately: both chunks span the whole range
    s_name.entries.emplace_back();
    for (uint64_t i = c; i < 100000; i += 2) s_name.entries.back().push_back(numbered("Supplier", i + 1));
  }
  out.push_back(std::move(s_name));
  Shape c_name{"c_name 23 x 65 535", {}};
  std::mt19937 rng(7);
  std::vector<uint64_t> customers(1500000);
  for (uint64_t i = 0; i < customers.size(); ++i) customers[i] = i + 1;
  std::shuffle(customers.begin(), customers.end(), rng);   // (c_name is not clustered by chunk in a table that was ever reordered: every chunk spans the range)
  for (uint64_t begin = 0; begin < customers.size(); begin += 65535) {
    c_name.entries.emplace_back();
    for (uint64_t i = begin; i < std::min<uint64_t>(customers.size(), begin + 65535); ++i) c_name.entries.back().push_back(numbered("Customer", customers[i]));
  }
  out.push_back(std::move(c_name));
  Shape high{"high cardinality 64 x 65 535, ~27 bytes", {}};
  for (uint64_t c = 0; c < 64; ++c) {
    high.entries.emplace_back();
    for (uint64_t i = 0; i < 65535; ++i) {
      std::string entry(20 + rng() % 15, 'a');
      for (auto& byte : entry) byte = static_cast<char>('a' + rng() % 26);
      high.entries.back().push_back(entry + std::to_string(c * 65535 + i));   // (distinct by construction)
    }
  }
  out.push_back(std::move(high));
  return out;
}

int main() {
  check_status(hy_init(0));
  float overhead = 0;
  check_status(hy_profile_event_overhead(&overhead));
  std::printf("(a) one column's dictionaries ordered: hy_string_dictionary_order (device) against the mirror's host ranking; ms, median of %d\n", RUNS);
  std::printf("    events = HIP events around the launch sequence (HY_KERNEL_STRING_RANK; an empty bracket: %.3f ms); call = host wall clock around the call + hy_synchronize\n", overhead);
  std::printf("    host ranking = wall clock of device_column_of_chunks(Ranks), device path off, minus the same column without ranks\n");
  std::printf("%-42s %10s %9s %10s %10s %13s %8s\n", "shape", "entries", "distinct", "events", "call", "host ranking", "host/dev");
  std::mt19937 rng(1);
  std::shared_ptr<Table> c_name_table;
  for (const auto& shape : shapes()) {
    const auto table = table_of(shape.entries, rng);
    if (shape.name.rfind("c_name", 0) == 0) c_name_table = table;
    const auto dictionary = device_string_dictionary(table, ColumnID{0});
    uint64_t total = 0;
    for (const auto& chunk : shape.entries) total += chunk.size();
    const auto ranks = DeviceBlock::acquire(4 * total + 64);
    uint32_t n_distinct = 0;
    for (int warm = 0; warm < 2; ++warm) check_status(hy_string_dictionary_order(dictionary->handle, HY_MEM_DEVICE, static_cast<int32_t*>(ranks->ptr), &n_distinct));
    std::vector<double> events, calls, host;
    for (int run = 0; run < RUNS; ++run) {
      check_status(hy_set_profiling(1));
      const auto begin = Clock::now();
      check_status(hy_string_dictionary_order(dictionary->handle, HY_MEM_DEVICE, static_cast<int32_t*>(ranks->ptr), nullptr));
      check_status(hy_synchronize());
      calls.push_back(ms_since(begin));
      float ms = 0;
      uint32_t launches = 0;
      check_status(hy_profile_read_kernel(HY_KERNEL_STRING_RANK, &ms, &launches));
      check_status(hy_set_profiling(0));
      events.push_back(ms);
    }
    device_string_ranking() = false;
    for (int run = 0; run < 3; ++run) {
      auto begin = Clock::now();
      { const auto with_ranks = device_column_of_chunks(table, ColumnID{0}, StringKeys::Ranks, 0, table->chunk_count()); check_status(hy_synchronize()); }
      const double ranked = ms_since(begin);
      begin = Clock::now();
      { const auto without = device_column_of_chunks(table, ColumnID{0}, StringKeys::None, 0, table->chunk_count()); check_status(hy_synchronize()); }
      host.push_back(ranked - ms_since(begin));
    }
    device_string_ranking() = true;
    std::printf("%-42s %10llu %9u %10.3f %10.3f %13.3f %8.1f\n", shape.name.c_str(), static_cast<unsigned long long>(total), n_distinct, median(events), median(calls), median(host),
                median(host) / median(calls));
    std::fflush(stdout);
  }

  std::printf("\n(b) Sort by one string key, c_name shape (1 500 000 rows, one per name), end to end: wall clock around Sort::execute(), ms\n");
  std::printf("    first = a table nothing was cached for (attribute vectors and dictionaries uploaded, ranks made, then the sort); second = the same table again\n");
  std::printf("%-14s %10s %10s\n", "ranking", "first", "second");
  for (const bool on_device : {true, false, true, false}) {
    device_string_ranking() = on_device;
    auto table = table_of(std::vector<std::vector<std::string>>(shapes()[2].entries), rng);
    auto wrapper = std::make_shared<TableWrapper>(table);
    wrapper->execute();
    double times[2];
    for (int call = 0; call < 2; ++call) {
      Sort sort(wrapper, {SortColumnDefinition{ColumnID{0}, SortMode::AscendingNullsFirst}});
      const auto begin = Clock::now();
      sort.execute();
      check_status(hy_synchronize());
      times[call] = ms_since(begin);
    }
    std::printf("%-14s %10.2f %10.2f\n", on_device ? "device (int32)" : "host (int64)", times[0], times[1]);
    std::fflush(stdout);
  }
  device_string_ranking() = true;
  hy_shutdown();
  return 0;
}

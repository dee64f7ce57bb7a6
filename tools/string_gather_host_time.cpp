// string_gather_host_time.cpp -- what the C++ mirror (hyrise_amd/host/hyrise_host.hpp) pays to materialise a string column from RowIDs on the
// host: AggregateHash::resident_output's loop for a string GROUP BY column -- one AllTypeVariant per representative row read through
// operator[], then make_value_segment<std::string> per output chunk.  Built and run by tools/string_gather_timing.py, which compares it with
// hy_string_column_gather over the same column and RowIDs.  Prints one line per shape: "<bytes per string> <median ms of 3>".
// Shapes (the same generator as tools/string_gather_timing.py): ROWS distinct strings of 18 and of 70 bytes in chunks of 65 535 rows, every
// row once, in a shuffled order (one group per customer: the Q18 c_name shape).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;
using Clock = std::chrono::steady_clock;

static std::string entry_of(uint64_t i, size_t bytes) {
  char number[32];
  std::snprintf(number, sizeof(number), "#%09llu", static_cast<unsigned long long>(i));
  return std::string(bytes - 10, 'C') + number;
}

int main(int argc, char** argv) {
  const uint64_t rows = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1500000;
  for (const size_t bytes : {size_t{18}, size_t{70}}) {
    std::mt19937 rng(7);
    std::vector<uint64_t> order(rows);
    for (uint64_t i = 0; i < rows; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    auto table = std::make_shared<Table>(TableColumnDefinitions{{"s", DataType::String, false}}, TableType::Data);
    for (uint64_t begin = 0; begin < rows; begin += Chunk::DEFAULT_SIZE) {
      std::vector<std::string> chunk;
      for (uint64_t i = begin; i < std::min<uint64_t>(rows, begin + Chunk::DEFAULT_SIZE); ++i) chunk.push_back(entry_of(order[i], bytes));
      table->append_chunk(Segments{std::make_shared<ValueSegment<std::string>>(std::move(chunk), std::nullopt)});
    }
    ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);
    std::vector<RowID> row_ids(rows);
    for (uint64_t i = 0; i < rows; ++i) row_ids[i] = RowID{static_cast<ChunkID>(i / Chunk::DEFAULT_SIZE), static_cast<ChunkOffset>(i % Chunk::DEFAULT_SIZE)};
    std::shuffle(row_ids.begin(), row_ids.end(), rng);
    std::vector<double> times;
    for (int run = 0; run < 3; ++run) {
      const auto start = Clock::now();
      std::vector<std::shared_ptr<AbstractSegment>> segments;
      for (uint64_t begin = 0; begin < rows; begin += Chunk::DEFAULT_SIZE) {
        std::vector<std::vector<AllTypeVariant>> cells;
        for (uint64_t r = begin; r < std::min<uint64_t>(rows, begin + Chunk::DEFAULT_SIZE); ++r)
          cells.push_back({(*table->get_chunk(row_ids[r].chunk_id)->get_segment(ColumnID{0}))[row_ids[r].chunk_offset]});
        segments.push_back(make_value_segment<std::string>(cells, ColumnID{0}, false));
      }
      times.push_back(std::chrono::duration<double, std::milli>(Clock::now() - start).count());
    }
    std::sort(times.begin(), times.end());
    std::printf("%zu %.3f\n", bytes, times[1]);
    std::fflush(stdout);
  }
  return 0;
}

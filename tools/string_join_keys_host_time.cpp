// string_join_keys_host_time.cpp -- what the C++ mirror (hyrise_amd/host/hyrise_host.hpp) pays to make JoinHash's string keys on the host:
// string_join_id for every dictionary entry of every chunk of both key columns, as device_column_of_chunks calls it under
// StringKeys::JoinIds.  The registry is process-wide, so ONE measurement per process: the registry is cold, as it is for the first join
// over a pair of columns.  Built and run by tools/string_join_keys_timing.py, which compares it with hy_column_string_join_keys over the
// same dictionaries.  Usage: string_join_keys_host_time_bin small|large; prints the milliseconds of the calls alone (the entries of a
// chunk are made before the clock starts).
// Shapes (the same generator as tools/string_join_keys_timing.py): small -- 916 chunks x the 7 ship modes on either side; large -- 64 chunks
// x 65 535 entries of 27 bytes on either side, distinct within a side, a third of them shared between the sides.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../hyrise_amd/host/hyrise_host.hpp"

using namespace hyrise_amd;
using Clock = std::chrono::steady_clock;

static std::vector<std::string> chunk_entries(bool large, int side, uint32_t chunk) {
  if (!large) return {"AIR", "FOB", "MAIL", "RAIL", "REG AIR", "SHIP", "TRUCK"};
  std::vector<std::string> entries;
  entries.reserve(65535);
  for (uint64_t i = 0; i < 65535; ++i) {
    char number[32];
    std::snprintf(number, sizeof(number), "%010llu", static_cast<unsigned long long>((side == 0 ? 2 : 3) * (i * 64 + chunk)));
    entries.push_back(std::string(17, 'K') + number);
  }
  return entries;
}

int main(int argc, char** argv) {
  const bool large = argc > 1 && std::strcmp(argv[1], "large") == 0;
  const uint32_t n_chunks = large ? 64 : 916;
  double ms = 0;
  int64_t sink = 0;
  for (int side = 0; side < 2; ++side) {
    for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
      const auto entries = chunk_entries(large, side, chunk);
      std::vector<int64_t> ids;
      const auto start = Clock::now();
      for (const auto& entry : entries) ids.push_back(string_join_id(entry));
      ms += std::chrono::duration<double, std::milli>(Clock::now() - start).count();
      sink ^= ids.back();
    }
  }
  std::printf("%.3f %lld\n", ms, static_cast<long long>(sink & 1));
  return 0;
}

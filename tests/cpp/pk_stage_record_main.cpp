// pk_emit's compact staged record and LDS footprint (hyrise_amd/csrc/join_pk_stage.hpp), checked on the host:
//   unpack(pack(row, null partner, delta), base) gives back row, null partner, the row's wave and base + delta, for every row of a
//   tile, both null-partner bits, the deltas 0, 1, 65 534, 65 535 and rank bases up to the largest that keeps the rank in 32 bits;
//   three workgroups of the compact flavour fit a CU's 160 KB of LDS at every radix the route accepts, the compact footprint is
//   smaller than the 8-byte one, and pk_cut_slice's words fit into it.
// Prints "ok" and returns 0, or says what failed and returns 1.
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../hyrise_amd/csrc/join_pk_stage.hpp"

int main() {
  const uint32_t deltas[] = {0u, 1u, 65534u, 65535u};
  const uint32_t bases[] = {0u, 1u, 65535u, 65536u, 59'986'052u, 0xFFFF0000u};
  unsigned long checked = 0;
  for (uint32_t row = 0; row < PK_TILE; ++row) {
    for (uint32_t null_partner = 0; null_partner < 2; ++null_partner) {
      for (uint32_t delta : deltas) {
        const uint32_t record = pk_compact_pack(row, null_partner, delta);
        for (uint32_t base : bases) {
          const PkCompactPair pair = pk_compact_unpack(record, base);
          if (pair.row != row || pair.null_partner != null_partner || pair.wave != row / PK_WAVE_ROWS || pair.rank != base + delta) {
            std::printf("row %u null %u delta %u base %u -> row %u null %u wave %u rank %u\n", row, null_partner, delta, base, pair.row, pair.null_partner, pair.wave, pair.rank);
            return 1;
          }
          ++checked;
        }
      }
      // a row without a partner packs whatever its lookup left: what does not fit falls off the word, row and null partner stay
      const uint32_t record = pk_compact_pack(row, null_partner, 0xFFFFFFFFu - row);
      if (pk_compact_row(record) != row || pk_compact_null(record) != (null_partner != 0)) { std::printf("row %u: an untrusted delta reached the row\n", row); return 1; }
    }
  }
  for (uint32_t radix_bits = 0; radix_bits <= PK_COMPACT_MAX_RADIX_BITS; ++radix_bits) {
    const uint32_t partitions = 1u << radix_bits;
    const size_t compact = 4 * pk_emit_lds_words(partitions, true), wide = 4 * pk_emit_lds_words(partitions, false);
    if (3 * compact > PK_LDS_PER_CU || compact >= wide || compact < 4 * size_t{PK_CUT_WORDS} || pk_stage_words(partitions, true) % 4 != 0 ||
        pk_stage_words(partitions, true) < size_t{PK_TILE} + partitions + 2) {
      std::printf("radix %u: compact %zu bytes, wide %zu bytes\n", radix_bits, compact, wide);
      return 1;
    }
  }
  std::printf("ok %lu records, compact LDS %zu / %zu bytes at radix 7 / 8\n", checked, 4 * pk_emit_lds_words(128, true), 4 * pk_emit_lds_words(256, true));
  return 0;
}

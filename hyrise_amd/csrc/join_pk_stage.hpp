// join_pk_stage.hpp -- pk_emit's tile geometry, its LDS footprint and the 4-byte staged record of its compact flavour
// (included by join_pkfk.hpp inside namespace hy).  Plain arithmetic on fixed-width integers and nothing else, so that a host program
// can include it on its own and check it (tests/cpp/pk_stage_record_main.cpp); the includer provides <cstddef> and <cstdint>.
#pragma once

#ifndef HY_PK_TILE
#define HY_PK_TILE 8192
#endif
#ifndef HY_PK_WAVES_PER_SIMD
#define HY_PK_WAVES_PER_SIMD 4   // pk_emit: workgroups per CU x waves per workgroup / 4 (the register budget: 512 / this)
#endif
#ifndef HY_PK_COMPACT_WAVES_PER_SIMD
#define HY_PK_COMPACT_WAVES_PER_SIMD 6   // pk_emit's compact flavour: three workgroups per CU (its LDS allows three: pk_emit_lds_words)
#endif
#if defined(__HIPCC__)
#define HY_PK_HOST_DEVICE __host__ __device__
#else
#define HY_PK_HOST_DEVICE
#endif

constexpr uint32_t PK_TILE = HY_PK_TILE;                 // rows per probe tile: a slice (8192) or half a slice (-DHY_PK_TILE=4096: A/B builds)
constexpr uint32_t PK_ROUNDS = 16;                       // rows per lane
constexpr uint32_t PK_THREADS = PK_TILE / PK_ROUNDS;     // 512
constexpr uint32_t PK_WAVES = PK_THREADS / 64;           // 8
constexpr uint32_t PK_WAVE_ROWS = PK_TILE / PK_WAVES;    // 1024 consecutive rows per wave
constexpr uint32_t PK_LINES = PK_TILE / 16;              // 128-byte output lines of 16 pairs a tile's pairs can fill
constexpr uint32_t PK_CUT_WORDS = PK_WAVES * 1024 + 2 * PK_WAVES * PK_ROUNDS;   // what pk_cut_slice takes of pk_emit's LDS
constexpr uint32_t PK_COMPACT_MAX_RADIX_BITS = 8;        // (MAX_PARTITIONS of join.hip: 256)
constexpr size_t PK_LDS_PER_CU = 160 * 1024;             // gfx950
static_assert(PK_TILE <= (1u << 13), "a staged pair keeps its row in 13 bits");

// ---- the compact record ------------------------------------------------------------------------------------------------------
// row in the tile (13 bits) | null partner << 13 (never set by an Inner join) | (partner's rank - the wave's rank base) << 16.
// The wave of a row is row / PK_WAVE_ROWS, its rank base one LDS word per wave: the smallest rank among the wave's rows that have a
// partner.  Why 16 bits hold the difference: a wave's 1024 rows lie in one FrameOfReference block whose offsets are stored 1 or 2 bytes
// wide, so its keys are block minimum + [0, 65 535]; the rank of a present key is the number of present build keys below it, so
// between the ranks of two partners of the wave lie at most 65 535 present keys:
//   0 <= rank - base < 65 536   for every row of the wave that has a partner.
// Rows without a partner (a null partner, an Anti join's row, a row behind the tile's last) pack whatever their lookup left: the shift
// drops what does not fit, and nothing reads their rank.
constexpr uint32_t PK_COMPACT_ROW = PK_TILE - 1, PK_COMPACT_NULL_BIT = 13, PK_COMPACT_DELTA_SHIFT = 16;
static_assert(PK_COMPACT_ROW < (1u << PK_COMPACT_NULL_BIT) && PK_WAVE_ROWS == 1024, "row, null partner and delta share one word; wave = row >> 10");
struct PkCompactPair { uint32_t row, null_partner, wave, rank; };
HY_PK_HOST_DEVICE constexpr uint32_t pk_compact_pack(uint32_t row, uint32_t null_partner, uint32_t delta) {
  return row | null_partner << PK_COMPACT_NULL_BIT | delta << PK_COMPACT_DELTA_SHIFT;
}
HY_PK_HOST_DEVICE constexpr uint32_t pk_compact_row(uint32_t record) { return record & PK_COMPACT_ROW; }
HY_PK_HOST_DEVICE constexpr uint32_t pk_compact_wave(uint32_t record) { return pk_compact_row(record) / PK_WAVE_ROWS; }
HY_PK_HOST_DEVICE constexpr bool pk_compact_null(uint32_t record) { return (record >> PK_COMPACT_NULL_BIT) & 1u; }
HY_PK_HOST_DEVICE constexpr uint32_t pk_compact_rank(uint32_t record, uint32_t wave_base) { return wave_base + (record >> PK_COMPACT_DELTA_SHIFT); }
HY_PK_HOST_DEVICE constexpr PkCompactPair pk_compact_unpack(uint32_t record, uint32_t wave_base) {
  return PkCompactPair{pk_compact_row(record), pk_compact_null(record) ? 1u : 0u, pk_compact_wave(record), pk_compact_rank(record, wave_base)};
}

// ---- pk_emit's LDS, in 4-byte words --------------------------------------------------------------------------------------------
// staged pairs, one spare slot per partition and two more: {row | null partner << 21, partner's rank} of 8 bytes, or compact records
// of 4 (rounded to whole 16 bytes: the line table behind them is read in 8-byte pieces) | pairs per (wave, partition), then the first
// slot of (wave, partition); after the staging the copy-out's line table (PK_LINES x 2 words) in the same words | global pair index of
// staging slot 0 per partition | first global pair index of the run per partition, then its first interior line (bits 16..) and its
// pairs (bits 0..15) | 32 words: wave totals of the partition scan, reserved slots and interior lines, a counter per wave for rows
// without a pair, (compact) a rank base per wave.
HY_PK_HOST_DEVICE constexpr size_t pk_stage_words(uint32_t partitions, bool compact) {
  return compact ? (size_t{PK_TILE} + partitions + 2 + 3) / 4 * 4 : 2 * (size_t{PK_TILE} + partitions + 2);
}
HY_PK_HOST_DEVICE constexpr size_t pk_wave_pairs_words(uint32_t partitions) {
  return size_t{PK_WAVES} * partitions > 2 * size_t{PK_LINES} ? size_t{PK_WAVES} * partitions : 2 * size_t{PK_LINES};
}
HY_PK_HOST_DEVICE constexpr size_t pk_emit_lds_words(uint32_t partitions, bool compact = false) {
  return pk_stage_words(partitions, compact) + pk_wave_pairs_words(partitions) + 3 * size_t{partitions} + 32;
}
static_assert(PK_LINES == PK_THREADS, "the copy-out's line table is filled thread = line");
static_assert(2 * PK_LINES <= PK_WAVES * 256, "the line table must not make 256 partitions' LDS larger");
static_assert(PK_WAVES * 1024 <= PK_TILE, "the rows' stored words go round through the staging area: 1024 words per wave, compact records included");
static_assert(pk_emit_lds_words(1, true) >= PK_CUT_WORDS && pk_emit_lds_words(1, false) >= PK_CUT_WORDS, "pk_cut_slice runs in pk_emit's LDS");
static_assert(3 * 4 * pk_emit_lds_words(1u << PK_COMPACT_MAX_RADIX_BITS, true) <= PK_LDS_PER_CU, "three compact workgroups per CU at the widest radix");

// hy_options.hpp -- the library's process-wide options (include/hyrise_amd.h HY_OPT_*): which of several equivalent paths / launch
// shapes an operator takes.  An array of atomics filled with the defaults; hy_set_option stores, the operators load.  No getenv in a
// release build: the debug aids (traces, host timelines, kernels with parts switched off -- "results are wrong then") exist only
// under -DHY_DEBUG_SWITCHES (tools/build_variant.sh debug -DHY_DEBUG_SWITCHES), where HY_DEBUG_ENV reads the environment.
#pragma once

#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "../../include/hyrise_amd.h"

namespace hy {

extern std::atomic<int64_t> g_options[HY_OPT_COUNT];   // runtime.hip
inline int64_t option(uint32_t id) { return g_options[id].load(std::memory_order_relaxed); }

// What rounds 4-5 exposed as options and round 6 fixed (every setting gave the same results; the A/B timings that chose these values are in
// profiles/r03_scan_stores.txt, r04_join_variants.txt, r05_step_ab.txt and DESIGN.md).  One of them is an option again,
// HY_OPT_LDS_ORDERED_ATOMICS: where the LDS serves the lanes of a returning atomic in order (probed once per process) pairs are ranked with
// one such atomic each, and the device's answer picks the kernels of five call sites (lds_atomics_are_lane_ordered, join.hip); 0 makes that
// function answer "no" without the probe, so that the tests run what a device without the order would run.
constexpr int64_t FIXED_SCAN_WGS_PER_CU = 8;        // resident scan workgroups per CU (upper bound)
constexpr int64_t FIXED_SCAN_NT_STORES = 0;         // scan_slices writes its RowIDs with write-back stores
constexpr int64_t FIXED_PART_SLICES = 0;            // one scan part per chunk
constexpr int64_t FIXED_JOIN_IDENTITY = 1;          // a sorted build column of equally sized chunks is read in place (rank = row number)
constexpr int64_t FIXED_JOIN_FETCH_AHEAD = 1;       // probe segments are read through SliceViews (wide loads)
constexpr int64_t FIXED_JOIN_WGS_PER_CU = 0;        // persistent probe kernels: what the occupancy query says
constexpr int64_t FIXED_JOIN_EMIT_TILE_GROUP = 64;  // pk_emit: consecutive tiles per XCD (one front of 8 x 64 tiles moves through the probe side)
constexpr int64_t FIXED_JOIN_CLEAN_TABLES = 1;      // a hinted wave fill's filter comes zeroed: the join before cleared it (the table needs no zeroing)
constexpr int64_t FIXED_SCAN_JOB_CACHE = 1;         // a data column remembers the per-chunk jobs of its last four literal predicates
constexpr int64_t FIXED_AGG_PARTITIONS = 1;         // many groups take the hash-partitioned path
constexpr int64_t FIXED_AGG_LDS_BUDGET = 32768;     // bytes of LDS a partition table may take
constexpr int64_t FIXED_AGG_SPLIT = 0;              // workgroups per partition: derived
constexpr int64_t FIXED_AGG_JOINT_HISTOGRAM = 1;    // two 1-byte measure columns are counted in one pair histogram
constexpr int64_t FIXED_FUSED_SHARED_PREFIX = 1;    // fused inputs that begin with an earlier input continue on its stack

// HY_OPT_STRING_SPARSE_GATHER = 1: n rows out of a string column of `rows` rows and E dictionary entries take the sparse route (string_gather.hip)
// when n <= (rows + E) / STRING_SPARSE_DIVISOR -- rows + E is the work the dense route does whatever n is.  Measured in
// profiles/string_gather_sparse.txt (tools/string_gather_sparse_timing.py): the sparse route took 0.04 - 0.79 of the
// dense route's time at every n measured in both shapes; the largest n / (rows + E) that BOTH shapes were measured at is 1.7e-2 (l_shipdate,
// n = 2^20: 0.46; c_name at 2.2e-2: 0.37), and 1 / 64 lies below it.  Nothing was measured beyond: the rule stops where the measurements do.
constexpr int64_t STRING_SPARSE_DIVISOR = 64;

}  // namespace hy

#ifdef HY_DEBUG_SWITCHES
#define HY_DEBUG_ENV(name) getenv(name)
#else
#define HY_DEBUG_ENV(name) (static_cast<const char*>(nullptr))
#endif

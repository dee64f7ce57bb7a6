/*
 * hyrise_amd.h -- C ABI of the MI355X-native execution hot path for Hyrise.
 *
 * This is the drop-in boundary: the three read-only operators whose `_on_execute()` bodies
 * (reference: src/lib/operators/abstract_read_only_operator.hpp:20-22) are replaced call these
 * entry points with plain pointers and sizes.  No C++ types, no torch types, no exceptions cross
 * this line.  Every function returns an `hy_status`; a non-zero status has a message retrievable
 * through `hy_last_error()` (the Hyrise adapter turns it into `Fail(...)`, i.e. std::logic_error,
 * reference: src/lib/utils/assert.hpp:48-70).  `HY_ERR_UNSUPPORTED` means "shape not handled on
 * the device; run the stock CPU operator" and is never an execution failure.
 *
 * Layout contract (all restated from the reference):
 *   RowID            {u32 chunk_id, u32 chunk_offset}, NULL_ROW_ID = {~0u, ~0u}   types.hpp:97-117,150
 *   ValueSegment<T>  T values[n] (+ optional null bitmap)                        value_segment.hpp:84-85
 *   DictionarySegment<T>  sorted unique T dictionary[d]; attribute vector of value ids as
 *                    u8/u16/u32 (FixedWidthInteger); NULL == value id d           dictionary_segment.hpp:88-90
 *   FrameOfReferenceSegment<int32>  i32 block_minima[ceil(n/2048)], offsets as u8/u16/u32,
 *                    optional null bitmap; value = (i32)offset + minimum           frame_of_reference_segment.hpp:49,94-97
 *   null bitmap      libstdc++ vector<bool> words: bit (i % 64) of u64 word (i / 64)
 *   ReferenceSegment pos list of RowIDs into the chunks of another column          reference_segment.hpp:20-48
 */
#ifndef HYRISE_AMD_H_
#define HYRISE_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HY_ABI_VERSION 4   /* 2: hy_segment carries sorted_by and bits; 3: hy_join_result flags / status (HY_JOIN_ASYNC), hy_set_option;
                            * 4: hy_result_pool_*, hy_poslist_gather (device-resident PosLists behind _on_execute()), 15 options (were 33) */

typedef int32_t hy_status;
enum {
  HY_OK = 0,
  HY_ERR_INVALID = 1,     /* malformed argument: the adapter raises std::logic_error            */
  HY_ERR_UNSUPPORTED = 2, /* shape not handled on the device: adapter runs the stock CPU path    */
  HY_ERR_DEVICE = 3,      /* HIP runtime failure (message carries the hipError string)            */
  HY_ERR_CAPACITY = 4     /* caller-provided output buffer too small                              */
};

/* Mirrors hyrise::DataType (all_type_variant.hpp:34-39,52). */
enum { HY_TYPE_NULL = 0, HY_TYPE_INT = 1, HY_TYPE_LONG = 2, HY_TYPE_FLOAT = 3, HY_TYPE_DOUBLE = 4, HY_TYPE_STRING = 5 };

/* Mirrors hyrise::PredicateCondition, same numeric order (types.hpp:160-179). */
enum {
  HY_PRED_EQUALS = 0, HY_PRED_NOT_EQUALS = 1, HY_PRED_LESS_THAN = 2, HY_PRED_LESS_THAN_EQUALS = 3,
  HY_PRED_GREATER_THAN = 4, HY_PRED_GREATER_THAN_EQUALS = 5,
  HY_PRED_BETWEEN_INCLUSIVE = 6, HY_PRED_BETWEEN_LOWER_EXCLUSIVE = 7, HY_PRED_BETWEEN_UPPER_EXCLUSIVE = 8,
  HY_PRED_BETWEEN_EXCLUSIVE = 9,
  HY_PRED_IN = 10, HY_PRED_NOT_IN = 11, HY_PRED_LIKE = 12, HY_PRED_NOT_LIKE = 13, HY_PRED_LIKE_INSENSITIVE = 14,
  HY_PRED_NOT_LIKE_INSENSITIVE = 15, HY_PRED_IS_NULL = 16, HY_PRED_IS_NOT_NULL = 17
};

/* Mirrors hyrise::JoinMode, same numeric order (types.hpp:210). */
enum {
  HY_JOIN_INNER = 0, HY_JOIN_LEFT = 1, HY_JOIN_RIGHT = 2, HY_JOIN_FULL_OUTER = 3, HY_JOIN_CROSS = 4, HY_JOIN_SEMI = 5,
  HY_JOIN_ANTI_NULL_AS_TRUE = 6, HY_JOIN_ANTI_NULL_AS_FALSE = 7
};

/* Aggregate functions handled by AggregateHash (window_function_traits.hpp:11-77). */
enum {
  HY_AGG_MIN = 0, HY_AGG_MAX = 1, HY_AGG_SUM = 2, HY_AGG_AVG = 3, HY_AGG_COUNT = 4, HY_AGG_COUNT_DISTINCT = 5,
  HY_AGG_STDDEV_SAMP = 6, HY_AGG_ANY = 7
};

enum { HY_ENC_UNENCODED = 0, HY_ENC_DICTIONARY = 1, HY_ENC_FRAME_OF_REFERENCE = 2, HY_ENC_REFERENCE = 3,
       HY_ENC_MVCC = 4 /* not a column encoding: a chunk's MvccData, see hy_validate */,
       HY_ENC_RUN_LENGTH = 5 /* RunLengthSegment<T> (run_length_segment.hpp): data = run values (T[aux_size]), aux = inclusive end
                              * positions (uint32_t[aux_size]), nulls = per-run NULL flags as BYTES (uint8_t[aux_size], cast), width =
                              * sizeof(T).  The runs stay runs in device memory: hy_table_scan reads them in place (one search of
                              * the end positions per eight rows, run_length_segment_iterable.hpp:100-160); the other operators read a
                              * ValueSegment twin that a device kernel decodes from them the first time one of them asks. */ };

/* HY_ENC_LZ4 = 6: an LZ4Segment<T> of a numeric type (lz4_segment.hpp:25-60, lz4_segment.cpp:125-226): `data` points at ONE hy_lz4_blocks
 * (host memory: such a segment is handed over with HY_MEM_HOST), width = sizeof(T), nulls = the optional null bitmap like a ValueSegment's.
 * The blocks -- compressed one by one with LZ4_compress_*_usingDict against the segment's dictionary, so that each decompresses on its own --
 * travel to the device as they are and a kernel decompresses them there (one wavefront per block, the block's output staged in LDS); the
 * column then holds the ValueSegment the segment was compressed from (the reference, too, decompresses an LZ4Segment to scan it).
 * LZ4 string segments stay with the host like every string payload. */
enum { HY_ENC_LZ4 = 6 };
typedef struct hy_lz4_blocks {
  const void* const* blocks;      /* [block_count] the compressed blocks (pmr_vector<pmr_vector<char>>: one buffer each)             */
  const uint32_t* block_bytes;    /* [block_count] their compressed sizes                                                           */
  uint32_t block_count;
  uint32_t block_size;            /* decompressed bytes of every block but the last (LZ4Encoder::BLOCK_SIZE = 16 384), at most 65 536  */
  uint32_t last_block_size;       /* ... of the last                                                                                */
  uint32_t dictionary_bytes;      /* 0: a single block, compressed without a dictionary                                            */
  const void* dictionary;
} hy_lz4_blocks;

/* hy_segment::sorted_by: the chunk is individually sorted by this column (Chunk::individually_sorted_by, chunk.hpp:160-176;
 * HY_SORT_* = hyrise::SortMode + 1, types.hpp:219).  ColumnVsValue / ColumnBetween scans then find the matching row range with
 * binary searches instead of reading the segment (sorted_segment_search.hpp:20-384, column_vs_value_table_scan_impl.cpp:46-55). */
enum { HY_SORT_NONE = 0, HY_SORT_ASCENDING_NULLS_FIRST = 1, HY_SORT_DESCENDING_NULLS_FIRST = 2, HY_SORT_ASCENDING_NULLS_LAST = 3,
       HY_SORT_DESCENDING_NULLS_LAST = 4 };

/* Where the pointers of a descriptor / result live. */
enum { HY_MEM_HOST = 0, HY_MEM_DEVICE = 1 };

#define HY_INVALID_VALUE_ID 0xFFFFFFFFu /* "not found" (types.hpp:152), NOT the NULL value id */
#define HY_FOR_BLOCK_SIZE 2048u         /* frame_of_reference_segment.hpp:49 */
#define HY_INVALID_COLUMN 0xFFFFu       /* COUNT(*) argument (INVALID_COLUMN_ID)                      */

typedef struct hy_row_id {
  uint32_t chunk_id;
  uint32_t chunk_offset;
} hy_row_id;

typedef struct hy_column hy_column; /* opaque: one column of a table, chunk by chunk, resident on the device */

/*
 * One segment (= one column of one chunk).  Plain views of what Hyrise keeps in pmr_vectors.
 *   UNENCODED          data = T values[size]                       width = sizeof(T)
 *   DICTIONARY         data = attribute vector (value ids)          width = 1|2|4 (FixedWidthInteger), or width = 0 and
 *                      bits = 1..32: a BitPackingVector (bitpacking_vector_type.hpp:18) -- compact::vector<uint32_t, 0, uint64_t>:
 *                      element i occupies bits [i * bits, (i + 1) * bits) of a little-endian stream of 64-bit words.  It stays
 *                      packed in device memory: hy_table_scan unpacks in registers (bitpacking_decompressor.hpp:35-37), the other
 *                      operators read a FixedWidthInteger twin unpacked on the device on first use
 *                      aux  = T dictionary[aux_size] sorted unique; may be NULL for HY_TYPE_STRING
 *                      (then comparisons must be passed as pre-resolved value ids, see hy_predicate)
 *   FRAME_OF_REFERENCE data = offset values                         width = 1|2|4, or bit-packed (width = 0, bits) like DICTIONARY
 *                      aux  = int32 block_minima[aux_size]
 *   REFERENCE          data = hy_row_id pos_list[size]  (NULL => EntireChunkPosList{ref_chunk_id,size})
 *                      ref  = the referenced column (data segments only; reference_segment.hpp:36-38)
 * nulls: optional bitmap (see header comment); NULL when the segment stores no NULLs.
 * Dictionary segments carry NULLs as value id == aux_size instead (dictionary_segment.cpp:139-141).
 */
typedef struct hy_segment {
  uint32_t encoding;   /* HY_ENC_* */
  uint32_t data_type;  /* HY_TYPE_* of the logical column */
  uint32_t size;       /* rows in this chunk */
  uint32_t width;      /* bytes per element of `data` */
  const void* data;
  const void* aux;
  uint32_t aux_size;
  uint32_t ref_chunk_id;     /* REFERENCE: common chunk id if the pos list references a single chunk, else ~0u */
  const uint64_t* nulls;
  const hy_column* ref;      /* REFERENCE only */
  uint32_t sorted_by;        /* HY_SORT_*: 0 unless the chunk is flagged as sorted by this column */
  uint32_t bits;             /* bits per element of a BitPackingVector in `data` (width == 0), else 0 */
} hy_segment;

/* A literal as the scan implementations receive it after the lossless cast (table_scan.cpp:312-452). */
typedef union hy_value {
  int32_t i32;
  int64_t i64;
  float f32;
  double f64;
  uint32_t value_id;
} hy_value;

/*
 * Predicate of ColumnVsValue / ColumnBetween / ColumnIsNull scans.
 *   condition   HY_PRED_*; two-sided (between) conditions use value and value2.
 *   value_type  HY_TYPE_* of value/value2; must equal the column type (ColumnVsValueTableScanImpl asserts this,
 *               column_vs_value_table_scan_impl.cpp:34-36).
 *   Dictionary segments whose dictionary is not on the device (strings): the caller resolves the literal per chunk
 *   exactly as column_vs_value_table_scan_impl.cpp:211-226 / column_between_table_scan_impl.cpp:112-124 do and passes
 *   per_chunk_lower / per_chunk_upper (value ids, HY_INVALID_VALUE_ID = past the end) plus, for =/!=,
 *   per_chunk_found (1 if dictionary[lower] == literal).  Arrays have one entry per chunk of the column.
 */
typedef struct hy_predicate {
  uint32_t condition;
  uint32_t value_type;
  hy_value value;
  hy_value value2;
  const uint32_t* per_chunk_lower;
  const uint32_t* per_chunk_upper;
  const uint8_t* per_chunk_found;
  uint32_t column_is_nullable; /* Table::column_is_nullable(); matters for dictionary "matches all" early-outs */
  uint32_t reserved;
  /* HY_PRED_LIKE / NOT_LIKE / LIKE_INSENSITIVE / NOT_LIKE_INSENSITIVE on dictionary (incl. FixedString) segments
   * (ColumnLikeTableScanImpl::_scan_dictionary_segment, column_like_table_scan_impl.cpp:69-140): the adapter runs Hyrise's
   * LikeMatcher over every chunk's dictionary (`_find_matches_in_dictionary`: one matcher call per DISTINCT string -- a few thousand
   * for p_type, 15 million at SF10 for o_comment; hy_table_scan_like does this pass on the device instead) and passes the result as
   * bitmaps: bit v of the words starting at match_words[match_word_offsets[c]] says whether value id v of data chunk c
   * satisfies the predicate (the matcher already applies NOT); match_word_offsets has one entry per data chunk plus the
   * end.  The device scans the attribute vectors against the bitmaps; the NULL value id never matches. */
  const uint64_t* match_words;
  const uint64_t* match_word_offsets;
} hy_predicate;

/* Per-chunk classification the scan reports (TableScan::PerformanceData counters, table_scan.hpp:56-69). */
enum {
  HY_CHUNK_SCANNED = 0,      /* PosList materialised in `matches`                                              */
  HY_CHUNK_ALL_MATCH = 1,    /* every row matches: count == size, NO RowIDs written (EntireChunkPosList)        */
  HY_CHUNK_NONE_MATCH = 2    /* early-out, count == 0                                                           */
};

/*
 * Result of a scan.  `matches` holds the PosLists of all chunks back to back, in input-chunk order; chunk c owns
 * matches[offsets[c] .. offsets[c+1]).  Positions are relative to the *input* chunk (scan_chunk() contract,
 * abstract_dereferenced_column_table_scan_impl.cpp:75-80), ascending, bit-identical to the CPU operator's PosList.
 * All arrays are caller-allocated, in the memory space `mem`.
 */
typedef struct hy_scan_result {
  uint32_t mem;            /* HY_MEM_HOST | HY_MEM_DEVICE */
  uint32_t flags;          /* HY_SCAN_* */
  hy_row_id* matches;      /* capacity RowIDs */
  uint64_t capacity;
  uint64_t* offsets;       /* [n_chunks + 1] */
  uint32_t* counts;        /* [n_chunks] matches per chunk (== size for ALL_MATCH chunks) */
  uint8_t* chunk_state;    /* [n_chunks] HY_CHUNK_* */
  uint64_t total_matches;  /* filled for HY_MEM_HOST results; for device results read offsets[n_chunks] */
} hy_scan_result;

#define HY_SCAN_MATERIALIZE_ALL_MATCH 1u /* also write RowIDs for ALL_MATCH chunks (what the CPU impl does internally) */
/* Layout of `matches`.  Host results are always back to back: offsets[c+1] == offsets[c] + RowIDs written for chunk c.
 * Device results use CHUNK REGIONS (the flag must be set to acknowledge it): chunk c's PosList starts at
 * offsets[c] = number of rows in all chunks before c and holds counts[c] RowIDs (none for an elided ALL_MATCH chunk);
 * offsets[n_chunks] = total rows; capacity must be >= total rows.  The kernel then needs no global prefix sum at all. */
#define HY_SCAN_CHUNK_REGIONS 2u

/* ---- runtime -------------------------------------------------------------------------------------------------- */
int32_t hy_abi_version(void);
hy_status hy_init(int32_t device);            /* selects the HIP device of the process (one process per GPU): every thread that calls
                                               * into the library afterwards is bound to it on its first call */
hy_status hy_shutdown(void);
const char* hy_last_error(void);              /* thread-local message of the last non-OK status */
hy_status hy_set_stream(void* hip_stream);    /* thread-local stream used for all launches; NULL = default stream     */
hy_status hy_synchronize(void);
hy_status hy_device_malloc(void** ptr, size_t bytes);
hy_status hy_device_free(void* ptr);
hy_status hy_memcpy_h2d(void* dst, const void* src, size_t bytes);
hy_status hy_memcpy_d2h(void* dst, const void* src, size_t bytes);
hy_status hy_device_count(int32_t* count);
/* Measurement hook: when enabled (> 0), operator calls time their dominant kernel (scan_slices, join probe, aggregate
 * accumulate) with a pair of HIP events on the launch stream; enabled = n > 1 times every n-th call only (a timed
 * launch costs several microseconds of stream time).  hy_profile_read() waits for the recorded events and returns the
 * summed elapsed time and the number of timed launches since profiling was (re-)enabled. */
hy_status hy_set_profiling(int32_t enabled);
hy_status hy_profile_read(float* total_milliseconds, uint32_t* launches);
/* The same per kernel, without resetting: an operator chain (bench.py's TableScan + JoinHash step) reads the time of each of its
 * timed kernels separately before hy_profile_read() clears the session. */
enum { HY_KERNEL_OTHER = 0, HY_KERNEL_SCAN = 1, HY_KERNEL_JOIN_PROBE = 2, HY_KERNEL_JOIN_COUNT = 3, HY_KERNEL_JOIN_BUILD = 4, HY_KERNEL_AGGREGATE = 5,
       HY_KERNEL_PROJECTION = 6, HY_KERNEL_LIKE = 7 /* like_match, the dictionary matcher */,
       HY_KERNEL_STRING_RANK = 8 /* string_rank, one string dictionary ordered against another; the launch sequence of hy_string_dictionary_order */, HY_KERNEL_KINDS = 9 };
hy_status hy_profile_read_kernel(uint32_t kernel, float* total_milliseconds, uint32_t* launches);
/* What such an event pair measures beyond the kernel itself (the pair is stamped from the dispatch packet): the elapsed time of an
 * empty kernel, median of 32 launches, measured once per process.  A profiler's per-kernel duration is shorter by about this much. */
hy_status hy_profile_event_overhead(float* milliseconds);

/* ---- result-buffer pool: device memory for PosLists that outlive the call that wrote them -----------------------------------------
 * The reference's operators hand their results on as tables whose ReferenceSegments share PosLists (AbstractPosList,
 * storage/pos_lists/abstract_pos_list.hpp:18-75; reference_segment.hpp:36-38; table_scan.cpp:207-210; join_output_writing.cpp:95-200): a PosList
 * lives as long as a table references it.  An adapter that keeps operator chains in HBM (DevicePosList in hyrise_amd/host/hyrise_host.hpp,
 * INTEGRATION.md section 3) takes the memory of such PosLists from this pool and gives it back when the PosList object dies; blocks are
 * handed out again in stream order (the next owner's stream waits for what the last owner's stream still had queued), hipMalloc runs only when
 * nothing fits.  Process-wide per device, thread-safe.
 *   hy_result_pool_acquire       one buffer of at least `bytes` bytes (a scan's PosLists, a gathered PosList)
 *   hy_result_pool_acquire_pair  the two PosLists of a join with `rows` RowIDs each: every list an allocation of its own, the first starting on
 *                                a 2 MiB boundary, the second 1.25 MiB past one -- two streams written at the same index at the same time then
 *                                use different memory channels; prefers the pair a calibration kept
 *   hy_result_pool_release       either kind, one pointer at a time (NULL: nothing)
 *   hy_result_pool_calibrate     where a join's output lists lie in HBM decides the emit kernel's speed by up to 20 %, reproducibly per allocation
 *                                (profiles/r04_join_placement.txt, r05_placement_probe.txt): `candidates` fresh pairs for `rows` RowIDs are
 *                                allocated, the join left x right (mode) runs a few times into each (HIP events on the calling thread's stream),
 *                                the fastest pair stays in the pool as the one hy_result_pool_acquire_pair hands out first (with
 *                                HY_POOL_KEEP_MEDIAN the median candidate stays too, second in line -- what an uncalibrated pool gets on
 *                                average), the others are freed.  ms_per_candidate ([candidates], may be NULL): milliseconds per join;
 *                                *chosen: the fastest.  Run it once, outside any timed region, when the process knows its largest join.
 *   hy_result_pool_trim          frees every buffer of the calling thread's device that nobody holds (waits for the thread's stream) */
#define HY_POOL_KEEP_MEDIAN 1u
hy_status hy_result_pool_acquire(uint64_t bytes, void** ptr);
hy_status hy_result_pool_acquire_pair(uint64_t rows, hy_row_id** left, hy_row_id** right);
hy_status hy_result_pool_release(void* ptr);
hy_status hy_result_pool_calibrate(const hy_column* left, const hy_column* right, uint32_t mode, uint64_t rows, uint32_t candidates, uint32_t flags,
                                   float* ms_per_candidate, uint32_t* chosen);
hy_status hy_result_pool_trim(void);
hy_status hy_result_pool_stats(uint64_t* held_bytes, uint64_t* in_use_bytes, uint32_t* calibrated_pairs);
/* The calling thread's pool of TEMPORARY blocks (what operators take for exports, sort buffers and the like, and hand back in stream order;
 * hy_shutdown frees it): the bytes it holds between calls and its largest block.  Either pointer may be NULL. */
hy_status hy_temporary_pool_stats(uint64_t* held_bytes, uint64_t* largest_block_bytes);

/* ---- options: which of several equivalent paths / launch shapes an operator takes ---------------------------------------------
 * Process-wide integers with the defaults below.  EVERY setting produces the same results: the tests force each path with them and
 * compare it with the oracle, the tools time one path against another in one process.  The library reads no environment variable
 * (a build with -DHY_DEBUG_SWITCHES adds the trace / timing / parts-switched-off aids of DESIGN.md section 6; release builds do not
 * contain them). */
enum {
  HY_OPT_ALLOW_ANY_ARCH = 0,         /* 0    hy_init accepts a device that is not gfx950 (nothing is tuned for it)                    */
  HY_OPT_JOIN_RANK_TABLE = 1,        /* 1    unique dense-ish integer build keys get a rank table (else: the sorted directory)          */
  HY_OPT_JOIN_HINT = 2,              /* 1    later joins over a resident build column fill the table in one checked pass              */
  HY_OPT_JOIN_BREAK_HINT = 3,        /* 0    tests: hand the checked fill a hint that does not hold (the join must notice and rerun)   */
  HY_OPT_JOIN_PKFK = 4,              /* 1    the primary-key / foreign-key probe kernels (join_pkfk.hpp)                              */
  HY_OPT_JOIN_LDS_BUILD = 5,         /* 1    rank tables below 2^20 key values are staged in LDS ...                                  */
  HY_OPT_JOIN_LDS_BUILD_TILES = 6,   /* 2048 ... from this many probe tiles on                                                        */
  HY_OPT_JOIN_FILL_WGS_PER_CU = 7,   /* 4    the checked one-pass fill wave by wave (rank_table_fill_waves: this many resident workgroups per
                                      *      CU, <= 8); 0 = one short-lived workgroup per slice (rank_table_fill_checked)              */
  HY_OPT_JOIN_HAND_OVER_RANKS = 8,   /* 2^20 Inner PK-FK joins whose probe keys have no locality, whose probe side has at least this many rows and whose
                                      *      rank table has a megabyte or more: pass 1 leaves the partners' ranks behind (4 bytes a probe row), pass 2
                                      *      reads them back instead of looking every key up again; 0 = never, 1 = whenever the keys lack locality */
  HY_OPT_AGG_PARTITION_BITS = 9,     /* 0    partition bits of the many-groups path, 0 = derived from the row count; > 0 also forces the path */
  HY_OPT_AGG_SPILL_SHIFT = 10,       /* 3    aggregate_rows gives up when rows >> shift left its LDS tables                           */
  HY_OPT_AGG_SMALL_DOMAIN = 11,      /* 1    sd_groups / sd_wide (aggregate_small.hpp) for the shapes they accept                     */
  HY_OPT_FUSED_SMALL_DOMAIN = 12,    /* 1    fused_small_domain for the shapes it accepts                                             */
  HY_OPT_SCAN_TWO_COLUMNS = 13,      /* 1    ColumnVsColumn over two data columns of W-byte vectors: the two-stream kernel with the chunks' dictionaries in LDS */
  HY_OPT_STAR_FUSED_PROBE = 14,      /* 1    hy_star_join_aggregate probes every dimension in ONE pass over the fact table (csrc/join_star.hpp) where the
                                      *      shape allows; 0 = one hy_join_hash per dimension                                                      */
  HY_OPT_STAR_FUSED_FINISH = 15,     /* 1    ... and groups the survivors where it finds them (star_finish) where every GROUP BY column and aggregate input
                                      *      is an int / long column: no RowIDs, exports, projection, hy_aggregate_hash; 0 = those four steps     */
  HY_OPT_LDS_ORDERED_ATOMICS = 16,  /* 1    the device decides (probed once per process) whether ranking rests on lane-ordered returning LDS atomics: the
                                      *      staged sort of sort_pairs_u32 and of the join's build side, the sort-then-fill of unsorted unique build keys,
                                      *      the PK-FK probe kernels, rt_probe_emit's one atomic per pair; 0 = tests: answer "not ordered" without
                                      *      asking the device -- the paths a device without that order takes (sort_scatter, rank_table_mark ..
                                      *      rank_table_scatter_rows, the general rank-table kernels, match-any ranking)                             */
  HY_OPT_PRODUCT_NONTEMPORAL = 17,  /* 0    hy_product writes its 16-byte vectors with nontemporal stores (1) or through the write-back L2 (0);
                                      *      tools/product_timing.py times one against the other in one process                                  */
  HY_OPT_JOIN_COMPACT_STAGE = 18,   /* 1    pk_emit stages 4-byte records (row, null partner, rank as a 16-bit delta on its wave's rank base) where every
                                      *      segment of the probe column is stored 1 or 2 bytes wide: three workgroups per CU instead of two;
                                      *      0 = the 8-byte records everywhere                                                                  */
  HY_OPT_STRING_SPARSE_GATHER = 19, /* 1    the string producers (hy_string_column_gather, hy_string_column_substr, hy_string_column_materialize) take the
                                      *      sparse route -- the column read at the rows asked for, only the entries those rows reference ranked
                                      *      (csrc/string_gather.hip) -- where the rows are few against the column's rows + dictionary entries
                                      *      (STRING_SPARSE_DIVISOR, csrc/hy_options.hpp); 0 = the dense route always (export of every source row,
                                      *      ranking of every entry); 2 = the sparse route always (tests, tools/string_gather_sparse_timing.py).
                                      *      Every setting gives the same bytes                                                                    */
  HY_OPT_COUNT = 20
  /* (rounds 4-5 had 33: launch shapes and store flavours whose A/B timings were flat twice are constants now -- csrc/hy_options.hpp --,
   *  the radix-partitioned join path, which lost to the rank table read in place by 1.7 x, is gone) */
};
hy_status hy_set_option(uint32_t option, int64_t value);
hy_status hy_get_option(uint32_t option, int64_t* value);

/* ---- several GPUs in one process, and the collectives between them (csrc/comm.hip: RCCL over xGMI) ----------------------------
 * Hyrise is one process whose operators run on scheduler workers (scheduler/operator_task.cpp:163-200): the multi-GPU shape is one
 * worker thread per GPU.  hy_bind_device makes the CALLING thread work on `device` (its stream, pools and every column it creates
 * belong to that device; threads that never call it use hy_init's device).  hy_comm_init_all creates one communicator per device of
 * the process (RCCL's single-process mode, ncclCommInitAll); hy_comm_init_rank one per process (id from hy_comm_unique_id, carried to
 * the other processes by the caller).  The collectives run on the calling thread's stream like a kernel launch (hy_synchronize waits
 * for them).  A thread that drives several devices' communicators brackets each collective for all of them with hy_comm_group_begin /
 * hy_comm_group_end.  What the sharded operators exchange: fixed-slot partial aggregates (all_reduce), (key, partial)
 * tables and build-side columns (all_gather), (key, RowID) tuples by key % G (all_to_all_v: grouped ncclSend / ncclRecv).
 * A device list that names ONE device n times (worker threads that share a GPU; RCCL refuses such a list) gets communicators that
 * exchange through that GPU's memory: same entry points, same results. */
typedef struct hy_comm hy_comm;
enum { HY_COMM_SUM = 0, HY_COMM_MIN = 1, HY_COMM_MAX = 2 };
enum { HY_COMM_ID_BYTES = 128 };
hy_status hy_bind_device(int32_t device);
hy_status hy_comm_unique_id(void* id_128_bytes);
hy_status hy_comm_init_rank(const void* id_128_bytes, uint32_t world, uint32_t rank, hy_comm** comm);
hy_status hy_comm_init_all(const int32_t* devices, uint32_t n_devices, hy_comm** comms /* [n_devices] */);
hy_status hy_comm_destroy(hy_comm* comm);
hy_status hy_comm_rank(const hy_comm* comm, uint32_t* rank, uint32_t* world);
hy_status hy_comm_group_begin(void);
hy_status hy_comm_group_end(void);
hy_status hy_comm_all_reduce(hy_comm* comm, const void* send, void* recv, uint64_t count, uint32_t data_type /* HY_TYPE_INT / LONG / FLOAT / DOUBLE */, uint32_t op);
hy_status hy_comm_all_gather(hy_comm* comm, const void* send, void* recv /* world x bytes_per_rank */, uint64_t bytes_per_rank);
/* send / recv: the bytes for / from rank 0, rank 1, ... back to back */
hy_status hy_comm_all_to_all_v(hy_comm* comm, const void* send, const uint64_t* send_bytes, void* recv, const uint64_t* recv_bytes);

/* ---- residency cache: a column made device-visible once (encoded segments are immutable,
 *      abstract_encoded_segment.hpp:12-17) ------------------------------------------------------------------------ */
/* mem == HY_MEM_HOST: segment buffers are copied to HBM and owned by the hy_column.
 * mem == HY_MEM_DEVICE: pointers are device pointers and stay owned by the caller; the call does not wait for the device: the column's
 *                       descriptor tables are complete in the order of the calling thread's stream (every entry point this thread calls
 *                       afterwards sees them; another thread synchronises with this one first -- hy_synchronize -- like for the data
 *                       the pointers name).  (One exception: a RunLength segment that comes with run null bytes -- the call reads them
 *                       back behind the thread's stream, to drop them where no run is NULL, as it does for host memory.)
 *   What a caller's device buffers must satisfy (tests/test_device_memory_columns_gpu.py runs every operator over buffers laid out to
 *   these rules and no better):
 *     alignment  every buffer on a multiple of its element size: `data` on `width` bytes (8 for a PosList and for the words of a
 *                BitPackingVector), `aux` on the dictionary's type width / 4 bytes (block minima, run ends, begin commit ids), `nulls` on 8
 *                bytes (a null bitmap), 4 (end commit ids) or 1 (the null bytes of a RunLength segment).  Nothing more is needed for a correct
 *                result: a segment whose `data` is not on a 16-byte or whose bitmap is not on an 8-byte boundary is read row by row where the
 *                arena's layout is read in groups of eight (scans, joins' dense materialise, the aggregates' plain 4-byte inputs, projections'
 *                plain operands take their general paths).
 *     slack      16 readable bytes behind the last element of every buffer -- what the library's own arena (HY_MEM_HOST) keeps: the last
 *                partial group of eight rows is fetched with full vector loads.  Their contents are never used: they may be another buffer's.
 *                A buffer must therefore not end its allocation.
 *     results    (audited per entry point: the widest store made at an address derived from the caller's pointer)
 *                hy_table_scan / hy_table_scan_columns / hy_validate, mem = HY_MEM_DEVICE: `matches` is written two RowIDs per 16-byte store at
 *                  even RowID indices -> `matches` on 16 bytes, `offsets` on 8, `counts` on 4, `chunk_state` any; otherwise HY_ERR_INVALID
 *                  before any launch.
 *                hy_join_hash / _predicates / _finish, mem = HY_MEM_DEVICE: two pairs per 16-byte store at even pair indices -> `left_pos` and
 *                  `right_pos` on 16 bytes, `slice_offsets` on 8; otherwise HY_ERR_INVALID before any launch.  (hy_result_pool_acquire_pair
 *                  and hy_result_pool_acquire hand out such blocks, with the 16 bytes of slack behind what was asked for.)
 *                hy_aggregate_hash / hy_scan_project_aggregate / hy_star_join_aggregate, mem = HY_MEM_DEVICE: copied into place (hipMemcpy):
 *                  any address; sensibly RowIDs on 8, values on their width.
 *                hy_sort / hy_sort_limit `out`: 16-byte stores where `out` is on 16 bytes, RowID by RowID otherwise -> 8.
 *                hy_join_sort_merge lists, hy_union_positions `out`: RowID by RowID -> 8, checked (HY_ERR_INVALID, nothing written).
 *                hy_product lists: 16-byte stores at the list's even slots, RowID by RowID at a region's odd head or tail -> 8, checked.
 *                hy_poslist_translate `out`, hy_column_export: element by element -> element size.
 *                hy_gather_row_ids / hy_poslist_gather `out`: 16-byte stores where positions and `out` are on 16 bytes, else RowID by RowID -> 8. */
hy_status hy_column_create(const hy_segment* segments, uint32_t n_chunks, uint32_t mem, hy_column** out);
hy_status hy_column_destroy(hy_column* column);
hy_status hy_column_row_count(const hy_column* column, uint64_t* rows);
hy_status hy_column_chunk_count(const hy_column* column, uint32_t* chunks);

/* ---- TableScan (replaces TableScan::_on_execute's per-chunk scan_chunk() fan-out, table_scan.cpp:97-240) --------- */
/* ColumnVsValue / ColumnBetween / ColumnIsNull (column_vs_value_table_scan_impl.cpp, column_between_table_scan_impl.cpp,
 * column_is_null_table_scan_impl.cpp), over data or reference columns.  excluded_chunks may be NULL.
 * Floating point compares as IEEE on every layout: -0.0 equals 0.0; a NaN row and a NaN literal (it is not refused) match only <>. */
hy_status hy_table_scan(const hy_column* column, const hy_predicate* predicate, const uint32_t* excluded_chunks,
                        uint32_t n_excluded, hy_scan_result* result);
/* `column IN (v1, ..., vk)` / `column NOT IN (...)` over a literal list -- the InExpressions that InExpressionRewriteRule leaves alone
 * (in_expression_rewrite_rule.hpp:31,38: lists of 4 .. 19 elements, longer ones whose elements differ in type) and that the reference's
 * TableScan hands to its ExpressionEvaluator (expression_evaluator.cpp:404-506).
 *   IN matches a row iff it is not NULL and operator== holds against at least one element; NOT IN iff it is not NULL and no element
 *   is equal.  Floating point compares with ==: -0.0 equals 0.0, a row that holds NaN is never IN and always NOT IN.  Order and
 *   duplicates of the elements do not matter.
 *   values      n_values non-NULL literals of exactly the column's type (value_type == the column's HY_TYPE_*), in host memory: the
 *               evaluator's fast path.  Lists with NULLs or elements of other types go through hy_in_list_cast first.
 *               n_values == 0: HY_ERR_INVALID (the reference's constant answer for an empty list is the adapter's business); more than
 *               HY_MAX_IN_LIST: HY_ERR_UNSUPPORTED; a NaN element or another value_type than the column's: HY_ERR_INVALID.  Nothing is
 *               written in any of these cases.
 *   per_chunk_value_ids   dictionary segments whose dictionary is not on the device (strings; value_type = HY_TYPE_STRING, `values` is
 *               not read): [n_data_chunks x n_values], entry [c * n_values + i] = the value id of element i in data chunk c's
 *               dictionary (lower_bound plus an equality check, as for per_chunk_lower / per_chunk_found) or HY_INVALID_VALUE_ID.
 *               For a reference column the data chunks are those of the referenced column.
 * Dictionary segments are scanned against a per-chunk bitmap over their value ids that the device builds from the list (one binary
 * search of the chunk's dictionary per element); every other segment's rows are searched in the sorted list. */
#define HY_MAX_IN_LIST 256
typedef struct hy_in_list {
  uint32_t value_type;
  uint32_t n_values;
  const hy_value* values;
  uint32_t negated;            /* 0: IN, 1: NOT IN */
  uint32_t column_is_nullable;
  const uint32_t* per_chunk_value_ids;
} hy_in_list;
/* Result contract, flags, alignment rules and `mem` handling: hy_table_scan's, bit for bit (data and reference columns, excluded_chunks
 * for data columns).  chunk_state reports HY_CHUNK_NONE_MATCH only for a dictionary chunk that holds none of the elements (IN) and for
 * excluded chunks; it never reports HY_CHUNK_ALL_MATCH. */
hy_status hy_table_scan_in_list(const hy_column* column, const hy_in_list* list, const uint32_t* excluded_chunks, uint32_t n_excluded,
                                hy_scan_result* result);
/* The list handling in front of hy_table_scan_in_list (rewrite_in_list_expression ORs `=` terms, whose literals
 * lossless_predicate_cast decides): every literal is cast to the column's type without loss; one that cannot be can equal no row and
 * is dropped; a NULL literal (HY_TYPE_NULL) is dropped and reported in *has_null -- it leaves IN as it is and makes NOT IN match
 * nothing.  out: room for n values; *n_out of them are written, in the order of the input.  A string literal against a numeric column
 * (HY_TYPE_STRING) is dropped as well; a string column takes no hy_value list: HY_ERR_INVALID.  Pure host arithmetic. */
hy_status hy_in_list_cast(uint32_t column_type, const uint32_t* literal_types, const hy_value* literals, uint32_t n, hy_value* out,
                          uint32_t* n_out, uint32_t* has_null);
/* ColumnVsColumn (column_vs_column_table_scan_impl.cpp:36-187): left <condition> right, both columns of one table.  String columns:
 * HY_ERR_UNSUPPORTED here -- the call has no dictionaries to read; hy_table_scan_columns_strings takes them. */
hy_status hy_table_scan_columns(const hy_column* left, const hy_column* right, uint32_t condition,
                                hy_scan_result* result);

/* ---- LIKE over string dictionaries in device memory (ColumnLikeTableScanImpl, column_like_table_scan_impl.cpp:69-159) ------------------
 * hy_predicate.match_words takes the LIKE family as bitmaps the HOST made, one matcher call per distinct string.  The entry points below
 * keep the dictionaries of a column's DictionarySegment<pmr_string> chunks in HBM beside the attribute vectors and run the matcher there.
 *
 * hy_string_dictionary: per data chunk of ONE column that chunk's dictionary entries in value-id order.  A chunk comes in one of two layouts:
 *   offsets != NULL   n_entries + 1 uint32_t byte offsets into `chars` (ascending; entry v = chars[offsets[v] .. offsets[v + 1])): what an
 *                     adapter packs once per column from a pmr_vector<pmr_string>.  Bytes are arbitrary; a '\0' inside an entry is data.
 *   offsets == NULL   n_entries slots of string_length bytes, read in place as FixedStringVector keeps them; an entry's length is
 *                     strnlen(slot, string_length) (fixed_string.cpp:86-99).
 *   n_entries == 0 is a legal chunk (the dictionary of a NULL-only segment); its pointers are not read.
 * mem == HY_MEM_HOST: the buffers are copied to HBM once and owned by the object (ascending offsets are checked: HY_ERR_INVALID).
 * mem == HY_MEM_DEVICE: the buffers stay the caller's, under hy_column_create's rules for caller-owned inputs: `offsets` on 4 bytes, `chars`
 *   at ANY byte address, 16 readable bytes behind the last element of each.  Creating the object is pure host work; the object owns the
 *   small tables the first launch uploads.  The caller's offsets are not read by the call, so a chunk with entries needs its `chars`
 *   (NULL: HY_ERR_INVALID) even where every entry is empty; with HY_MEM_HOST `chars` may be NULL then.
 * A chunk whose chars would take 2^32 bytes or more: HY_ERR_UNSUPPORTED.  Nothing is allocated for a dictionary that is refused. */
typedef struct hy_string_dictionary hy_string_dictionary; /* opaque */
typedef struct hy_string_dictionary_chunk {
  uint32_t n_entries;
  uint32_t string_length;    /* offsets == NULL: bytes per slot */
  const char* chars;
  const uint32_t* offsets;   /* [n_entries + 1], or NULL */
} hy_string_dictionary_chunk;
hy_status hy_string_dictionary_create(const hy_string_dictionary_chunk* chunks, uint32_t n_chunks, uint32_t mem, hy_string_dictionary** out);
hy_status hy_string_dictionary_destroy(hy_string_dictionary* dict);
/* The bitmap layout of hy_predicate.match_words / match_word_offsets: chunk c owns ceil(n_entries_c / 64) words from word_offsets[c];
 * word_offsets: host memory, [n_chunks + 1].  Pure host arithmetic. */
hy_status hy_string_dictionary_match_layout(const hy_string_dictionary* dict, uint64_t* word_offsets);
/* The pattern language, that of the mirror's LikeMatcher and hyrise_amd/like.py (like_matcher.cpp:32-55): `%` matches any run of bytes,
 * including none; `_` exactly one byte; everything else is literal.  Bytes, not code points.  The insensitive conditions fold ASCII A-Z on
 * both sides: the host folds the pattern once, the kernel an entry as it reads it.
 * hy_like_tokenize: the pattern as the kernel takes it -- one token per element: the literal byte, HY_LIKE_ANY_ONE or HY_LIKE_ANY_RUN (a run
 * of `%` is one token).  tokens: room for HY_MAX_LIKE_PATTERN.  Pure host work.  A condition outside HY_PRED_LIKE .. NOT_LIKE_INSENSITIVE:
 * HY_ERR_INVALID; a pattern of more than HY_MAX_LIKE_PATTERN bytes: HY_ERR_UNSUPPORTED (the adapter keeps its host matcher for it). */
#define HY_MAX_LIKE_PATTERN 256
#define HY_LIKE_ANY_ONE 0x100u
#define HY_LIKE_ANY_RUN 0x200u
hy_status hy_like_tokenize(const char* pattern, uint32_t pattern_bytes, uint32_t condition, uint16_t* tokens, uint32_t* n_tokens);
/* The matcher, one launch: bit v % 64 of match_words[word_offsets[c] + v / 64] is set iff entry v of chunk c satisfies the condition (NOT
 * applied); the tail bits of a chunk's last word are zero, under the NOT forms too.  mem == HY_MEM_DEVICE: the words stay in the caller's
 * device buffer (on 8 bytes, otherwise HY_ERR_INVALID; one 8-byte store per word), complete in the order of the calling thread's stream.
 * mem == HY_MEM_HOST: copied back; the call returns when they are there.  All refusals come before any launch. */
hy_status hy_like_matches(const hy_string_dictionary* dict, const char* pattern, uint32_t pattern_bytes, uint32_t condition, uint32_t mem,
                          uint64_t* match_words);
/* hy_table_scan for `column <LIKE condition> pattern` with the bitmaps made on the device: the matcher runs on the calling thread's stream
 * into the scratch arena, the scan reads the words where they are.  The result is hy_table_scan's for the same predicate with host-made
 * bitmaps, bit for bit (matches, offsets, counts, chunk states, every HY_SCAN_* flag, either result->mem; excluded_chunks for data columns).
 * `column` may be a reference column; `dict` then belongs to the referenced data column.  HY_ERR_INVALID when the column is no string column
 * or dict's chunk count or any n_entries differs from the data column's dictionary segments (aux_size); HY_ERR_UNSUPPORTED for unencoded
 * string segments and for patterns beyond HY_MAX_LIKE_PATTERN.  Nothing is launched or written in any of these cases. */
hy_status hy_table_scan_like(const hy_column* column, const hy_string_dictionary* dict, const char* pattern, uint32_t pattern_bytes,
                             uint32_t condition, uint32_t column_is_nullable, const uint32_t* excluded_chunks, uint32_t n_excluded,
                             hy_scan_result* result);

/* ---- ColumnVsColumn on two string columns (column_vs_column_table_scan_impl.cpp:145-187 with pmr_string on both sides) ----------------
 * Per chunk the left column's dictionary L is ordered against the right column's R (both sorted and duplicate-free, as DictionarySegment
 * keeps them), n_r = R's entry count:
 *     lo(v)   = number of right entries < L[v]                     (lower_bound)
 *     eq(v)   = lo(v) < n_r && R[lo(v)] == L[v]
 *     rank(v) = 2 * lo(v) - (eq(v) ? 0 : 1)                        (int32_t; -1 for an entry below every right entry that equals none)
 * The rank of right entry r is 2 * r, and L[v] <cond> R[r] holds iff rank(v) <cond> 2 * r for each of the six comparisons: with eq(v),
 * L[v] = R[lo] and 2lo against 2r decides; without, R[lo - 1] < L[v] < R[lo] and the odd 2lo - 1 lies strictly between 2(lo - 1) and 2lo.
 * Order is std::string's: bytes compared as unsigned, the shorter string first when it is the other's prefix; a '\0' inside an entry of
 * the offsets layout is data, an entry of the fixed-length layout ends at strnlen(slot, string_length).  A chunk without entries on
 * either side is legal (every lo is 0, eq false).  A right dictionary that is not sorted gives unspecified ranks; no byte outside the two
 * chunks' chars is read even then (entries are read exactly, the 16 bytes of slack are not touched).
 *
 * hy_string_dictionary_ranks: one launch for all chunks of the pair.  ranks: the sum of left's n_entries int32_t; chunk c's ranks start at
 * the sum of left's n_entries before c.  mem == HY_MEM_DEVICE: ranks stay in the caller's device buffer (on 4 bytes, otherwise
 * HY_ERR_INVALID), complete in the order of the calling thread's stream, no host round trip.  mem == HY_MEM_HOST: copied back; the call
 * returns when they are there.  HY_ERR_INVALID: dictionaries with different chunk counts, on different devices, or not on the calling
 * thread's device.  HY_ERR_UNSUPPORTED: a right chunk of 2^30 entries or more (2 * lo would overflow).  All refusals come before any launch. */
hy_status hy_string_dictionary_ranks(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem, int32_t* ranks);
/* hy_table_scan_columns for two string columns of one table: the ranking above runs on the calling thread's stream into the scratch arena,
 * both columns get an int32 dictionary stand-in for the length of the call (the ranks on the left, 0, 2, 4, ... on the right, over the
 * caller's attribute vectors and with the caller's NULL value ids -- for reference columns behind the same PosLists), and the row pass is
 * hy_table_scan_columns' own.  Result contract, flags, alignment rules and `mem` handling: hy_table_scan_columns', bit for bit.  The six
 * binary conditions only; a NULL on either side matches nothing.  Both columns are data columns, or both are reference columns whose
 * chunks hold the same PosLists (one reference table's columns: the caller's guarantee, as for hy_table_scan_columns); the dictionaries belong to the referenced data columns.  Passing the same column and
 * dictionary on both sides is legal.
 * HY_ERR_INVALID: a column that is no string column ("Trying to compare strings and non-strings"); a data column against a reference
 * column; a dictionary whose chunk count or any n_entries differs from its data column's
 * dictionary segments (aux_size); the refusals of hy_table_scan_columns and of hy_string_dictionary_ranks.  HY_ERR_UNSUPPORTED: unencoded
 * or LZ4 string segments, a right chunk of 2^30 entries or more.  Nothing is launched or written in any of these cases.
 * Ranks are not kept between calls. */
hy_status hy_table_scan_columns_strings(const hy_column* left, const hy_string_dictionary* left_dict, const hy_column* right,
                                        const hy_string_dictionary* right_dict, uint32_t condition, hy_scan_result* result);

/* ---- One string column's global order (what Sort and MIN / MAX need of a pmr_string column; the joins read the joint order below) ------
 * hy_string_dictionary_ranks orders chunk c of one column against chunk c of another.  The entry points below order ALL chunks of ONE
 * column against each other: for entry v of chunk c
 *     rank(c, v) = the number of DISTINCT strings, over all chunks of `dict`, that are smaller than the entry        (dense rank)
 * Equal strings in different chunks get equal ranks; ranks run 0 .. n_distinct - 1; a chunk's ranks ascend strictly with v (its dictionary
 * is sorted and duplicate-free).  Order is std::string's, as above: bytes compared as unsigned, a prefix first, a '\0' inside an entry of
 * the offsets layout is data, an entry of the fixed-length layout ends at strnlen(slot, string_length); the two layouts may be mixed across
 * chunks.  These are the numbers hyrise_amd/string_keys.py StringRanks and the mirror's host ranking produce, bit for bit.
 * On the device the chunks' dictionaries -- sorted runs already -- are merged pairwise in ceil(log2(n_chunks)) rounds (one launch each, one
 * binary search of the sibling run per entry), then a head flag per merged position, a prefix sum and a scatter: nothing crosses to the host.
 * A dictionary that is not sorted gives unspecified ranks; no byte outside the call's buffers is read or written even then.
 *
 * hy_string_dictionary_order   ranks: E = the sum of all n_entries int32_t; chunk c's ranks start at the sum of n_entries before c (the
 *   layout of hy_string_dictionary_ranks).  mem == HY_MEM_DEVICE: ranks stay in the caller's device buffer (on 4 bytes, otherwise
 *   HY_ERR_INVALID), complete in the order of the calling thread's stream.  mem == HY_MEM_HOST: copied back; the call returns when they are
 *   there.  n_distinct: HOST memory, may be NULL; when it is given the call waits for the stream.  E == 0: HY_OK, nothing is launched,
 *   *n_distinct = 0.  HY_ERR_INVALID: a null dict / ranks, a bad mem, a dictionary of another device than the calling thread's.
 *   HY_ERR_UNSUPPORTED: E >= 2^31.  All refusals come before any launch and any allocation.  Temporaries (16 bytes per entry) come from the
 *   thread's scratch arena; the launches are timed under HY_KERNEL_STRING_RANK.
 *
 * hy_column_string_ranks   the int32 stand-in of a string column: *out is a column of HY_TYPE_INT with `column`'s chunk layout whose row r
 *   holds the rank of row r's string (NULL where row r is NULL).  `column`: a data column of string dictionary segments, or a reference
 *   column over one; `dict`: the dictionaries of the DATA column (chunk count and every n_entries equal to the segments' aux_size, as for
 *   hy_table_scan_like).
 *     data column       *out has dictionary segments over the SAME attribute vectors -- the buffers are shared, not copied, whatever their
 *                       width or packing -- with aux = the chunk's ranks in HBM and the NULL value id still aux_size: a well-formed
 *                       DictionarySegment<int32>.  *out owns the rank buffer.
 *     reference column  *out is a reference column over the same PosLists (shared: host-uploaded, caller-owned device lists, entire-chunk
 *                       lists) whose referenced column is such a data stand-in, owned by *out.
 *   *out is an ordinary column for hy_sort, hy_sort_limit, hy_column_export, hy_column_gather and every other reader of int32 dictionary
 *   columns: ORDER BY a string column is hy_sort over it.  Lifetime: `column` (and the column it references) must outlive *out, as a
 *   referenced column outlives a reference column; `dict` may be destroyed as soon as the call has returned (the call waits for the
 *   ranking); hy_column_destroy(*out) frees the ranks.
 *   HY_ERR_INVALID: a null argument, a column that is no string column, a dictionary that disagrees with the data column's segments or lives
 *   on another device.  HY_ERR_UNSUPPORTED: unencoded or LZ4 string segments, E >= 2^31.  On any error *out is NULL and nothing stays
 *   allocated.  Ranks are not cached inside `dict`: every call ranks again. */
hy_status hy_string_dictionary_order(const hy_string_dictionary* dict, uint32_t mem, int32_t* ranks, uint32_t* n_distinct);
hy_status hy_column_string_ranks(const hy_column* column, const hy_string_dictionary* dict, hy_column** out);

/* ---- The keys two string columns join on (what JoinHash and JoinSortMerge need of two pmr_string columns of two tables) -----------------
 * The order above is one column's.  A join needs a stand-in that is consistent across TWO columns: for an entry of either dictionary
 *     rank(entry) = the number of DISTINCT strings, over all chunks of `left` AND `right` together, that are smaller than the entry
 *     id(entry)   = ((int64_t)rank(entry) + 1) << 20 | (hash(entry) & 0xFFFFF)
 * Equal strings on either side get equal ranks and equal ids; ranks run 0 .. n_distinct - 1.  Order is std::string's, as above (a '\0'
 * inside an entry of the offsets layout is data, an entry of the fixed-length layout ends at strnlen(slot, string_length)).  hash is
 * libstdc++'s std::hash<std::string> over exactly the entry's bytes (_Hash_bytes, libsupc++/hash_bytes.cc: seed 0xc70f6907,
 * mul 0xc6a4a7935bd1e995, 8-byte little-endian words, a tail of 1-7 bytes assembled from unsigned bytes, two final shift-mixes).  The id
 * formula is a contract: the reference's JoinHash takes its radix partition (hash & mask, radix_bits <= 8) and its Bloom index
 * (hash % 2^20) from the low bits, so hy_join_hash over the ids is the reference's join over the strings -- same partitions, same probe-row
 * and build-side order -- whatever unique number stands above bit 20.  The ranks feed hy_join_sort_merge and hy_join_nested_loop, the ids
 * hy_join_hash.
 * On the device the chunks of both dictionaries, laid end to end (left's first), go through hy_string_dictionary_order's merge sequence,
 * ceil(log2(n_l + n_r)) rounds; the ids take one more launch, a lane per entry.  The joint tables are built per call: the dictionaries stay
 * as they are.  Timed under HY_KERNEL_STRING_RANK; temporaries (16 bytes per entry of both sides, 4 more under the ids) come from the
 * thread's scratch arena.
 *
 * hy_string_dictionary_order_pair / hy_string_dictionary_join_ids   left_* / right_*: one int32_t rank / int64_t id per entry of that side,
 *   in the layout of hy_string_dictionary_order (chunk c's start at the sum of that side's n_entries before c).  mem == HY_MEM_DEVICE: they
 *   stay in the caller's device buffers (ranks on 4 bytes, ids on 8, otherwise HY_ERR_INVALID), complete in the order of the calling
 *   thread's stream.  mem == HY_MEM_HOST: copied back; the call returns when they are there.  n_distinct: HOST memory, may be NULL; when it
 *   is given the call waits for the stream.  The dictionaries may have different chunk counts; a side without entries is legal; no entries
 *   on either side: HY_OK, nothing is launched, *n_distinct = 0.  Passing the same dictionary on both sides (a self join) is legal.
 *   HY_ERR_INVALID: a null argument, a bad mem, dictionaries on different devices or not on the calling thread's.  HY_ERR_UNSUPPORTED: 2^31
 *   entries or more on both sides together.  All refusals come before any launch and any allocation; nothing is written.
 *
 * hy_column_string_join_keys   hy_column_string_ranks for two columns: *left_out / *right_out are the stand-ins of `left` / `right` --
 *   dictionary columns over the SAME attribute vectors (shared, not copied, at every width and packing) whose aux holds the chunk's ranks
 *   (HY_STRING_KEYS_RANKS: HY_TYPE_INT) or ids (HY_STRING_KEYS_HASH_IDS: HY_TYPE_LONG), the NULL value id still aux_size; for a reference
 *   column a reference column over the same PosLists whose referenced column is such a stand-in.  Either side may be a data or a reference
 *   column, independently; the two columns belong to different tables (or to one).  Lifetime and ownership: hy_column_string_ranks', per
 *   side -- each stand-in owns its keys, the columns outlive their stand-ins, the dictionaries may be destroyed once the call has returned.
 *   Refusals: hy_column_string_ranks', per side (HY_ERR_INVALID: a column that is no string column, a dictionary that disagrees with the
 *   segments' aux_size; HY_ERR_UNSUPPORTED: unencoded or LZ4 string segments), those of the two calls above, and HY_ERR_INVALID for an
 *   unknown `kind`.  On any error both outputs are NULL and nothing stays allocated.  Keys are not cached between calls: they depend on
 *   the pair, and every call makes them again. */
enum { HY_STRING_KEYS_RANKS = 0 /* int32 */, HY_STRING_KEYS_HASH_IDS = 1 /* int64 */ };
hy_status hy_string_dictionary_order_pair(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem,
                                          int32_t* left_ranks, int32_t* right_ranks, uint32_t* n_distinct);
hy_status hy_string_dictionary_join_ids(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem,
                                        int64_t* left_ids, int64_t* right_ids);
hy_status hy_column_string_join_keys(const hy_column* left, const hy_string_dictionary* left_dict, const hy_column* right,
                                     const hy_string_dictionary* right_dict, uint32_t kind, hy_column** left_out, hy_column** right_out);

/* ---- String columns made on the device (what AggregateHash's string GROUP BY columns, MIN / MAX / ANY over strings, and the materialised
 * string columns of Sort / Projection need: the way from RowIDs, or from ranks, back to strings) ----------------------------------------
 * Both calls write a NEW dictionary-encoded string column in HBM: *result is a column of HY_TYPE_STRING dictionary segments whose attribute
 * vectors are FixedWidthInteger uint32_t (a NULL row holds value id n_entries of its chunk, dictionary_segment.cpp:139-141), in one pooled
 * arena owned by the column under hy_column_gather's alignment rules; *result_dict has one offsets-layout chunk per output chunk: the
 * DISTINCT strings of that chunk's non-NULL rows in std::string order (bytes as unsigned, a prefix first, a '\0' inside an entry is data;
 * entries of fixed-slot source chunks end at strnlen).  Equal strings that sit in different source chunks are ONE output entry; an output
 * chunk of NULL rows only has n_entries == 0.  The pair is what hy_table_scan (value ids), hy_table_scan_like, hy_column_string_ranks and
 * hy_table_scan_columns_strings read.  *result_dict is owned by the library (hy_string_dictionary_destroy) and depends on none of the
 * inputs after the call has returned.  The output is fully determined by the input, byte for byte.
 * On the device: the source dictionary is ranked (hy_string_dictionary_order's launches), the rows are ordered by (output chunk, rank) with
 * two stable word sorts, head flags and a prefix sum give value ids and each chunk's entries, a 64-bit scan of the entries' lengths gives the
 * offsets, and a byte-parallel copy (16 output bytes per lane) writes the chars.  The host learns per output chunk the entry count and the
 * chars' bytes, in one copy of 16 bytes per chunk: no string byte and no per-row word crosses to it.  Temporaries come from the thread's
 * scratch arena and buffer pool; the launches are timed under HY_KERNEL_STRING_RANK.
 *
 * hy_string_column_gather   the rows of `column` at `positions`.  `column`: a data column of string dictionary segments, or a reference
 *   column over one; `dict`: the dictionaries of the DATA column, checked as hy_column_string_ranks checks them; positions: n RowIDs of
 *   `column`'s table in device memory, on 8 bytes (a NULL RowID, or one outside the table -- every RowID into a table without rows --, gives a NULL row).
 *   *result has ceil(n / chunk_rows) chunks, the last one shorter.  n == 0: HY_OK, a column and a dictionary of zero chunks, no launch.
 *   HY_ERR_INVALID: a null argument, chunk_rows == 0, a column that is no string column, a dictionary that disagrees with the
 *   data column's segments or lives on another device, positions off an 8-byte boundary.  HY_ERR_UNSUPPORTED: unencoded or LZ4 string
 *   segments, E >= 2^31 dictionary entries, n >= 2^32, an output chunk whose chars would take 2^32 bytes or more (known only after the
 *   lengths are summed on the device: the call then frees everything it took).  All other refusals come before any launch and any
 *   allocation.  On every error both out pointers are NULL and nothing stays allocated.
 *
 * hy_string_ranks_gather   the strings an int32 column of dense ranks stands for: `ranks` is an HY_TYPE_INT data column of unencoded
 *   segments (what hy_aggregate_hash_columns writes for MIN / MAX over a stand-in of hy_column_string_ranks), `dict` the dictionaries the
 *   ranks were made from.  *result has `ranks`' chunk layout; row r is NULL where `ranks` is NULL or holds a value outside
 *   0 .. n_distinct - 1 (nothing outside the buffers is read for it), else a string whose dense rank in `dict` is that value.  The refusals
 *   mirror those above. */
hy_status hy_string_column_gather(const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows,
                                  hy_column** result, hy_string_dictionary** result_dict);
hy_status hy_string_ranks_gather(const hy_string_dictionary* dict, const hy_column* ranks, hy_column** result, hy_string_dictionary** result_dict);
/* hy_string_column_substr   SUBSTR(column, start, length) as a new string column: the same pair as above, in `column`'s OWN chunk layout --
 *   row r of chunk c is SUBSTR of row r of chunk c, a NULL row stays NULL -- and *result_dict holds per output chunk the distinct RESULT
 *   strings (equal substrings of different source entries or source chunks are one entry, "" is an entry like any other).  `column` and
 *   `dict` are what hy_string_column_gather takes (a data column of string dictionary segments in either layout, or a reference column over
 *   one with PosLists in either memory space); start / length are the two literal arguments as int32 (the evaluator casts Long literals to
 *   Int first, expression_evaluator.cpp:1572-1578: the caller's job).  Semantics are the reference's _evaluate_substring
 *   (expression_evaluator.cpp:1597-1638) on bytes, with n the entry's size:
 *     length <= 0: "" (not NULL).  start < 0: s = start + n.  start == 0: s = 0 and length loses 1.  start > 0: s = start - 1.
 *     e = min(s + length, n), s = max(s, 0); the result is bytes [s, e) when s < n and e > s, else "".
 *   evaluated in 64-bit arithmetic (the reference's own int32 sum overflows for arguments near INT32_MAX; every pair of int32 arguments is
 *   answered here).  SUBSTR('HELLO', 0, 2) = 'H', (-1, 2) = 'O', (-8, 1) = '', (-8, 5) = 'HE'.  A multi-byte UTF-8 sequence may be cut.
 *   On the device a substring is a window (byte begin, byte length) into the chars that are in HBM already: one launch makes a window per
 *   source entry, the windowed entries are ranked by hy_string_dictionary_order's launches, and the rest is the gather's back end reading
 *   through the windows; no intermediate string is written.  A column of zero chunks: HY_OK, a column and a dictionary of zero chunks, no
 *   launch.  The refusals mirror hy_string_column_gather's: HY_ERR_INVALID for a null argument, a column that is no string column, a
 *   dictionary that disagrees with the data column or lives on another device; HY_ERR_UNSUPPORTED for unencoded or LZ4 string segments,
 *   E >= 2^31 source entries, 2^32 rows or more, an output chunk whose chars would take 2^32 bytes or more (the only refusal behind a
 *   launch).  On every error both out pointers are NULL and nothing stays allocated. */
hy_status hy_string_column_substr(const hy_column* column, const hy_string_dictionary* dict, int32_t start, int32_t length, hy_column** result,
                                  hy_string_dictionary** result_dict);
/* hy_string_column_materialize   the rows of `column` themselves as a new string column: the same pair as above in `column`'s OWN chunk
 *   layout (one output chunk per input chunk, same sizes) -- row r of chunk c is row r of chunk c, a NULL row or NULL RowID stays NULL --,
 *   *result_dict per output chunk the distinct strings of its non-NULL rows.  It is what Projection does with a forwarded string column of a
 *   reference table once another column of the projection is computed (projection.cpp:201-215 materialises it through the evaluator, one
 *   string per row): `column` is a data column of string dictionary segments or a reference column over one with PosLists in either memory
 *   space, `dict` the DATA column's dictionaries.  On the device it is hy_string_column_substr's path without windows; where the column's
 *   rows are few against the dictionary (HY_OPT_STRING_SPARSE_GATHER) only the entries they reference are ranked.  A column of zero chunks:
 *   HY_OK, a column and a dictionary of zero chunks, no launch.  The refusals are hy_string_column_substr's: HY_ERR_INVALID for a null
 *   argument, a column that is no string column, a dictionary that disagrees with the data column or lives on another device;
 *   HY_ERR_UNSUPPORTED for unencoded or LZ4 string segments, E >= 2^31 source entries, 2^32 rows or more, an output chunk whose chars would
 *   take 2^32 bytes or more (the only refusal behind a launch).  On every error both out pointers are NULL and nothing stays allocated. */
hy_status hy_string_column_materialize(const hy_column* column, const hy_string_dictionary* dict, hy_column** result, hy_string_dictionary** result_dict);
/* An offsets-layout chunk of a dictionary read back, whether the library owns its buffers (an upload, a gather's result) or the caller:
 * chunk_size gives n_entries and the bytes of its chars (offsets[n_entries]); read_chunk copies the n_entries + 1 offsets as they are and the
 * chars' bytes [0, offsets[n_entries]) to host memory (chars may be NULL when there are none).  A fixed-slot chunk with entries:
 * HY_ERR_UNSUPPORTED from both (the caller holds those bytes).  A chunk index past the end or a null pointer: HY_ERR_INVALID. */
hy_status hy_string_dictionary_chunk_size(const hy_string_dictionary* dict, uint32_t chunk, uint32_t* n_entries, uint64_t* chars_bytes);
hy_status hy_string_dictionary_read_chunk(const hy_string_dictionary* dict, uint32_t chunk, char* chars, uint32_t* offsets);

/* ---- Validate (replaces Validate::_on_execute / _validate_chunks, validate.cpp:32-55,87-314) ----
 * The MVCC visibility filter that sits in front of every TableScan of an SQL-driven plan.  The table's MvccData
 * (storage/mvcc_data.hpp) is passed as one "column" of HY_ENC_MVCC segments, one per chunk:
 *     data  = transaction ids  (uint32_t[size])       aux   = begin commit ids (uint32_t[size])
 *     nulls = END commit ids   (uint32_t[size], cast) aux_size = the chunk's max_begin_cid
 *     ref_chunk_id = the chunk's invalid_row_count, bit 31 set while the chunk is still mutable
 *     width = 4, data_type = HY_TYPE_INT
 * or, for a reference table, as a column of HY_ENC_REFERENCE segments whose `ref` is such an MVCC column.
 * A row is visible iff  snapshot < end_cid && ((snapshot >= begin_cid) != (row_tid == our_tid))   (validate.cpp:47-55).
 * Chunks that are entirely visible (immutable, snapshot >= max_begin_cid, no invalid rows, and the transaction has no
 * in-flight Delete: can_use_chunk_shortcut, validate.cpp:57-68,116-127) are reported as HY_CHUNK_ALL_MATCH (the adapter
 * emits an EntireChunkPosList / reuses the input pos list, validate.cpp:207-211,282-284).  The result has the layout of
 * hy_table_scan: positions inside the input chunks, in position order. */
hy_status hy_validate(const hy_column* mvcc, uint32_t our_tid, uint32_t snapshot_commit_id, uint32_t can_use_chunk_shortcut,
                      hy_scan_result* result);

/* The literal handling TableScan::create_impl performs before it picks a scan implementation (table_scan.cpp:336-366 for
 * `column OP literal`, :406-448 for `column BETWEEN a AND b`): each literal is cast to the column's type without loss
 * (lossless_cast.hpp:32-187) or, where that is impossible but an equivalent predicate exists, the predicate is adjusted --
 * `float_column < 3.1` becomes `float_column <= 3.0999999f` (lossless_predicate_cast.hpp:23-64, .cpp:14-73).  Pure host
 * arithmetic, no device needed.  literal2 is NULL for the binary conditions.  On HY_OK out->condition / value_type / value /
 * value2 are what hy_table_scan takes (the other fields are zeroed); HY_ERR_UNSUPPORTED where the reference falls back to its
 * ExpressionEvaluator scan (`float_column = 3.1`, a NULL literal, a bound that does not fit the column type).  String literals
 * are outside hy_value: against a string column they need no cast, against anything else there is none. */
hy_status hy_predicate_cast(uint32_t condition, uint32_t column_type, uint32_t literal_type, const hy_value* literal, uint32_t literal2_type,
                            const hy_value* literal2, hy_predicate* out);

/* The PosLists a scan hands to the next operator, WITHOUT leaving device memory (replaces the output assembly of
 * TableScan::_on_execute, table_scan.cpp:158-196: the matches of a scan over ReferenceSegments are translated through the
 * input PosList, so the output always references the data table, never another reference table).
 * `result`: a HY_MEM_DEVICE result of hy_table_scan / hy_table_scan_columns / hy_validate over `scanned`, produced with
 * HY_SCAN_CHUNK_REGIONS | HY_SCAN_MATERIALIZE_ALL_MATCH.  Over a reference column a match (c, o) is replaced by the RowID at
 * position o of chunk c's PosList ((ref_chunk_id, o) for an entire-chunk PosList), NULL RowIDs included as they are; over a
 * data column the RowIDs are copied.  `out` is device memory with room for `capacity` RowIDs:
 *   HY_POSLIST_DENSE          ONE back-to-back PosList, the chunks' matches in chunk order.  HY_ERR_CAPACITY with *n_out = the
 *                             needed capacity if `out` is too small.
 *   HY_POSLIST_CHUNK_REGIONS  one PosList per input chunk, chunk c's at out + result->offsets[c] (result->counts[c] RowIDs): the
 *                             reference's output shape -- an output chunk per input chunk, and a PosList that referenced one
 *                             chunk still does (guarantee_single_chunk, table_scan.cpp:176-178).  capacity >= the column's rows.
 * *n_out (host): RowIDs written in total -- the one value that crosses to the host (8 bytes; the call waits for the stream). */
enum { HY_POSLIST_DENSE = 0, HY_POSLIST_CHUNK_REGIONS = 1 };
hy_status hy_poslist_translate(const hy_column* scanned, const hy_scan_result* result, uint32_t layout, hy_row_id* out, uint64_t capacity, uint64_t* n_out);

/* The RowIDs a join hands on when an input was a reference table (write_output_segments, join_output_writing.cpp:95-200: the positions a
 * join finds in a reference table are dereferenced through the input's PosLists, so the output references the data table), WITHOUT leaving
 * device memory: out[i] = the RowID at position positions[i] = (chunk c, offset o) of `reference` -- a column of HY_ENC_REFERENCE segments
 * (any column of the input table that shares the PosLists in question) -- i.e. pos_list(c)[o], (ref_chunk_id, o) for an entire-chunk
 * PosList; a NULL position (outer joins) stays NULL_ROW_ID.  positions / out: device memory, n RowIDs each; queued on the calling thread's
 * stream. */
hy_status hy_poslist_gather(const hy_column* reference, const hy_row_id* positions, uint64_t n, hy_row_id* out);

/* ---- Sort (replaces the sorting of Sort::_on_execute, sort.cpp:287-379, and SortImpl::sort, :400-516) ------------------------------------
 * ONE stable lexicographic sort of a table's rows by keys[0], then keys[1], ...: sort.cpp applies the definitions from the last to the first,
 * each a stable sort (std::stable_sort, :486-505) of the order the later ones left, so ties keep input order -- chunk order, then position in
 * the chunk (for a reference table: the position in the chunk's PosList).  NULLs come first in both directions and keep their order among
 * themselves (:435-443); descending is std::greater with stable ties; float / double compare with std::less (-0.0 and 0.0 tie; NaN is not
 * supported).  A key column is a data or reference column of any numeric type and encoding; a string column is passed as a column of
 * order-preserving integer ranks (hy_column_string_ranks makes it in HBM; hyrise_amd/string_keys.py StringRanks on the host).  All key columns are columns of one table: the same chunk layout.
 * mode: HY_SORT_ASCENDING_NULLS_FIRST or HY_SORT_DESCENDING_NULLS_FIRST; the NULLS LAST modes are HY_ERR_INVALID (Sort asserts, :294-296).
 * out: DEVICE memory with room for `capacity` RowIDs; receives the INPUT TABLE's positions (chunk, offset) in sorted order -- the adapter
 * dereferences them through a reference input's PosLists with hy_poslist_gather once per column cluster (write_reference_output_table,
 * :161-252).  *n_out: the table's rows (HY_ERR_CAPACITY if they do not fit).  Tables of 2^32 rows or more: HY_ERR_UNSUPPORTED (32-bit row
 * ids).  Returns when `out` is complete. */
typedef struct hy_sort_key {
  const hy_column* column;
  uint32_t mode;       /* HY_SORT_* */
  uint32_t reserved;
} hy_sort_key;
hy_status hy_sort(const hy_sort_key* keys, uint32_t n_keys, hy_row_id* out, uint64_t capacity, uint64_t* n_out);

/* ---- Sort under a Limit (replaces Sort::_on_execute / SortImpl::sort, sort.cpp:287-516, followed by Limit::_on_execute, limit.cpp:47-127) ------
 * The first n = min(limit, rows) RowIDs of hy_sort's output, byte for byte, without sorting the rows that cannot be among them.  The sorted
 * order is lexicographic in keys[0] (NULLs first), keys[1], ..., and last the input row number (the stable sorts' ties), so its first n rows
 * are unique.  keys / modes / refusals: exactly hy_sort's (NULLS LAST and columns of different tables HY_ERR_INVALID, string and MVCC columns,
 * 2^32 rows or more HY_ERR_UNSUPPORTED).
 * out: DEVICE memory for `capacity` RowIDs; capacity >= n suffices, and nothing is written behind out[n).  *n_out = n; a smaller capacity is
 * HY_ERR_CAPACITY with *n_out set and nothing written.  limit == 0 or a table without rows: HY_OK, *n_out = 0, out may be NULL.
 * *path (may be NULL): 0 = every row was sorted and the result cut (hy_sort into a temporary), 1 = the selection ran first: a histogram over
 * the most significant digits of keys[0]'s order-preserving key finds the bucket that holds the n-th row (refined digit by digit while the
 * bucket is a large share of the table), the NULL rows, the rows below the bucket and the bucket's rows are compacted in ascending row order,
 * and hy_sort's chain of word sorts runs over those candidates only.
 * flags: 0 = the library chooses (limit >= rows: always path 0; a candidate set that is a large share of the table -- heavy ties on keys[0] --
 * falls back to path 0), HY_SORT_LIMIT_FORCE_FULL_SORT / HY_SORT_LIMIT_FORCE_SELECT (tests, A/B timing; FORCE_SELECT is correct at any size).
 * Both force flags, or any other bit: HY_ERR_INVALID.  Returns when `out` is complete. */
enum { HY_SORT_LIMIT_FORCE_FULL_SORT = 1, HY_SORT_LIMIT_FORCE_SELECT = 2 };
hy_status hy_sort_limit(const hy_sort_key* keys, uint32_t n_keys, uint64_t limit, uint32_t flags, hy_row_id* out, uint64_t capacity, uint64_t* n_out, uint32_t* path);

/* The rows of `column` at `positions` (device memory, n RowIDs of the column's table; a NULL RowID gives a NULL row) as a new device-resident
 * column of unencoded segments of chunk_rows rows (the last one shorter), each with a null vector, like hy_projection_arithmetic's result:
 * the numeric columns of Sort's materialised output (write_materialized_output_table, sort.cpp:58-150, when ForceMaterialization::Yes or a
 * column references more than one table, :339-379).  Reads any encoding, reference columns included.  hy_column_read_chunk copies a chunk
 * back; destroy it with hy_column_destroy. */
hy_status hy_column_gather(const hy_column* column, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows, hy_column** result);

/* ---- UnionPositions (replaces UnionPositions::_on_execute, union_positions.cpp:71-233) ------------------------------------------------------
 * The set union of two reference tables over the same data: what PredicateSplitUpRule (predicate_split_up_rule.cpp:174-195) makes of
 * `WHERE p OR q`.  Columns that share a PosList form a column cluster (:257-279); per input, the clusters' PosLists concatenated over all
 * chunks are the columns of a reference matrix, one row of n_clusters RowIDs per table row (:349-372).  Rows are ordered lexicographically
 * over the clusters, a RowID by (chunk_id, chunk_offset) as unsigned numbers -- NULL_ROW_ID is an ordinary, largest value.  Both matrices
 * are sorted and merged with std::set_union (:205-230): the output is ascending, and a row that the left input holds m times and the right
 * one n times appears max(m, n) times.  Equal rows are indistinguishable, so the output is fully determined.
 * left[c] / right[c]: one column of HY_ENC_REFERENCE segments per cluster (any column of the input that carries the cluster's PosLists, as
 * hy_poslist_gather's `reference`; host lists, device lists and NULL = entire-chunk lists); all clusters of a side have one chunk layout.  A
 * column without chunks is an input without rows.
 * out[c]: DEVICE memory for `capacity` RowIDs per cluster; capacity >= rows(left) + rows(right) always suffices.  *n_out: the output rows;
 * if they exceed `capacity` the call returns HY_ERR_CAPACITY with *n_out set (the lists then hold the first `capacity` rows).
 * *path (may be NULL): bit 0 = the left side was sorted by the library, bit 1 = the right side was.  A side that arrives in order (every row
 * >= its predecessor: a TableScan's output over a data table) is merged as it is; one pass over the side decides it.
 * flags: 0 or HY_UNION_FORCE_SORT (sort both sides whatever order they arrive in: tests, A/B timing).
 * n_clusters: 1 .. 8 (more: HY_ERR_UNSUPPORTED; 0: HY_ERR_INVALID).  rows(left) + rows(right) >= 2^32: HY_ERR_UNSUPPORTED (32-bit row ids).
 * Null arguments, a data column, clusters of different row counts: HY_ERR_INVALID.  The early results of the operator (an input without rows
 * returns the other input TABLE, :237-253) are the adapter's: this call then returns the other side's rows in ascending order.
 * Returns when `out` is complete, like hy_sort. */
enum { HY_UNION_FORCE_SORT = 1 };
hy_status hy_union_positions(const hy_column* const* left, const hy_column* const* right, uint32_t n_clusters, uint32_t flags, hy_row_id* const* out, uint64_t capacity,
                             uint64_t* n_out, uint32_t* path);

/* ---- Projection arithmetic (the ArithmeticExpressions a Projection evaluates through the
 * ExpressionEvaluator, operators/projection.cpp + expression/evaluation/expression_functors.hpp:127-213) -------------------
 * result = left <op> right, element-wise over a table's rows; an operand is a column of the table (data or reference
 * segments, any supported encoding) or a literal.  Same numeric order as hyrise::ArithmeticOperator
 * (expression/arithmetic_expression.hpp).  Semantics of the reference:
 *   result type  expression_common_type (expression_utils.cpp:172-204): Double if either is Double; Long with Float -> Double;
 *                Long with Int -> Long; Float if either is Float; else Int
 *   + - *        computed in std::common_type_t of the operand types, then cast to the result type; NULL if an operand is NULL
 *   /            NULL if an operand is NULL or the divisor is 0; computed in the result type (integers truncate)
 *   %            NULL as for /; `%` for two integral operands, std::fmod otherwise
 * The result is a new device-resident column of unencoded value segments (result type, chunked like the column operand(s),
 * with a null vector) that the following operator -- typically hy_aggregate_hash: Q1/Q6 never materialise the expression
 * on the host -- takes like any other column; hy_column_read_chunk copies a chunk back.  Destroy it with hy_column_destroy. */
enum { HY_ARITH_ADD = 0, HY_ARITH_SUB = 1, HY_ARITH_MUL = 2, HY_ARITH_DIV = 3, HY_ARITH_MOD = 4 };
typedef struct hy_operand {
  const hy_column* column;   /* NULL: the operand is `literal` */
  uint32_t literal_type;     /* HY_TYPE_INT / LONG / FLOAT / DOUBLE, or HY_TYPE_NULL for a NULL literal */
  hy_value literal;
} hy_operand;
hy_status hy_projection_arithmetic(uint32_t op, const hy_operand* left, const hy_operand* right, hy_column** result);
/* Copies one chunk of an unencoded device-resident column to host memory: values[rows] of the column's type and, if
 * null_words is not NULL, the null bitmap (bit i of word i/64; rows/64 rounded up words).  A chunk of a dictionary-encoded STRING column
 * gives its attribute vector instead: rows value ids of 1, 2 or 4 bytes (hy_string_column_gather's results: 4), NULL rows as the NULL
 * value id and the bitmap zero. */
hy_status hy_column_read_chunk(const hy_column* column, uint32_t chunk, void* values, uint64_t* null_words);
uint32_t hy_column_data_type(const hy_column* column);
uint32_t hy_column_chunk_rows(const hy_column* column, uint32_t chunk);

/* ---- Projection: one whole expression tree per output column, in one pass (operators/projection.cpp; the cell rules of
 * expression/evaluation/expression_evaluator.cpp and expression/evaluation/expression_functors.hpp) ----------------------------
 * A postfix program over the rows of one table: every node pops its operands from a stack of at most HY_MAX_PROJECTION_DEPTH
 * values and pushes one; exactly one value is left at the end -- the output cell.  One kernel launch evaluates the program for
 * all chunks and writes ONE result column; no intermediate column exists.  Node kinds, with the reference's semantics:
 *   COLUMN        columns[index]: a numeric column of the table -- data or reference segments of every supported encoding, host or
 *                 device PosLists, a NULL RowID is a NULL cell, caller-owned device columns (what hy_projection_arithmetic reads).
 *                 All columns of a program, tested ones included, share one chunk layout (HY_ERR_INVALID otherwise).
 *   LITERAL       literal_type / literal: Int, Long, Float, Double or HY_TYPE_NULL.
 *   ARITHMETIC    op = HY_ARITH_*: left op right, hy_projection_arithmetic's rules cell by cell (expression_functors.hpp:127-213).
 *   COMPARISON    op = HY_PRED_EQUALS .. HY_PRED_GREATER_THAN_EQUALS between two numeric operands.  The result is Int (the evaluator's
 *                 Bool = int32_t) 0 or 1, computed in std::common_type_t of the operand types (expression_functors.hpp:90-116: Int against
 *                 Float compares as float, Long against Float as float); > and >= are the swapped < and <= (expression_evaluator.cpp:73-90);
 *                 NULL if either side is NULL.
 *   COLUMN_TEST   tests[index]: a column and a predicate as hy_table_scan takes them (literal already cast, per-chunk value ids or match
 *                 bitmaps for dictionary string columns), or an IN list over a dictionary string column as hy_table_scan_in_list takes it.
 *                 Evaluated through the scan's normalised per-chunk jobs.  The result is Int 0 or 1 and NULL WHERE THE CELL IS NULL (the
 *                 evaluator's rule; a scan drops what is not TRUE); HY_PRED_IS_NULL / IS_NOT_NULL never yield NULL.
 *   IS_NULL / IS_NOT_NULL   of the top of the stack: Int 0 or 1, never NULL (expression_evaluator.cpp:382-402).
 *   AND / OR      ternary logic of TernaryAndEvaluator / TernaryOrEvaluator (expression_functors.hpp:41-84); operands are Int, non-zero is true.
 *   UNARY_MINUS   the operand's type; NULL stays NULL (expression_evaluator.cpp:965-988).
 *   CASE          pops otherwise, then, when (pushed in the order when, then, otherwise).  Result type expression_common_type(then,
 *                 otherwise), a NULL literal taking the other branch's type; a `when` that is NULL or 0 selects `otherwise`; the chosen
 *                 branch's value is static_cast to the result type, the NULL flag is the chosen branch's (expression_evaluator.cpp:726-759).
 *                 A chained CASE is a CASE in the `otherwise` position.
 * Floating point: every operation is a single IEEE operation in the stated type, nothing is reassociated or contracted.  NaN inputs
 * are outside the contract of COMPARISON (the swapped forms differ from the direct ones only there).
 * HY_ERR_UNSUPPORTED (message in hy_last_error): string columns outside COLUMN_TEST; the kinds HY_PROJ_BETWEEN .. HY_PROJ_PARAMETER and
 * Between conditions in a COLUMN_TEST (_evaluate_between_expression, expression_evaluator.cpp:590-656, yields FALSE, not NULL, for a
 * NULL operand on its fast path and two comparisons otherwise: left out, not approximated); IN lists over other than dictionary string
 * columns; unencoded string segments; MVCC columns; more than HY_MAX_PROJECTION_NODES nodes, HY_MAX_PROJECTION_DEPTH stack entries,
 * HY_MAX_PROJECTION_COLUMNS distinct columns or HY_MAX_PROJECTION_TESTS tests.
 * HY_ERR_INVALID: null arguments; a malformed program (stack underflow, not exactly one value left, an index out of range, operands of a
 * type the node does not take, a type that cannot be deduced); a program without any column (the evaluator's one-row result is the
 * adapter's business, as for hy_projection_arithmetic).
 * The result is a device-resident column in hy_projection_arithmetic's layout: unencoded value segments of the result type, chunked like
 * the input columns, every chunk with a null vector (tail bits zero; NULL cells hold T{}).  On error *result is NULL. */
#define HY_MAX_PROJECTION_NODES 32
#define HY_MAX_PROJECTION_DEPTH 6
#define HY_MAX_PROJECTION_COLUMNS 8
#define HY_MAX_PROJECTION_TESTS 4
enum { HY_PROJ_COLUMN = 0, HY_PROJ_LITERAL = 1, HY_PROJ_ARITHMETIC = 2, HY_PROJ_COMPARISON = 3, HY_PROJ_COLUMN_TEST = 4, HY_PROJ_IS_NULL = 5,
       HY_PROJ_IS_NOT_NULL = 6, HY_PROJ_AND = 7, HY_PROJ_OR = 8, HY_PROJ_UNARY_MINUS = 9, HY_PROJ_CASE = 10,
       /* named so that a translated plan can hand them over and be told: HY_ERR_UNSUPPORTED */
       HY_PROJ_BETWEEN = 11, HY_PROJ_CAST = 12, HY_PROJ_EXTRACT = 13, HY_PROJ_FUNCTION = 14, HY_PROJ_SUBQUERY = 15, HY_PROJ_PARAMETER = 16 };
typedef struct hy_projection_node {
  uint32_t kind;           /* HY_PROJ_* */
  uint32_t op;             /* ARITHMETIC: HY_ARITH_*; COMPARISON: HY_PRED_* */
  uint32_t index;          /* COLUMN: into columns[]; COLUMN_TEST: into tests[] */
  uint32_t literal_type;   /* LITERAL */
  hy_value literal;
} hy_projection_node;
typedef struct hy_projection_test {
  const hy_column* column;
  hy_predicate predicate;      /* read when in_list is NULL */
  const hy_in_list* in_list;   /* or: column [NOT] IN (...) over a dictionary string column (per_chunk_value_ids) */
} hy_projection_test;
typedef struct hy_projection_program {
  uint32_t n_nodes, n_columns, n_tests, reserved;
  const hy_column* columns[HY_MAX_PROJECTION_COLUMNS];
  hy_projection_test tests[HY_MAX_PROJECTION_TESTS];
  hy_projection_node nodes[HY_MAX_PROJECTION_NODES];
} hy_projection_program;
hy_status hy_projection_expression(const hy_projection_program* program, hy_column** result);

/* ---- TableScan over a predicate expression: the scan TableScan::create_impl falls back to (table_scan.cpp:312-452) when the predicate is
 * none of ColumnVsValue / ColumnBetween / ColumnVsColumn / ColumnIsNull / ColumnLike -- ExpressionEvaluatorTableScanImpl
 * (expression_evaluator_table_scan_impl.cpp:21-24), i.e. ExpressionEvaluator::evaluate_expression_to_pos_list
 * (expression_evaluator.cpp:1129-1311) -- in ONE launch: the program is evaluated per row, the matching rows are compacted into PosLists;
 * no intermediate column exists.  `l_extendedprice * (1 - l_discount) > 1000`, `a < b + 1`, `x = 1 OR y IS NULL`, `CASE ... END = 1`,
 * `int_column = 3.1` (what hy_predicate_cast answers with HY_ERR_UNSUPPORTED), a conjunction as one pass instead of k chained scans.
 *   program    a hy_projection_program exactly as hy_projection_expression takes it: the same node kinds, limits, type deduction and
 *              inputs (data and reference columns of every encoding, host or device PosLists, a NULL RowID is a NULL cell, caller-owned
 *              device columns); all columns share one chunk layout.
 *   match rule a row matches iff the program's value is not NULL and not 0.  That is evaluate_expression_to_pos_list's list: its AND / OR
 *              (set_intersection / set_union of the operands' lists, :1249-1265) keep exactly the rows where TernaryAnd / TernaryOr
 *              (expression_functors.hpp:41-84) are TRUE, given that every other node's list is "value TRUE" -- and its comparison, IS
 *              [NOT] NULL, IN and LIKE leaves append the rows whose value is neither NULL nor 0 (:1144-1247; Between goes through
 *              rewrite_between_expression, :1200).
 *   root       a COMPARISON, COLUMN_TEST, IS_NULL, IS_NOT_NULL, AND or OR node; anything else (arithmetic, CASE, a column, a literal,
 *              unary minus) is HY_ERR_INVALID -- the reference Fails with "Expression type cannot be evaluated to PosList" (:1307).  A program
 *              without any column is HY_ERR_INVALID as well (a TRUE / FALSE literal predicate is the adapter's business).
 *   BETWEEN    on the SPINE -- the root and every node all of whose ancestors are AND / OR -- a COLUMN_TEST may carry a Between condition
 *              (HY_PRED_BETWEEN_*, numeric, or over a dictionary string column with per_chunk_lower / per_chunk_upper): FALSE and NULL
 *              both drop the row there, so _evaluate_between_expression's fast path and its rewrite cannot be told apart.  Below the
 *              spine it stays HY_ERR_UNSUPPORTED, as do the node kinds HY_PROJ_BETWEEN .. HY_PROJ_PARAMETER.
 *   result     hy_table_scan's contract, bit for bit: positions relative to the input chunk, ascending (no re-ordering by referenced
 *              chunk: the evaluator's scan has none); HY_MEM_HOST and HY_MEM_DEVICE results; HY_SCAN_CHUNK_REGIONS as there; the
 *              alignment rules of a device result (`matches` on 16, `offsets` on 8, `counts` on 4 bytes: HY_ERR_INVALID before any launch
 *              -- the kernel itself stores RowID by RowID, 8 bytes); excluded_chunks for data columns; hy_poslist_translate reads the
 *              result with any column of the program as `scanned`.  chunk_state is HY_CHUNK_NONE_MATCH for excluded chunks and
 *              HY_CHUNK_SCANNED otherwise, NEVER HY_CHUNK_ALL_MATCH: every match is written, HY_SCAN_MATERIALIZE_ALL_MATCH changes nothing.
 * On any error nothing is written -- with hy_table_scan's one exception: a HY_MEM_HOST result whose `matches` is too small for the scan's
 * RowIDs (HY_ERR_CAPACITY) has its counts, chunk_state, offsets and total_matches filled in (total_matches is the capacity needed), no RowID. */
hy_status hy_table_scan_expression(const hy_projection_program* program, const uint32_t* excluded_chunks, uint32_t n_excluded,
                                   hy_scan_result* result);

/* ---- JoinHash (replaces JoinHash::_on_execute, join_hash.cpp:116-225,270-572) ----------------------------------- */
typedef struct hy_join_result {
  uint32_t mem;
  uint32_t radix_bits;            /* in: 0xFFFFFFFF = derive like JoinHash::calculate_radix_bits; out: value used      */
  hy_row_id* left_pos;            /* [capacity] RowIDs into the LEFT input                                             */
  hy_row_id* right_pos;           /* [capacity] RowIDs into the RIGHT input (Semi/Anti*: unused, may be NULL -- the     *
                                   *  probe side of those modes is the LEFT input and only left_pos is written)       */
  uint64_t capacity;
  uint64_t* slice_offsets;        /* [slice_capacity + 1] boundaries of the per-probe-slice PosLists                   */
  uint32_t slice_capacity;
  uint32_t n_slices;              /* out */
  uint64_t n_pairs;               /* out */
  uint32_t left_is_build;         /* out: JoinHash::PerformanceData::left_input_is_build_side                          */
  uint32_t flags;                 /* in: HY_JOIN_ASYNC or 0                                                            */
  struct hy_join_status* status;  /* in: HY_JOIN_ASYNC: device memory the join's last planning kernel writes; else unused */
} hy_join_result;

/* HY_JOIN_ASYNC (mem == HY_MEM_DEVICE only): the call returns as soon as the join's kernels are queued on the calling thread's
 * stream -- no host round trip, so a chain (the next scan, the next join) is queued while this one runs.  What the host normally
 * learns -- the pair count, the number of output PosLists, whether they fit the capacities (a join that does not fit writes
 * nothing), whether the build column still is what its key hint said (hy_join_hash below; if not, nothing is written either) --
 * goes to `status` in DEVICE memory, where a following kernel can read it; n_pairs / n_slices of the result are NOT valid until
 * hy_join_hash_finish has run.  Shapes whose build side needs a host decision (the first join over a column, duplicate or unsorted
 * build keys) run synchronously as always and fill `status` at the end: the flag is a permission, not a promise. */
#define HY_JOIN_ASYNC 1u
typedef struct hy_join_status {
  uint64_t n_pairs;
  uint32_t n_slices;
  uint32_t fits;                  /* 1: n_pairs <= capacity and n_slices <= slice_capacity, the PosLists are written        */
  uint32_t build_confirmed;       /* 0: the build column contradicted its key hint -- hy_join_hash_finish runs the join again */
  uint32_t error;                 /* a probe row with more than 4 194 303 partners (HY_ERR_UNSUPPORTED)                      */
  uint64_t reserved;
} hy_join_status;

/* Equi-join of two numeric columns (int32 / int64 / float / double, any two: both sides are cast to JoinHashTraits'
 * HashedType first, join_hash_traits.hpp:15-40 -- the larger integer type, the larger floating type, or THE floating
 * type of an integer x floating join -- and compared there; NaN keys find nothing).  String columns: HY_ERR_UNSUPPORTED
 * here -- the adapter joins them as DictionarySegment<int64> views whose dictionaries hold one id per distinct string,
 * unique << 20 | std::hash(string) & 0xFFFFF, which this join partitions and filters exactly like the strings
 * (INTEGRATION.md section 3).
 * Pair order == the CPU operator's concatenated probe() output (join_hash_steps.hpp:624-792): by radix partition
 * (std::hash<HashedType> of the key -- the identity for integers, libstdc++'s for float / double), then probe row, then
 * build-side insertion order.
 * A result that does not fit `capacity` / `slice_capacity` is HY_ERR_CAPACITY: nothing is written to the PosList or
 * slice_offsets buffers (device-memory results included -- the check happens on the device between the two probe passes),
 * n_pairs and n_slices report what the join needs.  With mem = HY_MEM_DEVICE the PosLists stay in HBM for the next
 * operator and the call makes no host round trip between the passes. */
hy_status hy_join_hash(const hy_column* left, const hy_column* right, uint32_t mode, hy_join_result* result);
/* Completes a HY_JOIN_ASYNC join (same arguments): waits for the calling thread's stream, reads result->status, fills n_pairs /
 * n_slices and returns what the synchronous call would have returned (HY_ERR_CAPACITY with the needed sizes; a build column that
 * contradicted its hint: the hint is dropped and the join runs again, synchronously, before this call returns).  A no-op for a
 * result without the flag. */
hy_status hy_join_hash_finish(const hy_column* left, const hy_column* right, uint32_t mode, hy_join_result* result);

/* A secondary join predicate  left_column <condition> right_column  (OperatorJoinPredicate, operator_join_predicate.hpp;
 * evaluated like MultiPredicateJoinEvaluator::satisfies_all_predicates, multi_predicate_join_evaluator.hpp:44-54, on every
 * pair the primary equality finds: join_hash_steps.hpp:727-747, 869-876).  The columns are columns of the join's LEFT and
 * RIGHT input table (same chunk layout as the respective key column), numeric, of any two types: the values are compared
 * in their common C++ type like the reference's comparator functors; a NULL on either side fails the predicate. */
typedef struct hy_join_predicate {
  const hy_column* left_column;
  const hy_column* right_column;
  uint32_t condition;             /* HY_PRED_EQUALS .. HY_PRED_GREATER_THAN_EQUALS */
  uint32_t reserved;
} hy_join_predicate;
#define HY_MAX_SECONDARY_PREDICATES 4
/* hy_join_hash with secondary predicates (n_secondary = 0: the same join).  HY_JOIN_ANTI_NULL_AS_TRUE with secondary
 * predicates is HY_ERR_UNSUPPORTED, as in JoinHash::supports (join_hash.cpp:39-44). */
hy_status hy_join_hash_predicates(const hy_column* left, const hy_column* right, uint32_t mode, const hy_join_predicate* secondary,
                                  uint32_t n_secondary, hy_join_result* result);
hy_status hy_join_hash_radix_bits(uint64_t build_rows, uint64_t probe_rows, uint32_t* radix_bits);
/* Upper bound for result->capacity without running the join (Semi/Anti: probe rows; others: exact pair count). */
hy_status hy_join_hash_count(const hy_column* left, const hy_column* right, uint32_t mode, uint64_t* n_pairs);

/* ---- JoinSortMerge (replaces JoinSortMerge::_on_execute, join_sort_merge.cpp: the join the translator takes where JoinHash does not
 * apply, lqp_translator.cpp:389-410 -- a non-equi primary predicate, or FULL OUTER) -------------------------------------------------------
 * left <condition> right over two columns of the SAME numeric type (int, long, float, double), any encoding hy_sort reads, reference
 * columns over host or device PosLists included.
 *   mode       HY_JOIN_INNER, LEFT, RIGHT or FULL_OUTER
 *   condition  HY_PRED_EQUALS, LESS_THAN, LESS_THAN_EQUALS, GREATER_THAN, GREATER_THAN_EQUALS; HY_PRED_NOT_EQUALS with HY_JOIN_INNER only
 * A column without chunks (an input table without rows) carries no type and joins with any column.
 * Everything else is HY_ERR_UNSUPPORTED and stays on the stock operator: Semi / Anti / Cross, <> with an outer mode, columns of different
 * types, strings, 2^32 rows or more on one side.  Secondary predicates are not part of this call.
 * A NULL key matches nothing.  Under LEFT / FULL_OUTER every left row without a partner (NULL keys included) appears once with right_pos =
 * NULL_ROW_ID ({~0u, ~0u}, as hy_join_hash's outer modes write it); RIGHT / FULL_OUTER does the same for right rows.  float / double
 * compare through hy_sort's order-preserving key, so -0.0 = +0.0.  NaN keys are outside the contract (the reference sorts them with
 * std::sort, which is undefined behaviour).
 * Order of the output -- the library's own contract; the reference's order depends on a cluster count derived from the row counts and on
 * parallel jobs, and its tests compare unordered, so parity with the reference is on the multiset of pairs.  "Position" is the row number in
 * the input column (chunk order, then offset); the written RowID is {chunk, offset} of the input table, as for hy_join_hash:
 *   1. the n_matched pairs first: left rows in ascending key order, ties by left position;
 *   2. under each left row its partners in ascending right key order, ties by right position;
 *   3. for <>, the partners below the key first, then the partners above it;
 *   4. then the n_left_outer unmatched left rows, by left position;
 *   5. then the unmatched right rows, by right position.
 * The result is a pure function of the inputs.  A result that does not fit `capacity` is HY_ERR_CAPACITY: nothing is written to left_pos /
 * right_pos, and n_pairs, n_matched and n_left_outer report what is needed (the check happens after the counting passes and before any
 * emitting kernel; hy_join_sort_merge_count runs exactly those passes).  mem = HY_MEM_DEVICE: the lists are device memory and stay in HBM
 * for the next operator.  Returns when the lists are complete. */
typedef struct hy_sort_merge_result {
  uint32_t mem;            /* HY_MEM_HOST | HY_MEM_DEVICE */
  uint32_t reserved;
  hy_row_id* left_pos;     /* [capacity] RowIDs into the LEFT input, NULL_ROW_ID for an unmatched right row  */
  hy_row_id* right_pos;    /* [capacity] RowIDs into the RIGHT input, NULL_ROW_ID for an unmatched left row  */
  uint64_t capacity;
  uint64_t n_pairs;        /* out: all rows written (or needed, with HY_ERR_CAPACITY) */
  uint64_t n_matched;      /* out: the leading pairs that satisfy the predicate; the outer rows follow */
  uint64_t n_left_outer;   /* out: unmatched left rows (after n_matched); the unmatched right rows follow them */
} hy_sort_merge_result;
hy_status hy_join_sort_merge(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, hy_sort_merge_result* result);
hy_status hy_join_sort_merge_count(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, uint64_t* n_pairs);

/* ---- JoinNestedLoop (replaces JoinNestedLoop::_on_execute, join_nested_loop.cpp: the third join the translator tries,
 * lqp_translator.cpp:389-410, whose supports() is `return true` -- every shape JoinHash and JoinSortMerge refuse) ---------------------------
 * left <condition> right AND every secondary predicate, all pairs compared on the device.
 *   mode       HY_JOIN_INNER, LEFT, RIGHT, FULL_OUTER, SEMI, ANTI_NULL_AS_FALSE, ANTI_NULL_AS_TRUE (HY_JOIN_CROSS is Product: HY_ERR_UNSUPPORTED)
 *   condition  HY_PRED_EQUALS .. HY_PRED_GREATER_THAN_EQUALS, under every mode
 *   keys       numeric columns of any two types, any encoding hy_column_export reads, reference columns over host or device PosLists; the
 *              values are compared in their common C++ type (hy_join_predicate's rule).  NaN keys are outside the contract.
 *   secondary  up to HY_MAX_SECONDARY_PREDICATES hy_join_predicate's, under every mode; their columns have the chunk layout of the join's
 *              input tables (otherwise HY_ERR_INVALID)
 * NULL rule (join_nested_loop.cpp:67-79, multi_predicate_join_evaluator.hpp:44-54): a NULL on either side of the primary or of a secondary
 * predicate fails that predicate -- under HY_JOIN_ANTI_NULL_AS_TRUE it satisfies it instead.
 * HY_ERR_UNSUPPORTED: string columns, MVCC columns, dictionaries without values, 2^32 rows or more on a side, rows(left) x rows(right) above
 * HY_NLJ_MAX_COMPARISONS (a kernel on a shared device must not run for many seconds), temporaries above HY_NLJ_MAX_TEMPORARY_BYTES -- all
 * decided before any kernel runs.
 * Order of the output == the reference's (join_nested_loop.cpp:141-236, a single-threaded walk): parity is byte for byte.  Let O be the left
 * input and I the right one; under HY_JOIN_RIGHT they are swapped, the primary condition and every secondary predicate flipped (:130-139).
 *   1. for every chunk co of O, for every chunk ci of I, for every row i of co, for every row j of ci in offset order: the pair (i, j) if it
 *      satisfies all predicates;
 *   2. LEFT / RIGHT / FULL_OUTER: behind all pairs of co the rows of co that matched nothing, in offset order, NULL_ROW_ID on the other side;
 *   3. FULL_OUTER: at the very end the rows of I that matched nothing, in position order, NULL_ROW_ID on the other side;
 *   4. SEMI / ANTI_*: no pairs; the left rows that matched (SEMI) or did not (ANTI_*) in position order, in left_pos only.
 * left_pos always holds RowIDs of the LEFT input (also under HY_JOIN_RIGHT), right_pos of the RIGHT input; a RowID is {chunk, offset} of the
 * input column, as for hy_join_hash.
 * A result that does not fit `capacity` is HY_ERR_CAPACITY: nothing is written and n_pairs reports what is needed (decided after the counting
 * passes, before any emitting kernel; hy_join_nested_loop_count runs exactly those passes).  The lists lie on 8-byte boundaries (otherwise
 * HY_ERR_INVALID, nothing written).  mem = HY_MEM_DEVICE: the lists stay in HBM for the next operator.  Returns when the lists are complete. */
#define HY_NLJ_MAX_COMPARISONS 250000000000ull   /* rows(left) x rows(right) of one call: under 2 s at the measured 1.35 * 10^11 comparisons per second */
#define HY_NLJ_MAX_TEMPORARY_BYTES (1ull << 31)   /* the call's exported operands, counters and offsets in device memory */
typedef struct hy_nested_loop_result {
  uint32_t mem;            /* HY_MEM_HOST | HY_MEM_DEVICE */
  uint32_t reserved;
  hy_row_id* left_pos;     /* [capacity] */
  hy_row_id* right_pos;    /* [capacity]; Semi / Anti*: unused, may be NULL */
  uint64_t capacity;
  uint64_t n_pairs;        /* out: rows written, or needed with HY_ERR_CAPACITY */
} hy_nested_loop_result;
hy_status hy_join_nested_loop(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, const hy_join_predicate* secondary,
                              uint32_t n_secondary, hy_nested_loop_result* result);
hy_status hy_join_nested_loop_count(const hy_column* left, const hy_column* right, uint32_t mode, uint32_t condition, const hy_join_predicate* secondary,
                                    uint32_t n_secondary, uint64_t* n_pairs);

/* ---- Product (replaces Product::_on_execute / _add_product_of_two_chunks, product.cpp:32-137: what the translator emits for every cross
 * join, lqp_translator.cpp:362 -- the one JoinMode the join operators route elsewhere) ---------------------------------------------------------
 * Both PosLists of left x right, written on the device in ONE launch.  `left` / `right`: any column of each input table -- only its chunk
 * layout and, for a column of HY_ENC_REFERENCE segments, its PosLists are read (host lists, device lists and NULL = entire-chunk lists, as
 * hy_poslist_gather's `reference`); type, encoding and values do not matter, string columns included.
 * Order of the output == the reference's, byte for byte:
 *   1. the chunk pairs run (cl, cr) with cl outermost (product.cpp:51-61); pair (cl, cr) owns the rows
 *      [pair_offsets[cl * n_right_chunks + cr], pair_offsets[cl * n_right_chunks + cr + 1]) of both lists -- one output chunk of the
 *      reference (:136) --, pair_offsets being the exclusive prefix sum of rows(cl) * rows(cr); a pair with an empty side owns nothing;
 *   2. row p of a pair pairs left offset p / rows(cr) with right offset p % rows(cr) (:119-122);
 *   3. a data column's RowID is {chunk, offset}; a reference column's is its PosList's entry at that offset ({ref_chunk_id, offset} for an
 *      entire-chunk list), NULL_ROW_ID entries -- an outer join's output -- included as they are (:123-127).
 * left_pos / right_pos: either may be NULL -- that side is not wanted (an input table whose columns sit behind k PosLists needs k lists for
 * its side, product.cpp:109-113: one more call per further list with only that side wanted); both NULL: HY_ERR_INVALID.  pair_offsets (host
 * memory, may be NULL) is written on HY_OK only.  mem = HY_MEM_DEVICE: the lists stay in HBM for the next operator; they lie on 8-byte
 * boundaries (otherwise HY_ERR_INVALID): two RowIDs per 16-byte store at the even slots of a list, one RowID per store where a pair's region
 * begins or ends on an odd slot.
 * Refusals, all decided before any kernel runs, nothing written: HY_ERR_CAPACITY with n_rows = what is needed when the result does not fit
 * `capacity`; HY_ERR_UNSUPPORTED when some pair's rows(cl) * rows(cr) does not fit a ChunkOffset (>= 2^32 - 1, :120) and for MVCC
 * pseudo-columns; HY_ERR_INVALID for null arguments, input PosLists or output lists off 8-byte boundaries.
 * hy_product_count: n_rows alone (pure host arithmetic, the same refusals).  Returns when the lists are complete. */
typedef struct hy_product_result {
  uint32_t mem;              /* HY_MEM_HOST | HY_MEM_DEVICE */
  uint32_t reserved;
  hy_row_id* left_pos;       /* [capacity] or NULL: this side not wanted */
  hy_row_id* right_pos;      /* [capacity] or NULL */
  uint64_t* pair_offsets;    /* host, [n_left_chunks * n_right_chunks + 1], or NULL */
  uint64_t capacity;
  uint64_t n_rows;           /* out: rows written, or needed with HY_ERR_CAPACITY */
} hy_product_result;
hy_status hy_product(const hy_column* left, const hy_column* right, hy_product_result* result);
hy_status hy_product_count(const hy_column* left, const hy_column* right, uint64_t* n_rows);

/* write_output_chunks' chunking of a join result (join_output_writing.cpp:245-296; JoinHash always allows the merge,
 * join_hash.cpp:563): one output chunk per non-empty PosList of slice_offsets[0 .. n_slices], after merging a PosList of fewer
 * than 1000 pairs with its successors while the sum stays below 4000.  chunk_offsets (room for n_slices + 1 values) receives
 * the pair ranges of the output chunks, *n_chunks their number.  Host arrays; pure host arithmetic. */
hy_status hy_join_output_chunks(const uint64_t* slice_offsets, uint32_t n_slices, uint64_t* chunk_offsets, uint32_t* n_chunks);

/* ---- AggregateHash (replaces AggregateHash::_on_execute, aggregate_hash.cpp:1180-1372) -------------------------- */
typedef struct hy_aggregate_spec {
  uint32_t function;              /* HY_AGG_* */
  const hy_column* column;        /* NULL for COUNT(*) */
} hy_aggregate_spec;

typedef struct hy_aggregate_column {
  uint32_t data_type;             /* out: HY_TYPE_* of the result column (window_function_traits.hpp)                 */
  uint32_t reserved;
  void* values;                   /* [group_capacity] int64 / double / int32 / float                                   */
  uint8_t* is_null;               /* [group_capacity] 1 = NULL (a group that saw only NULLs)                           */
} hy_aggregate_column;

typedef struct hy_aggregate_result {
  uint32_t mem;                   /* HY_MEM_HOST, or HY_MEM_DEVICE: group_row_ids / values / is_null are device buffers (the
                                   * groups are ordered on the host either way; a device result is uploaded once, so that an
                                   * operator chain can end on the device)                                              */
  uint32_t group_capacity;
  uint32_t n_groups;              /* out */
  uint32_t reserved;
  hy_row_id* group_row_ids;       /* [group_capacity] representative row per group (write_groupby_output)              */
  hy_aggregate_column* columns;   /* [n_aggregates] */
} hy_aggregate_result;

/* Group order == the CPU operator's: first occurrence, or ascending key under the immediate-key shortcut
 * (aggregate_hash.cpp:388-401, 770-804).  Up to sixteen GROUP BY columns (the reference: any number, aggregate_hash.cpp:1184-1198); more
 * answer HY_ERR_UNSUPPORTED. */
hy_status hy_aggregate_hash(const hy_column* const* groupby_columns, uint32_t n_groupby,
                            const hy_aggregate_spec* aggregates, uint32_t n_aggregates, hy_aggregate_result* result);

/* ---- AggregateHash whose output table stays in HBM (aggregate_hash.cpp:248-293, 422-540, 1301-1361, 1375-1460) ----------------
 * hy_aggregate_hash's result -- same groups, group order, values, NULL flags and representative rows as with HY_MEM_HOST on the same
 * arguments, bit for bit: the same kernels compute them -- as the columns of the operator's output table, where the next operator reads
 * them (a HAVING scan, Sort, a join): nothing but the group count comes to the host.
 *   aggregate_columns[a]  one column per aggregate: unencoded value segments of the result type hy_aggregate_hash reports
 *                         (window_function_traits.hpp), chunks of chunk_rows rows (the last one shorter; AggregateHash writes chunks of
 *                         Chunk::DEFAULT_SIZE = 65 535, :248-293), every chunk with a null vector (bit i of word i / 64, tail bits zero;
 *                         all zero for COUNT) -- hy_column_gather's layout: one pooled arena owned by the column, chunk values 256-byte
 *                         aligned with 16 spare bytes.  hy_column_read_chunk copies a chunk back; the caller destroys every handle with
 *                         hy_column_destroy.  Zero groups: columns of zero chunks.
 *   groupby_columns[g]    GROUP BY column g at the representative rows (write_groupby_output, :422-540): hy_column_gather over
 *                         group_row_ids, which never leave the device.  NULL where no column is made: bit g of skip_groupby_mask set (the
 *                         caller's word for "these are stand-ins for strings -- AggregateKey names --, I materialise the strings from
 *                         the RowIDs"), or a column hy_column_gather refuses.
 *   group_row_ids         the representative rows, n_groups RowIDs in DEVICE memory taken from the result-buffer pool
 *                         (hy_result_pool_acquire).  The CALLER owns the buffer and gives it back with hy_result_pool_release; NULL when
 *                         there is no group.
 * Two paths.  GROUP BY present, more than 4096 groups, only MIN / MAX / SUM / AVG / COUNT, fewer than 2^32 rows: the groups are ordered on
 * the device and the finish kernels write RowIDs and cells straight into the buffers above.  Everything else -- up to 4096 groups,
 * COUNT(DISTINCT), STDDEV_SAMP, ANY, no GROUP BY (over an empty input: the one row of NULLs / zero counts, :1422-1432), more aggregates
 * than one pass has accumulators for -- is finished on the host as in hy_aggregate_hash and uploaded once into the same layout: such
 * results are small, or rare where they are large.  (More aggregates than one pass holds: the passes write host arrays sized by the input's
 * rows, not by the groups -- that path costs in proportion to the input.)
 * More than sixteen GROUP BY columns: HY_ERR_UNSUPPORTED, like hy_aggregate_hash.  On any error no handle and no buffer is left to the
 * caller (everything in `out` is NULL / 0).  Returns when the columns are complete. */
typedef struct hy_aggregate_columns {
  uint64_t skip_groupby_mask;      /* in: bit g set = no output column for GROUP BY column g                                */
  uint32_t n_groups;               /* out */
  uint32_t reserved;
  hy_column** aggregate_columns;   /* out: [n_aggregates], the caller's array (may be NULL when n_aggregates == 0)          */
  hy_column** groupby_columns;     /* out: [n_groupby], the caller's array (may be NULL when n_groupby == 0)                */
  hy_row_id* group_row_ids;        /* out: device memory of the result-buffer pool, owned by the caller                     */
} hy_aggregate_columns;
hy_status hy_aggregate_hash_columns(const hy_column* const* groupby_columns, uint32_t n_groupby, const hy_aggregate_spec* aggregates,
                                    uint32_t n_aggregates, uint32_t chunk_rows, hy_aggregate_columns* out);

/* ---- fused TableScan(s) -> Projection -> AggregateHash over ONE data table --------------------
 * The plan shape of TPC-H Q1 / Q6 (tpch_queries.cpp:60-80, 206-210): a chain of ColumnVsValue / Between / IsNull / LIKE scans
 * on columns of one table (table_scan.cpp:97-240), a Projection of arithmetic expressions over the survivors
 * (operators/projection.cpp, expression_functors.hpp:127-213) and an AggregateHash of them (aggregate_hash.cpp:1180-1372).
 * The reference materialises a PosList per scan and an ExpressionResult vector per expression node; hy_table_scan ->
 * hy_poslist_translate -> hy_projection_arithmetic -> hy_aggregate_hash do the same in HBM.  This entry point evaluates the
 * whole chain in ONE pass over the table: a row is tested against every filter (the same normalised per-chunk tests
 * hy_table_scan evaluates: NULL never matches), the expressions are computed for the rows that pass -- cell by cell with
 * the types and NULL rules of hy_projection_arithmetic -- and fed to the accumulators of hy_aggregate_hash.  No PosList and
 * no expression column is written.  Results are those of the chain: same groups, same group order, same values (sums
 * of floating-point inputs within the tolerance hy_aggregate_hash states); group_row_ids name rows of the DATA table (the
 * chain's name rows of its last intermediate table).
 * Expressions are in postfix order over at most HY_MAX_EXPRESSION_NODES nodes and three stack slots:
 * l_extendedprice * (1 - l_discount) is  COLUMN l_extendedprice, LITERAL 1, COLUMN l_discount, ARITHMETIC SUB, ARITHMETIC MUL.
 * Validate as a filter (the plan shape of a SQL pipeline: GetTable -> Validate -> scans -> Projection -> Aggregate): a filter whose
 * `column` is the table's MvccData (HY_ENC_MVCC segments, see hy_validate) with predicate.condition = HY_FILTER_VALIDATE,
 * predicate.value.value_id = our transaction id, predicate.value2.value_id = the snapshot commit id and
 * predicate.column_is_nullable = can_use_chunk_shortcut keeps the rows hy_validate keeps (validate.cpp:47-68).
 * All columns are data columns (no reference segments) of one table.  HY_ERR_UNSUPPORTED: more than HY_MAX_FILTERS filters,
 * aggregate functions other than MIN / MAX / SUM / AVG / COUNT, string expressions, expressions that read more than six
 * distinct columns between them or need a fourth stack slot -- run the chain instead. */
enum { HY_EXPR_COLUMN = 0, HY_EXPR_LITERAL = 1, HY_EXPR_ARITHMETIC = 2 };
enum { HY_MAX_EXPRESSION_NODES = 12, HY_MAX_FILTERS = 4 };
enum { HY_FILTER_VALIDATE = 0x100 /* hy_filter.predicate.condition of a Validate filter; not a PredicateCondition */ };
typedef struct hy_expression_node {
  uint32_t kind;                  /* HY_EXPR_*                                                                         */
  uint32_t op;                    /* HY_EXPR_ARITHMETIC: HY_ARITH_*, applied to the two results below it on the stack  */
  const hy_column* column;        /* HY_EXPR_COLUMN                                                                    */
  uint32_t literal_type;          /* HY_EXPR_LITERAL: HY_TYPE_* (HY_TYPE_NULL: the NULL literal)                       */
  uint32_t reserved;
  hy_value literal;
} hy_expression_node;
typedef struct hy_expression {
  uint32_t n_nodes;
  uint32_t reserved;
  hy_expression_node nodes[HY_MAX_EXPRESSION_NODES];
} hy_expression;
typedef struct hy_filter {
  const hy_column* column;
  hy_predicate predicate;         /* as for hy_table_scan (literals already cast: hy_predicate_cast)                   */
} hy_filter;
typedef struct hy_fused_aggregate {
  uint32_t function;              /* HY_AGG_MIN / MAX / SUM / AVG / COUNT                                              */
  uint32_t reserved;
  const hy_expression* input;     /* NULL for COUNT(*)                                                                 */
} hy_fused_aggregate;
hy_status hy_scan_project_aggregate(const hy_filter* filters, uint32_t n_filters, const hy_column* const* groupby_columns, uint32_t n_groupby,
                                    const hy_fused_aggregate* aggregates, uint32_t n_aggregates, hy_aggregate_result* result);

/* ---- a star join as one call (BASELINE.json configs[4], the SSB star joins; csrc/plan.hip) ------------------------------------
 * The operator tree Hyrise runs for   fact JOIN dim_1 ... JOIN dim_k  GROUP BY ...  -- a TableScan per filtered dimension, one JoinHash
 * per dimension (the filtered dimension as build side, the join result so far as probe side, in the order given), a Projection for
 * the aggregates' arithmetic, an AggregateHash -- made by ONE function: exactly the calls of the entry points above an adapter would
 * make (hy_table_scan, hy_poslist_translate, hy_column_create, hy_column_export, hy_join_hash, hy_gather_row_ids,
 * hy_projection_arithmetic, hy_aggregate_hash), with every intermediate in device memory and no interpreter between them.  No
 * counterpart in the reference (its scheduler runs the operators one by one); the groups and their cells are those of the operator chain.
 * Where the shape allows (int32 primary keys with a range of at most 2^26 values, foreign keys as int32 values / FrameOfReference offsets
 * without NULLs) every dimension is probed in ONE pass over the fact table instead (csrc/join_star.hpp, HY_OPT_STAR_FUSED_PROBE): the join
 * result's rows -- and with them the groups, ordered by their first row -- then come in the fact table's row order, not in the order the
 * last JoinHash of the chain would leave them in.  Where, in addition, every GROUP BY column (one to four) and every aggregate input (at most
 * eight aggregates: MIN / MAX / SUM / AVG / COUNT) is an int / long column -- at most four distinct columns of the fact table and four of
 * the dimensions among them, and at most 4096 groups --, the Projection and the AggregateHash happen inside that join
 * (HY_OPT_STAR_FUSED_FINISH): the rows that survive every dimension are grouped where they are found; same groups, order, cells and
 * representative rows as the steps it replaces.
 * Columns are named as (table, column): table 0 = the fact table, d + 1 = dimension d; every column is a DATA column (numeric, or a
 * dictionary of key names / join ids) of its table.  An aggregate reads `left` alone (op = HY_STAR_NO_OP), `left <op> right`
 * (HY_ARITH_*: hy_projection_arithmetic), or nothing (left.column = NULL: COUNT(*)).  *joined_rows: rows of the join result.
 * NULLs: a foreign key that is NULL finds no partner, a NULL aggregate input is skipped, NULL GROUP BY cells are a group of their own -- as in
 * the operator chain (the plan's intermediate tables carry null vectors where a cell is NULL; such plans keep to the join-by-join / RowID paths). */
enum { HY_MAX_STAR_DIMENSIONS = 8, HY_MAX_STAR_AGGREGATES = 8 };
#define HY_STAR_NO_OP 0xFFFFFFFFu
typedef struct hy_star_dimension {
  const hy_column* key;            /* the dimension's key column: the build side of its join                                     */
  const hy_column* filter_column;  /* a column of the dimension that `predicate` tests; NULL: the dimension is not filtered        */
  hy_predicate predicate;
  const hy_column* fact_key;       /* the fact table's foreign key to this dimension                                             */
} hy_star_dimension;
typedef struct hy_star_column {
  uint32_t table;                  /* 0 = the fact table, d + 1 = dimension d                                                    */
  uint32_t reserved;
  const hy_column* column;
} hy_star_column;
typedef struct hy_star_aggregate {
  uint32_t function;               /* HY_AGG_*                                                                                   */
  uint32_t op;                     /* HY_STAR_NO_OP or HY_ARITH_*                                                                */
  hy_star_column left, right;
} hy_star_aggregate;
hy_status hy_star_join_aggregate(const hy_star_dimension* dimensions, uint32_t n_dimensions, const hy_star_column* groupby, uint32_t n_groupby,
                                 const hy_star_aggregate* aggregates, uint32_t n_aggregates, hy_aggregate_result* result, uint64_t* joined_rows);

/* The same star join over FILTERED tables: a conjunction of up to HY_MAX_STAR_FILTERS tests per dimension, a conjunction of tests on the
 * fact table itself, and an aggregate that may have no GROUP BY column -- the thirteen SSB queries as one call each (Q1.x filter lineorder
 * and group nothing; Q3.x / Q4.x put two predicates or an IN list on a dimension).  The operator tree it stands for: the fact filters as
 * chained TableScans on the fact table, run first (a NULL cell drops the row); per dimension a chain of TableScans, its filters in the order
 * given; then the JoinHashes, the Projection and the AggregateHash of hy_star_join_aggregate.  A filter is what hy_table_scan takes
 * (`predicate`, read where in_list is NULL) or what hy_table_scan_in_list takes (`in_list`: column [NOT] IN (...), at most HY_MAX_IN_LIST
 * elements; a string column's list carries per-chunk value ids); its column is a DATA column of the table it filters.
 * Where hy_star_join_aggregate's fused probe applies and every fact filter column is a plain data column (Unencoded / FrameOfReference /
 * Dictionary segments with 1-, 2- or 4-byte vectors), the fact filters are tested inside the one pass over the fact table, before the
 * dimensions are asked, and a dimension's filters are tested where its direct table is built; other shapes (RunLength or bit-packed filter
 * columns, non-int32 keys, NULL foreign keys) run the chain with hy_table_scan / hy_table_scan_in_list, hy_poslist_translate and the
 * join-by-join path -- the same groups and cells.  *joined_rows: the rows left after the fact filters and every join.  Group order: the fact
 * table's row order on the fused probe, the last join's order otherwise (as hy_star_join_aggregate).
 * n_groupby == 0: the result is hy_aggregate_hash's for the same rows without a GROUP BY column -- ONE row; over no rows COUNT is 0 and
 * every other aggregate NULL.  On the fused probe with HY_OPT_STAR_FUSED_FINISH that row is reduced inside the join: per workgroup in
 * registers and LDS, one addition per workgroup to the single accumulator row, no hash table.
 * HY_ERR_INVALID: null arguments, n_dimensions outside 1 .. HY_MAX_STAR_DIMENSIONS, a filter column that is not a column of its table, a
 * string column's list given as hy_value elements.  HY_ERR_UNSUPPORTED: more than HY_MAX_STAR_FILTERS filters on a table, and whatever the
 * scan of a filter refuses.  Nothing is written on error. */
enum { HY_MAX_STAR_FILTERS = 4 };
typedef struct hy_star_filter {
  const hy_column* column;         /* a DATA column of the table it filters                                                      */
  hy_predicate predicate;          /* as hy_table_scan takes it; read when in_list is NULL                                       */
  const hy_in_list* in_list;       /* or: column [NOT] IN (...), as hy_table_scan_in_list takes it                               */
} hy_star_filter;
typedef struct hy_star_dimension_where {
  const hy_column* key;            /* the dimension's key column: the build side of its join                                     */
  const hy_column* fact_key;       /* the fact table's foreign key to this dimension                                             */
  const hy_star_filter* filters;   /* a conjunction; n_filters == 0: the dimension is not filtered                               */
  uint32_t n_filters, reserved;
} hy_star_dimension_where;
hy_status hy_star_join_aggregate_where(const hy_star_dimension_where* dimensions, uint32_t n_dimensions,
                                       const hy_star_filter* fact_filters, uint32_t n_fact_filters,
                                       const hy_star_column* groupby, uint32_t n_groupby,
                                       const hy_star_aggregate* aggregates, uint32_t n_aggregates,
                                       hy_aggregate_result* result, uint64_t* joined_rows);

/* ---- multi-GPU exchange (the reference is one process: these have no counterpart there) ----------------
 * Sharding an operator over GPUs adds one exchange step per operator (hyrise_amd/distributed.py: one process per GPU, RCCL):
 * the broadcast-build JoinHash all-gathers the build side's join column, the repartitioned JoinHash sends every (key, RowID)
 * to the GPU  std::hash(key) % parts  (the integer itself: JoinHash's own hash function, join_hash_steps.hpp:352), the
 * sharded AggregateHash all-reduces per-group partials.  The buffers of those collectives are produced and consumed on the
 * device by the entry points below; all pointers are DEVICE pointers unless stated. */
/* The column's values decoded into values[rows] (the column's type; NULL rows: 0) and, if nulls is not NULL, nulls[rows] bytes. */
hy_status hy_column_export(const hy_column* column, void* values, uint8_t* nulls);
/* Rows per destination of a hash repartition of an integer join column (NULL keys never find a partner: they are not sent).
 * counts[parts] is a HOST array. */
hy_status hy_repartition_count(const hy_column* column, uint32_t parts, uint64_t* counts);
/* The (key, RowID) tuples grouped by destination, (chunk, row) order inside each: keys_out (int32 for an int column, int64 for a
 * long column) and row_ids_out hold the tuples of destination 0, then 1, ...; counts[parts] (HOST) as above.  The RowIDs carry
 * chunk_id + chunk_id_offset (the shard's first chunk in the whole table). */
hy_status hy_repartition_pack(const hy_column* column, uint32_t parts, uint32_t chunk_id_offset, void* keys_out, hy_row_id* row_ids_out,
                              uint64_t capacity, uint64_t* counts);
/* out[i] = table[positions[i].chunk_id * chunk_rows + positions[i].chunk_offset] (NULL_ROW_ID stays): the PosList of a join over
 * received tuple arrays (presented as a column of chunk_rows-row chunks) back to the RowIDs that travelled with the keys. */
hy_status hy_gather_row_ids(const hy_row_id* table, uint64_t table_rows, uint32_t chunk_rows, const hy_row_id* positions, uint64_t n,
                            hy_row_id* out);

#ifdef __cplusplus
}
#endif
#endif /* HYRISE_AMD_H_ */

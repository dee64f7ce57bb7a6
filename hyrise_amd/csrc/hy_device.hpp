// hy_device.hpp -- internal declarations shared by the HIP translation units behind include/hyrise_amd.h.
// gfx950 (MI355X / CDNA4) only: wave64, 256 CUs in 8 XCDs, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hyrise_amd.h"
#include "hy_options.hpp"

namespace hy {

// ---- device-side view of one segment (48 bytes, read through the scalar/L2 path by every workgroup) ---------------
struct DevSegment {
  const void* data;            // values | attribute vector | FoR offsets | pos list (hy_row_id)
  const void* aux;             // dictionary | block minima
  const uint64_t* nulls;       // null bitmap or nullptr
  const DevSegment* ref;       // REFERENCE: segments of the referenced column
  uint32_t size;
  uint32_t aux_size;
  uint32_t ref_chunk_id;
  uint8_t encoding;
  uint8_t data_type;
  uint8_t width;               // bytes per element of `data`; SEG_PACKED | b: a bit-packed attribute / offset vector of b bits per element
  uint8_t flags;               // SEG_UNALIGNED | HY_SORT_* << SEG_SORT_SHIFT
};
enum : uint8_t { SEG_UNALIGNED = 1, SEG_SORT_SHIFT = 4, SEG_PACKED = 0x80 };
// (the struct stays 48 bytes -- three 16-byte scalar loads, and the streaming scan keeps two of them in scalar registers)
__host__ __device__ inline bool seg_is_packed(const DevSegment& s) { return (s.width & SEG_PACKED) != 0; }
__host__ __device__ inline uint32_t seg_bits(const DevSegment& s) { return s.width & 0x7Fu; }
__host__ __device__ inline uint32_t seg_sorted_by(const DevSegment& s) { return s.flags >> SEG_SORT_SHIFT; }

// A contiguous run of at most SLICE_ROWS rows of one chunk: the unit of work of the scan / materialise kernels.
struct Slice {
  uint32_t chunk;
  uint32_t row_begin;
  uint32_t row_count;
  uint32_t first_of_chunk;     // 1 if row_begin == 0
};

// What a kernel that runs AHEAD of its data needs to know about a slice, in one 32-byte record (one scalar load instead of
// the slice -> segment descriptor -> data chain): where the rows' stored words are and how to read them.
struct SliceView {
  const void* data;            // the chunk's values / offsets (VIEW_GENERIC: unused, the kernel goes through DevSegment)
  const void* aux;             // FrameOfReference: block minima
  uint32_t chunk;
  uint32_t row_begin;
  uint32_t row_count;
  uint32_t kind;               // VIEW_*
};
enum : uint32_t { VIEW_GENERIC = 0, VIEW_INT32 = 1, VIEW_FOR8 = 2, VIEW_FOR16 = 3, VIEW_FOR32 = 4 };   // int32 values | FoR offsets of 1 / 2 / 4 bytes, no NULLs

// A part: at most PART_SLICES consecutive slices of ONE chunk -- the unit a scan workgroup owns.  A Hyrise chunk
// (<= 65 535 rows) is exactly one part, so its PosList is produced by one workgroup without any inter-workgroup traffic.
struct Part {
  uint32_t first_slice;
  uint32_t n_slices;
  uint32_t chunk;
  uint32_t part_in_chunk;
  uint32_t parts_in_chunk;
  uint32_t first_part;          // index of the chunk's part 0
  uint32_t first_row;           // chunk offset of the part's first row
  uint32_t reserved;
  uint64_t region_base;         // first RowID slot of the chunk's output region (= rows in all chunks before it)
};
constexpr uint32_t PART_SLICES = 8;   // upper bound (LDS sizing); the actual part length is chosen per column

constexpr uint32_t WG_THREADS = 256;
constexpr uint32_t ROWS_PER_THREAD = 32;
constexpr uint32_t SLICE_ROWS = WG_THREADS * ROWS_PER_THREAD;   // 8192

// hipFuncSetAttribute applies to the calling thread's current device: a kernel that asks for more dynamic LDS than a workgroup gets by default
// is registered once per DEVICE and call site (a process-wide flag would leave the second GPU of a one-process plan -- hy_bind_device, one
// worker thread per GPU -- with the default limit and its launches failing).
class OncePerDevice {
 public:
  bool pending(uint64_t* bit) const {
    int device = 0;
    (void)hipGetDevice(&device);
    *bit = 1ull << (static_cast<unsigned>(device) & 63u);
    return (done_.load(std::memory_order_acquire) & *bit) == 0;
  }
  void done(uint64_t bit) { done_.fetch_or(bit, std::memory_order_release); }

 private:
  std::atomic<uint64_t> done_{0};
};

}  // namespace hy

// What the first JoinHash over a resident build column learned about its keys (join.hip: rank_table_fill_checked): later joins
// fill their rank table in one pass sized by it and CHECK it in the same pass -- it saves no work on the keys, only a host round
// trip and the second read.  state: 0 nothing known, 1 valid, 2 do not use (a check failed once).
struct hy_join_key_hint {
  std::atomic<uint32_t> state{0};
  std::atomic<uint32_t> unique{0};          // no key twice (a column with duplicates still serves Semi / Anti joins: presence bits only)
  std::atomic<uint64_t> key_min{0}, key_max{0};
  std::atomic<uint32_t> has_duplicates{0};  // rank_table_mark met a key twice: later joins over the column go straight to the sorted directory
  std::atomic<uint32_t> probe_locality{0};  // as a PROBE side: 0 not looked at, 1 neighbouring rows hold neighbouring keys, 2 they do not (probe_key_locality, join.hip)
};

// The per-chunk jobs of a ColumnVsValue / Between / IsNull predicate (prepare_jobs, scan.hip: one dictionary bound search and the all /
// none early-outs per chunk) are a pure function of the column's segments -- immutable once encoded, abstract_encoded_segment.hpp:12-17 --
// and of the predicate's literal words: a data column keeps the job tables of the last few predicates it was scanned with (a prepared
// statement's scan, a benchmark's repeated query), later scans with the same literal read them instead of searching 916 dictionaries
// again (one launch, 6 us at SF10 in front of a 60 us scan).  Every row is still tested by the scan kernel.
struct hy_scan_job_cache {
  struct Entry {
    uint8_t key[40];        // condition | value_type | value | value2 | column_is_nullable | materialize_all | no_ranges
    void* jobs = nullptr;   // [n_chunks + 1] ScanJob, device memory owned by the column
    hipStream_t stream = nullptr;   // the stream the jobs were prepared on: scans on another stream prepare their own
    uint64_t used = 0;
  };
  std::mutex mutex;
  Entry entries[4];
  uint64_t clock = 0;
};

// The opaque ABI type.
struct hy_column {
  uint32_t n_chunks = 0;
  uint32_t data_type = HY_TYPE_NULL;
  uint64_t rows = 0;
  int device = 0;                           // the device of the thread that created it: operators refuse a column of another device
  bool is_reference = false;
  bool is_mvcc = false;                     // HY_ENC_MVCC segments: a table's MvccData, only hy_validate reads it
  bool multi_chunk_reference = false;       // some pos list spans several referenced chunks
  bool has_dictionary_without_values = false;
  uint32_t stream_width = 0;                // 1|2|4 if every segment is an aligned W-byte id/offset/int32 vector, else 0
  const hy_column* ref = nullptr;
  std::vector<hy_segment> host_segments;    // caller's descriptors (pointers patched to device addresses)
  std::vector<uint64_t> row_base;           // [n_chunks + 1] prefix sum of sizes
  hy::DevSegment* d_segments = nullptr;
  hy::Slice* d_slices = nullptr;
  hy::SliceView* d_slice_views = nullptr;   // [n_slices]
  uint32_t n_slices = 0;
  hy::Part* d_parts = nullptr;
  uint32_t n_parts = 0;
  uint64_t* d_row_base = nullptr;           // [n_chunks + 1] device copy of row_base
  uint32_t* d_first_slice = nullptr;        // [n_chunks + 1] index of every chunk's first slice (the last entry: n_slices)
  bool descriptors_pooled = false;          // the five descriptor tables above are pieces of ONE pooled block (column->pooled), uploaded with one copy
  std::vector<void*> owned;                 // device allocations freed with the column
  std::vector<std::pair<size_t, void*>> pooled;   // ... or handed back to the buffer pool (operator results)
  mutable hy_join_key_hint join_hint;
  mutable hy_scan_job_cache scan_jobs;
  // smallest / largest non-NULL value of an int32 data column (join_star.hpp: the range a dimension's direct table spans): computed once --
  // the segments are immutable -- by the first star join that uses the column as a dimension key.  state 1: valid, 2: the column holds no value
  mutable std::atomic<uint32_t> extent_state{0};
  mutable std::atomic<int64_t> extent_min{0}, extent_max{0};
  mutable std::atomic<uint64_t> aggregate_hint{0};   // aggregate.hip: which path the last GROUP BY led by this column ended on (signature of the column set << 8 | partition bits + 1)
  mutable std::atomic<uint64_t> star_aggregate_hint{0};   // plan.hip: the same for the GROUP BY of a star join whose first GROUP BY column this is (its aggregate reads intermediate columns)
  // RunLength segments and bit-packed vectors stay compressed in device memory; TableScan reads them in place.  The operators that
  // gather rows (joins, aggregates, projections, exchanges, reference columns) read `plain`: the same column as Value / FixedWidthInteger
  // segments, decoded ON THE DEVICE from the resident compressed buffers the first time one of them asks (plain_column, runtime.hip).
  bool has_compressed = false;
  bool has_sorted = false;                  // some chunk is flagged as sorted by this column (hy_segment::sorted_by): its scan may take JOB_RANGE jobs
  mutable std::mutex plain_mutex;
  mutable hy_column* plain = nullptr;       // owned
  hy_column* stand_in = nullptr;            // owned: the data stand-in a reference column of hy_column_string_ranks reads through (`ref`)
};

namespace hy {

// ---- like.hip: string dictionaries in device memory and the LIKE matcher over them ---------------------------------------------------
// One chunk's dictionary as the matcher reads it (32 bytes: two 16-byte scalar loads).
struct LikeChunk {
  const char* chars;
  const uint32_t* offsets;     // [n_entries + 1] byte offsets into chars, or nullptr: slots of string_length bytes
  uint32_t n_entries;
  uint32_t string_length;
  uint64_t first_word;         // where the chunk's bitmap words begin (hy_string_dictionary::word_offsets)
};
// The 256 consecutive entries a matcher workgroup owns: four bitmap words.
struct LikeBlock {
  uint32_t chunk;
  uint32_t first_entry;        // a multiple of 256
};
// A LIKE pattern as the kernel takes it (hy_like_tokenize): one token per pattern element, runs of `%` collapsed into one.
constexpr uint16_t LIKE_ANY_ONE = 0x100, LIKE_ANY_RUN = 0x200;
struct LikeProgram {
  uint16_t tokens[HY_MAX_LIKE_PATTERN];   // a literal byte (folded under the insensitive conditions) | LIKE_ANY_ONE | LIKE_ANY_RUN
  uint32_t n_tokens;
  uint32_t negated;
  uint32_t insensitive;
};

}  // namespace hy

// The opaque ABI type: the dictionaries of one column's DictionarySegment<pmr_string> chunks, value-id order, resident in HBM.
struct hy_string_dictionary {
  uint32_t n_chunks = 0;
  uint32_t mem = HY_MEM_HOST;
  int device = 0;
  std::vector<hy::LikeChunk> chunks;            // (chars / offsets: device addresses)
  std::vector<hy::LikeBlock> blocks;
  std::vector<uint64_t> word_offsets;           // [n_chunks + 1]
  std::vector<uint64_t> entry_offsets;          // [n_chunks + 1] prefix sum of n_entries: where a chunk's ranks begin (string_order.hip)
  mutable std::vector<void*> owned;             // device allocations freed with the object
  mutable std::vector<uint64_t> chars_bytes;    // [n_chunks] bytes of an offsets chunk's chars (offsets[n_entries]); ~0: caller-owned offsets nobody has read yet
  // The three tables above in device memory, uploaded by the first launch that needs them (creating a dictionary over caller-owned
  // device buffers is pure host work).
  mutable std::mutex tables_mutex;
  mutable hy::LikeChunk* d_chunks = nullptr;
  mutable hy::LikeBlock* d_blocks = nullptr;
  mutable uint64_t* d_word_offsets = nullptr;
  mutable uint64_t* d_entry_offsets = nullptr;
};

namespace hy {

int this_thread_device();   // runtime.hip: the device the calling thread is bound to
hy_status like_program(const char* pattern, uint32_t pattern_bytes, uint32_t condition, LikeProgram* program, const char* entry_point);
hy_status like_dictionary_tables(const hy_string_dictionary* dict);   // ensures d_chunks / d_blocks / d_word_offsets / d_entry_offsets
// queues the matcher on `stream`: d_words[word_offsets[c] + v / 64] bit v % 64 for every entry v of every chunk c (tail bits zero)
hy_status like_launch(const hy_string_dictionary* dict, const LikeProgram& program, uint64_t* d_words, hipStream_t stream);

// ---- string_order.hip, string_gather.hip, string_substr.hip, string_join_keys.hip: the operators over string dictionaries ------------------
// (Scratch and Carver are declared below; every temporary of these files is a block of a *_layout: sizing is a dry run of the layout.)
struct Scratch;
struct Carver;
// The two refusals of a dictionary, before any launch and any allocation: it lives on the calling thread's device; `total` entries fit int32 ranks.
hy_status dictionary_device_check(const hy_string_dictionary* dict, const char* entry_point);
hy_status entries_fit_ranks(uint64_t total, const char* entry_point);
// Refusals of a (left, right) pair ordered chunk by chunk (hy_string_dictionary_ranks): chunk counts, devices, a right chunk of 2^30 entries or more.
hy_status string_order_check(const hy_string_dictionary* left, const hy_string_dictionary* right, const char* entry_point);
hy_status column_order_check(const hy_string_dictionary* dict, const char* entry_point);   // both refusals above, of a dictionary that is to be ordered
hy_status string_column_check(const hy_column* column, const hy_string_dictionary* dict, const char* entry_point);   // ... of a string column and its dictionary
// queues the ranking on `stream`: d_ranks[left->entry_offsets[c] + v] for every entry v of every chunk c of `left`
hy_status string_order_launch(const hy_string_dictionary* left, const hy_string_dictionary* right, int32_t* d_ranks, hipStream_t stream);
// The int32 stand-ins of a pair of string columns (hy_table_scan_columns_strings): every segment descriptor of the data columns copied with
// data_type int32 and `aux` = the chunk's ranks (left) / the table 0, 2, 4, ... (right, filled here: n_evens entries); the descriptors of
// reference columns (null: a data column) copied with `ref` = those copies.  One launch on `stream`.
struct StringTwins {
  const DevSegment* left_data; const DevSegment* right_data;   // [n_data_chunks]
  DevSegment* left_data_twin; DevSegment* right_data_twin;
  const DevSegment* left_reference; const DevSegment* right_reference;   // [n_chunks] or nullptr
  DevSegment* left_reference_twin; DevSegment* right_reference_twin;
  const uint64_t* entry_offsets;   // the left dictionary's, device memory
  const int32_t* ranks;
  int32_t* evens;
  uint32_t n_data_chunks, n_chunks, n_evens;
};
hy_status string_twins_launch(const StringTwins& twins, hipStream_t stream);
// The merge sequence (one column's global string order, hy_string_dictionary_order) for the other translation units: its temporaries for
// `total` > 0 positions, and the three sequences over them.  *blocks.n_distinct is the number of distinct strings, in device memory.
struct MergeBlocks {
  uint64_t* ping;
  uint64_t* pong;
  uint32_t* tile_heads;
  uint32_t* n_distinct;
};
void merge_layout(Carver& carver, uint64_t total, MergeBlocks& blocks);
struct EntryWindow {   // bytes [begin, begin + length) of a dictionary entry
  uint32_t begin;
  uint32_t length;
};
struct SubstrArguments {
  int32_t start, length;
};
// A window at the entry's first byte (start 0 or 1, or an empty result; no window at all) keeps a sorted run of entries sorted: the merge
// may start from whole chunks.  Any other window does not, and the merge starts from single positions.
inline bool windows_keep_order(const SubstrArguments* substr) { return !substr || substr->length <= 0 || substr->start == 0 || substr->start == 1; }
// d_ranks[entry_offsets[c] + v], total = entry_offsets[n_chunks] > 0.  With d_windows (one EntryWindow per entry, at entry_offsets[c] + v) the
// entries are ordered as their windows read; `sorted_chunks` says that every chunk's windowed entries still ascend (equal neighbours allowed).
hy_status column_order_launch(const hy_string_dictionary* dict, const MergeBlocks& blocks, int32_t* d_ranks, hipStream_t stream, const EntryWindow* d_windows = nullptr,
                              bool sorted_chunks = true);
// The sparse route (HY_OPT_STRING_SPARSE_GATHER, string_gather.hip): the column read at the rows asked for, the entries they reference -- the
// SUBSET, U <= min(n, E) of them in ascending entry order -- as a table of (address, length) that the ranking and the back end read instead
// of the dictionary, and ranks per subset index.  A row's entry is then its index into the table.
struct SubsetEntry {   // the bytes of a referenced entry, seen through its window if there is one
  const uint8_t* bytes;
  uint32_t length;
  uint32_t reserved;
};
// the order of a table of `total` > 0 entries whose chunk runs [d_run_offsets[c], d_run_offsets[c + 1]) each ascend (by_position: they need
// not -- the merge starts from single positions); d_ranks[i] for table entry i
hy_status table_order_launch(const SubsetEntry* d_table, const uint64_t* d_run_offsets, uint32_t n_chunks, uint64_t total, bool by_position, const MergeBlocks& blocks, int32_t* d_ranks,
                             hipStream_t stream);
// the merge sequence over the chunks of two dictionaries laid end to end -- the tables are the caller's, in device memory (chunks [n_chunks],
// blocks [n_blocks] with joint chunk indices, entry_offsets [n_chunks + 1]); positions below `split` are the left dictionary's.  total > 0.
struct PairTables {
  const LikeChunk* chunks;
  const LikeBlock* blocks;
  const uint64_t* entry_offsets;
  uint32_t n_chunks, n_blocks;
  uint64_t total, split;
};
hy_status pair_order_launch(const PairTables& tables, const MergeBlocks& blocks, int32_t* d_left_ranks, int32_t* d_right_ranks, hipStream_t stream);
// An output in the caller's device memory, or in host memory behind a twin carved from the arena: `parts` of the twin are copied to the
// host, then *n_distinct (if asked for), and the stream is waited for.  A device output without n_distinct returns without a synchronise:
// it is complete in the order of the calling thread's stream.
struct TwinPart {
  void* host;
  const void* device;
  size_t bytes;
};
hy_status outputs_to_caller(uint32_t mem, const TwinPart* parts, uint32_t n_parts, const uint32_t* d_n_distinct, uint32_t* n_distinct, hipStream_t stream);
// The int32 stand-in of a string column over a table of E int32_t in device memory (entry v of data chunk c reads d_table[entry_offsets[c] + v]):
// the caller's attribute vectors and PosLists, shared.  A reference column's stand-in owns its data stand-in; the table stays the caller's.
// data_type HY_TYPE_LONG: a table of E int64_t, an int64 stand-in (the join ids of string_join_keys.hip).
hy_status string_stand_in(const hy_column* column, const hy_string_dictionary* dict, void* d_table, hy_column** out, uint32_t data_type = HY_TYPE_INT);
// A table of keys of its own allocation and the stand-in over it, which owns the table once it is made (hy_column_string_ranks,
// hy_column_string_join_keys).  drop(): what a call that gives up does, after it has synchronised -- the stand-in with its table, or the table alone.
struct KeyColumn {
  void* d_keys = nullptr;
  hy_column* stand_in = nullptr;
  hy_status alloc(size_t bytes);
  hy_status make_stand_in(const hy_column* column, const hy_string_dictionary* dict, uint32_t data_type);
  void drop();
};
// string_gather.hip: the four producers of string columns (hy_string_column_gather, hy_string_ranks_gather, hy_string_column_substr,
// hy_string_column_materialize) as one request: resolved once, then run as stages (DESIGN.md sections 4.17 - 4.20).
struct OutChunks {   // the output chunks' sizes on the host
  std::vector<uint32_t> sizes;
  uint32_t chunk_rows = 0;   // 0: the sizes are another column's (uploaded as row_base / vector_at)
  uint64_t n = 0;
};
enum class StringRoute : uint32_t { ColumnRows, RowIds, Ranks, Sparse };   // Sparse: the column read at `positions`, or (nullptr) at its own rows
struct StringRequest {
  const char* name = nullptr;                   // the entry point's
  const hy_column* column = nullptr;            // the string column; Ranks: the int32 column of ranks
  const hy_string_dictionary* dict = nullptr;
  const hy_row_id* positions = nullptr;
  uint64_t n = 0;                               // output rows
  const SubstrArguments* substr = nullptr;
  OutChunks out;
  StringRoute route = StringRoute::ColumnRows;
  hy_column** result = nullptr;
  hy_string_dictionary** result_dict = nullptr;
};
// Every refusal, and the results without rows (*answered), before anything is allocated or launched.  `route`: ColumnRows, RowIds or Ranks --
// the resolver turns the first two into Sparse where string_sparse_route says so.  chunk_rows: RowIds only.
hy_status string_request(StringRoute route, const char* name, const hy_column* column, const hy_string_dictionary* dict, const hy_row_id* positions, uint64_t n, uint32_t chunk_rows,
                         const SubstrArguments* substr, hy_column** result, hy_string_dictionary** result_dict, StringRequest* request, bool* answered);
hy_status string_request_run(const StringRequest& request);
// string_substr.hip, for the stages of a request: the windows of every entry; every row's entry from the exported stand-in over 0, 1, 2, ...
void entry_windows_launch(const hy_string_dictionary* dict, const SubstrArguments& substr, EntryWindow* d_windows, hipStream_t stream);
void entries_of_rows_launch(const int32_t* values, const uint8_t* nulls, uint64_t n, uint64_t n_source_entries, int32_t* d_entry, hipStream_t stream);
// scan.hip: `dict` is the string dictionary of `column`'s data column, chunk by chunk, on `column`'s device; `which`: "", "left " or "right "
hy_status check_dictionary(const hy_string_dictionary* dict, const hy_column* column, const char* which, const char* entry_point);

// ---- errors ---------------------------------------------------------------------------------------------------------
hy_status fail(hy_status code, const char* fmt, ...);
void clear_error();   // a refusal that the caller answered itself: hy_last_error is empty again
hy_status on_this_device(const hy_column* column, const char* entry_point);   // runtime.hip: the calling thread's device holds the column
hy_status plain_column(const hy_column* column, const hy_column** plain);      // runtime.hip: `column` itself, or its decoded twin (see hy_column::plain)
#define HY_HIP(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t err__ = (expr);                                                                            \
    if (err__ != hipSuccess)                                                                              \
      return ::hy::fail(HY_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), __FILE__, __LINE__); \
  } while (0)
#define HY_TRY(expr)                    \
  do {                                  \
    hy_status st__ = (expr);            \
    if (st__ != HY_OK) return st__;     \
  } while (0)

hipStream_t current_stream();
void bind_thread_device();   // hipSetDevice(the device hy_init chose) once per thread

// Pinned, device-mapped host memory of this thread (grow-only): small results that kernels store straight into host
// memory, read by the host after a stream synchronise -- instead of one blit kernel and host round trip per hipMemcpyAsync.
hy_status pinned_staging(size_t bytes, void** host, void** device);

// join.hip: stable LSD radix sort of (key, id) pairs by key (see there)
hy_status sort_pairs_u32(uint32_t** keys, uint32_t** ids, uint32_t* keys_tmp, uint32_t* ids_tmp, uint64_t n, uint32_t key_bits, hipStream_t stream);

// Optional HIP-event bracket around the dominant kernel of an operator call (hy_set_profiling / hy_last_kernel_ms).
void release_thread_join_state();   // join.hip: frees the calling thread's pinned mailbox (hy_shutdown)
void profile_begin(hipStream_t stream, uint32_t kind = HY_KERNEL_OTHER);   // kind: HY_KERNEL_* (hy_profile_read_kernel)
void profile_end(hipStream_t stream);
bool profile_events(hipEvent_t* start, hipEvent_t* stop, uint32_t kind = HY_KERNEL_OTHER);   // per-kernel pair for hipExtLaunchKernelGGL

// ---- per-thread scratch (status words for decoupled look-back, job tables, temporaries) ----------------------------
// Every operator call of a thread reuses one growing arena; thread-safe because it is thread-local, as are streams.
struct Scratch {
  void* base = nullptr;
  size_t capacity = 0;
  size_t used = 0;
  uint32_t* ticket = nullptr;     // monotonically increasing work-ticket counter (never reset: base passed per launch)
  uint32_t ticket_base = 0;
  uint32_t epoch = 0;             // tag of the current launch in look-back status words (30 bits, never 0)
  uint64_t* status = nullptr;     // look-back status words; used for NOTHING else, so stale words carry older epochs
  size_t status_capacity = 0;
  hy_status reserve(size_t bytes);   // ensure capacity (may reallocate: only call before carving)
  hy_status begin_launch(size_t status_words, uint32_t tickets);  // new epoch; returns with status/ticket_base valid
  void* carve(size_t bytes);         // 256-byte aligned sub-allocation of the arena
  void reset() { used = 0; }
};
Scratch& scratch();

template <typename T>
inline T* carve(Scratch& s, size_t count) {
  return static_cast<T*>(s.carve(sizeof(T) * (count ? count : 1)));
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A bump allocator of 256-byte aligned device blocks over one of three backers: the thread's Scratch, a caller's block (whose size is the
// caller's promise), or no memory at all -- then it only counts, and `used` is what the same takes need: sizing is a dry run of the layout.
// A block that does not fit is recorded, not returned: one check of `failed` behind the last take.
struct Carver {
  Scratch* arena = nullptr;
  char* block = nullptr;
  size_t used = 0;       // bytes from the first block's begin to the last block's end
  bool failed = false;
  void* take_bytes(size_t bytes) {
    const size_t offset = align_up(used, 256);
    used = offset + bytes;
    if (arena) {
      void* at = arena->carve(bytes);
      failed |= at == nullptr;
      return at;
    }
    return block ? block + offset : nullptr;
  }
  template <typename T>
  T* take(size_t count) { return static_cast<T*>(take_bytes(sizeof(T) * (count ? count : 1))); }
};
// The thread's arena sized by a dry run of `layout`, then the layout run against it: one reserve, before any carve, and one check.
template <typename Layout>
inline hy_status reserve_and_carve(Layout&& layout) {
  Carver sizing;
  layout(sizing);
  HY_TRY(scratch().reserve(sizing.used));
  Carver carver{&scratch()};
  layout(carver);
  return carver.failed ? fail(HY_ERR_DEVICE, "scratch arena exhausted") : HY_OK;
}


// Temporary device buffers come from a per-thread pool of power-of-two blocks that is reused across calls in stream
// order (hipMalloc/hipFree cost ~100 us each and synchronise the device); hy_shutdown releases the calling thread's pool.
hy_status pool_acquire(size_t bytes, void** ptr, size_t* capacity);
void pool_release(void* ptr, size_t capacity);

struct DeviceBuffer {
  void* ptr = nullptr;
  size_t capacity = 0;
  bool borrowed = false;   // `ptr` belongs to somebody else (borrow): nothing is given back
  hy_status alloc(size_t bytes);
  void borrow(void* block);
  ~DeviceBuffer();
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  template <typename T> T* as() const { return static_cast<T*>(ptr); }
};
inline void swap(DeviceBuffer& a, DeviceBuffer& b) {   // the blocks change owners, nothing is given back
  std::swap(a.ptr, b.ptr);
  std::swap(a.capacity, b.capacity);
  std::swap(a.borrowed, b.borrowed);
}


// ---- aggregate.hip: which path a GROUP BY should take, for callers whose input columns do not live long enough to remember it themselves
// (hy_column::aggregate_hint does that for resident columns; the intermediate tables of hy_star_join_aggregate are new in every call).
// t_aggregate_recommended: after a hy_aggregate_hash of this thread -- 0: aggregate_rows is fine, b + 1: start on the partitioned path with b
// bits next time (the call ended there, or it met more groups than a workgroup's LDS table holds in an input of a few million rows).
// t_aggregate_next_path: set before a call -- b + 1 starts that call on the partitioned path with b bits (consumed by the call).
extern thread_local uint32_t t_aggregate_recommended, t_aggregate_next_path;

// exchange.hip: hy_column_export with the chunks' first rows given (device array [n_chunks], in elements; nullptr: the column's own)
hy_status export_column_at(const hy_column* column, void* values, uint8_t* nulls, const uint64_t* d_row_base);

// ---- join_star.hpp (join.hip): the probes of a star join fused into one pass over the fact table (hy_star_join_aggregate, plan.hip) ------
struct StarProbeFilter {       // one test of a conjunction, evaluated row by row where the table is walked anyway
  const hy_column* column;     // a plain data column of the table (Unencoded / FrameOfReference / Dictionary segments)
  const struct ScanJob* jobs;  // its per-chunk jobs in device memory (prepare_scan_jobs: a predicate's, or an IN list's)
  bool in_list;                // ... an IN list's
};
struct StarProbeDimension {
  const hy_column* key;        // the dimension's key column (int32, unique among `rows`)
  const hy_row_id* rows;       // the dimension rows that take part (device memory): the rows that pass its filters, or all of them -- or nullptr:
                               // every row of the key column's table that passes `filters` (tested by the kernels that build the dimension's tables)
  StarProbeFilter filters[HY_MAX_STAR_FILTERS];   // rows == nullptr: the dimension's filters
  uint32_t n_filters;          // ... 0: none
  uint64_t n_rows;             // how many -- or, with d_n_rows / a filter, at most how many
  const uint64_t* d_n_rows;    // the count in device memory (a scan's total that no host has read), or nullptr
  const hy_column* fact_key;   // the fact table's foreign key to this dimension
  bool want_rows;              // the caller reads columns of this dimension at the surviving rows
};
// fact_rows / dimension_rows[d]: the RowIDs of the fact table and of dimension d per row of fact JOIN dim_1 ... JOIN dim_k (Inner), in the
// fact table's row order.  *applicable = false: this shape is not for the fused probe (keys that are not int32 / not unique / too
// sparse, foreign-key segments the probe does not stream) -- nothing was produced.
// The plan's Projection + AggregateHash inside the join (star_finish, join_star.hpp): asked for with `finish`, answered in `groups` --
// groups->done: the join result was grouped where it was found (no RowIDs were written); otherwise the RowIDs are there as without it.
// n_groupby == 0: ONE group, reduced per workgroup and added to a single accumulator row (counts[0] == 0: the join result is empty).
// fact_filters: tests on the fact table's own columns, evaluated inside the probe pass before the dimensions are asked.
struct StarFinishColumnSpec { uint32_t table; const hy_column* column; };   // table 0 = the fact table, d + 1 = dimension d; column nullptr: none
struct StarFinishRequest {
  uint32_t n_groupby, n_aggregates;
  StarFinishColumnSpec groupby[4];
  struct { uint32_t function, op; StarFinishColumnSpec left, right; } aggregates[8];
};
struct StarFinishGroups {
  bool done = false;
  uint32_t n_groups = 0;
  uint32_t input_type[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // type of every aggregate's input value (HY_TYPE_INT / HY_TYPE_LONG)
  std::vector<uint64_t> keys, first, last, values, counts;   // [n][4], [n], [n], [n][8], [n]: first / last = row numbers of the join result
};
hy_status star_probe_rows(const StarProbeDimension* dimensions, uint32_t n_dimensions, DeviceBuffer& fact_rows, std::vector<std::unique_ptr<DeviceBuffer>>& dimension_rows,
                          uint64_t* n_rows, bool* applicable, const StarFinishRequest* finish = nullptr, StarFinishGroups* groups = nullptr,
                          const StarProbeFilter* fact_filters = nullptr, uint32_t n_fact_filters = 0);
hy_status star_all_rows_of(const hy_column* column, DeviceBuffer& rows);   // every row of a data column's table as a PosList
// scan.hip: the kernels of hy_poslist_translate queued on the current stream, nothing read back -- dense_offsets: [n_chunks + 1] device words,
// the last of them the number of RowIDs written
hy_status poslist_translate_queued(const hy_column* scanned, const hy_scan_result* result, uint32_t layout, hy_row_id* out, uint64_t capacity, uint64_t* dense_offsets);
// scan.hip: the chunk regions a scan with a HY_MEM_HOST result writes in device memory, and what regions_to_host_result takes behind them
// (`total` RowIDs: at most the scanned column's rows) -- laid out from the caller's Carver, for sizing and for carving alike
struct ScanRegions {
  hy_row_id* matches;
  uint64_t* offsets;
  uint32_t* counts;
  uint8_t* state;
};
struct DenseRegions {
  uint64_t* offsets;
  hy_row_id* matches;
};
void scan_regions_layout(Carver& carver, uint32_t n_chunks, uint64_t rows, ScanRegions& regions);
void dense_regions_layout(Carver& carver, uint32_t n_chunks, uint64_t total, DenseRegions& dense);
// scan.hip: a scan's chunk regions in device memory -> the caller's HY_MEM_HOST result (counts, chunk states, the regions packed back to back through the
// thread's scratch arena, behind what the scan carved from it: dense_regions_layout).  d_overflow: the scan's overflow word, or nullptr
hy_status regions_to_host_result(const hy_row_id* d_matches, const uint64_t* d_offsets, const uint32_t* d_counts, const uint8_t* d_state, uint32_t* d_overflow, uint32_t n_chunks,
                                 bool materialize_all, hy_scan_result* result);

}  // namespace hy

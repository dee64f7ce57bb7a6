// result_pool.hip -- device memory for operator RESULTS (PosLists of scans and joins) that outlives the call that wrote it.
//
// The reference's operators return tables whose ReferenceSegments share PosLists (table_scan.cpp:207-210, join_output_writing.cpp:95-200); a
// PosList lives as long as some table references it.  Behind `_on_execute()` the adapter keeps such PosLists in HBM (DevicePosList,
// hyrise_amd/host/hyrise_host.hpp), so their memory has the lifetime of a C++ object on the host -- not of a call --
// and comes from this pool: process-wide per device, blocks handed out again in stream order (a released block carries the event of the
// releasing thread's stream; the next owner's stream waits for it), hipMalloc only when nothing fits.
//
// A join writes TWO lists at the same pair index at the same time.  Where they lie decides pk_emit's speed by up to 20 % (DESIGN.md section 4.2,
// profiles/r04_join_placement.txt, r05_placement_probe.txt): the two streams should not meet in the same memory channels -- the second list starts
// 1.25 MiB past the 2 MiB grid the first starts on -- and which stretch of HBM an allocation landed in matters by itself.  hy_result_pool_calibrate
// is the policy bench.py used to run in Python (rounds 4-5): n candidate pairs, a few joins into each, the fastest stays in the pool as the pair
// hy_result_pool_acquire_pair prefers.
#include "hy_device.hpp"

#include <algorithm>
#include <cstring>

namespace hy {
namespace {

constexpr size_t PERIOD = size_t{2} << 20;       // the grid both lists of a pair start on ...
constexpr size_t PAIR_OFFSET = size_t{5} << 18;  // ... the second one 1.25 MiB past it
constexpr uint32_t UNRANKED = 0xFFFFFFFFu;

// A block owns its allocation and its event: new_block allocates, the first release on the block's own device creates the event, free_block
// destroys both.  It turns in_use in new_block and in take (once the wait is queued), and free in release / ~Calibration.
struct Block {
  void* base = nullptr;         // what hipMalloc returned; nullptr: a free slot
  char* user = nullptr;         // what callers get
  size_t usable = 0;            // bytes from `user` on
  int device = 0;
  bool in_use = false;
  bool paired = false;          // one list of a Pair
  hipEvent_t released = nullptr;   // recorded on the releasing thread's stream (created by the first release, not between allocations)
  bool pending = false;         // `released` marks work the next owner's stream waits for
};
struct Pair {
  int left = -1, right = -1;    // indices into g_blocks; left < 0: a dead entry, which the next new pair takes
  uint32_t rank = UNRANKED;     // calibration: 0 = the fastest candidate, 1 = the median one; uncalibrated pairs come after them
  bool dead() const { return left < 0; }
};

std::mutex g_mutex;
std::vector<Block> g_blocks;
std::vector<Pair> g_pairs;

// Readable bytes behind what a caller asked for: a list handed on as an HY_MEM_DEVICE column must not end its allocation (include/hyrise_amd.h,
// hy_column_create).  A fresh block has 0.75 MiB or more behind the request; a reused one is only taken if it keeps this much.
constexpr size_t RESULT_SLACK = 16;

int this_device() {
  bind_thread_device();
  int device = 0;
  (void)hipGetDevice(&device);
  return device;
}

// a fresh block, in use by the caller
hy_status new_block(size_t bytes, size_t offset_on_grid, bool paired, int* index) {
  Block b;
  b.device = this_device();
  const size_t padded = bytes + 2 * PERIOD;
  const hipError_t err = hipMalloc(&b.base, padded);
  if (err != hipSuccess) return fail(HY_ERR_DEVICE, "result pool: hipMalloc(%zu) failed: %s", padded, hipGetErrorString(err));
  char* base = static_cast<char*>(b.base);
  b.user = base + (PERIOD - reinterpret_cast<uintptr_t>(base) % PERIOD) % PERIOD + offset_on_grid;
  b.usable = padded - static_cast<size_t>(b.user - base);
  b.paired = paired;
  b.in_use = true;
  // a slot of a freed block is used again: indices stay valid
  for (size_t i = 0; i < g_blocks.size(); ++i) {
    if (!g_blocks[i].base) { g_blocks[i] = b; *index = static_cast<int>(i); return HY_OK; }
  }
  g_blocks.push_back(b);
  *index = static_cast<int>(g_blocks.size() - 1);
  return HY_OK;
}

void free_block(Block& b) {
  if (b.base) (void)hipFree(b.base);
  if (b.released) (void)hipEventDestroy(b.released);
  b = Block{};
}

// a pair of fresh blocks, both in use by the caller, in a dead entry of g_pairs or a new one; on failure nothing stays allocated
hy_status new_pair(size_t bytes, int* index) {
  int l = -1, r = -1;
  HY_TRY(new_block(bytes, 0, true, &l));
  const hy_status status = new_block(bytes, PAIR_OFFSET, true, &r);
  if (status != HY_OK) {
    free_block(g_blocks[l]);
    return status;
  }
  size_t p = 0;
  while (p < g_pairs.size() && !g_pairs[p].dead()) ++p;
  if (p == g_pairs.size()) g_pairs.emplace_back();
  g_pairs[p] = Pair{l, r, UNRANKED};
  *index = static_cast<int>(p);
  return HY_OK;
}

void drop_pair_locked(int p) {
  Pair& pair = g_pairs[p];
  if (pair.dead()) return;
  free_block(g_blocks[pair.left]);
  free_block(g_blocks[pair.right]);
  pair = Pair{};
}

// The new owner's launches come after whatever the last owners still had queued.  Every wait is queued before any block changes hands,
// so the blocks (both lists of a pair) are taken together or not at all.
hy_status take(std::initializer_list<Block*> blocks) {
  for (Block* b : blocks) {
    if (b->pending) HY_HIP(hipStreamWaitEvent(current_stream(), b->released, 0));
  }
  for (Block* b : blocks) {
    b->pending = false;
    b->in_use = true;
  }
  return HY_OK;
}

// What a calibration owns until it returns, whichever way it returns: its candidate pairs (in use while the joins write into them) and
// its two timing events.  At the end the stream is drained, the candidates marked `kept` go back to the pool free and the others are freed.
struct Calibration {
  struct Candidate { int pair; hy_row_id* left; hy_row_id* right; bool kept; };
  hipStream_t stream;
  std::vector<Candidate> candidates;
  hipEvent_t started = nullptr, stopped = nullptr;
  explicit Calibration(hipStream_t s) : stream(s) {}
  ~Calibration() {
    (void)hipStreamSynchronize(stream);
    if (started) (void)hipEventDestroy(started);
    if (stopped) (void)hipEventDestroy(stopped);
    const std::lock_guard<std::mutex> lock(g_mutex);
    for (const Candidate& c : candidates) {
      if (!c.kept) {
        drop_pair_locked(c.pair);
        continue;
      }
      g_blocks[g_pairs[c.pair].left].in_use = false;
      g_blocks[g_pairs[c.pair].right].in_use = false;
    }
  }
};

}  // namespace
}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_result_pool_acquire(uint64_t bytes, void** ptr) {
  if (!ptr) return fail(HY_ERR_INVALID, "hy_result_pool_acquire: null argument");
  *ptr = nullptr;
  const size_t wanted = static_cast<size_t>(std::max<uint64_t>(bytes, 256));
  const std::lock_guard<std::mutex> lock(g_mutex);
  const int device = this_device();
  int best = -1;
  for (size_t i = 0; i < g_blocks.size(); ++i) {
    const Block& b = g_blocks[i];
    if (!b.base || b.in_use || b.paired || b.device != device || b.usable < wanted + RESULT_SLACK || b.usable > 2 * wanted + (size_t{8} << 20)) continue;
    if (best < 0 || b.usable < g_blocks[best].usable) best = static_cast<int>(i);
  }
  if (best < 0) HY_TRY(new_block(wanted, 0, false, &best));
  else HY_TRY(take({&g_blocks[best]}));
  *ptr = g_blocks[best].user;
  return HY_OK;
}

hy_status hy_result_pool_acquire_pair(uint64_t rows, hy_row_id** left, hy_row_id** right) {
  if (!left || !right) return fail(HY_ERR_INVALID, "hy_result_pool_acquire_pair: null argument");
  *left = *right = nullptr;
  const size_t bytes = sizeof(hy_row_id) * static_cast<size_t>(std::max<uint64_t>(rows, 1));
  const std::lock_guard<std::mutex> lock(g_mutex);
  const int device = this_device();
  int best = -1;
  for (size_t p = 0; p < g_pairs.size(); ++p) {
    const Pair& pair = g_pairs[p];
    if (pair.dead()) continue;
    const Block& l = g_blocks[pair.left];
    const Block& r = g_blocks[pair.right];
    if (l.in_use || r.in_use || l.device != device || l.usable < bytes + RESULT_SLACK || r.usable < bytes + RESULT_SLACK) continue;
    // calibrated pairs first (by rank); among the others the tightest fit.  A pair sized for SF10's 480 MB lists is not spent on a
    // result of a few rows unless it is all there is: small results take blocks of their own (below)
    if (l.usable > 4 * bytes + (size_t{64} << 20)) continue;
    if (best < 0 || pair.rank < g_pairs[best].rank || (pair.rank == g_pairs[best].rank && l.usable < g_blocks[g_pairs[best].left].usable)) best = static_cast<int>(p);
  }
  if (best < 0) HY_TRY(new_pair(bytes, &best));
  else HY_TRY(take({&g_blocks[g_pairs[best].left], &g_blocks[g_pairs[best].right]}));
  *left = reinterpret_cast<hy_row_id*>(g_blocks[g_pairs[best].left].user);
  *right = reinterpret_cast<hy_row_id*>(g_blocks[g_pairs[best].right].user);
  return HY_OK;
}

hy_status hy_result_pool_release(void* ptr) {
  if (!ptr) return HY_OK;
  std::unique_lock<std::mutex> lock(g_mutex);
  size_t i = 0;
  while (i < g_blocks.size() && !(g_blocks[i].base && g_blocks[i].user == ptr)) ++i;
  if (i == g_blocks.size()) return fail(HY_ERR_INVALID, "hy_result_pool_release: not a buffer of the pool");
  if (!g_blocks[i].in_use) return fail(HY_ERR_INVALID, "hy_result_pool_release: the buffer is not in use");
  const int device = g_blocks[i].device;
  if (device == this_device()) {   // (every release of an operator's result: its last reference drops on a thread of its device)
    if (!g_blocks[i].released) HY_HIP(hipEventCreateWithFlags(&g_blocks[i].released, hipEventDisableTiming));
    HY_HIP(hipEventRecord(g_blocks[i].released, current_stream()));
    g_blocks[i].pending = true;
    g_blocks[i].in_use = false;
    return HY_OK;
  }
  // A thread of another device drops the last reference (a multi-GPU coordinator): its stream orders nothing on the block's device, and the
  // block's event cannot be recorded there.  Which streams of the block's device still read it is not known either, so the release waits for
  // that whole device -- outside the lock, which other devices' threads need meanwhile -- and leaves the block free with no event pending.
  // The caller's device is set back: its stream and pools belong to it.
  lock.unlock();
  int here = 0;
  HY_HIP(hipGetDevice(&here));
  HY_HIP(hipSetDevice(device));
  const hipError_t err = hipDeviceSynchronize();
  (void)hipSetDevice(here);
  if (err != hipSuccess) return fail(HY_ERR_DEVICE, "hy_result_pool_release: hipDeviceSynchronize on device %d failed: %s", device, hipGetErrorString(err));
  lock.lock();
  g_blocks[i].in_use = false;   // (index i: g_blocks may have grown meanwhile, but a block in use keeps its slot)
  return HY_OK;
}

hy_status hy_result_pool_trim(void) {
  const std::lock_guard<std::mutex> lock(g_mutex);
  const int device = this_device();
  HY_HIP(hipStreamSynchronize(current_stream()));
  for (size_t p = 0; p < g_pairs.size(); ++p) {
    if (g_pairs[p].dead()) continue;
    const Block& l = g_blocks[g_pairs[p].left];
    const Block& r = g_blocks[g_pairs[p].right];
    if (!l.in_use && !r.in_use && l.device == device) drop_pair_locked(static_cast<int>(p));
  }
  for (Block& b : g_blocks) {
    if (b.base && !b.in_use && !b.paired && b.device == device) free_block(b);
  }
  return HY_OK;
}

hy_status hy_result_pool_stats(uint64_t* held_bytes, uint64_t* in_use_bytes, uint32_t* calibrated_pairs) {
  const std::lock_guard<std::mutex> lock(g_mutex);
  uint64_t held = 0, used = 0;
  for (const Block& b : g_blocks) {
    if (!b.base) continue;
    held += b.usable;
    if (b.in_use) used += b.usable;
  }
  uint32_t calibrated = 0;
  for (const Pair& p : g_pairs) if (p.rank != UNRANKED) ++calibrated;   // (dead entries are unranked)
  if (held_bytes) *held_bytes = held;
  if (in_use_bytes) *in_use_bytes = used;
  if (calibrated_pairs) *calibrated_pairs = calibrated;
  return HY_OK;
}

hy_status hy_result_pool_calibrate(const hy_column* left, const hy_column* right, uint32_t mode, uint64_t rows, uint32_t candidates, uint32_t flags,
                                   float* ms_per_candidate, uint32_t* chosen) {
  if (!left || !right) return fail(HY_ERR_INVALID, "hy_result_pool_calibrate: null argument");
  if (candidates < 1 || candidates > 64) return fail(HY_ERR_INVALID, "hy_result_pool_calibrate: 1 .. 64 candidates");
  HY_TRY(on_this_device(left, "hy_result_pool_calibrate"));
  HY_TRY(on_this_device(right, "hy_result_pool_calibrate"));
  const bool one_list = mode == HY_JOIN_SEMI || mode == HY_JOIN_ANTI_NULL_AS_TRUE || mode == HY_JOIN_ANTI_NULL_AS_FALSE;
  const uint64_t capacity = std::max<uint64_t>(rows, 1);
  hipStream_t stream = current_stream();
  Calibration owned(stream);   // (declared before every lock below: its destructor takes the lock itself)
  {
    // candidates are NEW allocations (what is free in the pool already is not measured again: it keeps its rank)
    const std::lock_guard<std::mutex> lock(g_mutex);
    const size_t bytes = sizeof(hy_row_id) * static_cast<size_t>(capacity);
    for (uint32_t c = 0; c < candidates; ++c) {
      int p = -1;
      const hy_status status = new_pair(bytes, &p);
      if (status != HY_OK) {   // out of memory: calibrate over what there is
        if (owned.candidates.empty()) return status;
        break;
      }
      owned.candidates.push_back({p, reinterpret_cast<hy_row_id*>(g_blocks[g_pairs[p].left].user), reinterpret_cast<hy_row_id*>(g_blocks[g_pairs[p].right].user), false});
    }
  }
  DeviceBuffer slice_offsets, status_words;
  const uint32_t slice_capacity = static_cast<uint32_t>(capacity / 131070 + std::max(left->n_chunks, right->n_chunks) + 600);
  HY_TRY(slice_offsets.alloc(8 * (size_t{slice_capacity} + 2)));
  HY_TRY(status_words.alloc(sizeof(hy_join_status)));
  HY_HIP(hipEventCreate(&owned.started));
  HY_HIP(hipEventCreate(&owned.stopped));
  std::vector<float> times;
  constexpr int WARM = 3, TIMED = 4;
  for (const Calibration::Candidate& candidate : owned.candidates) {
    hy_join_result r;
    std::memset(&r, 0, sizeof(r));
    r.mem = HY_MEM_DEVICE;
    r.left_pos = candidate.left;
    r.right_pos = one_list ? candidate.left : candidate.right;
    r.capacity = capacity;
    r.slice_offsets = slice_offsets.as<uint64_t>();
    r.slice_capacity = slice_capacity;
    r.flags = HY_JOIN_ASYNC;
    r.status = status_words.as<hy_join_status>();
    hy_status outcome = HY_OK;
    for (int i = 0; i < WARM + TIMED && outcome == HY_OK; ++i) {   // (the first joins also leave the build column's key hint behind)
      if (i == WARM) (void)hipEventRecord(owned.started, stream);
      r.radix_bits = 0xFFFFFFFFu;
      outcome = hy_join_hash(left, right, mode, &r);
    }
    (void)hipEventRecord(owned.stopped, stream);
    if (outcome == HY_OK) outcome = hy_join_hash_finish(left, right, mode, &r);
    if (outcome != HY_OK) return outcome;
    (void)hipEventSynchronize(owned.stopped);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, owned.started, owned.stopped);
    times.push_back(ms / TIMED);
  }
  std::vector<size_t> order(times.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return times[a] < times[b]; });
  const size_t best = order[0], median = order[order.size() / 2];
  const std::lock_guard<std::mutex> lock(g_mutex);
  for (size_t c = 0; c < owned.candidates.size(); ++c) {
    if (ms_per_candidate) ms_per_candidate[c] = times[c];
    Calibration::Candidate& candidate = owned.candidates[c];
    if (c == best) {
      // earlier calibrations' winners give way: the newest measurement decides what acquire_pair prefers
      for (Pair& other : g_pairs) if (other.rank == 0) other.rank = 2;
      g_pairs[candidate.pair].rank = 0;
      candidate.kept = true;
    } else if (c == median && (flags & HY_POOL_KEEP_MEDIAN)) {
      for (Pair& other : g_pairs) if (other.rank == 1) other.rank = 3;
      g_pairs[candidate.pair].rank = 1;
      candidate.kept = true;
    }
  }
  for (size_t c = owned.candidates.size(); c < candidates; ++c) if (ms_per_candidate) ms_per_candidate[c] = 0.f;
  if (chosen) *chosen = static_cast<uint32_t>(best);
  return HY_OK;
}

}  // extern "C"

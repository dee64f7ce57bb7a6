// string_join_keys.hip -- the keys two string columns of two tables join on, made in HBM (hy_string_dictionary_order_pair,
// hy_string_dictionary_join_ids, hy_column_string_join_keys).
//
//   rank(entry) = the number of DISTINCT strings, over all chunks of the left AND the right dictionary, smaller than the entry
//   id(entry)   = (int64(rank) + 1) << 20 | (std::hash & 0xFFFFF)
//
// Equal strings on either side get equal keys.  The ranks are what hy_join_sort_merge and hy_join_nested_loop compare; the ids are what
// hy_join_hash takes for pmr_string keys (hyrise_amd/join_keys.py, the mirror's string_join_id): a unique number above bit 20 and the low 20
// bits of libstdc++'s hash, from which the reference takes its radix partition and its Bloom index.
//
// The joint order is string_order.hip's merge sequence over the chunks of both dictionaries laid end to end -- left's chunks are runs
// 0 .. n_l - 1, right's follow.  The sequence reads nothing but a LikeChunk table, a LikeBlock table and entry offsets, so the joint tables
// are built here per call, on the host, and uploaded into the thread's scratch arena: the hy_string_dictionary objects are const and shared.
//
// string_join_ids, ONE launch: a workgroup owns the 256 entries of one joint LikeBlock, a lane one entry.  It hashes exactly the entry's
// bytes (_Hash_bytes, libsupc++/hash_bytes.cc: seed 0xc70f6907, 8-byte little-endian words read at whatever byte address the entry has, a
// tail of 1-7 bytes assembled from unsigned bytes, two final shift-mixes), reads the entry's rank and writes one int64.  No byte outside
// the entry is read.  The dependent 64-bit multiplies bound it; next to the merge rounds that is nothing.
#include "hy_device.hpp"
#include "string_entries.hpp"

#include <algorithm>
#include <vector>

namespace hy {

namespace {

constexpr uint32_t IDS_WG = 256;   // = like.hip's LIKE_WG: the block table's unit

struct JoinIdArgs {
  const LikeChunk* chunks;          // the joint tables
  const LikeBlock* blocks;
  const uint64_t* entry_offsets;
  const int32_t* ranks;             // [total], by joint position
  int64_t* left_ids;                // positions below split
  int64_t* right_ids;               // the others, at position - split
  uint64_t split;
};

__device__ __forceinline__ uint64_t load_word64(const uint8_t* p) {   // eight bytes at any address, first byte least significant
  uint64_t w;
  __builtin_memcpy(&w, p, 8);
  return w;
}

__device__ __forceinline__ uint64_t shift_mix(uint64_t v) { return v ^ (v >> 47); }

__device__ __forceinline__ uint64_t hash_bytes(const Entry& e) {
  constexpr uint64_t mul = (uint64_t{0xc6a4a793} << 32) + uint64_t{0x5bd1e995};
  const uint32_t aligned = e.length & ~7u;
  uint64_t hash = uint64_t{0xc70f6907} ^ (uint64_t{e.length} * mul);
  for (uint32_t p = 0; p < aligned; p += 8) {
    hash ^= shift_mix(load_word64(e.bytes + p) * mul) * mul;
    hash *= mul;
  }
  if (e.length & 7) {
    uint64_t tail = 0;
    for (uint32_t n = e.length & 7; n-- > 0;) tail = (tail << 8) + e.bytes[aligned + n];
    hash ^= tail;
    hash *= mul;
  }
  hash = shift_mix(hash) * mul;
  return shift_mix(hash);
}

__global__ __launch_bounds__(IDS_WG) void string_join_ids(JoinIdArgs a) {
  const LikeBlock block = a.blocks[blockIdx.x];
  const LikeChunk chunk = a.chunks[block.chunk];
  const uint32_t v = block.first_entry + threadIdx.x;
  if (v >= chunk.n_entries) return;
  const uint64_t hash = hash_bytes(entry_of(chunk, v, chunk_bytes(chunk)));
  const uint64_t position = a.entry_offsets[block.chunk] + v;
  const int64_t id = (int64_t{a.ranks[position]} + 1) << 20 | static_cast<int64_t>(hash & 0xFFFFF);
  if (position >= a.split) a.right_ids[position - a.split] = id;
  else a.left_ids[position] = id;
}

// The joint tables on the host: left's chunks, then right's
struct JointTables {
  std::vector<LikeChunk> chunks;
  std::vector<LikeBlock> blocks;
  std::vector<uint64_t> entry_offsets;
  uint64_t split = 0, total = 0;
  JointTables(const hy_string_dictionary* left, const hy_string_dictionary* right) {
    chunks.reserve(size_t{left->n_chunks} + right->n_chunks);
    blocks.reserve(left->blocks.size() + right->blocks.size());
    entry_offsets.reserve(size_t{left->n_chunks} + right->n_chunks + 1);
    chunks.insert(chunks.end(), left->chunks.begin(), left->chunks.end());
    chunks.insert(chunks.end(), right->chunks.begin(), right->chunks.end());
    blocks.insert(blocks.end(), left->blocks.begin(), left->blocks.end());
    for (const LikeBlock& block : right->blocks) blocks.push_back(LikeBlock{block.chunk + left->n_chunks, block.first_entry});
    split = left->entry_offsets[left->n_chunks];
    total = split + right->entry_offsets[right->n_chunks];
    entry_offsets.insert(entry_offsets.end(), left->entry_offsets.begin(), left->entry_offsets.end());   // (n_l + 1 of them: the last is `split`)
    for (uint32_t c = 1; c <= right->n_chunks; ++c) entry_offsets.push_back(split + right->entry_offsets[c]);
  }
};

// what join_keys_launch reads and writes in the scratch arena: the joint tables, the merge's temporaries for the joint total, the ranks behind the ids
struct JoinKeyBlocks {
  LikeChunk* chunks;
  LikeBlock* blocks;
  uint64_t* entry_offsets;
  int32_t* joint_ranks;   // with ids
  MergeBlocks merge;
};

void join_keys_layout(Carver& carver, const JointTables& tables, bool ids, JoinKeyBlocks& b) {
  b.chunks = carver.take<LikeChunk>(tables.chunks.size());
  b.blocks = carver.take<LikeBlock>(tables.blocks.size());
  b.entry_offsets = carver.take<uint64_t>(tables.entry_offsets.size());
  b.joint_ranks = ids ? carver.take<int32_t>(tables.total) : nullptr;
  merge_layout(carver, tables.total, b.merge);
}

// Queues everything on `stream`: the tables' upload, the joint order and, with `ids`, string_join_ids.  d_left / d_right: int32 ranks, or
// int64 ids, in the layout of hy_string_dictionary_order per side.  tables.total > 0.
hy_status join_keys_launch(const JointTables& tables, bool ids, const JoinKeyBlocks& b, void* d_left, void* d_right, hipStream_t stream) {
  // (pageable memory: copied before the calls return)
  HY_HIP(hipMemcpyAsync(b.chunks, tables.chunks.data(), sizeof(LikeChunk) * tables.chunks.size(), hipMemcpyHostToDevice, stream));
  HY_HIP(hipMemcpyAsync(b.blocks, tables.blocks.data(), sizeof(LikeBlock) * tables.blocks.size(), hipMemcpyHostToDevice, stream));
  HY_HIP(hipMemcpyAsync(b.entry_offsets, tables.entry_offsets.data(), 8 * tables.entry_offsets.size(), hipMemcpyHostToDevice, stream));
  const PairTables pair{b.chunks, b.blocks, b.entry_offsets, static_cast<uint32_t>(tables.chunks.size()), static_cast<uint32_t>(tables.blocks.size()), tables.total, tables.split};
  if (!ids) return pair_order_launch(pair, b.merge, static_cast<int32_t*>(d_left), static_cast<int32_t*>(d_right), stream);
  HY_TRY(pair_order_launch(pair, b.merge, b.joint_ranks, b.joint_ranks + tables.split, stream));
  const JoinIdArgs args{b.chunks, b.blocks, b.entry_offsets, b.joint_ranks, static_cast<int64_t*>(d_left), static_cast<int64_t*>(d_right), tables.split};
  profile_begin(stream, HY_KERNEL_STRING_RANK);
  hipLaunchKernelGGL(string_join_ids, dim3(pair.n_blocks), dim3(IDS_WG), 0, stream, args);
  profile_end(stream);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

// The refusals of a pair of dictionaries, before any launch and any allocation
hy_status pair_check(const hy_string_dictionary* left, const hy_string_dictionary* right, const char* name) {
  if (left->device != right->device) return fail(HY_ERR_INVALID, "%s: the left dictionary lives on device %d, the right one on device %d", name, left->device, right->device);
  HY_TRY(dictionary_device_check(left, name));
  HY_TRY(entries_fit_ranks(left->entry_offsets[left->n_chunks] + right->entry_offsets[right->n_chunks], name));
  if (left->blocks.size() + right->blocks.size() > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups of entries", name);
  return HY_OK;
}

// hy_string_dictionary_order_pair (width 4) and hy_string_dictionary_join_ids (width 8)
hy_status dictionary_keys(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem, void* left_out, void* right_out, uint32_t* n_distinct, bool ids,
                          const char* name) {
  const size_t width = ids ? 8 : 4;
  if (!left || !right || !left_out || !right_out) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (mem != HY_MEM_HOST && mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "%s: bad memory space %u", name, mem);
  HY_TRY(pair_check(left, right, name));
  if (mem == HY_MEM_DEVICE && (reinterpret_cast<uintptr_t>(left_out) % width != 0 || reinterpret_cast<uintptr_t>(right_out) % width != 0))
    return fail(HY_ERR_INVALID, "%s: %s not on a %zu-byte boundary", name, ids ? "ids" : "ranks", width);
  const JointTables tables(left, right);
  if (!tables.total) {
    if (n_distinct) *n_distinct = 0;
    return HY_OK;
  }
  hipStream_t stream = current_stream();
  const bool host = mem == HY_MEM_HOST;
  JoinKeyBlocks blocks;
  char* d_twin = nullptr;
  HY_TRY(reserve_and_carve([&](Carver& carver) {
    if (host) d_twin = static_cast<char*>(carver.take_bytes(width * tables.total));
    join_keys_layout(carver, tables, ids, blocks);
  }));
  char* d_left = host ? d_twin : static_cast<char*>(left_out);
  char* d_right = host ? d_twin + width * tables.split : static_cast<char*>(right_out);
  HY_TRY(join_keys_launch(tables, ids, blocks, d_left, d_right, stream));
  const TwinPart parts[2] = {{left_out, d_left, width * tables.split}, {right_out, d_right, width * (tables.total - tables.split)}};
  return outputs_to_caller(mem, parts, 2, blocks.merge.n_distinct, n_distinct, stream);
}

}  // namespace

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_string_dictionary_order_pair(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem, int32_t* left_ranks, int32_t* right_ranks,
                                          uint32_t* n_distinct) {
  return dictionary_keys(left, right, mem, left_ranks, right_ranks, n_distinct, false, "hy_string_dictionary_order_pair");
}

hy_status hy_string_dictionary_join_ids(const hy_string_dictionary* left, const hy_string_dictionary* right, uint32_t mem, int64_t* left_ids, int64_t* right_ids) {
  return dictionary_keys(left, right, mem, left_ids, right_ids, nullptr, true, "hy_string_dictionary_join_ids");
}

hy_status hy_column_string_join_keys(const hy_column* left, const hy_string_dictionary* left_dict, const hy_column* right, const hy_string_dictionary* right_dict, uint32_t kind,
                                     hy_column** left_out, hy_column** right_out) {
  const char* name = "hy_column_string_join_keys";
  if (left_out) *left_out = nullptr;
  if (right_out) *right_out = nullptr;
  if (!left_out || !right_out) return fail(HY_ERR_INVALID, "%s: null output", name);
  if (!left || !left_dict || !right || !right_dict) return fail(HY_ERR_INVALID, "%s: null argument", name);
  if (kind != HY_STRING_KEYS_RANKS && kind != HY_STRING_KEYS_HASH_IDS) return fail(HY_ERR_INVALID, "%s: unknown kind of keys %u", name, kind);
  HY_TRY(string_column_check(left, left_dict, name));
  HY_TRY(string_column_check(right, right_dict, name));
  HY_TRY(pair_check(left_dict, right_dict, name));
  const bool ids = kind == HY_STRING_KEYS_HASH_IDS;
  const size_t width = ids ? 8 : 4;
  const JointTables tables(left_dict, right_dict);

  // the keys: one buffer per side, which that side's stand-in owns (16 bytes of slack behind the last key, like every dictionary of a column)
  hipStream_t stream = current_stream();
  KeyColumn left_keys, right_keys;
  auto give_up = [&](hy_status status) {
    (void)hipStreamSynchronize(stream);
    left_keys.drop();
    right_keys.drop();
    return status;
  };
  HY_TRY(left_keys.alloc(align_up(width * tables.split + 16, 256)));
  hy_status status = right_keys.alloc(align_up(width * (tables.total - tables.split) + 16, 256));
  if (status != HY_OK) return give_up(status);
  if (tables.total) {
    JoinKeyBlocks blocks;
    status = reserve_and_carve([&](Carver& carver) { join_keys_layout(carver, tables, ids, blocks); });
    if (status == HY_OK) status = join_keys_launch(tables, ids, blocks, left_keys.d_keys, right_keys.d_keys, stream);
    if (status != HY_OK) return give_up(status);
  }
  const uint32_t data_type = ids ? HY_TYPE_LONG : HY_TYPE_INT;
  status = left_keys.make_stand_in(left, left_dict, data_type);
  if (status == HY_OK) status = right_keys.make_stand_in(right, right_dict, data_type);
  if (status != HY_OK) return give_up(status);
  // (the dictionaries may die as soon as the call has returned: nothing queued reads them any more)
  const hipError_t err = hipStreamSynchronize(stream);
  if (err != hipSuccess) return give_up(fail(HY_ERR_DEVICE, "%s: making the keys failed: %s", name, hipGetErrorString(err)));
  *left_out = left_keys.stand_in;
  *right_out = right_keys.stand_in;
  return HY_OK;
}

}  // extern "C"

// like.hip -- the LIKE family's dictionary pass on the device (ColumnLikeTableScanImpl::_find_matches_in_dictionary,
// column_like_table_scan_impl.cpp:142-159): the dictionaries of a column's DictionarySegment<pmr_string> chunks live in HBM beside the
// attribute vectors (hy_string_dictionary), the matcher writes the per-chunk bitmaps over value ids that the scan kernels test
// (KIND_VALUE_ID_SET, scan.hip), and no string is looked at by the host.
//
// like_match, ONE launch per pattern: a workgroup owns 256 consecutive entries of one chunk (LikeBlock, a host-built table), a lane one
// entry, so a wave's ballot IS one bitmap word; lane 0 of the wave stores it (one 8-byte vector store).  Lanes past the chunk's last
// entry vote "no": the tail bits of a chunk's last word are zero under the NOT forms too.
// The entries of a workgroup are contiguous in `chars`: their byte range is staged into LDS with 16-byte loads at 16-byte-aligned global
// addresses (the LDS image keeps the range's address modulo 16; the one vector that begins in front of the range is read byte by byte, the
// last one ends inside the 16 bytes of slack every buffer has), and the lanes match out of LDS.  A range beyond STAGE_BYTES -- one
// 100 KB string among short ones -- is read from global memory in place; the choice is per workgroup and changes no result.
// The matching loop is the mirror's (LikeMatcher, hyrise_host.hpp): two pointers with one backtracking point, the last `%`.  The pattern
// arrives tokenised as a kernel argument (like_program) and is copied to LDS once per workgroup, because every lane indexes it on its own.
#include "hy_device.hpp"

#include <algorithm>
#include <cstring>

namespace hy {

namespace {

constexpr uint32_t LIKE_WG = 256;
constexpr uint32_t STAGE_BYTES = 32 * 1024;   // LDS per workgroup for the entries' bytes: 128 per entry on average, four workgroups per CU

struct LikeArgs {
  const LikeChunk* chunks;
  const LikeBlock* blocks;
  uint64_t* words;
};

// text(i): byte i of the entry.  tokens: in LDS.
template <typename Text>
__device__ __forceinline__ bool like_matches(const Text& text, uint32_t length, const uint16_t* tokens, uint32_t n_tokens, bool fold) {
  uint32_t t = 0, p = 0, star = 0xFFFFFFFFu, resume = 0;
  while (t < length) {
    const uint32_t token = p < n_tokens ? tokens[p] : 0xFFFFu;   // (0xFFFF: the pattern is used up -- equals no byte)
    if (token == LIKE_ANY_RUN) { star = p++; resume = t; continue; }
    uint32_t c = text(t);
    if (fold && c - 'A' < 26u) c += 'a' - 'A';
    if (token == LIKE_ANY_ONE || token == c) { ++p; ++t; }
    else if (star != 0xFFFFFFFFu) { p = star + 1; t = ++resume; }
    else return false;
  }
  while (p < n_tokens && tokens[p] == LIKE_ANY_RUN) ++p;
  return p == n_tokens;
}

template <typename Text>
__device__ __forceinline__ bool entry_matches(const Text& text, uint32_t slot_bytes, bool fixed, const uint16_t* tokens, const LikeProgram& program) {
  uint32_t length = slot_bytes;
  if (fixed) {   // FixedString: strnlen(slot, L), fixed_string.cpp:86-99
    length = 0;
    while (length < slot_bytes && text(length) != 0) ++length;
  }
  return like_matches(text, length, tokens, program.n_tokens, program.insensitive != 0);
}

__global__ __launch_bounds__(LIKE_WG) void like_match(LikeArgs a, LikeProgram program) {
  __shared__ __attribute__((aligned(16))) uint8_t s_text[STAGE_BYTES];
  __shared__ uint16_t s_tokens[HY_MAX_LIKE_PATTERN];
  const uint32_t tid = threadIdx.x;
  const LikeBlock block = a.blocks[blockIdx.x];
  const LikeChunk chunk = a.chunks[block.chunk];
  if (tid < program.n_tokens) s_tokens[tid] = program.tokens[tid];
  const uint32_t first = block.first_entry;
  const uint32_t n = min(LIKE_WG, chunk.n_entries - first);
  const bool fixed = chunk.offsets == nullptr;
  // the byte range of the workgroup's entries (a chunk's chars stay below 2^32 bytes: hy_string_dictionary_create)
  uint32_t begin = fixed ? first * chunk.string_length : chunk.offsets[first];
  uint32_t end = fixed ? (first + n) * chunk.string_length : chunk.offsets[first + n];
  if (end < begin) end = begin;
  const uint32_t range = end - begin;
  const char* base = chunk.chars + begin;
  const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(base)) & 15u;
  const bool staged = uint64_t{shift} + range <= STAGE_BYTES;   // (workgroup-uniform)
  if (staged) {
    const char* aligned = base - shift;
    const uint32_t vectors = (shift + range + 15) / 16;
    for (uint32_t v = tid; v < vectors; v += LIKE_WG) {
      if (v == 0 && shift) {   // begins in front of the range (perhaps in front of the buffer): only the range's bytes are read
        for (uint32_t b = shift; b < 16 && b < shift + range; ++b) s_text[b] = static_cast<uint8_t>(base[b - shift]);
      } else {
        *reinterpret_cast<uint4*>(s_text + 16 * v) = *reinterpret_cast<const uint4*>(aligned + 16 * size_t{v});
      }
    }
  }
  __syncthreads();

  bool hit = false;
  if (tid < n) {
    const uint32_t entry = first + tid;
    uint32_t from = fixed ? entry * chunk.string_length : chunk.offsets[entry];
    uint32_t to = fixed ? from + chunk.string_length : chunk.offsets[entry + 1];
    from = min(max(from, begin), end);   // (offsets that do not ascend read nothing outside the workgroup's range)
    to = min(max(to, from), end);
    if (staged) {
      const uint8_t* text = s_text + shift + (from - begin);
      hit = entry_matches([text](uint32_t i) -> uint32_t { return text[i]; }, to - from, fixed, s_tokens, program);
    } else {
      const uint8_t* text = reinterpret_cast<const uint8_t*>(chunk.chars) + from;
      hit = entry_matches([text](uint32_t i) -> uint32_t { return text[i]; }, to - from, fixed, s_tokens, program);
    }
    hit = hit != (program.negated != 0);
  }
  const uint64_t word = __ballot(hit);
  if ((tid & 63u) == 0 && tid < n) a.words[chunk.first_word + ((first + tid) >> 6)] = word;
}

bool like_condition(uint32_t condition) { return condition >= HY_PRED_LIKE && condition <= HY_PRED_NOT_LIKE_INSENSITIVE; }

}  // namespace

hy_status like_program(const char* pattern, uint32_t pattern_bytes, uint32_t condition, LikeProgram* program, const char* entry_point) {
  if (!like_condition(condition)) return fail(HY_ERR_INVALID, "%s: condition %u is none of LIKE / NOT LIKE / their insensitive forms", entry_point, condition);
  if (pattern_bytes && !pattern) return fail(HY_ERR_INVALID, "%s: null pattern", entry_point);
  if (pattern_bytes > HY_MAX_LIKE_PATTERN) return fail(HY_ERR_UNSUPPORTED, "%s: a pattern of %u bytes (more than HY_MAX_LIKE_PATTERN) stays with the host matcher", entry_point, pattern_bytes);
  std::memset(program, 0, sizeof(*program));
  program->insensitive = condition == HY_PRED_LIKE_INSENSITIVE || condition == HY_PRED_NOT_LIKE_INSENSITIVE;
  program->negated = condition == HY_PRED_NOT_LIKE || condition == HY_PRED_NOT_LIKE_INSENSITIVE;
  for (uint32_t i = 0; i < pattern_bytes; ++i) {
    uint8_t c = static_cast<uint8_t>(pattern[i]);
    if (c == '%') {
      if (program->n_tokens && program->tokens[program->n_tokens - 1] == LIKE_ANY_RUN) continue;   // `%%` is `%`
      program->tokens[program->n_tokens++] = LIKE_ANY_RUN;
    } else if (c == '_') {
      program->tokens[program->n_tokens++] = LIKE_ANY_ONE;
    } else {
      if (program->insensitive && c >= 'A' && c <= 'Z') c = static_cast<uint8_t>(c - 'A' + 'a');
      program->tokens[program->n_tokens++] = c;
    }
  }
  return HY_OK;
}

hy_status like_dictionary_tables(const hy_string_dictionary* dict) {
  std::lock_guard<std::mutex> lock(dict->tables_mutex);
  if (dict->d_word_offsets) return HY_OK;
  const size_t chunk_bytes = align_up(sizeof(LikeChunk) * std::max<size_t>(1, dict->chunks.size()), 256);
  const size_t block_bytes = align_up(sizeof(LikeBlock) * std::max<size_t>(1, dict->blocks.size()), 256);
  const size_t offset_bytes = 8 * dict->word_offsets.size();
  std::vector<char> image(chunk_bytes + block_bytes + 2 * offset_bytes, 0);
  if (!dict->chunks.empty()) std::memcpy(image.data(), dict->chunks.data(), sizeof(LikeChunk) * dict->chunks.size());
  if (!dict->blocks.empty()) std::memcpy(image.data() + chunk_bytes, dict->blocks.data(), sizeof(LikeBlock) * dict->blocks.size());
  std::memcpy(image.data() + chunk_bytes + block_bytes, dict->word_offsets.data(), offset_bytes);
  std::memcpy(image.data() + chunk_bytes + block_bytes + offset_bytes, dict->entry_offsets.data(), offset_bytes);
  bind_thread_device();
  char* tables = nullptr;
  HY_HIP(hipMalloc(reinterpret_cast<void**>(&tables), image.size()));
  dict->owned.push_back(tables);
  HY_HIP(hipMemcpy(tables, image.data(), image.size(), hipMemcpyHostToDevice));   // (complete before any stream of any thread reads it)
  dict->d_chunks = reinterpret_cast<LikeChunk*>(tables);
  dict->d_blocks = reinterpret_cast<LikeBlock*>(tables + chunk_bytes);
  dict->d_entry_offsets = reinterpret_cast<uint64_t*>(tables + chunk_bytes + block_bytes + offset_bytes);
  dict->d_word_offsets = reinterpret_cast<uint64_t*>(tables + chunk_bytes + block_bytes);
  return HY_OK;
}

hy_status like_launch(const hy_string_dictionary* dict, const LikeProgram& program, uint64_t* d_words, hipStream_t stream) {
  HY_TRY(like_dictionary_tables(dict));
  if (dict->blocks.empty()) return HY_OK;
  LikeArgs args{dict->d_chunks, dict->d_blocks, d_words};
  hipEvent_t started = nullptr, stopped = nullptr;
  profile_events(&started, &stopped, HY_KERNEL_LIKE);
  hipExtLaunchKernelGGL(like_match, dim3(static_cast<uint32_t>(dict->blocks.size())), dim3(LIKE_WG), 0, stream, started, stopped, 0, args, program);
  HY_HIP(hipGetLastError());
  return HY_OK;
}

}  // namespace hy

using namespace hy;

extern "C" {

hy_status hy_like_tokenize(const char* pattern, uint32_t pattern_bytes, uint32_t condition, uint16_t* tokens, uint32_t* n_tokens) {
  if (!tokens || !n_tokens) return fail(HY_ERR_INVALID, "hy_like_tokenize: null argument");
  *n_tokens = 0;
  LikeProgram program;
  HY_TRY(like_program(pattern, pattern_bytes, condition, &program, "hy_like_tokenize"));
  std::memcpy(tokens, program.tokens, sizeof(uint16_t) * program.n_tokens);
  *n_tokens = program.n_tokens;
  return HY_OK;
}

hy_status hy_string_dictionary_create(const hy_string_dictionary_chunk* chunks, uint32_t n_chunks, uint32_t mem, hy_string_dictionary** out) {
  if (!out) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: null output");
  *out = nullptr;
  if (n_chunks && !chunks) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: null chunks");
  if (mem != HY_MEM_HOST && mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: bad memory space %u", mem);
  // sizes first: nothing is allocated for a dictionary that is refused
  std::vector<uint64_t> char_bytes(n_chunks, 0);
  uint64_t n_blocks = 0;
  size_t allocation = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const hy_string_dictionary_chunk& chunk = chunks[c];
    const uint32_t n = chunk.n_entries;
    n_blocks += (uint64_t{n} + LIKE_WG - 1) / LIKE_WG;
    if (!n) continue;
    if (chunk.offsets) {
      if (reinterpret_cast<uintptr_t>(chunk.offsets) % 4 != 0) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: chunk %u: offsets not on a 4-byte boundary", c);
      if (mem == HY_MEM_HOST) {
        for (uint32_t i = 0; i < n; ++i)
          if (chunk.offsets[i] > chunk.offsets[i + 1]) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: chunk %u: offsets[%u] > offsets[%u]", c, i, i + 1);
        char_bytes[c] = chunk.offsets[n];
      }
    } else {
      char_bytes[c] = uint64_t{n} * chunk.string_length;
      if (char_bytes[c] >= (uint64_t{1} << 32)) return fail(HY_ERR_UNSUPPORTED, "hy_string_dictionary_create: chunk %u: %u x %u bytes of chars do not fit 32-bit offsets", c, n, chunk.string_length);
    }
    if (char_bytes[c] && !chunk.chars) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: chunk %u: null chars", c);
    // caller-owned offsets are not read here, so whether every entry is empty is unknown: the chunk needs its chars
    if (mem == HY_MEM_DEVICE && chunk.offsets && !chunk.chars) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: chunk %u: null chars", c);
    if (!chunk.offsets && chunk.string_length && !chunk.chars) return fail(HY_ERR_INVALID, "hy_string_dictionary_create: chunk %u: null chars", c);
    allocation += align_up(char_bytes[c] + 16, 256) + (chunk.offsets ? align_up(4 * (size_t{n} + 1) + 16, 256) : 0);
  }
  if (n_blocks > 0x7FFFFFFFull) return fail(HY_ERR_UNSUPPORTED, "hy_string_dictionary_create: more than 2^31 workgroups of entries");

  auto dict = std::make_unique<hy_string_dictionary>();
  dict->n_chunks = n_chunks;
  dict->mem = mem;
  dict->device = this_thread_device();
  dict->chunks.resize(n_chunks);
  dict->word_offsets.assign(size_t{n_chunks} + 1, 0);
  dict->entry_offsets.assign(size_t{n_chunks} + 1, 0);
  dict->chars_bytes.assign(n_chunks, ~0ull);
  for (uint32_t c = 0; c < n_chunks; ++c) if (mem == HY_MEM_HOST || !chunks[c].n_entries) dict->chars_bytes[c] = char_bytes[c];
  dict->blocks.reserve(n_blocks);
  char* cursor = nullptr;
  if (mem == HY_MEM_HOST && allocation) {
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&cursor), allocation);
    if (err != hipSuccess) return fail(HY_ERR_DEVICE, "hy_string_dictionary_create: hipMalloc(%zu) failed: %s", allocation, hipGetErrorString(err));
    dict->owned.push_back(cursor);
  }
  hy_status status = HY_OK;
  for (uint32_t c = 0; c < n_chunks && status == HY_OK; ++c) {
    const hy_string_dictionary_chunk& chunk = chunks[c];
    const uint32_t n = chunk.n_entries;
    LikeChunk& d = dict->chunks[c];
    d.n_entries = n;
    d.string_length = chunk.offsets ? 0 : chunk.string_length;
    d.first_word = dict->word_offsets[c];
    dict->word_offsets[c + 1] = dict->word_offsets[c] + (uint64_t{n} + 63) / 64;
    dict->entry_offsets[c + 1] = dict->entry_offsets[c] + n;
    for (uint32_t first = 0; first < n; first += LIKE_WG) dict->blocks.push_back(LikeBlock{c, first});
    if (!n) continue;
    if (mem == HY_MEM_DEVICE) {
      d.chars = chunk.chars;
      d.offsets = chunk.offsets;
      continue;
    }
    d.chars = cursor;
    if (char_bytes[c] && hipMemcpy(cursor, chunk.chars, char_bytes[c], hipMemcpyHostToDevice) != hipSuccess) status = HY_ERR_DEVICE;
    cursor += align_up(char_bytes[c] + 16, 256);
    if (chunk.offsets) {
      d.offsets = reinterpret_cast<const uint32_t*>(cursor);
      if (hipMemcpy(cursor, chunk.offsets, 4 * (size_t{n} + 1), hipMemcpyHostToDevice) != hipSuccess) status = HY_ERR_DEVICE;
      cursor += align_up(4 * (size_t{n} + 1) + 16, 256);
    }
  }
  if (status != HY_OK) {
    for (void* p : dict->owned) (void)hipFree(p);
    return fail(status, "hy_string_dictionary_create: the upload failed: %s", hipGetErrorString(hipGetLastError()));
  }
  *out = dict.release();
  return HY_OK;
}

hy_status hy_string_dictionary_destroy(hy_string_dictionary* dict) {
  if (!dict) return HY_OK;
  for (void* p : dict->owned) (void)hipFree(p);
  delete dict;
  return HY_OK;
}

hy_status hy_string_dictionary_match_layout(const hy_string_dictionary* dict, uint64_t* word_offsets) {
  if (!dict || !word_offsets) return fail(HY_ERR_INVALID, "hy_string_dictionary_match_layout: null argument");
  std::memcpy(word_offsets, dict->word_offsets.data(), 8 * dict->word_offsets.size());
  return HY_OK;
}

hy_status hy_like_matches(const hy_string_dictionary* dict, const char* pattern, uint32_t pattern_bytes, uint32_t condition, uint32_t mem, uint64_t* match_words) {
  if (!dict || !match_words) return fail(HY_ERR_INVALID, "hy_like_matches: null argument");
  if (mem != HY_MEM_HOST && mem != HY_MEM_DEVICE) return fail(HY_ERR_INVALID, "hy_like_matches: bad memory space %u", mem);
  LikeProgram program;
  HY_TRY(like_program(pattern, pattern_bytes, condition, &program, "hy_like_matches"));
  if (mem == HY_MEM_DEVICE && reinterpret_cast<uintptr_t>(match_words) % 8 != 0) return fail(HY_ERR_INVALID, "hy_like_matches: match_words not on an 8-byte boundary");
  HY_TRY(dictionary_device_check(dict, "hy_like_matches"));
  const uint64_t total_words = dict->word_offsets[dict->n_chunks];
  if (!total_words) return HY_OK;
  hipStream_t stream = current_stream();
  if (mem == HY_MEM_DEVICE) return like_launch(dict, program, match_words, stream);   // (complete in the order of the calling thread's stream)
  Scratch& sc = scratch();
  HY_TRY(sc.reserve(8 * total_words + 4096));
  uint64_t* d_words = carve<uint64_t>(sc, total_words);
  if (!d_words) return fail(HY_ERR_DEVICE, "scratch arena exhausted");
  HY_TRY(like_launch(dict, program, d_words, stream));
  HY_HIP(hipMemcpyAsync(match_words, d_words, 8 * total_words, hipMemcpyDeviceToHost, stream));
  HY_HIP(hipStreamSynchronize(stream));
  return HY_OK;
}

}  // extern "C"

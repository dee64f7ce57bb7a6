// hyrise_host.hpp -- C++ mirror of the slice of Hyrise's operator/storage interface that the hot path touches, written
// against the C ABI (include/hyrise_amd.h).  Hyrise itself cannot be built in this environment;
// this header lets the three operators be driven -- and tested -- exactly the way the reference's own tests drive them:
//
//     auto table   = load_table("int_float.tbl", ChunkOffset{2});            src/lib/utils/load_table.cpp:57-96
//     ChunkEncoder::encode_all_chunks(table, EncodingType::Dictionary);      src/lib/storage/chunk_encoder.hpp
//     auto wrapper = std::make_shared<TableWrapper>(table); wrapper->execute();
//     auto scan    = std::make_shared<TableScan>(wrapper, ColumnID{0}, PredicateCondition::GreaterThanEquals, 1234);
//     scan->execute();  scan->get_output();                                  operators/abstract_operator.hpp:133,143
//
// Names, argument meaning and error behaviour follow the reference: operators derive from AbstractReadOnlyOperator and
// implement `_on_execute()` (abstract_read_only_operator.hpp:20-22); scans and joins return TableType::References
// tables whose segments share PosLists (table_scan.cpp:207-210); failures throw std::logic_error (utils/assert.hpp:48-70).
// There is NO CPU implementation behind these classes: what the device library reports as HY_ERR_UNSUPPORTED (the
// shapes for which the real adapter keeps Hyrise's stock operator) surfaces as std::logic_error here.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/hyrise_amd.h"

namespace hyrise_amd {

// ---- types.hpp / all_type_variant.hpp ---------------------------------------------------------------------------------
using ChunkID = uint32_t;
using ChunkOffset = uint32_t;
using ColumnID = uint16_t;
constexpr ColumnID INVALID_COLUMN_ID = 0xFFFF;

enum class DataType : uint8_t { Null, Int, Long, Float, Double, String };
enum class PredicateCondition : uint8_t {
  Equals, NotEquals, LessThan, LessThanEquals, GreaterThan, GreaterThanEquals, BetweenInclusive, BetweenLowerExclusive,
  BetweenUpperExclusive, BetweenExclusive, In, NotIn, Like, NotLike, LikeInsensitive, NotLikeInsensitive, IsNull, IsNotNull
};
enum class JoinMode : uint8_t { Inner, Left, Right, FullOuter, Cross, Semi, AntiNullAsTrue, AntiNullAsFalse };
enum class WindowFunction : uint8_t { Min, Max, Sum, Avg, Count, CountDistinct, StandardDeviationSample, Any };
enum class EncodingType : uint8_t { Unencoded, Dictionary, FrameOfReference, LZ4 };
enum class TableType : uint8_t { Data, References };
enum class SortMode : uint8_t { AscendingNullsFirst, DescendingNullsFirst, AscendingNullsLast, DescendingNullsLast };   // types.hpp:219
struct SortColumnDefinition {   // types.hpp:245-251
  explicit SortColumnDefinition(ColumnID init_column, SortMode init_sort_mode = SortMode::AscendingNullsFirst) : column(init_column), sort_mode(init_sort_mode) {}
  ColumnID column;
  SortMode sort_mode;
};

struct NullValue {};
using AllTypeVariant = std::variant<NullValue, int32_t, int64_t, float, double, std::string>;
inline bool variant_is_null(const AllTypeVariant& v) { return v.index() == 0; }
inline DataType data_type_from_all_type_variant(const AllTypeVariant& v) { return static_cast<DataType>(v.index()); }

struct RowID {
  ChunkID chunk_id;
  ChunkOffset chunk_offset;
  bool is_null() const { return chunk_offset == 0xFFFFFFFFu; }
  bool operator==(const RowID& o) const { return chunk_id == o.chunk_id && chunk_offset == o.chunk_offset; }
};
static_assert(sizeof(RowID) == sizeof(hy_row_id), "RowID must be the ABI's 8-byte {chunk_id, chunk_offset}");
constexpr RowID NULL_ROW_ID{0xFFFFFFFFu, 0xFFFFFFFFu};

[[noreturn]] inline void Fail(const std::string& message) { throw std::logic_error(message); }
inline void Assert(bool condition, const char* message) { if (!condition) Fail(message); }   // (no std::string built on the passing path: thousands of ReferenceSegments per output table assert)
inline void Assert(bool condition, const std::string& message) { if (!condition) Fail(message); }
inline void check_status(hy_status status) { if (status != HY_OK) Fail(std::string("hyrise_amd: ") + hy_last_error()); }

// ---- storage ---------------------------------------------------------------------------------------------------------
class AbstractPosList {
 public:
  virtual ~AbstractPosList() = default;
  virtual size_t size() const = 0;
  virtual RowID operator[](size_t index) const = 0;
  virtual bool references_single_chunk() const = 0;
  virtual ChunkID common_chunk_id() const = 0;
};

class RowIDPosList : public AbstractPosList {   // pos_lists/row_id_pos_list.hpp:22-143
 public:
  RowIDPosList() = default;
  explicit RowIDPosList(std::vector<RowID> init) : rows(std::move(init)) {}
  size_t size() const override { return rows.size(); }
  RowID operator[](size_t index) const override { return rows[index]; }
  void guarantee_single_chunk() { _single = true; }
  bool references_single_chunk() const override { return _single; }
  ChunkID common_chunk_id() const override { return rows.empty() ? 0xFFFFFFFFu : rows[0].chunk_id; }
  std::vector<RowID> rows;

 private:
  bool _single = false;
};

class EntireChunkPosList : public AbstractPosList {   // pos_lists/entire_chunk_pos_list.hpp:8-44
 public:
  EntireChunkPosList(ChunkID chunk_id, ChunkOffset size) : _chunk_id(chunk_id), _size(size) {}
  size_t size() const override { return _size; }
  RowID operator[](size_t index) const override { return RowID{_chunk_id, static_cast<ChunkOffset>(index)}; }
  bool references_single_chunk() const override { return true; }
  ChunkID common_chunk_id() const override { return _chunk_id; }

 private:
  ChunkID _chunk_id;
  ChunkOffset _size;
};

// ---- PosLists that stay in HBM ------------------------------------------------------------------------------------------------
// The reference's PosLists are polymorphic (AbstractPosList, pos_lists/abstract_pos_list.hpp:18-75; ReferenceSegment holds a
// shared_ptr<const AbstractPosList>, reference_segment.hpp:36-38): an operator that understands a subclass reads it directly, everybody
// else goes through size() / operator[] / begin().  DevicePosList is that subclass for this library: the RowIDs lie in a block of the
// library's result-buffer pool (hy_result_pool_*), the operators below hand the device pointer to the next call (a scan's PosLists as the
// reference column of a join, a join's as the input of an aggregate) and nothing crosses the host link; code that indexes the list gets
// a host copy made on first use.  The block goes back to the pool when the last PosList in it dies.
// What the release orders: on a thread of the block's device, only the work queued on THAT thread's stream (the pool records an event
// there; the next owner's stream waits for it) -- a reader on any other stream must have finished before the last reference drops.  Every
// operator below synchronises before it returns, which is what makes that hold.  On a thread of another device the release waits for the
// block's whole device instead.
struct DeviceBlock {
  explicit DeviceBlock(void* init) : ptr(init) {}
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  ~DeviceBlock() { if (ptr) (void)hy_result_pool_release(ptr); }
  static std::shared_ptr<DeviceBlock> acquire(uint64_t bytes) {
    void* p = nullptr;
    check_status(hy_result_pool_acquire(bytes, &p));
    return std::make_shared<DeviceBlock>(p);
  }
  // ONE transfer for every PosList of the block (a scan's 916 lists, a join's 458): the lists then index this copy
  void prefetch_to_host(size_t rows) const {
    std::call_once(_once, [&] {
      _host.resize(rows);
      if (rows) check_status(hy_memcpy_d2h(_host.data(), ptr, rows * sizeof(RowID)));
      _published.store(rows ? _host.data() : nullptr, std::memory_order_release);
    });
  }
  const RowID* host_copy() const { return _published.load(std::memory_order_acquire); }
  void* ptr;

 private:
  mutable std::once_flag _once;
  mutable std::vector<RowID> _host;
  mutable std::atomic<const RowID*> _published{nullptr};
};

// Hands every operator's device results to the next operator without a host copy (default).  false: the operators ask the library for
// HY_MEM_HOST results, as rounds 1-5 did -- tests compare the two.
inline bool& device_resident_results() { static bool enabled = true; return enabled; }
// AggregateHash's string outputs -- string GROUP BY columns, MIN / MAX / ANY over a string column -- are made in HBM (hy_string_column_gather,
// hy_string_ranks_gather) where the column is wholly dictionary-encoded; false: on the host, from the representative RowIDs and the ranks.
inline bool& device_string_results() { static bool enabled = true; return enabled; }

class DevicePosList : public AbstractPosList {
 public:
  static constexpr ChunkID NO_COMMON_CHUNK = 0xFFFFFFFFu;
  DevicePosList(std::shared_ptr<const DeviceBlock> block, const hy_row_id* rows, size_t size, bool single_chunk = false, ChunkID common_chunk = NO_COMMON_CHUNK)
      : _block(std::move(block)), _rows(rows), _size(size), _single(single_chunk), _common(common_chunk) {}
  size_t size() const override { return _size; }
  // (a handful of lookups -- an aggregate's representative rows -- fetch eight bytes each; a reader that keeps indexing gets the copy)
  RowID operator[](size_t index) const override {
    if (!_copied.load(std::memory_order_acquire) && !_block->host_copy() && _single_fetches.fetch_add(1, std::memory_order_relaxed) < 16) {
      RowID row{};
      check_status(hy_memcpy_d2h(&row, _rows + index, sizeof(RowID)));
      return row;
    }
    return host_rows()[index];
  }
  bool references_single_chunk() const override { return _single; }
  ChunkID common_chunk_id() const override { return _single ? _common : NO_COMMON_CHUNK; }
  const hy_row_id* device_data() const { return _rows; }
  const std::shared_ptr<const DeviceBlock>& block() const { return _block; }
  bool on_host() const { return _copied.load(std::memory_order_acquire) || _block->host_copy() || _single_fetches.load(std::memory_order_relaxed) > 0; }   // some row has crossed the link
  // begin() of the reference's interface: the rows in host memory, copied on first use (from the block's copy if somebody prefetched it)
  const RowID* host_rows() const {
    if (const auto* all = _block->host_copy()) return all + (_rows - static_cast<const hy_row_id*>(_block->ptr));
    std::call_once(_once, [&] { _host.resize(_size); if (_size) check_status(hy_memcpy_d2h(_host.data(), _rows, _size * sizeof(RowID))); _copied.store(true, std::memory_order_release); });
    return _host.data();
  }

 private:
  std::shared_ptr<const DeviceBlock> _block;
  const hy_row_id* _rows;
  size_t _size;
  bool _single;
  ChunkID _common;
  mutable std::once_flag _once;
  mutable std::vector<RowID> _host;
  mutable std::atomic<bool> _copied{false};
  mutable std::atomic<uint32_t> _single_fetches{0};
};

class Table;

class AbstractSegment {
 public:
  explicit AbstractSegment(DataType type) : _data_type(type) {}
  virtual ~AbstractSegment() = default;
  virtual ChunkOffset size() const = 0;
  virtual AllTypeVariant operator[](ChunkOffset offset) const = 0;   // slow, test-side access like the reference's
  DataType data_type() const { return _data_type; }

 private:
  DataType _data_type;
};

template <typename T> constexpr DataType data_type_of() {
  if constexpr (std::is_same_v<T, int32_t>) return DataType::Int;
  else if constexpr (std::is_same_v<T, int64_t>) return DataType::Long;
  else if constexpr (std::is_same_v<T, float>) return DataType::Float;
  else if constexpr (std::is_same_v<T, double>) return DataType::Double;
  else return DataType::String;
}

inline std::vector<uint64_t> pack_null_words(const std::vector<bool>& nulls) {   // libstdc++ vector<bool> word order
  std::vector<uint64_t> words((nulls.size() + 63) / 64, 0);
  for (size_t i = 0; i < nulls.size(); ++i) if (nulls[i]) words[i / 64] |= uint64_t{1} << (i % 64);
  return words;
}

template <typename T>
class ValueSegment : public AbstractSegment {   // storage/value_segment.hpp:15-90
 public:
  ValueSegment(std::vector<T> values, std::optional<std::vector<bool>> nulls) : AbstractSegment(data_type_of<T>()), _values(std::move(values)), _nulls(std::move(nulls)) {
    if (_nulls) _null_words = pack_null_words(*_nulls);
  }
  ChunkOffset size() const override { return static_cast<ChunkOffset>(_values.size()); }
  bool is_nullable() const { return _nulls.has_value(); }
  const std::vector<T>& values() const { return _values; }
  const std::vector<uint64_t>& null_words() const { return _null_words; }
  bool is_null(ChunkOffset offset) const { return _nulls && (*_nulls)[offset]; }
  AllTypeVariant operator[](ChunkOffset offset) const override { if (is_null(offset)) return NullValue{}; return _values[offset]; }

 private:
  std::vector<T> _values;
  std::optional<std::vector<bool>> _nulls;
  std::vector<uint64_t> _null_words;
};

// A value segment whose rows lie in HBM: chunk `chunk_index` of an hy_column an operator left there (hy_aggregate_hash_columns' output
// columns).  The next operator takes the hy_column itself (device_column_of_chunks); code that indexes the segment gets a host copy of the
// chunk, fetched once on first use -- DevicePosList's lazy copy, for values.  The hy_column dies with its last segment.
struct DeviceColumnOwner {
  explicit DeviceColumnOwner(hy_column* init) : handle(init) {}
  DeviceColumnOwner(const DeviceColumnOwner&) = delete;
  DeviceColumnOwner& operator=(const DeviceColumnOwner&) = delete;
  ~DeviceColumnOwner() { if (handle) hy_column_destroy(handle); }
  hy_column* handle;
};
// How many DeviceValueSegments have fetched their chunk to the host so far (tests: a chain that stays in HBM leaves it alone).
inline std::atomic<uint64_t>& device_value_segment_fetches() { static std::atomic<uint64_t> fetches{0}; return fetches; }

template <typename T>
class DeviceValueSegment : public AbstractSegment {
 public:
  DeviceValueSegment(std::shared_ptr<const DeviceColumnOwner> owner, uint32_t chunk_index, ChunkOffset size)
      : AbstractSegment(data_type_of<T>()), _owner(std::move(owner)), _chunk_index(chunk_index), _size(size) {}
  ChunkOffset size() const override { return _size; }
  const std::shared_ptr<const DeviceColumnOwner>& owner() const { return _owner; }
  uint32_t chunk_index() const { return _chunk_index; }
  const std::vector<T>& values() const { fetch(); return _values; }
  const std::vector<uint64_t>& null_words() const { fetch(); return _null_words; }
  AllTypeVariant operator[](ChunkOffset offset) const override {
    fetch();
    if ((_null_words[offset / 64] >> (offset % 64)) & 1) return NullValue{};
    return _values[offset];
  }

 private:
  void fetch() const {
    std::call_once(_once, [&] {
      _values.resize(_size);
      _null_words.assign((size_t{_size} + 63) / 64, 0);
      if (_size) check_status(hy_column_read_chunk(_owner->handle, _chunk_index, _values.data(), _null_words.data()));
      device_value_segment_fetches().fetch_add(1, std::memory_order_relaxed);
    });
  }
  std::shared_ptr<const DeviceColumnOwner> _owner;
  uint32_t _chunk_index;
  ChunkOffset _size;
  mutable std::once_flag _once;
  mutable std::vector<T> _values;
  mutable std::vector<uint64_t> _null_words;
};

// FixedWidthIntegerVector<u8/u16/u32> (fixed_width_integer_compressor.cpp:33-44)
struct CompressedVector {
  uint32_t width = 4;
  std::vector<uint8_t> bytes;
  static CompressedVector compress(const std::vector<uint32_t>& values, uint32_t max_value) {
    CompressedVector out;
    out.width = max_value <= 0xFF ? 1 : max_value <= 0xFFFF ? 2 : 4;
    out.bytes.resize(values.size() * out.width + 16);
    for (size_t i = 0; i < values.size(); ++i) std::memcpy(out.bytes.data() + i * out.width, &values[i], out.width);
    return out;
  }
  uint32_t get(size_t i) const { uint32_t v = 0; std::memcpy(&v, bytes.data() + i * width, width); return v; }
};

template <typename T>
class DictionarySegment : public AbstractSegment {   // storage/dictionary_segment.hpp:19-91
 public:
  DictionarySegment(std::vector<T> dictionary, CompressedVector attribute_vector, ChunkOffset size)
      : AbstractSegment(data_type_of<T>()), _dictionary(std::move(dictionary)), _attribute_vector(std::move(attribute_vector)), _size(size) {}
  ChunkOffset size() const override { return _size; }
  const std::vector<T>& dictionary() const { materialize(); return _dictionary; }
  const CompressedVector& attribute_vector() const { materialize(); return _attribute_vector; }
  uint32_t unique_values_count() const { materialize(); return static_cast<uint32_t>(_dictionary.size()); }
  uint32_t lower_bound(const T& value) const {   // dictionary_segment.cpp:94-106
    materialize();
    const auto it = std::lower_bound(_dictionary.begin(), _dictionary.end(), value);
    return it == _dictionary.end() ? HY_INVALID_VALUE_ID : static_cast<uint32_t>(it - _dictionary.begin());
  }
  uint32_t upper_bound(const T& value) const {   // :108-119
    materialize();
    const auto it = std::upper_bound(_dictionary.begin(), _dictionary.end(), value);
    return it == _dictionary.end() ? HY_INVALID_VALUE_ID : static_cast<uint32_t>(it - _dictionary.begin());
  }
  AllTypeVariant operator[](ChunkOffset offset) const override {
    materialize();
    const auto vid = _attribute_vector.get(offset);
    if (vid >= _dictionary.size()) return NullValue{};
    return _dictionary[vid];
  }

 protected:
  virtual void materialize() const {}   // (DeviceStringDictionarySegment: the dictionary and the attribute vector are fetched on first use)
  mutable std::vector<T> _dictionary;
  mutable CompressedVector _attribute_vector;
  ChunkOffset _size;
};

// A DictionarySegment<pmr_string> whose attribute vector and dictionary lie in HBM: chunk `chunk_index` of the pair that hy_string_column_gather /
// hy_string_ranks_gather made (AggregateHash's string outputs).  The next operator takes the two handles (device_column_of_chunks,
// device_string_dictionary) and uploads nothing; code that reads the segment as a DictionarySegment gets a host copy, fetched once on first
// use and counted.  Both handles die with the last segment.
struct DeviceStringResult {
  DeviceStringResult(hy_column* column_handle, hy_string_dictionary* dictionary_handle) : column(std::make_shared<const DeviceColumnOwner>(column_handle)), dictionary(dictionary_handle) {}
  DeviceStringResult(const DeviceStringResult&) = delete;
  DeviceStringResult& operator=(const DeviceStringResult&) = delete;
  ~DeviceStringResult() { if (dictionary) hy_string_dictionary_destroy(dictionary); }
  std::shared_ptr<const DeviceColumnOwner> column;
  hy_string_dictionary* dictionary;
};
inline std::atomic<uint64_t>& device_string_segment_fetches() { static std::atomic<uint64_t> fetches{0}; return fetches; }

class DeviceStringDictionarySegment : public DictionarySegment<std::string> {
 public:
  DeviceStringDictionarySegment(std::shared_ptr<const DeviceStringResult> result, uint32_t chunk_index, ChunkOffset size)
      : DictionarySegment<std::string>({}, CompressedVector{}, size), _result(std::move(result)), _chunk_index(chunk_index) {}
  const std::shared_ptr<const DeviceStringResult>& result() const { return _result; }
  const std::shared_ptr<const DeviceColumnOwner>& owner() const { return _result->column; }
  uint32_t chunk_index() const { return _chunk_index; }

 protected:
  void materialize() const override {
    std::call_once(_once, [&] {
      uint32_t n_entries = 0;
      uint64_t chars_bytes = 0;
      check_status(hy_string_dictionary_chunk_size(_result->dictionary, _chunk_index, &n_entries, &chars_bytes));
      std::string chars(chars_bytes, '\0');
      std::vector<uint32_t> offsets(size_t{n_entries} + 1, 0), value_ids(std::max<size_t>(1, _size), 0);
      check_status(hy_string_dictionary_read_chunk(_result->dictionary, _chunk_index, chars.data(), offsets.data()));
      if (_size) check_status(hy_column_read_chunk(_result->column->handle, _chunk_index, value_ids.data(), nullptr));
      value_ids.resize(_size);
      _dictionary.clear();
      for (uint32_t v = 0; v < n_entries; ++v) _dictionary.emplace_back(chars, offsets[v], offsets[v + 1] - offsets[v]);
      _attribute_vector = CompressedVector::compress(value_ids, n_entries);
      device_string_segment_fetches().fetch_add(1, std::memory_order_relaxed);
    });
  }

 private:
  std::shared_ptr<const DeviceStringResult> _result;
  uint32_t _chunk_index;
  mutable std::once_flag _once;
};

class FrameOfReferenceSegment : public AbstractSegment {   // storage/frame_of_reference_segment.hpp:37-98
 public:
  FrameOfReferenceSegment(std::vector<int32_t> minima, CompressedVector offsets, std::optional<std::vector<bool>> nulls, ChunkOffset size)
      : AbstractSegment(DataType::Int), _minima(std::move(minima)), _offsets(std::move(offsets)), _nulls(std::move(nulls)), _size(size) {
    if (_nulls) _null_words = pack_null_words(*_nulls);
  }
  ChunkOffset size() const override { return _size; }
  const std::vector<int32_t>& block_minima() const { return _minima; }
  const CompressedVector& offset_values() const { return _offsets; }
  bool has_nulls() const { return _nulls.has_value(); }
  const std::vector<uint64_t>& null_words() const { return _null_words; }
  AllTypeVariant operator[](ChunkOffset offset) const override {
    if (_nulls && (*_nulls)[offset]) return NullValue{};
    return static_cast<int32_t>(_offsets.get(offset) + static_cast<uint32_t>(_minima[offset / HY_FOR_BLOCK_SIZE]));
  }

 private:
  std::vector<int32_t> _minima;
  CompressedVector _offsets;
  std::optional<std::vector<bool>> _nulls;
  std::vector<uint64_t> _null_words;
  ChunkOffset _size;
};

// LZ4Segment<T> of a numeric type (storage/lz4_segment.hpp:25-118): the values' bytes in blocks of BLOCK_SIZE, every block compressed on its
// own.  The device path takes the blocks as they are (HY_ENC_LZ4 + hy_lz4_blocks) and decompresses them with a kernel.
template <typename T>
class LZ4Segment : public AbstractSegment {
 public:
  static constexpr size_t BLOCK_SIZE = 16384;   // lz4_encoder.hpp:61
  LZ4Segment(std::vector<std::vector<char>> blocks, std::optional<std::vector<bool>> nulls, std::vector<char> dictionary, size_t block_size, size_t last_block_size, ChunkOffset size)
      : AbstractSegment(data_type_of<T>()), _blocks(std::move(blocks)), _nulls(std::move(nulls)), _dictionary(std::move(dictionary)), _block_size(block_size),
        _last_block_size(last_block_size), _size(size) {
    if (_nulls) _null_words = pack_null_words(*_nulls);
    for (const auto& block : _blocks) { _block_pointers.push_back(block.data()); _block_bytes.push_back(static_cast<uint32_t>(block.size())); }
    _descriptor.blocks = _block_pointers.data();
    _descriptor.block_bytes = _block_bytes.data();
    _descriptor.block_count = static_cast<uint32_t>(_blocks.size());
    _descriptor.block_size = static_cast<uint32_t>(_block_size);
    _descriptor.last_block_size = static_cast<uint32_t>(_last_block_size);
    _descriptor.dictionary_bytes = static_cast<uint32_t>(_dictionary.size());
    _descriptor.dictionary = _dictionary.empty() ? nullptr : _dictionary.data();
  }
  ChunkOffset size() const override { return _size; }
  AllTypeVariant operator[](ChunkOffset offset) const override {   // (the mirror's own decoder: decompress(), lz4_segment.cpp:125-136)
    if (_nulls && (*_nulls)[offset]) return NullValue{};
    return decompress()[offset];
  }
  std::vector<T> decompress() const {
    std::vector<char> bytes;
    for (size_t b = 0; b < _blocks.size(); ++b) {
      const auto& in = _blocks[b];
      const size_t start = bytes.size();
      size_t i = 0;
      while (i < in.size()) {
        const auto token = static_cast<uint8_t>(in[i++]);
        size_t literals = token >> 4;
        if (literals == 15) { uint8_t extra; do { extra = static_cast<uint8_t>(in[i++]); literals += extra; } while (extra == 255); }
        bytes.insert(bytes.end(), in.begin() + i, in.begin() + i + literals);
        i += literals;
        if (i >= in.size()) break;
        const size_t offset = static_cast<uint8_t>(in[i]) | static_cast<size_t>(static_cast<uint8_t>(in[i + 1])) << 8;
        i += 2;
        size_t length = (token & 15) + 4;
        if ((token & 15) == 15) { uint8_t extra; do { extra = static_cast<uint8_t>(in[i++]); length += extra; } while (extra == 255); }
        for (size_t k = 0; k < length; ++k) {
          const ptrdiff_t from = static_cast<ptrdiff_t>(bytes.size() - start) - static_cast<ptrdiff_t>(offset);
          bytes.push_back(from >= 0 ? bytes[start + from] : _dictionary[_dictionary.size() + from]);
        }
      }
    }
    std::vector<T> values(_size);
    std::memcpy(values.data(), bytes.data(), std::min(bytes.size(), sizeof(T) * _size));
    return values;
  }
  const hy_lz4_blocks& descriptor() const { return _descriptor; }
  bool has_nulls() const { return _nulls.has_value(); }
  const std::vector<uint64_t>& null_words() const { return _null_words; }

 private:
  std::vector<std::vector<char>> _blocks;
  std::optional<std::vector<bool>> _nulls;
  std::vector<char> _dictionary;
  size_t _block_size, _last_block_size;
  ChunkOffset _size;
  std::vector<uint64_t> _null_words;
  std::vector<const void*> _block_pointers;
  std::vector<uint32_t> _block_bytes;
  hy_lz4_blocks _descriptor{};
};

class ReferenceSegment : public AbstractSegment {   // storage/reference_segment.hpp:20-48
 public:
  ReferenceSegment(std::shared_ptr<const Table> table, ColumnID column_id, std::shared_ptr<const AbstractPosList> pos_list);
  ChunkOffset size() const override { return static_cast<ChunkOffset>(_pos_list->size()); }
  const std::shared_ptr<const Table>& referenced_table() const { return _table; }
  ColumnID referenced_column_id() const { return _column_id; }
  const std::shared_ptr<const AbstractPosList>& pos_list() const { return _pos_list; }
  AllTypeVariant operator[](ChunkOffset offset) const override;

 private:
  std::shared_ptr<const Table> _table;
  ColumnID _column_id;
  std::shared_ptr<const AbstractPosList> _pos_list;
};

using Segments = std::vector<std::shared_ptr<AbstractSegment>>;

using TransactionID = uint32_t;
using CommitID = uint32_t;
constexpr CommitID MAX_COMMIT_ID = 0xFFFFFFFFu - 1;        // storage/mvcc_data.hpp
constexpr TransactionID INVALID_TRANSACTION_ID = 0;

struct MvccData {   // storage/mvcc_data.hpp: three arrays, one entry per row of the chunk
  explicit MvccData(size_t size, CommitID begin_commit_id = MAX_COMMIT_ID)
      : tids(size, INVALID_TRANSACTION_ID), begin_cids(size, begin_commit_id), end_cids(size, MAX_COMMIT_ID), max_begin_cid(begin_commit_id) {}
  TransactionID get_tid(ChunkOffset row) const { return tids[row]; }
  CommitID get_begin_cid(ChunkOffset row) const { return begin_cids[row]; }
  CommitID get_end_cid(ChunkOffset row) const { return end_cids[row]; }
  void set_tid(ChunkOffset row, TransactionID tid) { tids[row] = tid; }
  void set_begin_cid(ChunkOffset row, CommitID cid) { begin_cids[row] = cid; }
  void set_end_cid(ChunkOffset row, CommitID cid) { end_cids[row] = cid; }
  std::vector<TransactionID> tids;
  std::vector<CommitID> begin_cids, end_cids;
  CommitID max_begin_cid;
};

class Chunk {   // storage/chunk.hpp:38-218
 public:
  static constexpr ChunkOffset DEFAULT_SIZE = 65535;
  explicit Chunk(Segments segments) : _segments(std::move(segments)) {}
  Chunk(Segments segments, std::shared_ptr<MvccData> mvcc_data) : _segments(std::move(segments)), _mvcc_data(std::move(mvcc_data)) {}
  bool has_mvcc_data() const { return _mvcc_data != nullptr; }
  const std::shared_ptr<MvccData>& mvcc_data() const { return _mvcc_data; }
  bool is_mutable() const { return _is_mutable; }
  void set_immutable() { _is_mutable = false; }
  uint32_t invalid_row_count() const { return _invalid_row_count; }
  void increase_invalid_row_count(uint32_t count) { _invalid_row_count += count; }
  ChunkOffset size() const { return _segments.empty() ? 0 : _segments[0]->size(); }
  const std::shared_ptr<AbstractSegment>& get_segment(ColumnID column_id) const { return _segments.at(column_id); }
  void replace_segment(ColumnID column_id, std::shared_ptr<AbstractSegment> segment) { _segments.at(column_id) = std::move(segment); }
  ColumnID column_count() const { return static_cast<ColumnID>(_segments.size()); }
  // chunk.hpp:160-176: the scan of a column the chunk is flagged as sorted by takes the SortedSegmentSearch path (HY_SORT_* on the descriptor)
  const std::vector<SortColumnDefinition>& individually_sorted_by() const { return _sorted_by; }
  void set_individually_sorted_by(const SortColumnDefinition& sorted_by) { _sorted_by = {sorted_by}; }
  void set_individually_sorted_by(const std::vector<SortColumnDefinition>& sorted_by) { _sorted_by = sorted_by; }

 private:
  Segments _segments;
  std::vector<SortColumnDefinition> _sorted_by;
  std::shared_ptr<MvccData> _mvcc_data;
  bool _is_mutable = true;
  uint32_t _invalid_row_count = 0;
};

struct TableColumnDefinition {
  std::string name;
  DataType data_type;
  bool nullable;
};
using TableColumnDefinitions = std::vector<TableColumnDefinition>;

struct ColumnCache;   // device-resident columns of one table (residency cache)

class Table : public std::enable_shared_from_this<Table> {   // storage/table.hpp
 public:
  Table(TableColumnDefinitions definitions, TableType type, ChunkOffset target_chunk_size = Chunk::DEFAULT_SIZE)
      : _definitions(std::move(definitions)), _type(type), _target_chunk_size(target_chunk_size) {}
  Table(TableColumnDefinitions definitions, TableType type, std::vector<std::shared_ptr<Chunk>> chunks)
      : _definitions(std::move(definitions)), _type(type), _target_chunk_size(Chunk::DEFAULT_SIZE), _chunks(std::move(chunks)) {}
  ~Table();
  const TableColumnDefinitions& column_definitions() const { return _definitions; }
  ColumnID column_count() const { return static_cast<ColumnID>(_definitions.size()); }
  DataType column_data_type(ColumnID id) const { return _definitions.at(id).data_type; }
  bool column_is_nullable(ColumnID id) const { return _definitions.at(id).nullable; }
  const std::string& column_name(ColumnID id) const { return _definitions.at(id).name; }
  TableType type() const { return _type; }
  ChunkID chunk_count() const { return static_cast<ChunkID>(_chunks.size()); }
  ChunkOffset target_chunk_size() const { return _target_chunk_size; }
  const std::shared_ptr<Chunk>& get_chunk(ChunkID id) const { return _chunks.at(id); }
  uint64_t row_count() const { uint64_t n = 0; for (const auto& c : _chunks) n += c->size(); return n; }
  void append_chunk(Segments segments) { _chunks.push_back(std::make_shared<Chunk>(std::move(segments))); }
  void append_chunk(Segments segments, std::shared_ptr<MvccData> mvcc_data) { _chunks.push_back(std::make_shared<Chunk>(std::move(segments), std::move(mvcc_data))); }
  // Table::append(row): rows are collected and cut into ValueSegments of target_chunk_size rows by finalize().
  void append(std::vector<AllTypeVariant> row) { _pending.push_back(std::move(row)); if (_pending.size() == _target_chunk_size) finalize(); }
  void finalize();
  AllTypeVariant get_value(ColumnID column_id, uint64_t row) const {
    for (const auto& chunk : _chunks) { if (row < chunk->size()) return (*chunk->get_segment(column_id))[static_cast<ChunkOffset>(row)]; row -= chunk->size(); }
    Fail("row index out of range");
  }
  std::vector<std::vector<AllTypeVariant>> get_rows() const {
    std::vector<std::vector<AllTypeVariant>> rows;
    for (const auto& chunk : _chunks)
      for (ChunkOffset r = 0; r < chunk->size(); ++r) {
        std::vector<AllTypeVariant> row;
        for (ColumnID c = 0; c < column_count(); ++c) row.push_back((*chunk->get_segment(c))[r]);
        rows.push_back(std::move(row));
      }
    return rows;
  }
  // table.hpp: every value of these columns lies in one chunk only (JoinSortMerge's Inner + Equals output, join_sort_merge.cpp:940-958)
  const std::vector<ColumnID>& value_clustered_by() const { return _value_clustered_by; }
  void set_value_clustered_by(std::vector<ColumnID> columns) { _value_clustered_by = std::move(columns); }
  mutable std::shared_ptr<ColumnCache> device_columns;

 private:
  std::vector<ColumnID> _value_clustered_by;
  TableColumnDefinitions _definitions;
  TableType _type;
  ChunkOffset _target_chunk_size;
  std::vector<std::shared_ptr<Chunk>> _chunks;
  std::vector<std::vector<AllTypeVariant>> _pending;
};

inline ReferenceSegment::ReferenceSegment(std::shared_ptr<const Table> table, ColumnID column_id, std::shared_ptr<const AbstractPosList> pos_list)
    : AbstractSegment(table->column_data_type(column_id)), _table(std::move(table)), _column_id(column_id), _pos_list(std::move(pos_list)) {
  Assert(_table->type() == TableType::Data, "ReferenceSegments must not reference reference tables (table_scan.cpp:140-148)");
}
inline AllTypeVariant ReferenceSegment::operator[](ChunkOffset offset) const {
  const RowID row = (*_pos_list)[offset];
  if (row.is_null()) return NullValue{};
  return (*_table->get_chunk(row.chunk_id)->get_segment(_column_id))[row.chunk_offset];
}

template <typename T>
std::shared_ptr<AbstractSegment> make_value_segment(const std::vector<std::vector<AllTypeVariant>>& rows, ColumnID column, bool nullable) {
  std::vector<T> values;
  std::vector<bool> nulls;
  for (const auto& row : rows) {
    const bool is_null = variant_is_null(row[column]);
    Assert(!is_null || nullable, "NULL in a non-nullable column");
    nulls.push_back(is_null);
    values.push_back(is_null ? T{} : std::get<T>(row[column]));
  }
  return std::make_shared<ValueSegment<T>>(std::move(values), nullable ? std::optional<std::vector<bool>>(std::move(nulls)) : std::nullopt);
}

inline void Table::finalize() {
  if (_pending.empty()) return;
  Segments segments;
  for (ColumnID c = 0; c < column_count(); ++c) {
    switch (_definitions[c].data_type) {
      case DataType::Int: segments.push_back(make_value_segment<int32_t>(_pending, c, _definitions[c].nullable)); break;
      case DataType::Long: segments.push_back(make_value_segment<int64_t>(_pending, c, _definitions[c].nullable)); break;
      case DataType::Float: segments.push_back(make_value_segment<float>(_pending, c, _definitions[c].nullable)); break;
      case DataType::Double: segments.push_back(make_value_segment<double>(_pending, c, _definitions[c].nullable)); break;
      default: segments.push_back(make_value_segment<std::string>(_pending, c, _definitions[c].nullable)); break;
    }
  }
  _chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
  _pending.clear();
}

// ---- load_table (utils/load_table.cpp:22-96) ----------------------------------------------------------------------------
inline std::vector<std::string> split_string_by_delimiter(const std::string& line, char delimiter) {
  std::vector<std::string> out;
  std::stringstream stream(line);
  std::string cell;
  while (std::getline(stream, cell, delimiter)) out.push_back(cell);
  if (!line.empty() && line.back() == delimiter) out.emplace_back();
  return out;
}

inline std::shared_ptr<Table> load_table(const std::string& file_name, ChunkOffset chunk_size = Chunk::DEFAULT_SIZE) {
  std::ifstream infile(file_name);
  Assert(infile.is_open(), "load_table: Could not find file '" + file_name + "'.");
  std::string line;
  std::getline(infile, line);
  const auto names = split_string_by_delimiter(line, '|');
  std::getline(infile, line);
  const auto types = split_string_by_delimiter(line, '|');
  TableColumnDefinitions definitions;
  for (size_t i = 0; i < names.size(); ++i) {
    const auto parts = split_string_by_delimiter(types[i], '_');
    const bool nullable = parts.size() > 1 && parts[1] == "null";
    DataType type;
    if (parts[0] == "int") type = DataType::Int;
    else if (parts[0] == "long") type = DataType::Long;
    else if (parts[0] == "float") type = DataType::Float;
    else if (parts[0] == "double") type = DataType::Double;
    else if (parts[0] == "string") type = DataType::String;
    else Fail("Invalid data type '" + parts[0] + "' for column '" + names[i] + "'.");
    definitions.push_back({names[i], type, nullable});
  }
  auto table = std::make_shared<Table>(definitions, TableType::Data, chunk_size);
  while (std::getline(infile, line)) {
    auto cells = split_string_by_delimiter(line, '|');
    cells.resize(definitions.size());
    std::vector<AllTypeVariant> row;
    for (size_t c = 0; c < definitions.size(); ++c) {
      if (definitions[c].nullable && cells[c] == "null") { row.emplace_back(NullValue{}); continue; }
      switch (definitions[c].data_type) {
        case DataType::Int: row.emplace_back(static_cast<int32_t>(std::stol(cells[c]))); break;
        case DataType::Long: row.emplace_back(static_cast<int64_t>(std::stoll(cells[c]))); break;
        case DataType::Float: row.emplace_back(std::stof(cells[c])); break;
        case DataType::Double: row.emplace_back(std::stod(cells[c])); break;
        default: row.emplace_back(cells[c]); break;
      }
    }
    table->append(std::move(row));
  }
  table->finalize();
  return table;
}

// ---- ChunkEncoder (dictionary_encoder.hpp:33-103, frame_of_reference_encoder.hpp:25-122) --------------------------------
struct ChunkEncoder {
  template <typename T>
  static std::shared_ptr<AbstractSegment> encode_dictionary(const ValueSegment<T>& segment) {
    std::vector<T> dictionary;
    for (ChunkOffset i = 0; i < segment.size(); ++i) if (!segment.is_null(i)) dictionary.push_back(segment.values()[i]);
    std::sort(dictionary.begin(), dictionary.end());
    dictionary.erase(std::unique(dictionary.begin(), dictionary.end()), dictionary.end());
    const auto null_value_id = static_cast<uint32_t>(dictionary.size());
    std::vector<uint32_t> ids(segment.size());
    for (ChunkOffset i = 0; i < segment.size(); ++i) {
      ids[i] = segment.is_null(i) ? null_value_id
                                  : static_cast<uint32_t>(std::lower_bound(dictionary.begin(), dictionary.end(), segment.values()[i]) - dictionary.begin());
    }
    return std::make_shared<DictionarySegment<T>>(std::move(dictionary), CompressedVector::compress(ids, null_value_id), segment.size());
  }
  static std::shared_ptr<AbstractSegment> encode_frame_of_reference(const ValueSegment<int32_t>& segment) {
    const auto n = segment.size();
    std::vector<int32_t> minima;
    std::vector<uint32_t> offsets(n);
    std::vector<bool> nulls(n, false);
    bool any_null = false;
    uint32_t max_offset = 0;
    for (ChunkOffset begin = 0; begin < n; begin += HY_FOR_BLOCK_SIZE) {
      const auto end = std::min<ChunkOffset>(n, begin + HY_FOR_BLOCK_SIZE);
      int32_t minimum = INT32_MAX;
      for (auto i = begin; i < end; ++i) {
        nulls[i] = segment.is_null(i);
        any_null |= nulls[i];
        if (!nulls[i]) minimum = std::min(minimum, segment.values()[i]);
      }
      minima.push_back(minimum);
      for (auto i = begin; i < end; ++i) {
        const int32_t value = nulls[i] ? minimum : segment.values()[i];
        offsets[i] = static_cast<uint32_t>(value) - static_cast<uint32_t>(minimum);
        max_offset = std::max(max_offset, offsets[i]);
      }
    }
    return std::make_shared<FrameOfReferenceSegment>(std::move(minima), CompressedVector::compress(offsets, max_offset),
                                                     any_null ? std::optional<std::vector<bool>>(std::move(nulls)) : std::nullopt, n);
  }
  // One LZ4 block (lz4_Block_format.md) by a greedy matcher over 4-byte words -- enough to produce what liblz4 would also accept; the
  // mirror has no zstd dictionary trainer, so its blocks are compressed without one (each still decompresses on its own).
  static std::vector<char> lz4_compress_block(const char* in, size_t n) {
    std::vector<char> out;
    std::vector<int32_t> last(1 << 12, -1);
    size_t anchor = 0, i = 0;
    auto emit = [&](size_t literal_end, size_t offset, size_t length) {   // length 0: the closing literals
      const size_t literals = literal_end - anchor;
      out.push_back(static_cast<char>((std::min<size_t>(literals, 15) << 4) | (length ? std::min<size_t>(length - 4, 15) : 0)));
      if (literals >= 15) { size_t rest = literals - 15; while (rest >= 255) { out.push_back(static_cast<char>(255)); rest -= 255; } out.push_back(static_cast<char>(rest)); }
      out.insert(out.end(), in + anchor, in + literal_end);
      if (!length) return;
      out.push_back(static_cast<char>(offset & 0xFF));
      out.push_back(static_cast<char>(offset >> 8));
      if (length - 4 >= 15) { size_t rest = length - 4 - 15; while (rest >= 255) { out.push_back(static_cast<char>(255)); rest -= 255; } out.push_back(static_cast<char>(rest)); }
    };
    while (i + 12 < n) {   // (the format wants the last five bytes as literals and no match within the last twelve)
      uint32_t word;
      std::memcpy(&word, in + i, 4);
      const uint32_t slot = (word * 2654435761u) >> 20;
      const int32_t candidate = last[slot];
      last[slot] = static_cast<int32_t>(i);
      uint32_t there = 0;
      if (candidate >= 0) std::memcpy(&there, in + candidate, 4);
      if (candidate < 0 || there != word || i - candidate > 65535) { ++i; continue; }
      size_t length = 4;
      while (i + length + 5 < n && in[candidate + length] == in[i + length]) ++length;
      emit(i, i - candidate, length);
      i += length;
      anchor = i;
    }
    emit(n, 0, 0);
    return out;
  }
  template <typename T>
  static std::shared_ptr<AbstractSegment> encode_lz4(const ValueSegment<T>& segment) {
    const auto n = segment.size();
    std::vector<T> values(segment.values().begin(), segment.values().end());
    std::vector<bool> nulls(n, false);
    bool any_null = false;
    for (ChunkOffset i = 0; i < n; ++i) { nulls[i] = segment.is_null(i); any_null |= nulls[i]; if (nulls[i]) values[i] = T{}; }
    const auto* bytes = reinterpret_cast<const char*>(values.data());
    const size_t total = sizeof(T) * n, block_size = LZ4Segment<T>::BLOCK_SIZE;
    std::vector<std::vector<char>> blocks;
    for (size_t begin = 0; begin < total; begin += block_size) blocks.push_back(lz4_compress_block(bytes + begin, std::min(block_size, total - begin)));
    const size_t last_block_size = total == 0 ? 0 : (total % block_size ? total % block_size : block_size);
    return std::make_shared<LZ4Segment<T>>(std::move(blocks), any_null ? std::optional<std::vector<bool>>(std::move(nulls)) : std::nullopt, std::vector<char>{}, block_size, last_block_size, n);
  }
  // encode_all_chunks(table, SegmentEncodingSpec{type}); unsupported (type, data type) pairs stay unencoded like
  // load_and_encode_table in table_scan_test.cpp:63-75.
  static void encode_all_chunks(const std::shared_ptr<Table>& table, EncodingType type) {
    if (type == EncodingType::Unencoded) return;
    for (ChunkID chunk_id = 0; chunk_id < table->chunk_count(); ++chunk_id) {
      const auto& chunk = table->get_chunk(chunk_id);
      for (ColumnID c = 0; c < table->column_count(); ++c) {
        const auto segment = chunk->get_segment(c);
        std::shared_ptr<AbstractSegment> encoded;
        if (type == EncodingType::FrameOfReference) {
          if (const auto* ints = dynamic_cast<const ValueSegment<int32_t>*>(segment.get())) encoded = encode_frame_of_reference(*ints);
        } else if (type == EncodingType::LZ4) {   // (LZ4 string segments stay on the CPU path: strings keep their dictionary encoding here)
          if (const auto* i32 = dynamic_cast<const ValueSegment<int32_t>*>(segment.get())) encoded = encode_lz4(*i32);
          else if (const auto* i64 = dynamic_cast<const ValueSegment<int64_t>*>(segment.get())) encoded = encode_lz4(*i64);
          else if (const auto* f32 = dynamic_cast<const ValueSegment<float>*>(segment.get())) encoded = encode_lz4(*f32);
          else if (const auto* f64 = dynamic_cast<const ValueSegment<double>*>(segment.get())) encoded = encode_lz4(*f64);
          else if (const auto* str = dynamic_cast<const ValueSegment<std::string>*>(segment.get())) encoded = encode_dictionary(*str);
        } else if (const auto* i32 = dynamic_cast<const ValueSegment<int32_t>*>(segment.get())) encoded = encode_dictionary(*i32);
        else if (const auto* i64 = dynamic_cast<const ValueSegment<int64_t>*>(segment.get())) encoded = encode_dictionary(*i64);
        else if (const auto* f32 = dynamic_cast<const ValueSegment<float>*>(segment.get())) encoded = encode_dictionary(*f32);
        else if (const auto* f64 = dynamic_cast<const ValueSegment<double>*>(segment.get())) encoded = encode_dictionary(*f64);
        else if (const auto* str = dynamic_cast<const ValueSegment<std::string>*>(segment.get())) encoded = encode_dictionary(*str);
        if (encoded) chunk->replace_segment(c, encoded);
      }
    }
  }
};

// ---- marshalling into the C ABI (what INTEGRATION.md section 1 does inside Hyrise) --------------------------------------
struct DeviceColumn {
  hy_column* handle = nullptr;
  std::vector<hy_segment> descriptors;
  std::vector<std::vector<int64_t>> key_names;   // string GROUP BY columns: AggregateKeyEntry names per chunk
  std::shared_ptr<const DeviceColumnOwner> resident;   // `handle` is a column an operator left in HBM: its segments own it
  std::shared_ptr<DeviceColumn> strings;   // `handle` is hy_column_string_ranks' stand-in of this column, whose buffers it reads: destroyed before it
  bool device_ranking = true;              // StringKeys::Ranks: what device_string_ranking() said when the column was made
  ~DeviceColumn() { if (handle && !resident) hy_column_destroy(handle); }
};

// How a DictionarySegment<pmr_string> is presented to the device: the value ids alone (scans), or with a dictionary of int64
// stand-ins for the strings -- AggregateKey names (GROUP BY), join ids (JoinHash) or ranks among the column's distinct strings in byte
// order (Sort; hyrise_amd/string_keys.py StringRanks).  The ranks of a whole dictionary-encoded column are made on the device and are int32
// (device_string_rank_column); the host makes them, as int64, for everything else.
enum class StringKeys { None, AggregateKeyNames, JoinIds, Ranks };
// The dictionaries of a string column's DictionarySegment chunks in HBM (hy_string_dictionary): what the LIKE matcher reads on the device.
struct DeviceStringDictionary {
  hy_string_dictionary* handle = nullptr;
  std::shared_ptr<const DeviceStringResult> resident;   // `handle` is the dictionary of a column an operator left in HBM: its segments own it
  ~DeviceStringDictionary() { if (handle && !resident) hy_string_dictionary_destroy(handle); }
};
struct ColumnCache {
  std::map<std::pair<ColumnID, StringKeys>, std::shared_ptr<DeviceColumn>> columns;
  std::map<ColumnID, std::shared_ptr<DeviceStringDictionary>> string_dictionaries;
};
inline Table::~Table() = default;

template <typename T> constexpr uint32_t abi_type() { return static_cast<uint32_t>(data_type_of<T>()); }

// AggregateKeyEntry name of a string (aggregate_hash.cpp:852-914); strings of 5+ characters get map ids from 5e9 on.
inline int64_t string_key_name(const std::string& s, std::map<std::string, int64_t>& long_strings) {
  const auto byte = [&](size_t i) { return static_cast<int64_t>(static_cast<uint8_t>(s[i])); };
  switch (s.size()) {
    case 0: return 1;
    case 1: return 2 + byte(0);
    case 2: return 258 + (byte(1) << 8) + byte(0);
    case 3: return 65794 + (byte(2) << 16) + (byte(1) << 8) + byte(0);
    case 4: return 16843010ll + (byte(3) << 24) + (byte(2) << 16) + (byte(1) << 8) + byte(0);
    default: {
      const auto it = long_strings.emplace(s, 5000000000ll + static_cast<int64_t>(long_strings.size())).first;
      return it->second;
    }
  }
}

// JoinHash on pmr_string keys.  The reference hashes them with std::hash (join_hash_steps.hpp:282,352,573: Bloom index =
// hash % 2^20, radix partition = hash & mask) and compares them in the hash table; the device joins 64-bit integers whose
// partition and Bloom index are their low bits.  So every distinct string gets the id  unique number << 20 | hash & 0xFFFFF:
// equal ids <=> equal strings, id & mask == hash & mask for radix_bits <= 8, id % 2^20 == the Bloom index -- the join over the
// ids is the reference's join over the strings (same partitions, probe-row order, build-side insertion order).  The hash is
// libstdc++'s (_Hash_bytes, libsupc++/hash_bytes.cc, seed 0xc70f6907), spelled out so that the ids do not depend on the
// standard library this file is compiled with (same restatement as hyrise_amd/join_keys.py, pinned in tests/test_oracle_join.py).
inline uint64_t libstdcxx_hash_bytes(const void* data, size_t length) {
  const uint64_t mul = (uint64_t{0xc6a4a793} << 32) + uint64_t{0x5bd1e995};
  const auto shift_mix = [](uint64_t v) { return v ^ (v >> 47); };
  const auto* bytes = static_cast<const unsigned char*>(data);
  const size_t aligned = length & ~size_t{7};
  uint64_t hash = uint64_t{0xc70f6907} ^ (length * mul);
  for (size_t p = 0; p < aligned; p += 8) {
    uint64_t word;
    std::memcpy(&word, bytes + p, 8);
    hash ^= shift_mix(word * mul) * mul;
    hash *= mul;
  }
  if (length & 7) {
    uint64_t tail = 0;
    for (size_t n = length & 7; n-- > 0;) tail = (tail << 8) + bytes[aligned + n];
    hash ^= tail;
    hash *= mul;
  }
  hash = shift_mix(hash) * mul;
  return shift_mix(hash);
}

inline int64_t string_join_id(const std::string& s) {   // one registry for all tables: cached columns stay valid across joins
  static std::mutex mutex;
  static std::map<std::string, int64_t> ids;
  const std::lock_guard<std::mutex> lock(mutex);
  const auto [it, inserted] = ids.emplace(s, 0);
  if (inserted) it->second = static_cast<int64_t>(ids.size() << 20 | (libstdcxx_hash_bytes(s.data(), s.size()) & 0xFFFFF));
  return it->second;
}

// `string_keys`: what a string dictionary column's dictionary is replaced with (see StringKeys).
inline std::shared_ptr<DeviceColumn> device_column(const std::shared_ptr<const Table>& table, ColumnID column_id, StringKeys string_keys = StringKeys::None);

// One PosList as the `data` / `ref_chunk_id` of an HY_ENC_REFERENCE descriptor; counts which memory the lists of a column lie in.
inline void describe_pos_list(const AbstractPosList& pos_list, hy_segment& d, size_t& host_lists, size_t& device_lists) {
  if (const auto* entire = dynamic_cast<const EntireChunkPosList*>(&pos_list)) {
    d.data = nullptr; d.ref_chunk_id = entire->common_chunk_id();
  } else if (const auto* on_device = dynamic_cast<const DevicePosList*>(&pos_list)) {
    d.data = on_device->device_data();
    d.ref_chunk_id = on_device->references_single_chunk() && on_device->size() ? on_device->common_chunk_id() : 0xFFFFFFFFu;
    if (on_device->size()) ++device_lists; else d.data = nullptr, d.ref_chunk_id = 0;   // (an empty list: nothing to read in either memory)
  } else {
    const auto& rows = static_cast<const RowIDPosList&>(pos_list);
    d.data = rows.rows.data();
    d.ref_chunk_id = rows.references_single_chunk() && rows.size() ? rows.common_chunk_id() : 0xFFFFFFFFu;
    ++host_lists;
  }
}

// The hy_column whose consecutive chunks 0 .. n - 1 ARE the segments [chunk_begin, chunk_end) of the column (an operator's device-resident
// output read as a whole), or nullptr: a mixed or partial range is fetched and described like any ValueSegment.  The handle lives on the
// device of the thread that ran the operator: a worker bound to another GPU (multi_gpu.hpp) asks for chunk ranges of its own shard, which are
// partial and take the fetched path; the whole column of another device's operator is refused by the library (on_this_device).
inline std::shared_ptr<const DeviceColumnOwner> resident_column_of_chunks(const Table& table, ColumnID column_id, ChunkID chunk_begin, ChunkID chunk_end);

// The chunks [chunk_begin, chunk_end) of one column on the CALLING THREAD's device (not cached: the residency cache of a table holds
// whole columns on the process's device; the shards of a DeviceGroup worker, multi_gpu.hpp, belong to that worker).
inline std::shared_ptr<DeviceColumn> device_column_of_chunks(const std::shared_ptr<const Table>& table, ColumnID column_id, StringKeys string_keys, ChunkID chunk_begin,
                                                             ChunkID chunk_end) {
  auto column = std::make_shared<DeviceColumn>();
  const auto chunk_count = chunk_end - chunk_begin;
  // (a string column whose dictionary is to be replaced by key names, join ids or host ranks is read through its segments, fetched)
  const bool as_it_is = string_keys == StringKeys::None || table->column_data_type(column_id) != DataType::String;
  if (const auto resident = as_it_is ? resident_column_of_chunks(*table, column_id, chunk_begin, chunk_end) : nullptr) {   // every chunk of one hy_column in HBM: that handle, as it is
    column->resident = resident;
    column->handle = resident->handle;
    return column;
  }
  column->descriptors.assign(chunk_count, hy_segment{});
  column->key_names.resize(chunk_count);
  std::map<std::string, int64_t> long_strings;
  std::shared_ptr<DeviceColumn> referenced;
  size_t host_lists = 0, device_lists = 0;
  std::vector<std::string> rank_order;   // StringKeys::Ranks: the distinct strings of the chunks' dictionaries, in byte order
  if (string_keys == StringKeys::Ranks) {
    for (ChunkID table_chunk = chunk_begin; table_chunk < chunk_end; ++table_chunk) {
      if (const auto* s = dynamic_cast<const DictionarySegment<std::string>*>(table->get_chunk(table_chunk)->get_segment(column_id).get()))
        rank_order.insert(rank_order.end(), s->dictionary().begin(), s->dictionary().end());
    }
    std::sort(rank_order.begin(), rank_order.end());
    rank_order.erase(std::unique(rank_order.begin(), rank_order.end()), rank_order.end());
  }
  for (ChunkID table_chunk = chunk_begin; table_chunk < chunk_end; ++table_chunk) {
    const ChunkID chunk_id = table_chunk - chunk_begin;
    const auto segment = table->get_chunk(table_chunk)->get_segment(column_id);
    hy_segment& d = column->descriptors[chunk_id];
    d.size = segment->size();
    d.data_type = static_cast<uint32_t>(segment->data_type());
    d.ref_chunk_id = 0xFFFFFFFFu;
    for (const auto& sorted_by : table->get_chunk(table_chunk)->individually_sorted_by()) {   // column_vs_value_table_scan_impl.cpp:46-55
      if (sorted_by.column == column_id) d.sorted_by = static_cast<uint32_t>(sorted_by.sort_mode) + 1;   // HY_SORT_* = SortMode + 1
    }
    bool ok = false;
    const auto describe_value = [&](auto* typed) {
      using T = std::decay_t<decltype(typed->values()[0])>;
      d.encoding = HY_ENC_UNENCODED; d.width = sizeof(T); d.data = typed->values().data();
      d.nulls = typed->is_nullable() ? typed->null_words().data() : nullptr;
      ok = true;
    };
    const auto describe_lz4 = [&](auto* typed) {   // the blocks as they are: the library decompresses them on the device
      using T = std::decay_t<decltype(typed->decompress()[0])>;
      d.encoding = HY_ENC_LZ4; d.width = sizeof(T); d.data = &typed->descriptor();
      d.nulls = typed->has_nulls() ? typed->null_words().data() : nullptr;
      ok = true;
    };
    const auto describe_dictionary = [&](auto* typed) {
      d.encoding = HY_ENC_DICTIONARY; d.width = typed->attribute_vector().width; d.data = typed->attribute_vector().bytes.data();
      d.aux = typed->dictionary().data(); d.aux_size = typed->unique_values_count();
      ok = true;
    };
    const auto describe_fetched = [&](auto* typed) {   // a chunk of a device-resident column on its own: through its host copy
      using T = std::decay_t<decltype(typed->values()[0])>;
      d.encoding = HY_ENC_UNENCODED; d.width = sizeof(T); d.data = typed->values().data();
      d.nulls = typed->null_words().data();
      ok = true;
    };
    if (const auto* s = dynamic_cast<const ValueSegment<int32_t>*>(segment.get())) describe_value(s);
    else if (const auto* s = dynamic_cast<const DeviceValueSegment<int32_t>*>(segment.get())) describe_fetched(s);
    else if (const auto* s = dynamic_cast<const DeviceValueSegment<int64_t>*>(segment.get())) describe_fetched(s);
    else if (const auto* s = dynamic_cast<const DeviceValueSegment<float>*>(segment.get())) describe_fetched(s);
    else if (const auto* s = dynamic_cast<const DeviceValueSegment<double>*>(segment.get())) describe_fetched(s);
    else if (const auto* s = dynamic_cast<const ValueSegment<int64_t>*>(segment.get())) describe_value(s);
    else if (const auto* s = dynamic_cast<const ValueSegment<float>*>(segment.get())) describe_value(s);
    else if (const auto* s = dynamic_cast<const ValueSegment<double>*>(segment.get())) describe_value(s);
    else if (const auto* s = dynamic_cast<const LZ4Segment<int32_t>*>(segment.get())) describe_lz4(s);
    else if (const auto* s = dynamic_cast<const LZ4Segment<int64_t>*>(segment.get())) describe_lz4(s);
    else if (const auto* s = dynamic_cast<const LZ4Segment<float>*>(segment.get())) describe_lz4(s);
    else if (const auto* s = dynamic_cast<const LZ4Segment<double>*>(segment.get())) describe_lz4(s);
    else if (const auto* s = dynamic_cast<const DictionarySegment<int32_t>*>(segment.get())) describe_dictionary(s);
    else if (const auto* s = dynamic_cast<const DictionarySegment<int64_t>*>(segment.get())) describe_dictionary(s);
    else if (const auto* s = dynamic_cast<const DictionarySegment<float>*>(segment.get())) describe_dictionary(s);
    else if (const auto* s = dynamic_cast<const DictionarySegment<double>*>(segment.get())) describe_dictionary(s);
    else if (const auto* s = dynamic_cast<const DictionarySegment<std::string>*>(segment.get())) {
      d.encoding = HY_ENC_DICTIONARY; d.width = s->attribute_vector().width; d.data = s->attribute_vector().bytes.data();
      d.aux_size = s->unique_values_count();
      if (string_keys != StringKeys::None) {   // GROUP BY / join key: the dictionary becomes int64 key names / join ids
        for (const auto& entry : s->dictionary()) {
          if (string_keys == StringKeys::Ranks) column->key_names[chunk_id].push_back(std::lower_bound(rank_order.begin(), rank_order.end(), entry) - rank_order.begin());
          else column->key_names[chunk_id].push_back(string_keys == StringKeys::JoinIds ? string_join_id(entry) : string_key_name(entry, long_strings));
        }
        d.aux = column->key_names[chunk_id].data();
        d.data_type = HY_TYPE_LONG;
      } else {
        d.aux = nullptr;   // scans compare value ids; literals are resolved per chunk by the caller
      }
      ok = true;
    } else if (const auto* s = string_keys == StringKeys::JoinIds ? dynamic_cast<const ValueSegment<std::string>*>(segment.get()) : nullptr) {
      // an unencoded string chunk as a join key: the rows' ids, one registry lookup per row (JoinHash's host route)
      for (ChunkOffset row = 0; row < s->size(); ++row) column->key_names[chunk_id].push_back(s->is_null(row) ? 0 : string_join_id(s->values()[row]));   // (a NULL row's placeholder gets no id)
      d.encoding = HY_ENC_UNENCODED; d.width = 8; d.data = column->key_names[chunk_id].data(); d.data_type = HY_TYPE_LONG;
      d.nulls = s->is_nullable() ? s->null_words().data() : nullptr;
      ok = true;
    } else if (const auto* s = dynamic_cast<const FrameOfReferenceSegment*>(segment.get())) {
      d.encoding = HY_ENC_FRAME_OF_REFERENCE; d.width = s->offset_values().width; d.data = s->offset_values().bytes.data();
      d.aux = s->block_minima().data(); d.aux_size = static_cast<uint32_t>(s->block_minima().size());
      d.nulls = s->has_nulls() ? s->null_words().data() : nullptr;
      ok = true;
    } else if (const auto* s = dynamic_cast<const ReferenceSegment*>(segment.get())) {
      if (!referenced) referenced = device_column(s->referenced_table(), s->referenced_column_id(), string_keys);
      d.encoding = HY_ENC_REFERENCE; d.width = 8; d.ref = referenced->handle;
      if (string_keys != StringKeys::None && s->data_type() == DataType::String) d.data_type = HY_TYPE_LONG;
      describe_pos_list(*s->pos_list(), d, host_lists, device_lists);
      ok = true;
    }
    if (!ok) Fail("segment kind not handled by the device path (the Hyrise adapter keeps the stock operator here)");
  }
  // PosLists that lie in HBM are read where they are (HY_MEM_DEVICE: a reference column's only buffers are its PosLists); a table that
  // mixes them with host PosLists is handed over from the host
  if (device_lists && host_lists) {
    for (ChunkID table_chunk = chunk_begin; table_chunk < chunk_end; ++table_chunk) {
      const auto* s = dynamic_cast<const ReferenceSegment*>(table->get_chunk(table_chunk)->get_segment(column_id).get());
      if (const auto* on_device = s ? dynamic_cast<const DevicePosList*>(s->pos_list().get()) : nullptr) column->descriptors[table_chunk - chunk_begin].data = on_device->host_rows();
    }
  }
  check_status(hy_column_create(column->descriptors.data(), chunk_count, device_lists && !host_lists ? HY_MEM_DEVICE : HY_MEM_HOST, &column->handle));
  return column;
}

inline std::shared_ptr<const DeviceColumnOwner> resident_column_of_chunks(const Table& table, ColumnID column_id, ChunkID chunk_begin, ChunkID chunk_end) {
  std::shared_ptr<const DeviceColumnOwner> owner;
  for (ChunkID k = chunk_begin; k < chunk_end; ++k) {
    const auto* segment = table.get_chunk(k)->get_segment(column_id).get();
    std::shared_ptr<const DeviceColumnOwner> of_segment;
    uint32_t index = 0;
    const auto look = [&](auto* typed) { if (typed) { of_segment = typed->owner(); index = typed->chunk_index(); } };
    look(dynamic_cast<const DeviceValueSegment<int32_t>*>(segment));
    look(dynamic_cast<const DeviceValueSegment<int64_t>*>(segment));
    look(dynamic_cast<const DeviceValueSegment<float>*>(segment));
    look(dynamic_cast<const DeviceValueSegment<double>*>(segment));
    look(dynamic_cast<const DeviceStringDictionarySegment*>(segment));
    if (!of_segment || index != k - chunk_begin || (owner && owner != of_segment)) return nullptr;
    owner = of_segment;
  }
  if (!owner) return nullptr;
  uint32_t chunks_of_column = 0;
  check_status(hy_column_chunk_count(owner->handle, &chunks_of_column));
  return chunks_of_column == chunk_end - chunk_begin ? owner : nullptr;
}

// StringKeys::Ranks of a whole column: ranked on the device (hy_column_string_ranks); false: on the host, by sorting the dictionaries' entries
// (tests and tools/string_order_time.py run both).
inline bool& device_string_ranking() { static bool enabled = true; return enabled; }
inline std::shared_ptr<DeviceColumn> device_string_rank_column(const std::shared_ptr<const Table>& table, ColumnID column_id);

inline std::shared_ptr<DeviceColumn> device_column(const std::shared_ptr<const Table>& table, ColumnID column_id, StringKeys string_keys) {
  if (!table->device_columns) table->device_columns = std::make_shared<ColumnCache>();
  auto& slot = table->device_columns->columns[{column_id, string_keys}];
  if (slot && string_keys == StringKeys::Ranks && slot->device_ranking != device_string_ranking()) slot = nullptr;   // (made under the other setting)
  if (!slot && string_keys == StringKeys::Ranks && device_string_ranking()) slot = device_string_rank_column(table, column_id);
  if (!slot) {
    slot = device_column_of_chunks(table, column_id, string_keys, 0, table->chunk_count());
    slot->device_ranking = device_string_ranking();
  }
  return slot;
}

// One chunk's dictionary as hy_string_dictionary_chunk takes a pmr_vector<pmr_string>: the entries' bytes back to back, n + 1 offsets.
inline void pack_string_dictionary(const std::vector<std::string>& dictionary, std::string& chars, std::vector<uint32_t>& offsets) {
  chars.clear();
  offsets.assign(1, 0);
  for (const auto& entry : dictionary) {
    chars.append(entry);
    Assert(chars.size() < (uint64_t{1} << 32), "a chunk's dictionary of 4 GiB or more");
    offsets.push_back(static_cast<uint32_t>(chars.size()));
  }
}

// The residency cache's string dictionaries: packed and uploaded once per (data table, column), dropped with the table.
inline std::shared_ptr<DeviceStringDictionary> device_string_dictionary(const std::shared_ptr<const Table>& table, ColumnID column_id) {
  if (!table->device_columns) table->device_columns = std::make_shared<ColumnCache>();
  auto& slot = table->device_columns->string_dictionaries[column_id];
  if (slot) return slot;
  const auto chunk_count = table->chunk_count();
  {   // every chunk of one gathered column: its dictionary, where it lies
    std::shared_ptr<const DeviceStringResult> resident;
    bool whole = chunk_count > 0;
    for (ChunkID c = 0; c < chunk_count && whole; ++c) {
      const auto* segment = dynamic_cast<const DeviceStringDictionarySegment*>(table->get_chunk(c)->get_segment(column_id).get());
      whole = segment && segment->chunk_index() == c && (!resident || resident == segment->result());
      if (whole) resident = segment->result();
    }
    uint32_t chunks_of_column = 0;
    if (whole) check_status(hy_column_chunk_count(resident->column->handle, &chunks_of_column));
    if (whole && chunks_of_column == chunk_count) {
      auto dictionary = std::make_shared<DeviceStringDictionary>();
      dictionary->handle = resident->dictionary;
      dictionary->resident = resident;
      slot = dictionary;
      return slot;
    }
  }
  std::vector<std::string> chars(chunk_count);
  std::vector<std::vector<uint32_t>> offsets(chunk_count);
  std::vector<hy_string_dictionary_chunk> chunks(chunk_count);
  for (ChunkID c = 0; c < chunk_count; ++c) {
    const auto* segment = dynamic_cast<const DictionarySegment<std::string>*>(table->get_chunk(c)->get_segment(column_id).get());
    Assert(segment, "unencoded string segments stay on the CPU path");
    pack_string_dictionary(segment->dictionary(), chars[c], offsets[c]);
    chunks[c].n_entries = static_cast<uint32_t>(segment->dictionary().size());
    chunks[c].string_length = 0;
    chunks[c].chars = chars[c].data();
    chunks[c].offsets = offsets[c].data();
  }
  auto dictionary = std::make_shared<DeviceStringDictionary>();
  check_status(hy_string_dictionary_create(chunks.data(), chunk_count, HY_MEM_HOST, &dictionary->handle));
  slot = dictionary;
  return slot;
}

// A string column as a sort key without any string work on the host: every chunk a DictionarySegment<pmr_string>, or a ReferenceSegment over
// one column of such chunks.  The column goes to the device as it does for a scan (value ids alone, or PosLists over them), its data
// column's dictionaries as they do for LIKE, and hy_column_string_ranks orders them in HBM and hands back the int32 stand-in, which reads the
// string column's buffers in place.  nullptr: not such a column, or the library refused it -- the caller ranks on the host.
// Is the column a string column whose every chunk is a DictionarySegment<pmr_string>, or a ReferenceSegment over one column of such chunks?
// Then data_table / data_column_id name the column that holds the dictionaries.
inline bool string_dictionary_column(const std::shared_ptr<const Table>& table, ColumnID column_id, std::shared_ptr<const Table>& data_table, ColumnID& data_column_id) {
  const auto chunk_count = table->chunk_count();
  if (chunk_count == 0 || table->column_data_type(column_id) != DataType::String) return false;
  data_table = table;
  data_column_id = column_id;
  if (const auto* first = dynamic_cast<const ReferenceSegment*>(table->get_chunk(0)->get_segment(column_id).get())) {
    data_table = first->referenced_table();
    data_column_id = first->referenced_column_id();
    for (ChunkID k = 0; k < chunk_count; ++k) {
      const auto* segment = dynamic_cast<const ReferenceSegment*>(table->get_chunk(k)->get_segment(column_id).get());
      if (!segment || segment->referenced_table() != data_table || segment->referenced_column_id() != data_column_id) return false;
    }
  }
  if (data_table->chunk_count() == 0) return false;
  for (ChunkID k = 0; k < data_table->chunk_count(); ++k) {
    if (!dynamic_cast<const DictionarySegment<std::string>*>(data_table->get_chunk(k)->get_segment(data_column_id).get())) return false;
  }
  return true;
}

inline std::shared_ptr<DeviceColumn> device_string_rank_column(const std::shared_ptr<const Table>& table, ColumnID column_id) {
  std::shared_ptr<const Table> data_table;
  ColumnID data_column_id = column_id;
  if (!string_dictionary_column(table, column_id, data_table, data_column_id)) return nullptr;
  auto column = std::make_shared<DeviceColumn>();
  column->strings = device_column(table, column_id, StringKeys::None);
  const auto dictionary = device_string_dictionary(data_table, data_column_id);
  if (hy_column_string_ranks(column->strings->handle, dictionary->handle, &column->handle) != HY_OK) return nullptr;
  return column;
}

// The keys two string columns join on, made on the device (hy_column_string_join_keys); false: JoinHash's ids come from string_join_id on the
// host, and JoinSortMerge does not take string keys (tests/cpp/string_join_keys_tests.cpp runs both).
inline bool& device_string_join_keys() { static bool enabled = true; return enabled; }
inline std::atomic<uint64_t>& device_string_join_key_pairs() { static std::atomic<uint64_t> pairs{0}; return pairs; }   // joins whose keys hy_column_string_join_keys made

// The stand-ins of a pair of string key columns -- HY_STRING_KEYS_HASH_IDS for JoinHash, HY_STRING_KEYS_RANKS for JoinSortMerge -- without any
// string work on the host: both columns wholly dictionary-encoded (string_dictionary_column), each sent as it is for a scan, its data
// column's dictionaries as they are for LIKE.  The stand-ins belong to the join, not to the column cache: they depend on the partner column.
// false: the switch is off, one of the columns is not such a column, or the library refused the pair -- the caller takes its host route.
inline bool device_string_join_key_columns(const std::shared_ptr<const Table>& left, ColumnID left_id, const std::shared_ptr<const Table>& right, ColumnID right_id, uint32_t kind,
                                           std::shared_ptr<DeviceColumn>& left_keys, std::shared_ptr<DeviceColumn>& right_keys) {
  if (!device_string_join_keys()) return false;
  std::shared_ptr<const Table> left_data, right_data;
  ColumnID left_data_id = left_id, right_data_id = right_id;
  if (!string_dictionary_column(left, left_id, left_data, left_data_id) || !string_dictionary_column(right, right_id, right_data, right_data_id)) return false;
  auto l = std::make_shared<DeviceColumn>(), r = std::make_shared<DeviceColumn>();
  l->strings = device_column(left, left_id, StringKeys::None);
  r->strings = device_column(right, right_id, StringKeys::None);
  const auto left_dictionary = device_string_dictionary(left_data, left_data_id), right_dictionary = device_string_dictionary(right_data, right_data_id);
  if (hy_column_string_join_keys(l->strings->handle, left_dictionary->handle, r->strings->handle, right_dictionary->handle, kind, &l->handle, &r->handle) != HY_OK) return false;
  device_string_join_key_pairs().fetch_add(1, std::memory_order_relaxed);
  left_keys = l;
  right_keys = r;
  return true;
}

// LIKE scans match their dictionaries on the device (hy_table_scan_like); false: on the host, bitmaps through hy_predicate.match_words.
inline bool& device_like_matching() { static bool enabled = true; return enabled; }

// ---- operators ---------------------------------------------------------------------------------------------------------
class AbstractOperator {   // operators/abstract_operator.hpp
 public:
  AbstractOperator(std::shared_ptr<const AbstractOperator> left = nullptr, std::shared_ptr<const AbstractOperator> right = nullptr)
      : _left_input(std::move(left)), _right_input(std::move(right)) {}
  virtual ~AbstractOperator() = default;
  virtual const std::string& name() const = 0;
  void execute() {   // abstract_operator.cpp:78-136
    Assert(!_executed, "Operator has already been executed.");
    _output = _on_execute();
    _executed = true;
  }
  std::shared_ptr<const Table> get_output() const { Assert(_executed, "Operator has not been executed."); return _output; }
  std::shared_ptr<const Table> left_input_table() const { return _left_input->get_output(); }
  std::shared_ptr<const Table> right_input_table() const { return _right_input->get_output(); }
  void never_clear_output() {}

 protected:
  virtual std::shared_ptr<const Table> _on_execute() = 0;
  std::shared_ptr<const AbstractOperator> _left_input, _right_input;
  std::shared_ptr<const Table> _output;
  bool _executed = false;
};
using AbstractReadOnlyOperator = AbstractOperator;   // abstract_read_only_operator.hpp:18-22: ignores the transaction context

class TableWrapper : public AbstractReadOnlyOperator {   // operators/table_wrapper.hpp
 public:
  explicit TableWrapper(std::shared_ptr<const Table> table) : _table(std::move(table)) {}
  const std::string& name() const override { static const std::string n = "TableWrapper"; return n; }

 protected:
  std::shared_ptr<const Table> _on_execute() override { return _table; }
  std::shared_ptr<const Table> _table;
};

inline hy_value to_hy_value(const AllTypeVariant& v) {
  hy_value out{};
  switch (v.index()) {
    case 1: out.i32 = std::get<int32_t>(v); break;
    case 2: out.i64 = std::get<int64_t>(v); break;
    case 3: out.f32 = std::get<float>(v); break;
    case 4: out.f64 = std::get<double>(v); break;
    default: break;
  }
  return out;
}

inline bool is_between(PredicateCondition c) { return c >= PredicateCondition::BetweenInclusive && c <= PredicateCondition::BetweenExclusive; }

// The result buffers of a scan-shaped call (hy_table_scan / hy_table_scan_columns / hy_validate) in HBM: HY_SCAN_CHUNK_REGIONS -- chunk c's
// PosList starts at matches + row_base[c] and holds counts[c] RowIDs -- so the output table's PosLists are views into ONE pooled block.
// What the host needs to assemble the output table (table_scan.cpp:129-220 looks at every chunk's match count) are the counts and chunk
// states: five bytes per chunk cross the link, the RowIDs do not.
struct DeviceScanOutput {
  std::shared_ptr<DeviceBlock> matches, bookkeeping;
  std::vector<uint64_t> row_base;
  std::vector<uint32_t> counts;
  std::vector<uint8_t> states;
  hy_scan_result result{};
  uint64_t rows = 0;

  DeviceScanOutput(const Table& in_table, bool materialize_all_match) {
    const auto chunk_count = in_table.chunk_count();
    row_base.assign(size_t{chunk_count} + 1, 0);
    for (ChunkID c = 0; c < chunk_count; ++c) row_base[c + 1] = row_base[c] + in_table.get_chunk(c)->size();
    rows = row_base[chunk_count];
    counts.assign(std::max<ChunkID>(1, chunk_count), 0);
    states.assign(std::max<ChunkID>(1, chunk_count), 0);
    matches = DeviceBlock::acquire(std::max<uint64_t>(1, rows) * sizeof(RowID));
    const size_t n = std::max<ChunkID>(1, chunk_count);
    bookkeeping = DeviceBlock::acquire(8 * (n + 1) + 5 * n + 16);
    auto* base = static_cast<char*>(bookkeeping->ptr);
    result.mem = HY_MEM_DEVICE;
    result.flags = HY_SCAN_CHUNK_REGIONS | (materialize_all_match ? HY_SCAN_MATERIALIZE_ALL_MATCH : 0u);
    result.matches = static_cast<hy_row_id*>(matches->ptr);
    result.capacity = std::max<uint64_t>(1, rows);
    result.offsets = reinterpret_cast<uint64_t*>(base);
    result.counts = reinterpret_cast<uint32_t*>(base + 8 * (n + 1));
    result.chunk_state = reinterpret_cast<uint8_t*>(base + 8 * (n + 1) + 4 * n);
  }
  // after the call: counts and states of every chunk, one transfer (waits for the calling thread's stream: the PosLists are complete)
  void fetch(ChunkID chunk_count) {
    const size_t n = std::max<ChunkID>(1, chunk_count);
    std::vector<char> staged(5 * n);
    check_status(hy_memcpy_d2h(staged.data(), result.counts, 5 * n));
    std::memcpy(counts.data(), staged.data(), 4 * n);
    std::memcpy(states.data(), staged.data() + 4 * n, n);
  }
  std::shared_ptr<AbstractPosList> pos_list_of(ChunkID chunk_id) const {
    return std::make_shared<DevicePosList>(matches, result.matches + row_base[chunk_id], counts[chunk_id], true, chunk_id);
  }
};

// A scan over a reference table hands on PosLists into the DATA table: its matches are translated through the input's PosLists, once per
// distinct PosList (table_scan.cpp:158-196).  Here: once per group of columns that share their PosLists in every chunk, by ONE
// hy_poslist_translate into a pooled block (chunk regions: chunk c's translated list at block + row_base[c]).  `out` must have been
// produced with materialize_all_match.  group_of_column[c] indexes `blocks`; a null block: that group's columns are not describable to
// the device (the caller translates on the host through the lazy copies).
inline void translate_through_input_lists(const std::shared_ptr<const Table>& in_table, const DeviceScanOutput& out, std::vector<size_t>& group_of_column,
                                          std::vector<std::shared_ptr<DeviceBlock>>& blocks) {
  std::map<std::vector<const AbstractPosList*>, size_t> groups;
  group_of_column.clear();
  blocks.clear();
  for (ColumnID c = 0; c < in_table->column_count(); ++c) {
    std::vector<const AbstractPosList*> key;
    for (ChunkID k = 0; k < in_table->chunk_count(); ++k) key.push_back(std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(k)->get_segment(c))->pos_list().get());
    const auto [it, inserted] = groups.emplace(std::move(key), blocks.size());
    group_of_column.push_back(it->second);
    if (!inserted) continue;
    std::shared_ptr<DeviceBlock> block;
    try {
      const auto through = device_column(in_table, c);
      block = DeviceBlock::acquire(std::max<uint64_t>(1, out.rows) * sizeof(RowID));
      uint64_t written = 0;
      check_status(hy_poslist_translate(through->handle, &out.result, HY_POSLIST_CHUNK_REGIONS, static_cast<hy_row_id*>(block->ptr), std::max<uint64_t>(1, out.rows), &written));
    } catch (const std::logic_error&) {
      block = nullptr;
    }
    blocks.push_back(std::move(block));
  }
}

// TableScan over `column <condition> value [AND value2]` / `column IS [NOT] NULL` / `column <condition> column2`
// (the shapes create_impl maps to ColumnVsValue / ColumnBetween / ColumnIsNull / ColumnVsColumn, table_scan.cpp:312-452).
// LikeMatcher (expression/evaluation/like_matcher.hpp): `%` any run of chars, `_` one char, the rest literal; the
// *Insensitive conditions lower-case pattern and input.  Iterative two-pointer match instead of the reference's
// token/regex variants -- same language, no std::regex.
class LikeMatcher {
 public:
  LikeMatcher(std::string pattern, PredicateCondition condition) : _pattern(std::move(pattern)) {
    Assert(condition == PredicateCondition::Like || condition == PredicateCondition::NotLike || condition == PredicateCondition::LikeInsensitive ||
               condition == PredicateCondition::NotLikeInsensitive, "Expected PredicateCondition (Not)Like or (Not)LikeInsensitive.");
    _insensitive = condition == PredicateCondition::LikeInsensitive || condition == PredicateCondition::NotLikeInsensitive;
    _negated = condition == PredicateCondition::NotLike || condition == PredicateCondition::NotLikeInsensitive;
    if (_insensitive) to_lower(_pattern);
  }
  bool operator()(const std::string& input) const {
    if (!_insensitive) return matches(input) != _negated;
    auto lowered = input;
    to_lower(lowered);
    return matches(lowered) != _negated;
  }

 private:
  static void to_lower(std::string& s) { for (auto& c : s) if (c >= 'A' && c <= 'Z') c = static_cast<char>(c - 'A' + 'a'); }
  bool matches(const std::string& text) const {
    size_t t = 0, p = 0, star = std::string::npos, resume = 0;
    while (t < text.size()) {
      if (p < _pattern.size() && _pattern[p] == '%') { star = p++; resume = t; }
      else if (p < _pattern.size() && (_pattern[p] == '_' || _pattern[p] == text[t])) { ++p; ++t; }
      else if (star != std::string::npos) { p = star + 1; t = ++resume; }
      else return false;
    }
    while (p < _pattern.size() && _pattern[p] == '%') ++p;
    return p == _pattern.size();
  }
  std::string _pattern;
  bool _insensitive = false, _negated = false;
};

struct Expression;   // (defined with Projection, below)

class TableScan : public AbstractReadOnlyOperator {
 public:
  // A predicate expression: the scan create_impl leaves to ExpressionEvaluatorTableScanImpl (table_scan.cpp:450-451), on the device through
  // hy_table_scan_expression (scan_expression(), defined behind Projection, whose lowering it uses)
  TableScan(std::shared_ptr<const AbstractOperator> in, std::shared_ptr<const Expression> predicate) : AbstractReadOnlyOperator(std::move(in)), _predicate(std::move(predicate)) {
    Assert(_predicate != nullptr, "TableScan: a predicate expression is needed");
  }
  TableScan(std::shared_ptr<const AbstractOperator> in, ColumnID column_id, PredicateCondition condition, AllTypeVariant value = NullValue{},
            std::optional<AllTypeVariant> value2 = std::nullopt)
      : AbstractReadOnlyOperator(std::move(in)), _column_id(column_id), _condition(condition), _value(std::move(value)), _value2(std::move(value2)) {}
  TableScan(std::shared_ptr<const AbstractOperator> in, ColumnID left_column, PredicateCondition condition, ColumnID right_column, bool /*column_vs_column*/)
      : AbstractReadOnlyOperator(std::move(in)), _column_id(left_column), _condition(condition), _right_column_id(right_column) {}
  // `column IN (list)` / `column NOT IN (list)` over literals (PredicateCondition::In / NotIn): the InExpressions the optimizer leaves
  // to the ExpressionEvaluator (expression_evaluator.cpp:404-506), on the device through hy_table_scan_in_list
  TableScan(std::shared_ptr<const AbstractOperator> in, ColumnID column_id, PredicateCondition condition, std::vector<AllTypeVariant> list)
      : AbstractReadOnlyOperator(std::move(in)), _column_id(column_id), _condition(condition), _list(std::move(list)) {
    Assert(condition == PredicateCondition::In || condition == PredicateCondition::NotIn, "A literal list belongs to In / NotIn.");
  }
  const std::string& name() const override { static const std::string n = "TableScan"; return n; }
  std::vector<ChunkID> excluded_chunk_ids;
  size_t num_chunks_with_early_out = 0, num_chunks_with_all_rows_matching = 0;   // TableScan::PerformanceData (table_scan.hpp:56-69)

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto in_table = left_input_table();
    const auto chunk_count = in_table->chunk_count();
    const auto column = _predicate ? nullptr : device_column(in_table, _column_id);
    // Device-resident results (the default): the PosLists stay in a pooled block of HBM, the output table's ReferenceSegments hold
    // DevicePosLists into it.  Host results: the library copies the RowIDs back (the boundary as rounds 1-5 used it).
    std::unique_ptr<DeviceScanOutput> on_device;
    if (device_resident_results()) on_device = std::make_unique<DeviceScanOutput>(*in_table, in_table->type() == TableType::References);
    std::vector<RowID> matches(on_device ? 1 : std::max<uint64_t>(1, in_table->row_count()));
    std::vector<uint64_t> offsets(chunk_count + 1);
    std::vector<uint32_t> counts(std::max<ChunkID>(1, chunk_count));
    std::vector<uint8_t> states(std::max<ChunkID>(1, chunk_count));
    hy_scan_result result{};
    result.mem = HY_MEM_HOST;
    result.matches = reinterpret_cast<hy_row_id*>(matches.data());
    result.capacity = in_table->row_count();
    result.offsets = offsets.data();
    result.counts = counts.data();
    result.chunk_state = states.data();
    if (on_device) result = on_device->result;
    bool scan_done = false;
    if (_predicate) {
      if (!scan_expression(in_table, &result, counts, states)) on_device.reset();   // (a constant predicate: counts and states say all or nothing, no RowIDs are needed)
    } else if (_right_column_id) {
      const bool left_is_string = in_table->column_data_type(_column_id) == DataType::String;
      const bool right_is_string = in_table->column_data_type(*_right_column_id) == DataType::String;
      // column_vs_column_table_scan_impl.cpp:153-155
      Assert(left_is_string == right_is_string, "Trying to compare strings and non-strings");
      const auto right_column = device_column(in_table, *_right_column_id);
      if (left_is_string && chunk_count) {
        // Two string columns: their dictionaries are ordered against each other where they live, in HBM, and the row pass is the numeric
        // one (hy_table_scan_columns_strings).  The dictionaries are the data table's, as for LIKE.
        auto data_table = in_table;
        auto left_data_column_id = _column_id, right_data_column_id = *_right_column_id;
        if (in_table->type() == TableType::References) {
          const auto left_ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(_column_id));
          const auto right_ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(*_right_column_id));
          Assert(left_ref->referenced_table() == right_ref->referenced_table(), "string ColumnVsColumn scans over columns of two referenced tables stay on the CPU path");
          data_table = left_ref->referenced_table();
          left_data_column_id = left_ref->referenced_column_id();
          right_data_column_id = right_ref->referenced_column_id();
        }
        const auto left_dictionary = device_string_dictionary(data_table, left_data_column_id);
        const auto right_dictionary = device_string_dictionary(data_table, right_data_column_id);
        check_status(hy_table_scan_columns_strings(column->handle, left_dictionary->handle, right_column->handle, right_dictionary->handle, static_cast<uint32_t>(_condition), &result));
      } else {
        check_status(hy_table_scan_columns(column->handle, right_column->handle, static_cast<uint32_t>(_condition), &result));
      }
    } else {
      hy_predicate predicate{};
      predicate.condition = static_cast<uint32_t>(_condition);
      predicate.column_is_nullable = in_table->column_is_nullable(_column_id);
      const bool null_test = _condition == PredicateCondition::IsNull || _condition == PredicateCondition::IsNotNull;
      std::vector<uint32_t> lower, upper;
      std::vector<uint8_t> found;
      const bool like = _condition == PredicateCondition::Like || _condition == PredicateCondition::NotLike ||
                        _condition == PredicateCondition::LikeInsensitive || _condition == PredicateCondition::NotLikeInsensitive;
      std::vector<uint64_t> match_words, match_word_offsets;
      const bool in_list = _condition == PredicateCondition::In || _condition == PredicateCondition::NotIn;
      if (in_list) {
        // The ABI takes the evaluator's fast path only (a non-empty list of non-NULL literals of the column's type); what is constant is
        // answered here: `x IN ()` is false and `x NOT IN ()` true for every row (expression_evaluator.cpp:415-419), a NULL element leaves IN
        // as it is and makes NOT IN match nothing, a list without any element that can equal a row matches nothing (IN) / every non-NULL row.
        const bool negated = _condition == PredicateCondition::NotIn;
        const auto column_type = in_table->column_data_type(_column_id);
        std::vector<hy_value> values(_list.size() + 1);
        std::vector<uint32_t> value_ids;
        uint32_t n_values = 0, has_null = 0;
        if (column_type == DataType::String) {
          std::vector<std::string> strings;
          for (const auto& element : _list) {
            if (variant_is_null(element)) has_null = 1;
            else if (std::holds_alternative<std::string>(element)) strings.push_back(std::get<std::string>(element));   // (a number equals no string)
          }
          n_values = static_cast<uint32_t>(strings.size());
          resolve_string_list(in_table, _column_id, strings, value_ids);
        } else {
          std::vector<uint32_t> types;
          std::vector<hy_value> literals;
          for (const auto& element : _list) {
            types.push_back(static_cast<uint32_t>(data_type_from_all_type_variant(element)));
            literals.push_back(element.index() >= 1 && element.index() <= 4 ? to_hy_value(element) : hy_value{});
          }
          check_status(hy_in_list_cast(static_cast<uint32_t>(column_type), types.data(), literals.data(), static_cast<uint32_t>(_list.size()), values.data(), &n_values, &has_null));
        }
        enum class Constant { No, NoRows, AllRows, NotNullRows } constant = Constant::No;
        if (chunk_count == 0) constant = Constant::NoRows;   // (a table without chunks has no rows to test, and its device column no type)
        else if (_list.empty()) constant = negated ? Constant::AllRows : Constant::NoRows;
        else if (negated && has_null) constant = Constant::NoRows;
        else if (n_values == 0) constant = negated ? Constant::NotNullRows : Constant::NoRows;
        if (constant == Constant::NoRows || constant == Constant::AllRows) {
          on_device.reset();
          for (ChunkID c = 0; c < chunk_count; ++c) {
            const bool excluded = std::find(excluded_chunk_ids.begin(), excluded_chunk_ids.end(), c) != excluded_chunk_ids.end();
            counts[c] = constant == Constant::AllRows && !excluded ? in_table->get_chunk(c)->size() : 0;
            states[c] = counts[c] ? HY_CHUNK_ALL_MATCH : HY_CHUNK_NONE_MATCH;
          }
          scan_done = true;   // (nothing to evaluate: no RowIDs are needed for chunks that match entirely or not at all)
        } else if (constant == Constant::NotNullRows) {
          predicate.condition = HY_PRED_IS_NOT_NULL;
        } else {
          if (n_values > HY_MAX_IN_LIST) throw std::logic_error("TableScan: IN lists of more than HY_MAX_IN_LIST elements are semi joins (InExpressionRewriteRule)");
          hy_in_list list{};
          list.value_type = static_cast<uint32_t>(column_type);
          list.n_values = n_values;
          list.values = values.data();
          list.negated = negated;
          list.column_is_nullable = in_table->column_is_nullable(_column_id);
          list.per_chunk_value_ids = column_type == DataType::String ? value_ids.data() : nullptr;
          check_status(hy_table_scan_in_list(column->handle, &list, excluded_chunk_ids.data(), static_cast<uint32_t>(excluded_chunk_ids.size()), &result));
          scan_done = true;   // (the scan has run)
        }
      } else if (like) {
        // ColumnLikeTableScanImpl (column_like_table_scan_impl.cpp:28-36)
        Assert(in_table->column_data_type(_column_id) == DataType::String, "LIKE operator only applicable on string columns.");
        Assert(std::holds_alternative<std::string>(_value), "Right parameter must be a string.");
        // The dictionaries are matched where they live, in HBM (hy_table_scan_like); the host matcher keeps what the library refuses
        // (a pattern beyond HY_MAX_LIKE_PATTERN) and everything when device_like_matching() is off.
        if (device_like_matching() && chunk_count) {
          auto data_table = in_table;
          auto data_column_id = _column_id;
          if (in_table->type() == TableType::References) {
            const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(_column_id));
            data_table = ref->referenced_table();
            data_column_id = ref->referenced_column_id();
          }
          const auto dictionary = device_string_dictionary(data_table, data_column_id);
          const auto& pattern = std::get<std::string>(_value);
          const auto status = hy_table_scan_like(column->handle, dictionary->handle, pattern.data(), static_cast<uint32_t>(pattern.size()), static_cast<uint32_t>(_condition),
                                                 predicate.column_is_nullable, excluded_chunk_ids.data(), static_cast<uint32_t>(excluded_chunk_ids.size()), &result);
          if (status != HY_ERR_UNSUPPORTED) {
            check_status(status);
            scan_done = true;   // (the scan has run)
          }
        }
        if (!scan_done) find_matches_in_dictionaries(in_table, _column_id, _condition, _value, match_words, match_word_offsets, predicate);
      } else if (!null_test) {
        const auto column_type = in_table->column_data_type(_column_id);
        if (column_type == DataType::String) {
          // ColumnVsValueTableScanImpl asserts matching types (column_vs_value_table_scan_impl.cpp:34-36)
          Assert(data_type_from_all_type_variant(_value) == DataType::String, "Cannot scan: column and value data type do not match.");
          predicate.value_type = static_cast<uint32_t>(DataType::String);
          resolve_string_literal(in_table, _column_id, _condition, _value, _value2, lower, upper, found, predicate);
        } else {
          // TableScan::create_impl casts the literal(s) to the column's type, adjusting the condition where only that is
          // lossless (table_scan.cpp:336-366, 406-448); where neither works the stock ExpressionEvaluator scan runs.
          const hy_value first = to_hy_value(_value), second = _value2 ? to_hy_value(*_value2) : hy_value{};
          hy_predicate cast{};
          const auto status = hy_predicate_cast(static_cast<uint32_t>(_condition), static_cast<uint32_t>(column_type), static_cast<uint32_t>(data_type_from_all_type_variant(_value)),
                                                &first, _value2 ? static_cast<uint32_t>(data_type_from_all_type_variant(*_value2)) : HY_TYPE_NULL, _value2 ? &second : nullptr, &cast);
          const auto numeric_literal = [](const AllTypeVariant& v) { return v.index() >= 1 && v.index() <= 4; };
          // a string literal against a numeric column is an invalid plan, not a scan for the evaluator (table_scan_test.cpp:383-405: std::logic_error)
          Assert(status != HY_ERR_UNSUPPORTED || (numeric_literal(_value) && (!_value2 || numeric_literal(*_value2))), "Cannot scan: column and value data type do not match.");
          if (status == HY_ERR_UNSUPPORTED) {
            // No lossless cast (`float_column = 3.1`, `int_column < 3.5`, a literal outside the column type's range): the reference falls
            // back to its ExpressionEvaluator scan (table_scan.cpp:346-366, 450), and so does the adapter -- the stock operator runs.
            // The mirror's stand-in for it: every row compared with the literal in the common type (expression_functors.hpp).
            on_device.reset();
            matches.resize(std::max<uint64_t>(1, in_table->row_count()));
            evaluate_on_host(in_table, matches, offsets, counts, states);
            scan_done = true;
          } else {
            check_status(status);
            predicate.condition = cast.condition, predicate.value_type = cast.value_type, predicate.value = cast.value, predicate.value2 = cast.value2;
          }
        }
      }
      if (!scan_done) check_status(hy_table_scan(column->handle, &predicate, excluded_chunk_ids.data(), static_cast<uint32_t>(excluded_chunk_ids.size()), &result));
    }
    // ---- output assembly, table_scan.cpp:129-220 ----
    std::vector<size_t> group_of_column;
    std::vector<std::shared_ptr<DeviceBlock>> translated;
    const RowID* device_matches_on_host = nullptr;   // (only for column groups the device could not translate)
    if (on_device) {
      on_device->fetch(chunk_count);
      counts = on_device->counts;
      states = on_device->states;
      offsets = on_device->row_base;   // (chunk regions)
      bool any_partial = false;
      for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) any_partial = any_partial || (counts[chunk_id] && counts[chunk_id] != in_table->get_chunk(chunk_id)->size());
      if (in_table->type() == TableType::References && any_partial) {
        translate_through_input_lists(in_table, *on_device, group_of_column, translated);
        if (std::any_of(translated.begin(), translated.end(), [](const auto& b) { return !b; })) {
          on_device->matches->prefetch_to_host(on_device->rows);
          device_matches_on_host = on_device->matches->host_copy();
        }
      }
    }
    std::vector<std::shared_ptr<Chunk>> output_chunks;
    for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
      if (states[chunk_id] == HY_CHUNK_NONE_MATCH) ++num_chunks_with_early_out;
      if (states[chunk_id] == HY_CHUNK_ALL_MATCH) ++num_chunks_with_all_rows_matching;
      if (counts[chunk_id] == 0) continue;   // :132-134
      const auto chunk_in = in_table->get_chunk(chunk_id);
      const bool all = counts[chunk_id] == chunk_in->size();
      Segments out_segments;
      if (in_table->type() == TableType::References) {
        if (all) {   // forward the chunk (:151-156)
          for (ColumnID c = 0; c < in_table->column_count(); ++c) out_segments.push_back(chunk_in->get_segment(c));
        } else {     // translate through every distinct input pos list once (:158-196)
          std::map<const AbstractPosList*, std::shared_ptr<AbstractPosList>> filtered;
          for (ColumnID c = 0; c < in_table->column_count(); ++c) {
            const auto ref = std::static_pointer_cast<ReferenceSegment>(chunk_in->get_segment(c));
            auto& list = filtered[ref->pos_list().get()];
            if (!list && on_device && translated[group_of_column[c]]) {   // already translated, in HBM
              const auto& block = translated[group_of_column[c]];
              list = std::make_shared<DevicePosList>(block, static_cast<const hy_row_id*>(block->ptr) + offsets[chunk_id], counts[chunk_id], ref->pos_list()->references_single_chunk(),
                                                     ref->pos_list()->common_chunk_id());
            } else if (!list) {
              const RowID* chunk_matches = on_device ? device_matches_on_host + offsets[chunk_id] : matches.data() + offsets[chunk_id];
              auto rows = std::make_shared<RowIDPosList>();
              for (uint64_t m = 0; m < counts[chunk_id]; ++m) rows->rows.push_back((*ref->pos_list())[chunk_matches[m].chunk_offset]);
              if (ref->pos_list()->references_single_chunk()) rows->guarantee_single_chunk();
              list = rows;
            }
            out_segments.push_back(std::make_shared<ReferenceSegment>(ref->referenced_table(), ref->referenced_column_id(), list));
          }
        }
      } else {
        std::shared_ptr<AbstractPosList> pos_list;
        if (all) pos_list = std::make_shared<EntireChunkPosList>(chunk_id, chunk_in->size());   // :201-205
        else if (on_device) pos_list = on_device->pos_list_of(chunk_id);
        else {
          auto rows = std::make_shared<RowIDPosList>(std::vector<RowID>(matches.begin() + offsets[chunk_id], matches.begin() + offsets[chunk_id + 1]));
          rows->guarantee_single_chunk();
          pos_list = rows;
        }
        for (ColumnID c = 0; c < in_table->column_count(); ++c) out_segments.push_back(std::make_shared<ReferenceSegment>(in_table, c, pos_list));
      }
      output_chunks.push_back(std::make_shared<Chunk>(std::move(out_segments)));
    }
    return std::make_shared<Table>(in_table->column_definitions(), TableType::References, std::move(output_chunks));
  }

 private:
  // The stock scan's stand-in (see _on_execute): a numeric column against numeric literals, row by row, both sides in the common type
  // (two integers: int64; otherwise double -- what the ExpressionEvaluator's comparison functors promote to).  NULL matches nothing.
  void evaluate_on_host(const std::shared_ptr<const Table>& in_table, std::vector<RowID>& matches, std::vector<uint64_t>& offsets, std::vector<uint32_t>& counts,
                        std::vector<uint8_t>& states) const {
    const auto as_double = [](const AllTypeVariant& v) {
      return std::visit([](const auto& x) -> double { if constexpr (std::is_arithmetic_v<std::decay_t<decltype(x)>>) return static_cast<double>(x); else return 0.0; }, v);
    };
    const auto integral = [](const AllTypeVariant& v) { return v.index() == 1 || v.index() == 2; };
    const auto as_long = [](const AllTypeVariant& v) { return v.index() == 1 ? static_cast<int64_t>(std::get<int32_t>(v)) : std::get<int64_t>(v); };
    const auto compare = [&](const AllTypeVariant& cell, const AllTypeVariant& literal) {   // -1, 0, 1
      if (integral(cell) && integral(literal)) { const int64_t a = as_long(cell), b = as_long(literal); return a < b ? -1 : a > b ? 1 : 0; }
      const double a = as_double(cell), b = as_double(literal);
      return a < b ? -1 : a > b ? 1 : 0;
    };
    const auto matches_row = [&](const AllTypeVariant& cell) {
      if (variant_is_null(cell)) return false;
      const int first = compare(cell, _value);
      switch (_condition) {
        case PredicateCondition::Equals: return first == 0;
        case PredicateCondition::NotEquals: return first != 0;
        case PredicateCondition::LessThan: return first < 0;
        case PredicateCondition::LessThanEquals: return first <= 0;
        case PredicateCondition::GreaterThan: return first > 0;
        case PredicateCondition::GreaterThanEquals: return first >= 0;
        default: break;
      }
      Assert(_value2.has_value(), "BETWEEN needs two literals.");
      const int second = compare(cell, *_value2);
      const bool lower_inclusive = _condition == PredicateCondition::BetweenInclusive || _condition == PredicateCondition::BetweenUpperExclusive;
      const bool upper_inclusive = _condition == PredicateCondition::BetweenInclusive || _condition == PredicateCondition::BetweenLowerExclusive;
      return (lower_inclusive ? first >= 0 : first > 0) && (upper_inclusive ? second <= 0 : second < 0);
    };
    uint64_t written = 0;
    for (ChunkID chunk_id = 0; chunk_id < in_table->chunk_count(); ++chunk_id) {
      const auto segment = in_table->get_chunk(chunk_id)->get_segment(_column_id);
      offsets[chunk_id] = written;
      const bool excluded = std::find(excluded_chunk_ids.begin(), excluded_chunk_ids.end(), chunk_id) != excluded_chunk_ids.end();
      for (ChunkOffset offset = 0; !excluded && offset < segment->size(); ++offset) {
        if (matches_row((*segment)[offset])) matches[written++] = RowID{chunk_id, offset};
      }
      counts[chunk_id] = static_cast<uint32_t>(written - offsets[chunk_id]);
      states[chunk_id] = HY_CHUNK_SCANNED;
    }
    offsets[in_table->chunk_count()] = written;
  }

 public:   // (static: Projection lowers its string column tests through the same three functions)
  // DictionarySegment<pmr_string>: resolve the literal per chunk like _get_search_value_id
  // (column_vs_value_table_scan_impl.cpp:211-226) and column_between_table_scan_impl.cpp:112-124.
  static void resolve_string_literal(const std::shared_ptr<const Table>& in_table, ColumnID _column_id, PredicateCondition _condition, const AllTypeVariant& _value, const std::optional<AllTypeVariant>& _value2, std::vector<uint32_t>& lower,
                                     std::vector<uint32_t>& upper, std::vector<uint8_t>& found, hy_predicate& predicate) {
    auto data_table = in_table;
    auto column_id = _column_id;
    if (in_table->type() == TableType::References && in_table->chunk_count()) {
      const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(_column_id));
      data_table = ref->referenced_table();
      column_id = ref->referenced_column_id();
    }
    const auto& value = std::get<std::string>(_value);
    for (ChunkID c = 0; c < data_table->chunk_count(); ++c) {
      const auto* dict = dynamic_cast<const DictionarySegment<std::string>*>(data_table->get_chunk(c)->get_segment(column_id).get());
      Assert(dict, "unencoded string segments stay on the CPU path");
      if (is_between(_condition)) {
        const auto& value2 = std::get<std::string>(*_value2);
        const bool lower_inclusive = _condition == PredicateCondition::BetweenInclusive || _condition == PredicateCondition::BetweenUpperExclusive;
        const bool upper_inclusive = _condition == PredicateCondition::BetweenInclusive || _condition == PredicateCondition::BetweenLowerExclusive;
        lower.push_back(lower_inclusive ? dict->lower_bound(value) : dict->upper_bound(value));
        upper.push_back(upper_inclusive ? dict->upper_bound(value2) : dict->lower_bound(value2));
        found.push_back(0);
      } else {
        const auto lb = dict->lower_bound(value);
        lower.push_back(lb);
        upper.push_back(dict->upper_bound(value));
        found.push_back(lb != HY_INVALID_VALUE_ID && dict->dictionary()[lb] == value);
      }
    }
    predicate.value_type = HY_TYPE_STRING;
    predicate.per_chunk_lower = lower.data();
    predicate.per_chunk_upper = upper.data();
    predicate.per_chunk_found = found.data();
  }

  // DictionarySegment<pmr_string>: every element's value id in every data chunk's dictionary (lower_bound plus an equality check), or
  // HY_INVALID_VALUE_ID -- hy_in_list::per_chunk_value_ids, [n_data_chunks x n_values]
  static void resolve_string_list(const std::shared_ptr<const Table>& in_table, ColumnID _column_id, const std::vector<std::string>& strings, std::vector<uint32_t>& value_ids) {
    auto data_table = in_table;
    auto column_id = _column_id;
    if (in_table->type() == TableType::References && in_table->chunk_count()) {
      const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(_column_id));
      data_table = ref->referenced_table();
      column_id = ref->referenced_column_id();
    }
    for (ChunkID c = 0; c < data_table->chunk_count(); ++c) {
      const auto* dict = dynamic_cast<const DictionarySegment<std::string>*>(data_table->get_chunk(c)->get_segment(column_id).get());
      Assert(dict, "unencoded string segments stay on the CPU path");
      for (const auto& value : strings) {
        const auto lb = dict->lower_bound(value);
        value_ids.push_back(lb != HY_INVALID_VALUE_ID && dict->dictionary()[lb] == value ? lb : HY_INVALID_VALUE_ID);
      }
    }
    if (value_ids.empty()) value_ids.push_back(HY_INVALID_VALUE_ID);
  }

  // _find_matches_in_dictionary per data chunk (column_like_table_scan_impl.cpp:142-159): bit i of chunk c's words says
  // whether dictionary entry i satisfies the (possibly negated) pattern; the device tests value ids against it.
  static void find_matches_in_dictionaries(const std::shared_ptr<const Table>& in_table, ColumnID _column_id, PredicateCondition _condition, const AllTypeVariant& _value,
                                           std::vector<uint64_t>& words, std::vector<uint64_t>& word_offsets, hy_predicate& predicate) {
    auto data_table = in_table;
    auto column_id = _column_id;
    if (in_table->type() == TableType::References && in_table->chunk_count()) {
      const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(_column_id));
      data_table = ref->referenced_table();
      column_id = ref->referenced_column_id();
    }
    const LikeMatcher matcher(std::get<std::string>(_value), _condition);
    word_offsets.push_back(0);
    for (ChunkID c = 0; c < data_table->chunk_count(); ++c) {
      const auto* dict = dynamic_cast<const DictionarySegment<std::string>*>(data_table->get_chunk(c)->get_segment(column_id).get());
      Assert(dict, "unencoded string segments stay on the CPU path");
      const auto& dictionary = dict->dictionary();
      const size_t base = words.size();
      words.resize(base + (dictionary.size() + 63) / 64, 0);
      for (size_t i = 0; i < dictionary.size(); ++i) if (matcher(dictionary[i])) words[base + i / 64] |= uint64_t{1} << (i % 64);
      word_offsets.push_back(words.size());
    }
    if (words.empty()) words.push_back(0);
    predicate.value_type = HY_TYPE_STRING;
    predicate.match_words = words.data();
    predicate.match_word_offsets = word_offsets.data();
  }

 private:
  // _predicate through hy_table_scan_expression into `result` (true), or -- a constant predicate -- answered in counts / states (false)
  bool scan_expression(const std::shared_ptr<const Table>& in_table, hy_scan_result* result, std::vector<uint32_t>& counts, std::vector<uint8_t>& states) const;

  ColumnID _column_id = 0;
  PredicateCondition _condition = PredicateCondition::Equals;
  AllTypeVariant _value;
  std::optional<AllTypeVariant> _value2;
  std::optional<ColumnID> _right_column_id;
  std::vector<AllTypeVariant> _list;   // In / NotIn
  std::shared_ptr<const Expression> _predicate;
};

// ---- Validate (operators/validate.hpp, validate.cpp:87-314) -------------------------------------------------------------
struct TransactionContext {   // concurrency/transaction_context.hpp: what Validate reads of it
  TransactionContext(TransactionID transaction_id, CommitID snapshot_commit_id, bool has_in_flight_delete = false)
      : _tid(transaction_id), _snapshot(snapshot_commit_id), _delete(has_in_flight_delete) {}
  TransactionID transaction_id() const { return _tid; }
  CommitID snapshot_commit_id() const { return _snapshot; }
  bool has_in_flight_delete() const { return _delete; }   // read_write_operators() contains a Delete (validate.cpp:116-127)

 private:
  TransactionID _tid;
  CommitID _snapshot;
  bool _delete;
};

// The MvccData of a data table as a column of HY_ENC_MVCC segments.  Mutable chunks change under writers, so this column is
// rebuilt per call (the Hyrise adapter caches the immutable chunks).
inline std::shared_ptr<DeviceColumn> mvcc_column(const std::shared_ptr<const Table>& table) {
  auto column = std::make_shared<DeviceColumn>();
  const auto chunk_count = table->chunk_count();
  column->descriptors.assign(chunk_count, hy_segment{});
  for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
    const auto& chunk = table->get_chunk(chunk_id);
    Assert(chunk->has_mvcc_data(), "Trying to use Validate on a table that has no MVCC data.");
    const auto& mvcc = *chunk->mvcc_data();
    hy_segment& d = column->descriptors[chunk_id];
    d.encoding = HY_ENC_MVCC; d.data_type = HY_TYPE_INT; d.size = chunk->size(); d.width = 4;
    d.data = mvcc.tids.data(); d.aux = mvcc.begin_cids.data(); d.nulls = reinterpret_cast<const uint64_t*>(mvcc.end_cids.data());
    d.aux_size = mvcc.max_begin_cid;
    d.ref_chunk_id = chunk->invalid_row_count() | (chunk->is_mutable() ? 1u << 31 : 0u);
  }
  check_status(hy_column_create(column->descriptors.data(), chunk_count, HY_MEM_HOST, &column->handle));
  return column;
}

class Validate : public AbstractReadOnlyOperator {
 public:
  explicit Validate(std::shared_ptr<const AbstractOperator> in) : AbstractReadOnlyOperator(std::move(in)) {}
  const std::string& name() const override { static const std::string n = "Validate"; return n; }
  void set_transaction_context(std::shared_ptr<TransactionContext> context) { _context = std::move(context); }
  static bool is_row_visible(TransactionID our_tid, CommitID snapshot_commit_id, TransactionID row_tid, CommitID begin_cid, CommitID end_cid) {
    return snapshot_commit_id < end_cid && ((snapshot_commit_id >= begin_cid) != (row_tid == our_tid));   // validate.cpp:47-55
  }

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    if (!_context) Fail("Validate cannot be called without a transaction context.");   // validate.cpp:87-89
    const auto in_table = left_input_table();
    const auto chunk_count = in_table->chunk_count();
    // the table that owns the MvccData: the input itself or the table its reference segments point to (:186-199)
    auto mvcc_table = in_table;
    if (in_table->type() == TableType::References && chunk_count) {
      mvcc_table = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(0)->get_segment(0))->referenced_table();
    }
    const auto mvcc = mvcc_column(mvcc_table);
    std::shared_ptr<DeviceColumn> input = mvcc;
    if (in_table->type() == TableType::References) {   // the input's pos lists over the MVCC column
      input = std::make_shared<DeviceColumn>();
      input->descriptors.assign(chunk_count, hy_segment{});
      size_t host_lists = 0, device_lists = 0;
      for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
        const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(chunk_id)->get_segment(0));
        hy_segment& d = input->descriptors[chunk_id];
        d.encoding = HY_ENC_REFERENCE; d.data_type = HY_TYPE_INT; d.size = ref->size(); d.width = 8; d.ref = mvcc->handle;
        describe_pos_list(*ref->pos_list(), d, host_lists, device_lists);
      }
      if (device_lists && host_lists) {   // (a mixed table is handed over from the host, see device_column_of_chunks)
        for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
          const auto ref = std::static_pointer_cast<ReferenceSegment>(in_table->get_chunk(chunk_id)->get_segment(0));
          if (const auto* on_device = dynamic_cast<const DevicePosList*>(ref->pos_list().get())) input->descriptors[chunk_id].data = on_device->host_rows();
        }
      }
      check_status(hy_column_create(input->descriptors.data(), chunk_count, device_lists && !host_lists ? HY_MEM_DEVICE : HY_MEM_HOST, &input->handle));
    }
    std::unique_ptr<DeviceScanOutput> on_device;
    if (device_resident_results()) on_device = std::make_unique<DeviceScanOutput>(*in_table, in_table->type() == TableType::References);
    std::vector<RowID> matches(on_device ? 1 : std::max<uint64_t>(1, in_table->row_count()));
    std::vector<uint64_t> offsets(chunk_count + 1);
    std::vector<uint32_t> counts(std::max<ChunkID>(1, chunk_count));
    std::vector<uint8_t> states(std::max<ChunkID>(1, chunk_count));
    hy_scan_result result{};
    result.mem = HY_MEM_HOST;
    result.matches = reinterpret_cast<hy_row_id*>(matches.data());
    result.capacity = in_table->row_count();
    result.offsets = offsets.data();
    result.counts = counts.data();
    result.chunk_state = states.data();
    if (on_device) result = on_device->result;
    check_status(hy_validate(input->handle, _context->transaction_id(), _context->snapshot_commit_id(), _context->has_in_flight_delete() ? 0 : 1, &result));
    std::shared_ptr<DeviceBlock> translated;   // reference input: the visible rows' RowIDs in the data table, chunk regions
    if (on_device) {
      on_device->fetch(chunk_count);
      counts = on_device->counts;
      states = on_device->states;
      offsets = on_device->row_base;
      bool any_partial = false;
      for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) any_partial = any_partial || (counts[chunk_id] && states[chunk_id] != HY_CHUNK_ALL_MATCH);
      if (in_table->type() == TableType::References && any_partial) {
        translated = DeviceBlock::acquire(std::max<uint64_t>(1, on_device->rows) * sizeof(RowID));
        uint64_t written = 0;
        check_status(hy_poslist_translate(input->handle, &on_device->result, HY_POSLIST_CHUNK_REGIONS, static_cast<hy_row_id*>(translated->ptr), std::max<uint64_t>(1, on_device->rows), &written));
      }
    }
    // ---- output assembly, validate.cpp:256-311 ----
    std::vector<std::shared_ptr<Chunk>> output_chunks;
    for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
      if (counts[chunk_id] == 0) continue;   // :299
      const auto chunk_in = in_table->get_chunk(chunk_id);
      const bool entirely_visible = states[chunk_id] == HY_CHUNK_ALL_MATCH;
      Segments out_segments;
      if (in_table->type() == TableType::References) {
        const auto first = std::static_pointer_cast<ReferenceSegment>(chunk_in->get_segment(0));
        std::shared_ptr<const AbstractPosList> pos_list = first->pos_list();   // reused when entirely visible (:207-211)
        if (!entirely_visible && on_device) {
          pos_list = std::make_shared<DevicePosList>(translated, static_cast<const hy_row_id*>(translated->ptr) + offsets[chunk_id], counts[chunk_id],
                                                     first->pos_list()->references_single_chunk(), first->pos_list()->common_chunk_id());
        } else if (!entirely_visible) {
          auto visible = std::make_shared<RowIDPosList>();
          for (uint64_t m = offsets[chunk_id]; m < offsets[chunk_id + 1]; ++m) visible->rows.push_back((*first->pos_list())[matches[m].chunk_offset]);
          if (first->pos_list()->references_single_chunk()) visible->guarantee_single_chunk();
          pos_list = visible;
        }
        for (ColumnID c = 0; c < in_table->column_count(); ++c) {
          const auto ref = std::static_pointer_cast<ReferenceSegment>(chunk_in->get_segment(c));
          out_segments.push_back(std::make_shared<ReferenceSegment>(ref->referenced_table(), ref->referenced_column_id(), pos_list));
        }
      } else {
        std::shared_ptr<AbstractPosList> pos_list;
        if (entirely_visible) pos_list = std::make_shared<EntireChunkPosList>(chunk_id, chunk_in->size());   // :282-284
        else if (on_device) pos_list = on_device->pos_list_of(chunk_id);
        else {
          auto rows = std::make_shared<RowIDPosList>(std::vector<RowID>(matches.begin() + offsets[chunk_id], matches.begin() + offsets[chunk_id + 1]));
          rows->guarantee_single_chunk();
          pos_list = rows;
        }
        for (ColumnID c = 0; c < in_table->column_count(); ++c) out_segments.push_back(std::make_shared<ReferenceSegment>(in_table, c, pos_list));
      }
      output_chunks.push_back(std::make_shared<Chunk>(std::move(out_segments)));
    }
    return std::make_shared<Table>(in_table->column_definitions(), TableType::References, std::move(output_chunks));
  }

 private:
  std::shared_ptr<TransactionContext> _context;
};

using ColumnIDPair = std::pair<ColumnID, ColumnID>;

struct OperatorJoinPredicate {   // operators/operator_join_predicate.hpp: left column <condition> right column
  ColumnIDPair column_ids;
  PredicateCondition predicate_condition;
};

class JoinHash : public AbstractReadOnlyOperator {   // operators/join_hash.hpp:33-36 (primary predicate: Equals)
 public:
  JoinHash(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right, JoinMode mode, ColumnIDPair column_ids,
           std::optional<size_t> radix_bits = std::nullopt, std::vector<OperatorJoinPredicate> secondary_predicates = {})
      : AbstractReadOnlyOperator(std::move(left), std::move(right)), _mode(mode), _column_ids(column_ids), _radix_bits(radix_bits),
        _secondary_predicates(std::move(secondary_predicates)) {}
  const std::string& name() const override { static const std::string n = "JoinHash"; return n; }
  size_t radix_bits = 0;
  bool left_input_is_build_side = false;   // JoinHash::PerformanceData

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    // string keys join as ids (see string_join_id); a string against a number stays with the stock operator
    const bool string_keys = left->column_data_type(_column_ids.first) == DataType::String;
    Assert(string_keys == (right->column_data_type(_column_ids.second) == DataType::String), "JoinHash: a string key against a numeric key is not run on the device");
    const auto keys = string_keys ? StringKeys::JoinIds : StringKeys::None;
    // ... made in HBM for the pair where both columns are wholly dictionary-encoded (hy_column_string_join_keys: another unique number above
    // the hash bits, the same join); otherwise, and when the library refuses, each column's ids from the host's registry
    std::shared_ptr<DeviceColumn> left_column, right_column;
    if (!string_keys || !device_string_join_key_columns(left, _column_ids.first, right, _column_ids.second, HY_STRING_KEYS_HASH_IDS, left_column, right_column)) {
      left_column = device_column(left, _column_ids.first, keys);
      right_column = device_column(right, _column_ids.second, keys);
    }
    // JoinHash::supports (join_hash.cpp:39-44)
    Assert(_mode != JoinMode::AntiNullAsTrue || _secondary_predicates.empty(), "JoinHash does not support secondary predicates with AntiNullAsTrue");
    std::vector<hy_join_predicate> secondary;
    std::vector<std::shared_ptr<DeviceColumn>> secondary_columns;   // (keeps the handles alive)
    for (const auto& predicate : _secondary_predicates) {
      const auto l = device_column(left, predicate.column_ids.first), r = device_column(right, predicate.column_ids.second);
      secondary_columns.push_back(l);
      secondary_columns.push_back(r);
      secondary.push_back(hy_join_predicate{l->handle, r->handle, static_cast<uint32_t>(predicate.predicate_condition), 0});
    }
    // One call: room for one partner per row of the larger input (every key / foreign-key join fits); a join that multiplies
    // rows reports what it needs with HY_ERR_CAPACITY (nothing written) and runs once more with exactly that.
    uint64_t capacity = std::max<uint64_t>(1, std::max(left->row_count(), right->row_count()));
    uint32_t slice_capacity = static_cast<uint32_t>(capacity / 131070 + std::max(left->chunk_count(), right->chunk_count()) + 300);
    const bool semi_anti = _mode == JoinMode::Semi || _mode == JoinMode::AntiNullAsTrue || _mode == JoinMode::AntiNullAsFalse;
    const bool on_device = device_resident_results();
    std::vector<RowID> left_positions, right_positions;
    std::vector<uint64_t> slice_offsets;
    // Device-resident results: both PosLists in blocks of the library's result-buffer pool (the pair its calibration prefers, the second
    // list 1.25 MiB past the 2 MiB grid the first starts on); what the host reads to cut the output into chunks are the PosList
    // boundaries -- eight bytes per 131 070 pairs.
    std::shared_ptr<DeviceBlock> left_block, right_block, offsets_block;
    hy_join_result result{};
    for (int attempt = 0;; ++attempt) {
      slice_offsets.assign(size_t{slice_capacity} + 2, 0);
      result = hy_join_result{};
      result.radix_bits = _radix_bits ? static_cast<uint32_t>(*_radix_bits) : 0xFFFFFFFFu;
      result.capacity = capacity;
      result.slice_capacity = slice_capacity;
      if (on_device) {
        left_block.reset(); right_block.reset();   // (a second attempt: the first one's blocks go back first)
        hy_row_id* l = nullptr;
        hy_row_id* r = nullptr;
        check_status(hy_result_pool_acquire_pair(capacity, &l, &r));
        left_block = std::make_shared<DeviceBlock>(l);
        right_block = std::make_shared<DeviceBlock>(r);
        offsets_block = DeviceBlock::acquire(8 * (size_t{slice_capacity} + 2));
        result.mem = HY_MEM_DEVICE;
        result.left_pos = l;
        result.right_pos = semi_anti ? l : r;
        result.slice_offsets = static_cast<uint64_t*>(offsets_block->ptr);
      } else {
        left_positions.resize(capacity);
        right_positions.resize(capacity);
        result.mem = HY_MEM_HOST;
        result.left_pos = reinterpret_cast<hy_row_id*>(left_positions.data());
        result.right_pos = reinterpret_cast<hy_row_id*>(right_positions.data());
        result.slice_offsets = slice_offsets.data();
      }
      const auto status = hy_join_hash_predicates(left_column->handle, right_column->handle, static_cast<uint32_t>(_mode), secondary.data(), static_cast<uint32_t>(secondary.size()), &result);
      if (status == HY_ERR_CAPACITY && attempt == 0 && (result.n_pairs > capacity || result.n_slices > slice_capacity)) {
        capacity = std::max<uint64_t>(capacity, result.n_pairs);
        slice_capacity = std::max(slice_capacity, result.n_slices);
        continue;
      }
      check_status(status);
      break;
    }
    if (on_device) {
      if (semi_anti) right_block.reset();
      check_status(hy_memcpy_d2h(slice_offsets.data(), result.slice_offsets, 8 * (size_t{result.n_slices} + 1)));
    }
    radix_bits = result.radix_bits;
    left_input_is_build_side = result.left_is_build;
    // Output (write_output_chunks, join_output_writing.cpp:205-340): one chunk per non-empty PosList, small ones merged by the
    // reference's 1000 / 4000 rule (hy_join_output_chunks).  Columns: left input's, then right input's (Semi/Anti: left only).
    TableColumnDefinitions definitions = left->column_definitions();
    if (!semi_anti) for (const auto& d : right->column_definitions()) definitions.push_back({d.name, d.data_type, d.nullable || _mode == JoinMode::Left});
    if (_mode == JoinMode::Right) for (ColumnID c = 0; c < left->column_count(); ++c) definitions[c].nullable = true;
    std::vector<uint64_t> chunk_offsets(size_t{result.n_slices} + 1);
    uint32_t n_output_chunks = 0;
    check_status(hy_join_output_chunks(slice_offsets.data(), result.n_slices, chunk_offsets.data(), &n_output_chunks));
    std::vector<std::shared_ptr<Chunk>> chunks;
    if (on_device) {
      DeviceSide left_side(left, left_block, result.n_pairs), right_side(right, semi_anti ? nullptr : right_block, semi_anti ? 0 : result.n_pairs);
      for (uint32_t k = 0; k < n_output_chunks; ++k) {
        Segments segments;
        left_side.append(segments, chunk_offsets[k], chunk_offsets[k + 1]);
        if (!semi_anti) right_side.append(segments, chunk_offsets[k], chunk_offsets[k + 1]);
        chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
      }
      return std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
    }
    for (uint32_t k = 0; k < n_output_chunks; ++k) {
      const auto begin = chunk_offsets[k], end = chunk_offsets[k + 1];
      Segments segments;
      append_side(segments, left, std::vector<RowID>(left_positions.begin() + begin, left_positions.begin() + end));
      if (!semi_anti) append_side(segments, right, std::vector<RowID>(right_positions.begin() + begin, right_positions.begin() + end));
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
  }

 private:
  // (public: Sort writes its reference output the same way)
 public:
  // write_output_segments (join_output_writing.cpp:95-200) over PosLists in HBM: one side of the join result.  A data input's positions
  // ARE its RowIDs -- every output chunk's PosList is a view into the join's block.  A reference input's positions are dereferenced through
  // the input's PosLists (once per group of columns that share them: hy_poslist_gather over the WHOLE pair array into another pooled
  // block); a group the device cannot describe is dereferenced on the host through the lazy copies.
  struct DeviceSide {
    DeviceSide(const std::shared_ptr<const Table>& input, std::shared_ptr<DeviceBlock> positions, uint64_t n_pairs) : _input(input), _positions(std::move(positions)), _n(n_pairs) {
      if (!_positions || input->type() == TableType::Data) return;
      std::map<std::vector<const AbstractPosList*>, size_t> groups;
      for (ColumnID c = 0; c < input->column_count(); ++c) {
        std::vector<const AbstractPosList*> key;
        for (ChunkID k = 0; k < input->chunk_count(); ++k) key.push_back(std::static_pointer_cast<ReferenceSegment>(input->get_chunk(k)->get_segment(c))->pos_list().get());
        const auto [it, inserted] = groups.emplace(key, _resolved.size());
        _group_of_column.push_back(it->second);
        if (!inserted) continue;
        std::shared_ptr<DeviceBlock> resolved;
        if (_n) {
          try {
            const auto through = device_column(input, c);
            resolved = DeviceBlock::acquire(_n * sizeof(RowID));
            check_status(hy_poslist_gather(through->handle, static_cast<const hy_row_id*>(_positions->ptr), _n, static_cast<hy_row_id*>(resolved->ptr)));
          } catch (const std::logic_error&) {
            resolved = nullptr;
          }
        }
        _resolved.push_back(std::move(resolved));
        _lists.push_back(std::move(key));
      }
      if (_n) check_status(hy_synchronize());   // (the gathered lists are complete before another thread's operator may read them)
    }
    void append(Segments& segments, uint64_t begin, uint64_t end) {
      if (_input->type() == TableType::Data) {
        const auto pos_list = std::make_shared<DevicePosList>(_positions, static_cast<const hy_row_id*>(_positions->ptr) + begin, end - begin);
        for (ColumnID c = 0; c < _input->column_count(); ++c) segments.push_back(std::make_shared<ReferenceSegment>(_input, c, pos_list));
        return;
      }
      std::vector<std::shared_ptr<AbstractPosList>> of_group(_resolved.size());
      for (ColumnID c = 0; c < _input->column_count(); ++c) {
        const size_t g = _group_of_column[c];
        if (!of_group[g] && _resolved[g]) {
          of_group[g] = std::make_shared<DevicePosList>(_resolved[g], static_cast<const hy_row_id*>(_resolved[g]->ptr) + begin, end - begin);
        } else if (!of_group[g]) {
          _positions->prefetch_to_host(_n);
          const RowID* positions = _positions->host_copy();
          auto rows = std::make_shared<RowIDPosList>();
          for (uint64_t i = begin; i < end; ++i) rows->rows.push_back(positions[i].is_null() ? NULL_ROW_ID : (*_lists[g][positions[i].chunk_id])[positions[i].chunk_offset]);
          of_group[g] = rows;
        }
        const auto first = std::static_pointer_cast<ReferenceSegment>(_input->get_chunk(0)->get_segment(c));
        segments.push_back(std::make_shared<ReferenceSegment>(first->referenced_table(), first->referenced_column_id(), of_group[g]));
      }
    }

   private:
    std::shared_ptr<const Table> _input;
    std::shared_ptr<DeviceBlock> _positions;
    uint64_t _n;
    std::vector<size_t> _group_of_column;
    std::vector<std::shared_ptr<DeviceBlock>> _resolved;
    std::vector<std::vector<const AbstractPosList*>> _lists;
  };

  // write_output_segments (join_output_writing.cpp:95-200): reference inputs are dereferenced through their pos lists.
  static void append_side(Segments& segments, const std::shared_ptr<const Table>& input, std::vector<RowID> positions) {
    if (input->type() == TableType::Data) {
      const auto pos_list = std::make_shared<RowIDPosList>(std::move(positions));
      for (ColumnID c = 0; c < input->column_count(); ++c) segments.push_back(std::make_shared<ReferenceSegment>(input, c, pos_list));
      return;
    }
    std::map<std::vector<const AbstractPosList*>, std::shared_ptr<RowIDPosList>> cache;
    for (ColumnID c = 0; c < input->column_count(); ++c) {
      std::vector<const AbstractPosList*> lists;
      for (ChunkID k = 0; k < input->chunk_count(); ++k) lists.push_back(std::static_pointer_cast<ReferenceSegment>(input->get_chunk(k)->get_segment(c))->pos_list().get());
      auto& resolved = cache[lists];
      if (!resolved) {
        resolved = std::make_shared<RowIDPosList>();
        for (const auto& row : positions) resolved->rows.push_back(row.is_null() ? NULL_ROW_ID : (*lists[row.chunk_id])[row.chunk_offset]);
      }
      const auto first = std::static_pointer_cast<ReferenceSegment>(input->get_chunk(0)->get_segment(c));
      segments.push_back(std::make_shared<ReferenceSegment>(first->referenced_table(), first->referenced_column_id(), resolved));
    }
  }

 private:
  JoinMode _mode;
  ColumnIDPair _column_ids;
  std::optional<size_t> _radix_bits;
  std::vector<OperatorJoinPredicate> _secondary_predicates;
};

// What the join operators' supports() read of a join (operators/abstract_join_operator.hpp:18-41).
struct JoinConfiguration {
  JoinMode join_mode;
  PredicateCondition predicate_condition;
  DataType left_data_type, right_data_type;
  bool secondary_predicates;
};

// JoinSortMerge (operators/join_sort_merge.hpp): the join the translator takes where JoinHash does not apply -- a primary predicate <, <=, >,
// >= or <>, or FullOuter (lqp_translator.cpp:389-410) -- as ONE hy_join_sort_merge call.  Its two lists stay in pooled blocks of HBM; the
// output's PosLists are views into them (a data input) or into the blocks hy_poslist_gather dereferences them into (a reference input:
// JoinHash's DeviceSide).  The matched pairs, the unmatched left rows and the unmatched right rows each start a new output chunk, and inside
// a part a chunk holds Chunk::DEFAULT_SIZE pairs.  The order of the rows is the library's contract (include/hyrise_amd.h), not the
// reference's, whose order depends on its cluster count: the tables agree as multisets of rows.  What the library refuses -- string keys that
// are not wholly dictionary-encoded, key columns of different types, Semi / Anti / Cross, <> with an outer mode -- and joins with secondary predicates stay on the stock operator.
class JoinSortMerge : public AbstractReadOnlyOperator {
 public:
  JoinSortMerge(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right, JoinMode mode, OperatorJoinPredicate primary_predicate,
                std::vector<OperatorJoinPredicate> secondary_predicates = {})
      : AbstractReadOnlyOperator(std::move(left), std::move(right)), _mode(mode), _primary_predicate(primary_predicate), _secondary_predicates(std::move(secondary_predicates)) {}
  const std::string& name() const override { static const std::string n = "JoinSortMerge"; return n; }
  // join_sort_merge.cpp:43-47
  static bool supports(const JoinConfiguration& config) {
    return (config.predicate_condition != PredicateCondition::NotEquals || config.join_mode == JoinMode::Inner) && config.left_data_type == config.right_data_type &&
           config.join_mode != JoinMode::Semi && config.join_mode != JoinMode::AntiNullAsTrue && config.join_mode != JoinMode::AntiNullAsFalse;
  }
  uint64_t n_matched = 0, n_left_outer = 0;   // the output's three parts: matched pairs, unmatched left rows, then the unmatched right rows

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    Assert(_secondary_predicates.empty(), "JoinSortMerge: joins with secondary predicates are not run on the device");
    const auto ids = _primary_predicate.column_ids;
    // string keys join as their ranks among the distinct strings of BOTH columns, made in HBM (hy_column_string_join_keys): both columns
    // wholly dictionary-encoded and device_string_join_keys() on; every other case of a string key stays on the stock operator
    const bool left_strings = left->column_data_type(ids.first) == DataType::String, right_strings = right->column_data_type(ids.second) == DataType::String;
    std::shared_ptr<DeviceColumn> left_column, right_column;
    if (left_strings || right_strings) {
      Assert(left_strings && right_strings && device_string_join_key_columns(left, ids.first, right, ids.second, HY_STRING_KEYS_RANKS, left_column, right_column),
             "JoinSortMerge: string keys are not run on the device");
    } else {
      left_column = device_column(left, ids.first);
      right_column = device_column(right, ids.second);
    }
    // One call: room for one partner per row of the larger input; a join that needs more reports it with HY_ERR_CAPACITY (nothing written)
    // and runs once more with exactly that.
    uint64_t capacity = std::max<uint64_t>(1, std::max(left->row_count(), right->row_count()));
    const bool on_device = device_resident_results();
    std::vector<RowID> left_positions, right_positions;
    std::shared_ptr<DeviceBlock> left_block, right_block;
    hy_sort_merge_result result{};
    for (int attempt = 0;; ++attempt) {
      result = hy_sort_merge_result{};
      result.capacity = capacity;
      if (on_device) {
        left_block.reset(); right_block.reset();   // (a second attempt: the first one's blocks go back first)
        hy_row_id* l = nullptr;
        hy_row_id* r = nullptr;
        check_status(hy_result_pool_acquire_pair(capacity, &l, &r));
        left_block = std::make_shared<DeviceBlock>(l);
        right_block = std::make_shared<DeviceBlock>(r);
        result.mem = HY_MEM_DEVICE;
        result.left_pos = l;
        result.right_pos = r;
      } else {
        left_positions.resize(capacity);
        right_positions.resize(capacity);
        result.mem = HY_MEM_HOST;
        result.left_pos = reinterpret_cast<hy_row_id*>(left_positions.data());
        result.right_pos = reinterpret_cast<hy_row_id*>(right_positions.data());
      }
      const auto status = hy_join_sort_merge(left_column->handle, right_column->handle, static_cast<uint32_t>(_mode), static_cast<uint32_t>(_primary_predicate.predicate_condition), &result);
      if (status == HY_ERR_CAPACITY && attempt == 0 && result.n_pairs > capacity) {
        capacity = result.n_pairs;
        continue;
      }
      check_status(status);   // (HY_ERR_UNSUPPORTED included: there is no CPU implementation behind this class)
      break;
    }
    n_matched = result.n_matched;
    n_left_outer = result.n_left_outer;
    TableColumnDefinitions definitions;
    const bool left_nullable = _mode == JoinMode::Right || _mode == JoinMode::FullOuter, right_nullable = _mode == JoinMode::Left || _mode == JoinMode::FullOuter;
    for (const auto& d : left->column_definitions()) definitions.push_back({d.name, d.data_type, d.nullable || left_nullable});
    for (const auto& d : right->column_definitions()) definitions.push_back({d.name, d.data_type, d.nullable || right_nullable});
    // the chunks: every part starts a new one
    std::vector<std::pair<uint64_t, uint64_t>> cuts;
    const uint64_t part_ends[3] = {result.n_matched, result.n_matched + result.n_left_outer, result.n_pairs};
    for (uint64_t begin = 0, part = 0; part < 3; ++part) {
      for (; begin < part_ends[part]; begin = std::min<uint64_t>(begin + Chunk::DEFAULT_SIZE, part_ends[part])) cuts.emplace_back(begin, std::min<uint64_t>(begin + Chunk::DEFAULT_SIZE, part_ends[part]));
    }
    std::vector<std::shared_ptr<Chunk>> chunks;
    if (on_device) {
      JoinHash::DeviceSide left_side(left, left_block, result.n_pairs), right_side(right, right_block, result.n_pairs);
      for (const auto& [begin, end] : cuts) {
        Segments segments;
        left_side.append(segments, begin, end);
        right_side.append(segments, begin, end);
        chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
      }
    } else {
      for (const auto& [begin, end] : cuts) {
        Segments segments;
        JoinHash::append_side(segments, left, std::vector<RowID>(left_positions.begin() + begin, left_positions.begin() + end));
        JoinHash::append_side(segments, right, std::vector<RowID>(right_positions.begin() + begin, right_positions.begin() + end));
        chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
      }
    }
    // join_sort_merge.cpp:940-958: an Inner equi-join's chunks are sorted by both join columns and no value lies in two clusters.  The order
    // contract gives both: the pairs ascend by the left key, which is the right key.
    const bool sorted_output = _mode == JoinMode::Inner && _primary_predicate.predicate_condition == PredicateCondition::Equals;
    const ColumnID right_key = static_cast<ColumnID>(left->column_count() + ids.second);
    if (sorted_output) {
      for (const auto& chunk : chunks) {
        chunk->set_immutable();
        chunk->set_individually_sorted_by(std::vector<SortColumnDefinition>{SortColumnDefinition{ids.first, SortMode::AscendingNullsFirst}, SortColumnDefinition{right_key, SortMode::AscendingNullsFirst}});
      }
    }
    auto output = std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
    // (clustered means no value in two chunks: pairs cut every Chunk::DEFAULT_SIZE rows keep that only while they are one chunk)
    if (sorted_output && output->chunk_count() <= 1) output->set_value_clustered_by({ids.first, right_key});
    return output;
  }

 private:
  JoinMode _mode;
  OperatorJoinPredicate _primary_predicate;
  std::vector<OperatorJoinPredicate> _secondary_predicates;
};

// JoinNestedLoop (operators/join_nested_loop.hpp): the third join the translator tries (lqp_translator.cpp:389-410), which supports every
// configuration -- what JoinHash and JoinSortMerge refuse ends up here -- as ONE hy_join_nested_loop call.  The rows come in the reference's
// order (include/hyrise_amd.h), in ONE output chunk, or no chunk for an empty result (join_nested_loop.cpp:253-258); Semi / Anti outputs hold
// the left columns only.  The lists stay in pooled blocks of HBM as JoinSortMerge's do.  String columns in a predicate are not run on the device.
class JoinNestedLoop : public AbstractReadOnlyOperator {
 public:
  JoinNestedLoop(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right, JoinMode mode, OperatorJoinPredicate primary_predicate,
                 std::vector<OperatorJoinPredicate> secondary_predicates = {})
      : AbstractReadOnlyOperator(std::move(left), std::move(right)), _mode(mode), _primary_predicate(primary_predicate), _secondary_predicates(std::move(secondary_predicates)) {}
  const std::string& name() const override { static const std::string n = "JoinNestedLoop"; return n; }
  static bool supports(const JoinConfiguration& /*config*/) { return true; }   // join_nested_loop.cpp:87-89

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    std::vector<OperatorJoinPredicate> predicates{_primary_predicate};
    predicates.insert(predicates.end(), _secondary_predicates.begin(), _secondary_predicates.end());
    std::vector<std::shared_ptr<DeviceColumn>> columns;   // (keeps the handles alive)
    for (const auto& predicate : predicates) {
      Assert(left->column_data_type(predicate.column_ids.first) != DataType::String && right->column_data_type(predicate.column_ids.second) != DataType::String,
             "JoinNestedLoop: string columns are not run on the device");
      columns.push_back(device_column(left, predicate.column_ids.first));
      columns.push_back(device_column(right, predicate.column_ids.second));
    }
    std::vector<hy_join_predicate> secondary;
    for (size_t p = 1; p < predicates.size(); ++p) secondary.push_back(hy_join_predicate{columns[2 * p]->handle, columns[2 * p + 1]->handle, static_cast<uint32_t>(predicates[p].predicate_condition), 0});
    const bool semi_anti = _mode == JoinMode::Semi || _mode == JoinMode::AntiNullAsTrue || _mode == JoinMode::AntiNullAsFalse;
    // One call: room for one partner per row of the larger input; a join that needs more reports it with HY_ERR_CAPACITY (nothing written)
    // and runs once more with exactly that.
    uint64_t capacity = std::max<uint64_t>(1, std::max(left->row_count(), right->row_count()));
    const bool on_device = device_resident_results();
    std::vector<RowID> left_positions, right_positions;
    std::shared_ptr<DeviceBlock> left_block, right_block;
    hy_nested_loop_result result{};
    for (int attempt = 0;; ++attempt) {
      result = hy_nested_loop_result{};
      result.capacity = capacity;
      if (on_device) {
        left_block.reset(); right_block.reset();   // (a second attempt: the first one's blocks go back first)
        hy_row_id* l = nullptr;
        hy_row_id* r = nullptr;
        check_status(hy_result_pool_acquire_pair(capacity, &l, &r));
        left_block = std::make_shared<DeviceBlock>(l);
        right_block = std::make_shared<DeviceBlock>(r);
        result.mem = HY_MEM_DEVICE;
        result.left_pos = l;
        result.right_pos = r;
      } else {
        left_positions.resize(capacity);
        right_positions.resize(capacity);
        result.mem = HY_MEM_HOST;
        result.left_pos = reinterpret_cast<hy_row_id*>(left_positions.data());
        result.right_pos = reinterpret_cast<hy_row_id*>(right_positions.data());
      }
      const auto status = hy_join_nested_loop(columns[0]->handle, columns[1]->handle, static_cast<uint32_t>(_mode), static_cast<uint32_t>(_primary_predicate.predicate_condition), secondary.data(),
                                              static_cast<uint32_t>(secondary.size()), &result);
      if (status == HY_ERR_CAPACITY && attempt == 0 && result.n_pairs > capacity) {
        capacity = result.n_pairs;
        continue;
      }
      check_status(status);   // (HY_ERR_UNSUPPORTED included: there is no CPU implementation behind this class)
      break;
    }
    if (semi_anti) right_block.reset();
    TableColumnDefinitions definitions;
    const bool left_nullable = _mode == JoinMode::Right || _mode == JoinMode::FullOuter, right_nullable = _mode == JoinMode::Left || _mode == JoinMode::FullOuter;
    for (const auto& d : left->column_definitions()) definitions.push_back({d.name, d.data_type, d.nullable || left_nullable});
    if (!semi_anti) for (const auto& d : right->column_definitions()) definitions.push_back({d.name, d.data_type, d.nullable || right_nullable});
    std::vector<std::shared_ptr<Chunk>> chunks;
    if (result.n_pairs) {
      Segments segments;
      if (on_device) {
        JoinHash::DeviceSide left_side(left, left_block, result.n_pairs), right_side(right, semi_anti ? nullptr : right_block, semi_anti ? 0 : result.n_pairs);
        left_side.append(segments, 0, result.n_pairs);
        if (!semi_anti) right_side.append(segments, 0, result.n_pairs);
      } else {
        JoinHash::append_side(segments, left, std::vector<RowID>(left_positions.begin(), left_positions.begin() + result.n_pairs));
        if (!semi_anti) JoinHash::append_side(segments, right, std::vector<RowID>(right_positions.begin(), right_positions.begin() + result.n_pairs));
      }
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
  }

 private:
  JoinMode _mode;
  OperatorJoinPredicate _primary_predicate;
  std::vector<OperatorJoinPredicate> _secondary_predicates;
};

// Product (operators/product.hpp, product.cpp:32-137): what the translator emits for every cross join (lqp_translator.cpp:362).  The output has
// the left input's columns, then the right one's, and one chunk per pair of input chunks (cl, cr), cl outermost, empty pairs included; every
// segment references the table and column the input's segment references (a data input: the input itself), and the columns of a side that
// sat behind one input PosList share one output PosList.  hy_product writes the lists: one pooled block of HBM per side and input PosList,
// every chunk's PosList a view (block, pair_offsets[pair], rows) -- or, with device_resident_results(false), RowIDPosLists of the same
// contents.  DevicePosList inputs are read where they lie.  What the library refuses (and columns it cannot describe) takes the host loop.
class Product : public AbstractReadOnlyOperator {
 public:
  Product(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right) : AbstractReadOnlyOperator(std::move(left), std::move(right)) {}
  const std::string& name() const override { static const std::string n = "Product"; return n; }

 protected:
  // One input: its columns grouped by the PosLists they sit behind (a data input: one group), and per group the output's PosLists.
  struct Side {
    std::shared_ptr<const Table> table;
    std::vector<size_t> group_of_column;
    std::vector<std::vector<ColumnID>> columns_of_group;
    std::vector<std::vector<std::shared_ptr<const AbstractPosList>>> lists;   // [group][pair]

    explicit Side(std::shared_ptr<const Table> input) : table(std::move(input)) {
      std::map<std::vector<const AbstractPosList*>, size_t> groups;
      for (ColumnID c = 0; c < table->column_count(); ++c) {
        std::vector<const AbstractPosList*> key;
        if (table->type() == TableType::References)
          for (ChunkID k = 0; k < table->chunk_count(); ++k) key.push_back(std::static_pointer_cast<ReferenceSegment>(table->get_chunk(k)->get_segment(c))->pos_list().get());
        const auto [it, inserted] = groups.emplace(std::move(key), columns_of_group.size());
        group_of_column.push_back(it->second);
        if (inserted) columns_of_group.emplace_back();
        columns_of_group[it->second].push_back(c);
      }
      lists.resize(columns_of_group.size());
    }
    const AbstractPosList* input_list(size_t group, ChunkID chunk) const {   // nullptr: a data input
      if (table->type() == TableType::Data) return nullptr;
      return std::static_pointer_cast<ReferenceSegment>(table->get_chunk(chunk)->get_segment(columns_of_group[group][0]))->pos_list().get();
    }
    // A column of the group as the library takes it: only its chunk layout and PosLists are read, so any column the device path describes
    // serves (one that is resident already first).  Throws std::logic_error if there is none.
    std::shared_ptr<DeviceColumn> layout_column(size_t group) const {
      if (table->device_columns) {
        for (const auto& [key, column] : table->device_columns->columns)
          if (column && group_of_column[key.first] == group) return column;
      }
      for (const ColumnID c : columns_of_group[group]) {
        try { return device_column(table, c); } catch (const std::logic_error&) {}
      }
      Fail("Product: no column of the input is describable to the device");
    }
  };

  // product.cpp:114-128 on the host: the fallback for what the library refuses.
  static std::shared_ptr<RowIDPosList> host_pair_list(const Side& side, size_t group, bool is_left, ChunkID chunk, ChunkOffset left_rows, ChunkOffset right_rows) {
    const AbstractPosList* in = side.input_list(group, chunk);
    auto out = std::make_shared<RowIDPosList>();
    const size_t rows = size_t{left_rows} * right_rows;
    out->rows.reserve(rows);
    for (size_t p = 0; p < rows; ++p) {
      const auto offset = static_cast<ChunkOffset>(is_left ? p / right_rows : p % right_rows);
      out->rows.push_back(in ? (*in)[offset] : RowID{chunk, offset});
    }
    if (!in || in->references_single_chunk()) out->guarantee_single_chunk();
    return out;
  }

  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    TableColumnDefinitions definitions = left->column_definitions();
    definitions.insert(definitions.end(), right->column_definitions().begin(), right->column_definitions().end());
    const ChunkID n_left = left->chunk_count(), n_right = right->chunk_count();
    const size_t n_pairs = size_t{n_left} * n_right;
    std::vector<std::shared_ptr<Chunk>> chunks;
    if (!n_pairs) return std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
    std::vector<uint64_t> pair_offsets(n_pairs + 1, 0);
    for (ChunkID cl = 0; cl < n_left; ++cl)
      for (ChunkID cr = 0; cr < n_right; ++cr)
        pair_offsets[size_t{cl} * n_right + cr + 1] = pair_offsets[size_t{cl} * n_right + cr] + uint64_t{left->get_chunk(cl)->size()} * right->get_chunk(cr)->size();
    const uint64_t n_rows = pair_offsets[n_pairs];
    Side sides[2] = {Side(left), Side(right)};
    const bool on_device = device_resident_results();
    try {
      const auto left_layout = sides[0].layout_column(0), right_layout = sides[1].layout_column(0);   // (every call needs both inputs' chunk sizes)
      for (size_t s = 0; s < 2; ++s) {
        Side& side = sides[s];
        for (size_t g = 0; g < side.lists.size(); ++g) {
          const auto of_group = g == 0 ? (s == 0 ? left_layout : right_layout) : side.layout_column(g);
          hy_product_result result{};
          result.capacity = std::max<uint64_t>(1, n_rows);
          std::shared_ptr<DeviceBlock> block;
          std::vector<RowID> rows;
          hy_row_id* list = nullptr;
          if (on_device) {
            block = DeviceBlock::acquire(result.capacity * sizeof(RowID));
            list = static_cast<hy_row_id*>(block->ptr);
            result.mem = HY_MEM_DEVICE;
          } else {
            rows.resize(result.capacity);
            list = reinterpret_cast<hy_row_id*>(rows.data());
            result.mem = HY_MEM_HOST;
          }
          (s == 0 ? result.left_pos : result.right_pos) = list;
          check_status(hy_product(s == 0 ? of_group->handle : left_layout->handle, s == 0 ? right_layout->handle : of_group->handle, &result));
          Assert(result.n_rows == n_rows, "Product: the library counted other rows than the chunk sizes give");
          for (size_t pair = 0; pair < n_pairs; ++pair) {
            const ChunkID chunk = static_cast<ChunkID>(s == 0 ? pair / n_right : pair % n_right);
            const AbstractPosList* in = side.input_list(g, chunk);
            const bool single = !in || in->references_single_chunk();
            const ChunkID common = in ? in->common_chunk_id() : chunk;
            const uint64_t begin = pair_offsets[pair], size = pair_offsets[pair + 1] - begin;
            if (on_device) {
              side.lists[g].push_back(std::make_shared<DevicePosList>(block, list + begin, size, single, common));
            } else {
              auto out = std::make_shared<RowIDPosList>(std::vector<RowID>(rows.begin() + begin, rows.begin() + begin + size));
              if (single) out->guarantee_single_chunk();
              side.lists[g].push_back(std::move(out));
            }
          }
        }
      }
    } catch (const std::logic_error&) {   // HY_ERR_UNSUPPORTED, or an input no column of which the device path describes: the stock operator's loop
      for (size_t s = 0; s < 2; ++s) {
        for (size_t g = 0; g < sides[s].lists.size(); ++g) {
          sides[s].lists[g].clear();
          for (ChunkID cl = 0; cl < n_left; ++cl)
            for (ChunkID cr = 0; cr < n_right; ++cr)
              sides[s].lists[g].push_back(host_pair_list(sides[s], g, s == 0, s == 0 ? cl : cr, left->get_chunk(cl)->size(), right->get_chunk(cr)->size()));
        }
      }
    }
    for (size_t pair = 0; pair < n_pairs; ++pair) {
      Segments segments;
      for (size_t s = 0; s < 2; ++s) {
        const Side& side = sides[s];
        const ChunkID chunk = static_cast<ChunkID>(s == 0 ? pair / n_right : pair % n_right);
        for (ColumnID c = 0; c < side.table->column_count(); ++c) {
          const auto& pos_list = side.lists[side.group_of_column[c]][pair];
          if (side.table->type() == TableType::Data) {
            segments.push_back(std::make_shared<ReferenceSegment>(side.table, c, pos_list));
          } else {
            const auto in = std::static_pointer_cast<ReferenceSegment>(side.table->get_chunk(chunk)->get_segment(c));
            segments.push_back(std::make_shared<ReferenceSegment>(in->referenced_table(), in->referenced_column_id(), pos_list));
          }
        }
      }
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(definitions, TableType::References, std::move(chunks));
  }
};

// Sort (operators/sort.hpp, sort.cpp:287-516): ONE stable lexicographic sort of the input's rows on the device (hy_sort), whose result -- the
// input table's positions in sorted order -- stays in a pooled block of HBM; the output's PosLists are views into it (a data input) or into
// one block per column cluster that hy_poslist_gather dereferences it into (a reference input: JoinHash's DeviceSide), or the rows are
// materialised (hy_column_gather for numeric columns; string payloads stay on the host).
// row_limit: a LimitNode over the SortNode fused into the operator -- hy_sort_limit delivers the first min(row_limit, rows)
// positions only, and the output is built from those: the rows Limit(Sort(x), row_limit) has, as a table of Sort's own type and chunking.
class Sort : public AbstractReadOnlyOperator {
 public:
  enum class ForceMaterialization : bool { No = false, Yes = true };
  Sort(std::shared_ptr<const AbstractOperator> in, std::vector<SortColumnDefinition> sort_definitions, ChunkOffset output_chunk_size = Chunk::DEFAULT_SIZE,
       ForceMaterialization force_materialization = ForceMaterialization::No, std::optional<uint64_t> row_limit = std::nullopt)
      : AbstractReadOnlyOperator(std::move(in)), _sort_definitions(std::move(sort_definitions)), _output_chunk_size(output_chunk_size),
        _force_materialization(force_materialization), _row_limit(row_limit) {}
  const std::string& name() const override { static const std::string n = "Sort"; return n; }
  uint32_t path() const { return _path; }   // hy_sort_limit's *path (with a row_limit): 0 = every row was sorted, 1 = the selection ran first

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto input = left_input_table();
    Assert(!_sort_definitions.empty(), "Sort: no sort definition");
    for (const auto& definition : _sort_definitions) {   // sort.cpp:290-297
      Assert(definition.column != INVALID_COLUMN_ID, "Sort: Invalid column in sort definition");
      Assert(definition.column < input->column_count(), "Sort: Column ID is greater than table's column count");
      Assert(definition.sort_mode == SortMode::AscendingNullsFirst || definition.sort_mode == SortMode::DescendingNullsFirst, "Sort does not support NULLS LAST.");
    }
    Assert(_output_chunk_size > 0, "Sort: output_chunk_size must be positive");
    uint64_t rows = input->row_count();
    if (rows == 0) {   // :299-305
      if (_force_materialization == ForceMaterialization::Yes && input->type() == TableType::References) return std::make_shared<Table>(input->column_definitions(), TableType::Data);
      return input;
    }
    // the key columns, as the device reads them (string columns: ranks); a key it cannot read where it lies becomes a temporary data column
    std::vector<std::shared_ptr<DeviceColumn>> key_columns;
    std::vector<std::shared_ptr<const Table>> temporaries;
    std::vector<hy_sort_key> keys;
    for (const auto& definition : _sort_definitions) {
      const auto string_keys = input->column_data_type(definition.column) == DataType::String ? StringKeys::Ranks : StringKeys::None;
      std::shared_ptr<DeviceColumn> column;
      if (!references_several_columns(*input, definition.column)) {
        try { column = device_column(input, definition.column, string_keys); } catch (const std::logic_error&) { column = nullptr; }
      }
      if (!column) {
        temporaries.push_back(host_key_table(input, definition.column));
        column = device_column(temporaries.back(), 0);
      }
      key_columns.push_back(column);
      keys.push_back(hy_sort_key{column->handle, static_cast<uint32_t>(definition.sort_mode) + 1, 0});   // HY_SORT_* = SortMode + 1
    }
    const uint64_t sorted_rows = rows;
    if (_row_limit) rows = std::min(rows, *_row_limit);
    const auto positions = DeviceBlock::acquire(std::max<uint64_t>(rows, 1) * sizeof(RowID));
    uint64_t n_out = 0;
    if (_row_limit) check_status(hy_sort_limit(keys.data(), static_cast<uint32_t>(keys.size()), *_row_limit, 0, static_cast<hy_row_id*>(positions->ptr), rows, &n_out, &_path));
    else check_status(hy_sort(keys.data(), static_cast<uint32_t>(keys.size()), static_cast<hy_row_id*>(positions->ptr), sorted_rows, &n_out));
    Assert(n_out == rows, "Sort: the device sorted another number of rows");

    // :339-379: materialise when asked to, or when a column references more than one table or column
    bool must_materialize = _force_materialization == ForceMaterialization::Yes;
    for (ColumnID c = 0; !must_materialize && c < input->column_count(); ++c) must_materialize = references_several_columns(*input, c);
    auto output = must_materialize ? materialized_output(input, positions, rows) : reference_output(input, positions, rows);
    for (ChunkID k = 0; k < output->chunk_count(); ++k) {   // :381-389
      output->get_chunk(k)->set_immutable();
      output->get_chunk(k)->set_individually_sorted_by(_sort_definitions[0]);
    }
    return output;
  }

 private:
  static bool references_several_columns(const Table& input, ColumnID column_id) {
    if (input.type() != TableType::References) return false;
    const auto& first = static_cast<const ReferenceSegment&>(*input.get_chunk(0)->get_segment(column_id));
    for (ChunkID k = 1; k < input.chunk_count(); ++k) {
      const auto& segment = static_cast<const ReferenceSegment&>(*input.get_chunk(k)->get_segment(column_id));
      if (segment.referenced_table() != first.referenced_table() || segment.referenced_column_id() != first.referenced_column_id()) return true;
    }
    return false;
  }

  template <typename F>
  static void resolve_type(DataType type, F&& f) {
    switch (type) {
      case DataType::Int: f(int32_t{}); break;
      case DataType::Long: f(int64_t{}); break;
      case DataType::Float: f(float{}); break;
      case DataType::Double: f(double{}); break;
      case DataType::String: f(std::string{}); break;
      default: Fail("Sort: a column of type NULL");
    }
  }

  // A key column the device cannot read where it lies (a union's output referencing several tables, a ValueSegment<pmr_string>): its values,
  // read through the segments, as a data table of ValueSegments with the input's chunk layout -- strings as their ranks among the column's
  // distinct strings in byte order.
  static std::shared_ptr<Table> host_key_table(const std::shared_ptr<const Table>& input, ColumnID column_id) {
    const auto type = input->column_data_type(column_id);
    std::vector<std::string> rank_order;
    if (type == DataType::String) {
      for (ChunkID k = 0; k < input->chunk_count(); ++k) {
        const auto& segment = *input->get_chunk(k)->get_segment(column_id);
        for (ChunkOffset r = 0; r < segment.size(); ++r) {
          const auto value = segment[r];
          if (!variant_is_null(value)) rank_order.push_back(std::get<std::string>(value));
        }
      }
      std::sort(rank_order.begin(), rank_order.end());
      rank_order.erase(std::unique(rank_order.begin(), rank_order.end()), rank_order.end());
    }
    auto table = std::make_shared<Table>(TableColumnDefinitions{{"key", type == DataType::String ? DataType::Long : type, true}}, TableType::Data);
    resolve_type(type, [&](auto tag) {
      using T = decltype(tag);
      using Key = std::conditional_t<std::is_same_v<T, std::string>, int64_t, T>;
      for (ChunkID k = 0; k < input->chunk_count(); ++k) {
        const auto& segment = *input->get_chunk(k)->get_segment(column_id);
        std::vector<Key> values(segment.size());
        std::vector<bool> nulls(segment.size());
        for (ChunkOffset r = 0; r < segment.size(); ++r) {
          const auto value = segment[r];
          nulls[r] = variant_is_null(value);
          if (nulls[r]) continue;
          if constexpr (std::is_same_v<T, std::string>) values[r] = std::lower_bound(rank_order.begin(), rank_order.end(), std::get<std::string>(value)) - rank_order.begin();
          else values[r] = std::get<T>(value);
        }
        table->append_chunk(Segments{std::make_shared<ValueSegment<Key>>(std::move(values), std::move(nulls))});
      }
    });
    return table;
  }

  // write_reference_output_table (:161-252): chunks of output_chunk_size rows, every PosList a view into one pooled block per column cluster
  std::shared_ptr<Table> reference_output(const std::shared_ptr<const Table>& input, const std::shared_ptr<DeviceBlock>& positions, uint64_t rows) const {
    JoinHash::DeviceSide side(input, positions, rows);
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (uint64_t begin = 0; begin < rows; begin += _output_chunk_size) {
      Segments segments;
      side.append(segments, begin, std::min<uint64_t>(rows, begin + _output_chunk_size));
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(input->column_definitions(), TableType::References, std::move(chunks));
  }

  // write_materialized_output_table (:58-150): ValueSegments of output_chunk_size rows, nullable iff the column is; numeric columns gathered on
  // the device (hy_column_gather), wholly dictionary-encoded string columns as DictionarySegments made in HBM (hy_string_column_gather at the
  // sorted positions, device_string_results()), other strings -- and columns the device cannot read where they lie -- through the segments on the host
  std::shared_ptr<Table> materialized_output(const std::shared_ptr<const Table>& input, const std::shared_ptr<DeviceBlock>& positions, uint64_t rows) const {
    const uint64_t n_chunks = (rows + _output_chunk_size - 1) / _output_chunk_size;
    std::vector<Segments> segments(n_chunks, Segments(input->column_count()));
    for (ColumnID c = 0; c < input->column_count(); ++c) {
      const bool nullable = input->column_is_nullable(c);
      resolve_type(input->column_data_type(c), [&](auto tag) {
        using T = decltype(tag);
        hy_column* gathered = nullptr;
        std::shared_ptr<const DeviceStringResult> strings;
        if constexpr (std::is_same_v<T, std::string>) {
          std::shared_ptr<const Table> data_table;
          ColumnID data_column_id = c;
          if (device_string_results() && rows && !references_several_columns(*input, c) && string_dictionary_column(input, c, data_table, data_column_id)) {
            const auto column = device_column(input, c);
            const auto dictionary = device_string_dictionary(data_table, data_column_id);
            hy_column* made = nullptr;
            hy_string_dictionary* made_dictionary = nullptr;
            const auto status = hy_string_column_gather(column->handle, dictionary->handle, static_cast<const hy_row_id*>(positions->ptr), rows, _output_chunk_size, &made, &made_dictionary);
            if (status != HY_ERR_UNSUPPORTED) {
              check_status(status);
              strings = std::make_shared<const DeviceStringResult>(made, made_dictionary);
            }
          }
        }
        if constexpr (!std::is_same_v<T, std::string>) {
          if (!references_several_columns(*input, c)) {
            try {
              const auto column = device_column(input, c);
              check_status(hy_column_gather(column->handle, static_cast<const hy_row_id*>(positions->ptr), rows, _output_chunk_size, &gathered));
            } catch (const std::logic_error&) {
              gathered = nullptr;
            }
          }
        }
        for (uint64_t k = 0; k < n_chunks; ++k) {
          const uint64_t begin = k * _output_chunk_size, size = std::min<uint64_t>(_output_chunk_size, rows - begin);
          if (strings) {
            segments[k][c] = std::make_shared<DeviceStringDictionarySegment>(strings, static_cast<uint32_t>(k), static_cast<ChunkOffset>(size));
            continue;
          }
          std::vector<T> values(size);
          std::vector<bool> nulls(size);
          if (gathered) {
            if constexpr (!std::is_same_v<T, std::string>) {
              std::vector<uint64_t> words((size + 63) / 64);
              check_status(hy_column_read_chunk(gathered, static_cast<uint32_t>(k), values.data(), words.data()));
              for (uint64_t r = 0; r < size; ++r) nulls[r] = (words[r / 64] >> (r % 64)) & 1;
            }
          } else {
            positions->prefetch_to_host(rows);
            const RowID* sorted = positions->host_copy();
            for (uint64_t r = 0; r < size; ++r) {
              const RowID p = sorted[begin + r];
              const auto value = (*input->get_chunk(p.chunk_id)->get_segment(c))[p.chunk_offset];
              nulls[r] = variant_is_null(value);
              if (!nulls[r]) values[r] = std::get<T>(value);
            }
          }
          segments[k][c] = std::make_shared<ValueSegment<T>>(std::move(values), nullable ? std::optional<std::vector<bool>>(std::move(nulls)) : std::nullopt);
        }
        if (gathered) hy_column_destroy(gathered);
      });
    }
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (auto& chunk_segments : segments) chunks.push_back(std::make_shared<Chunk>(std::move(chunk_segments)));
    return std::make_shared<Table>(input->column_definitions(), TableType::Data, std::move(chunks));
  }

  std::vector<SortColumnDefinition> _sort_definitions;
  ChunkOffset _output_chunk_size;
  ForceMaterialization _force_materialization;
  std::optional<uint64_t> _row_limit;
  uint32_t _path = 0;
};

// Limit (operators/limit.hpp, limit.cpp:76-126): the input's first row_count rows, chunk by chunk until they are out, every output chunk an
// immutable reference chunk that keeps its input chunk's individually_sorted_by.  A PosList in HBM is cut as a DevicePosList view
// (block, offset, size) of the same pooled block -- nothing is copied or fetched to the host, the next operator reads it where it lies -- a host
// PosList is copied by prefix, and a data chunk gets RowID{chunk, 0 .. n).  Columns that shared a PosList share the cut one.
// The mirror has no expression classes: row_count is the evaluated count, and limit.cpp:55-71's checks (an integral type, one non-NULL row,
// not negative) belong to the adapter that evaluates the LimitNode's expression.
class Limit : public AbstractReadOnlyOperator {
 public:
  Limit(std::shared_ptr<const AbstractOperator> in, uint64_t row_count) : AbstractReadOnlyOperator(std::move(in)), _row_count(row_count) {}
  const std::string& name() const override { static const std::string n = "Limit"; return n; }

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto input = left_input_table();
    std::vector<std::shared_ptr<Chunk>> chunks;
    uint64_t index = 0;
    for (ChunkID k = 0; index < _row_count && k < input->chunk_count(); ++k) {
      const auto chunk = input->get_chunk(k);
      const auto size = static_cast<ChunkOffset>(std::min<uint64_t>(chunk->size(), _row_count - index));
      Segments segments;
      std::map<const AbstractPosList*, std::shared_ptr<const AbstractPosList>> cut;
      std::shared_ptr<RowIDPosList> of_data_chunk;
      for (ColumnID c = 0; c < input->column_count(); ++c) {
        if (const auto reference = std::dynamic_pointer_cast<const ReferenceSegment>(chunk->get_segment(c))) {
          auto& list = cut[reference->pos_list().get()];
          if (!list) list = prefix_of(reference->pos_list(), size);
          segments.push_back(std::make_shared<ReferenceSegment>(reference->referenced_table(), reference->referenced_column_id(), list));
          continue;
        }
        if (!of_data_chunk) {
          of_data_chunk = std::make_shared<RowIDPosList>();
          for (ChunkOffset r = 0; r < size; ++r) of_data_chunk->rows.push_back(RowID{k, r});
          of_data_chunk->guarantee_single_chunk();
        }
        segments.push_back(std::make_shared<ReferenceSegment>(input, c, of_data_chunk));
      }
      index += size;
      auto output_chunk = std::make_shared<Chunk>(std::move(segments));
      output_chunk->set_immutable();
      if (!chunk->individually_sorted_by().empty()) output_chunk->set_individually_sorted_by(chunk->individually_sorted_by());   // :117-122
      chunks.push_back(std::move(output_chunk));
    }
    return std::make_shared<Table>(input->column_definitions(), TableType::References, std::move(chunks));
  }

 private:
  static std::shared_ptr<const AbstractPosList> prefix_of(const std::shared_ptr<const AbstractPosList>& list, ChunkOffset size) {
    if (const auto* on_device = dynamic_cast<const DevicePosList*>(list.get()))
      return std::make_shared<DevicePosList>(on_device->block(), on_device->device_data(), size, on_device->references_single_chunk(), on_device->common_chunk_id());
    auto rows = std::make_shared<RowIDPosList>();
    for (ChunkOffset r = 0; r < size; ++r) rows->rows.push_back((*list)[r]);
    if (list->references_single_chunk()) rows->guarantee_single_chunk();
    return rows;
  }

  uint64_t _row_count;
};

inline bool same_column_definitions(const Table& a, const Table& b) {   // TableColumnDefinition::operator== (table_column_definition.cpp)
  if (a.column_count() != b.column_count()) return false;
  for (ColumnID c = 0; c < a.column_count(); ++c) {
    if (a.column_name(c) != b.column_name(c) || a.column_data_type(c) != b.column_data_type(c) || a.column_is_nullable(c) != b.column_is_nullable(c)) return false;
  }
  return true;
}

// operators/union_positions.hpp: the set union of two reference tables over the same data -- what PredicateSplitUpRule makes of `WHERE p OR q`
// (two TableScans over one input and a UnionNode, SetOperationMode::Positions).  Columns that share a PosList form a column cluster; each
// input is a matrix of one RowID per cluster and row; both are sorted and merged like std::set_union (a row m times left and n times right:
// max(m, n) times) by hy_union_positions, which reads the inputs' PosLists where they lie and leaves the output's in HBM.
class UnionPositions : public AbstractReadOnlyOperator {
 public:
  UnionPositions(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right) : AbstractReadOnlyOperator(std::move(left), std::move(right)) {}
  const std::string& name() const override { static const std::string n = "UnionPositions"; return n; }
  uint32_t path() const { return _path; }   // hy_union_positions' *path: bit 0 / 1 = the left / right input was sorted

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    // _prepare_operator (union_positions.cpp:237-253): the early results
    Assert(same_column_definitions(*left, *right), "Input tables do not have the same layout.");
    if (left->row_count() == 0) return right;
    if (right->row_count() == 0) return left;
    Assert(left->type() == TableType::References && right->type() == TableType::References, "UnionPositions does not support non-reference tables yet.");

    // :257-296: a cluster begins where the PosList of the first chunk changes, in either input
    const auto reference_segment = [](const Table& table, ChunkID chunk_id, ColumnID column_id) -> const ReferenceSegment& {
      const auto* segment = dynamic_cast<const ReferenceSegment*>(table.get_chunk(chunk_id)->get_segment(column_id).get());
      Assert(segment != nullptr, "UnionPositions: a reference table holds ReferenceSegments only");
      return *segment;
    };
    std::vector<ColumnID> cluster_offsets;
    for (const auto* table : {left.get(), right.get()}) {
      const AbstractPosList* current = nullptr;
      for (ColumnID c = 0; c < table->column_count(); ++c) {
        const auto* pos_list = reference_segment(*table, 0, c).pos_list().get();
        if (pos_list != current) { current = pos_list; cluster_offsets.push_back(c); }
      }
    }
    std::sort(cluster_offsets.begin(), cluster_offsets.end());
    cluster_offsets.erase(std::unique(cluster_offsets.begin(), cluster_offsets.end()), cluster_offsets.end());
    std::vector<std::shared_ptr<const Table>> referenced_tables;
    std::vector<ColumnID> referenced_column_ids;
    for (const auto cluster_begin : cluster_offsets) referenced_tables.push_back(reference_segment(*left, 0, cluster_begin).referenced_table());
    for (ColumnID c = 0; c < left->column_count(); ++c) referenced_column_ids.push_back(reference_segment(*left, 0, c).referenced_column_id());

    // :298-343 (a debug check there; host-side and cheap, so always): every chunk of both inputs has these clusters, tables and columns
    for (const auto* table : {left.get(), right.get()}) {
      for (ChunkID k = 0; k < table->chunk_count(); ++k) {
        const AbstractPosList* current = nullptr;
        size_t next_cluster = 0;
        for (ColumnID c = 0; c < table->column_count(); ++c) {
          if (next_cluster < cluster_offsets.size() && c == cluster_offsets[next_cluster]) { ++next_cluster; current = nullptr; }
          const auto& segment = reference_segment(*table, k, c);
          if (!current) current = segment.pos_list().get();
          Assert(current == segment.pos_list().get(), "Different PosLists in ColumnCluster");
          Assert(segment.referenced_table() == referenced_tables[next_cluster - 1], "ReferenceSegment (Chunk: " + std::to_string(k) + ", Column: " + std::to_string(c) + ") doesn't reference the same table as the segment at the same index in the first chunk of the left input table does");
          Assert(segment.referenced_column_id() == referenced_column_ids[c], "ReferenceSegment (Chunk: " + std::to_string(k) + ", Column: " + std::to_string(c) + ") doesn't reference the same column as the segment at the same index in the first chunk of the left input table does");
        }
      }
    }

    // one reference column per cluster and side (any column of the cluster carries its PosLists), one pooled block per cluster for the output
    const uint32_t n_clusters = static_cast<uint32_t>(cluster_offsets.size());
    std::vector<std::shared_ptr<DeviceColumn>> columns;
    std::vector<const hy_column*> handles[2];
    for (size_t side = 0; side < 2; ++side) {
      for (const auto cluster_begin : cluster_offsets) {
        columns.push_back(device_column(side == 0 ? left : right, cluster_begin));
        handles[side].push_back(columns.back()->handle);
      }
    }
    const uint64_t capacity = left->row_count() + right->row_count();
    std::vector<std::shared_ptr<DeviceBlock>> blocks;
    std::vector<hy_row_id*> lists;
    for (uint32_t c = 0; c < n_clusters; ++c) {
      blocks.push_back(DeviceBlock::acquire(capacity * sizeof(RowID)));
      lists.push_back(static_cast<hy_row_id*>(blocks.back()->ptr));
    }
    uint64_t rows = 0;
    check_status(hy_union_positions(handles[0].data(), handles[1].data(), n_clusters, 0, lists.data(), capacity, &rows, &_path));

    // :168-186: chunks of Chunk::DEFAULT_SIZE rows, one PosList per cluster and chunk, shared by the cluster's segments
    const bool on_device = device_resident_results();
    if (!on_device) for (const auto& block : blocks) block->prefetch_to_host(rows);
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (uint64_t begin = 0; begin < rows; begin += Chunk::DEFAULT_SIZE) {
      const uint64_t size = std::min<uint64_t>(Chunk::DEFAULT_SIZE, rows - begin);
      Segments segments;
      for (uint32_t c = 0; c < n_clusters; ++c) {
        std::shared_ptr<const AbstractPosList> pos_list;
        if (on_device) pos_list = std::make_shared<DevicePosList>(blocks[c], lists[c] + begin, size);
        else pos_list = std::make_shared<RowIDPosList>(std::vector<RowID>(blocks[c]->host_copy() + begin, blocks[c]->host_copy() + begin + size));
        const ColumnID cluster_end = c + 1 < n_clusters ? cluster_offsets[c + 1] : left->column_count();
        for (ColumnID column_id = cluster_offsets[c]; column_id < cluster_end; ++column_id)
          segments.push_back(std::make_shared<ReferenceSegment>(referenced_tables[c], referenced_column_ids[column_id], pos_list));
      }
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(left->column_definitions(), TableType::References, std::move(chunks));
  }

 private:
  uint32_t _path = 0;
};

// operators/union_all.hpp: the other operator PredicateSplitUpRule emits (SetOperationMode::All, when the predicates exclude each other):
// the output holds the chunks of both inputs -- their segments shared, nothing copied, nothing for the device to do.
class UnionAll : public AbstractReadOnlyOperator {
 public:
  UnionAll(std::shared_ptr<const AbstractOperator> left, std::shared_ptr<const AbstractOperator> right) : AbstractReadOnlyOperator(std::move(left), std::move(right)) {}
  const std::string& name() const override { static const std::string n = "UnionAll"; return n; }

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto left = left_input_table(), right = right_input_table();
    Assert(same_column_definitions(*left, *right), "Input tables must have same number of columns.");
    Assert(left->type() == right->type(), "Input tables must have the same type.");
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (const auto& input : {left, right}) {
      for (ChunkID k = 0; k < input->chunk_count(); ++k) {
        Segments segments;
        for (ColumnID c = 0; c < input->column_count(); ++c) segments.push_back(input->get_chunk(k)->get_segment(c));
        chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
      }
    }
    return std::make_shared<Table>(left->column_definitions(), left->type(), std::move(chunks));
  }
};

struct AggregateDefinition {   // WindowFunctionExpression over a PQPColumnExpression (INVALID_COLUMN_ID: COUNT(*))
  ColumnID column_id;
  WindowFunction function;
};

class AggregateHash : public AbstractReadOnlyOperator {   // operators/aggregate_hash.hpp:139-141
 public:
  AggregateHash(std::shared_ptr<const AbstractOperator> in, std::vector<AggregateDefinition> aggregates, std::vector<ColumnID> groupby_column_ids)
      : AbstractReadOnlyOperator(std::move(in)), _aggregates(std::move(aggregates)), _groupby(std::move(groupby_column_ids)) {}
  const std::string& name() const override { static const std::string n = "AggregateHash"; return n; }

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto input = left_input_table();
    std::vector<std::shared_ptr<DeviceColumn>> keep;
    std::vector<const hy_column*> groupby;
    // A string GROUP BY column that an operator left in HBM (DeviceStringDictionarySegments: AggregateHash's and Projection's SUBSTR outputs)
    // is grouped by its rank stand-in, made in HBM: key names would have to be made from its dictionaries on the host, which is a fetch.
    const auto string_keys_of = [&](ColumnID id) {
      if (input->column_data_type(id) != DataType::String) return StringKeys::None;
      const bool resident = input->chunk_count() > 0 && dynamic_cast<const DeviceStringDictionarySegment*>(input->get_chunk(ChunkID{0})->get_segment(id).get()) != nullptr;
      return resident && device_string_ranking() ? StringKeys::Ranks : StringKeys::AggregateKeyNames;
    };
    for (const auto id : _groupby) { keep.push_back(device_column(input, id, string_keys_of(id))); groupby.push_back(keep.back()->handle); }
    std::vector<hy_aggregate_spec> specs;
    bool string_aggregates = false;  // MIN / MAX / ANY over a string column: their output segments are made by resident_output
    for (const auto& aggregate : _aggregates) {
      hy_aggregate_spec spec{};
      spec.function = static_cast<uint32_t>(aggregate.function);
      if (aggregate.column_id != INVALID_COLUMN_ID) {
        // SUM / AVG / STDDEV_SAMP of strings are invalid (aggregate_test.cpp:232-262 expects std::logic_error)
        const bool arithmetic = aggregate.function == WindowFunction::Sum || aggregate.function == WindowFunction::Avg || aggregate.function == WindowFunction::StandardDeviationSample;
        Assert(!(arithmetic && input->column_data_type(aggregate.column_id) == DataType::String), "Aggregate function not available for strings.");
        const bool of_strings = input->column_data_type(aggregate.column_id) == DataType::String;
        if (of_strings && (aggregate.function == WindowFunction::Min || aggregate.function == WindowFunction::Max)) {
          // MIN / MAX of strings are MIN / MAX of their ranks among the column's distinct strings (made in HBM, or on the host: device_string_ranking)
          keep.push_back(device_column(input, aggregate.column_id, StringKeys::Ranks));
          spec.column = keep.back()->handle;
          string_aggregates = true;
        } else if (of_strings && aggregate.function == WindowFunction::Any) {
          spec.function = HY_AGG_COUNT;   // (a placeholder, COUNT(*): ANY is the value at the group's representative row)
          string_aggregates = true;
        } else {
          keep.push_back(device_column(input, aggregate.column_id));
          spec.column = keep.back()->handle;
        }
      } else {
        Assert(aggregate.function == WindowFunction::Count, "Only COUNT may have an invalid ColumnID.");   // aggregate_hash.cpp:1002
      }
      specs.push_back(spec);
    }
    std::vector<hy_aggregate_spec> call_specs = specs;
    if (groupby.empty() && std::all_of(specs.begin(), specs.end(), [](const auto& s) { return !s.column; })) {
      // a lone COUNT(*): pass the table's first column as an (ignored) ANY so that the library knows the chunk layout
      keep.push_back(device_column(input, ColumnID{0}));
      hy_aggregate_spec lone_spec{};
      lone_spec.function = HY_AGG_ANY;
      lone_spec.column = keep.back()->handle;
      call_specs.push_back(lone_spec);
    }
    if (device_resident_results() || string_aggregates) return resident_output(input, groupby, specs, call_specs);
    // Room for a group per input row, as the one call may need -- but not TOUCHED: value-initialised vectors of that size were 0.8 GB of page
    // faults (a quarter of a second) in front of an aggregate over 26 M joined rows that produces three groups.
    const uint32_t capacity = static_cast<uint32_t>(input->row_count() + 1);
    const std::unique_ptr<RowID[]> group_rows(new RowID[capacity]);
    std::vector<std::unique_ptr<uint64_t[]>> values;
    std::vector<std::unique_ptr<uint8_t[]>> nulls;
    std::vector<hy_aggregate_column> columns(std::max<size_t>(1, call_specs.size()));
    for (size_t a = 0; a < call_specs.size(); ++a) {
      values.emplace_back(new uint64_t[capacity]);
      nulls.emplace_back(new uint8_t[capacity]);
      columns[a].values = values[a].get();
      columns[a].is_null = nulls[a].get();
    }
    hy_aggregate_result result{};
    result.mem = HY_MEM_HOST;
    result.group_capacity = capacity;
    result.group_row_ids = reinterpret_cast<hy_row_id*>(group_rows.get());
    result.columns = columns.data();
    check_status(hy_aggregate_hash(groupby.data(), static_cast<uint32_t>(groupby.size()), call_specs.data(), static_cast<uint32_t>(call_specs.size()), &result));
    // ---- output (aggregate_hash.cpp:1301-1361): GROUP BY columns reference the input through the representative
    // rows, aggregate columns are ValueSegments; here both are materialised into one Data table of value segments.
    std::vector<DataType> result_types;
    for (size_t a = 0; a < specs.size(); ++a) result_types.push_back(static_cast<DataType>(columns[a].data_type));
    const TableColumnDefinitions definitions = output_definitions(*input, result_types);
    auto output = std::make_shared<Table>(definitions, TableType::Data, Chunk::DEFAULT_SIZE);
    for (uint32_t g = 0; g < result.n_groups; ++g) {
      std::vector<AllTypeVariant> row;
      for (const auto id : _groupby) row.push_back((*input->get_chunk(group_rows[g].chunk_id)->get_segment(id))[group_rows[g].chunk_offset]);
      for (size_t a = 0; a < specs.size(); ++a) {
        if (nulls[a][g]) { row.emplace_back(NullValue{}); continue; }
        switch (static_cast<DataType>(columns[a].data_type)) {
          case DataType::Int: row.emplace_back(reinterpret_cast<const int32_t*>(values[a].get())[g]); break;
          case DataType::Long: row.emplace_back(reinterpret_cast<const int64_t*>(values[a].get())[g]); break;
          case DataType::Float: row.emplace_back(reinterpret_cast<const float*>(values[a].get())[g]); break;
          default: row.emplace_back(reinterpret_cast<const double*>(values[a].get())[g]); break;
        }
      }
      output->append(std::move(row));
    }
    output->finalize();
    return output;
  }

  // aggregate_hash.cpp:1301-1361: the GROUP BY columns' definitions, then "FUNCTION(argument)" per aggregate with the given result type
  TableColumnDefinitions output_definitions(const Table& input, const std::vector<DataType>& result_types) const {
    TableColumnDefinitions definitions;
    for (const auto id : _groupby) definitions.push_back(input.column_definitions()[id]);
    for (size_t a = 0; a < result_types.size(); ++a) {
      const auto& aggregate = _aggregates[a];
      const std::string argument = aggregate.column_id == INVALID_COLUMN_ID ? "*" : input.column_name(aggregate.column_id);
      const bool needs_null = aggregate.function != WindowFunction::Count && aggregate.function != WindowFunction::CountDistinct;
      definitions.push_back({std::string(function_name(aggregate.function)) + "(" + argument + ")", result_types[a], needs_null});
    }
    return definitions;
  }
  static const char* function_name(WindowFunction function) {
    static const char* names[] = {"MIN", "MAX", "SUM", "AVG", "COUNT", "COUNT DISTINCT", "STDDEV_SAMP", "ANY"};
    return names[static_cast<int>(function)];
  }

  // The output table in HBM (hy_aggregate_hash_columns): same column definitions and chunking as the host path below builds cell by cell, the
  // numeric segments DeviceValueSegments over the library's output columns -- the next operator's device_column() hands the handles on.
  // String GROUP BY columns (passed as key names: the library makes no column for them) are read on the host through the representative rows.
  std::shared_ptr<const Table> resident_output(const std::shared_ptr<const Table>& input_table, const std::vector<const hy_column*>& groupby, const std::vector<hy_aggregate_spec>& specs,
                                               const std::vector<hy_aggregate_spec>& call_specs) const {
    const Table& input = *input_table;
    const auto string_aggregate = [&](size_t a) {
      const auto& aggregate = _aggregates[a];
      return aggregate.column_id != INVALID_COLUMN_ID && input.column_data_type(aggregate.column_id) == DataType::String &&
             (aggregate.function == WindowFunction::Min || aggregate.function == WindowFunction::Max || aggregate.function == WindowFunction::Any);
    };
    std::vector<hy_column*> aggregate_handles(std::max<size_t>(1, call_specs.size()), nullptr), groupby_handles(std::max<size_t>(1, groupby.size()), nullptr);
    hy_aggregate_columns result{};
    for (size_t g = 0; g < _groupby.size() && g < 64; ++g) if (input.column_data_type(_groupby[g]) == DataType::String) result.skip_groupby_mask |= uint64_t{1} << g;
    result.aggregate_columns = aggregate_handles.data();
    result.groupby_columns = groupby_handles.data();
    check_status(hy_aggregate_hash_columns(groupby.data(), static_cast<uint32_t>(groupby.size()), call_specs.data(), static_cast<uint32_t>(call_specs.size()), Chunk::DEFAULT_SIZE, &result));
    // (owners first: whatever throws below, every handle and the RowIDs are given back)
    const auto row_ids = std::make_shared<DeviceBlock>(result.group_row_ids);
    std::vector<std::shared_ptr<const DeviceColumnOwner>> groupby_owners, aggregate_owners;
    for (size_t g = 0; g < groupby.size(); ++g) groupby_owners.push_back(groupby_handles[g] ? std::make_shared<const DeviceColumnOwner>(groupby_handles[g]) : nullptr);
    for (size_t a = 0; a < call_specs.size(); ++a) aggregate_owners.push_back(std::make_shared<const DeviceColumnOwner>(aggregate_handles[a]));

    // the result types are the handles' (a column without chunks has none: window_function_traits.hpp:11-77, as the library types them)
    std::vector<DataType> result_types;
    for (size_t a = 0; a < specs.size(); ++a) {
      const auto& aggregate = _aggregates[a];
      DataType type = aggregate.column_id == INVALID_COLUMN_ID ? DataType::Long : input.column_data_type(aggregate.column_id);
      const bool is_float = type == DataType::Float || type == DataType::Double;
      if (aggregate.function == WindowFunction::Count || aggregate.function == WindowFunction::CountDistinct) type = DataType::Long;
      else if (aggregate.function == WindowFunction::Avg || aggregate.function == WindowFunction::StandardDeviationSample) type = DataType::Double;
      else if (aggregate.function == WindowFunction::Sum) type = is_float ? DataType::Double : DataType::Long;
      if (result.n_groups) type = static_cast<DataType>(hy_column_data_type(aggregate_handles[a]));
      if (string_aggregate(a)) type = DataType::String;   // (the handle holds ranks, or ANY's placeholder)
      result_types.push_back(type);
    }
    TableColumnDefinitions definitions = output_definitions(input, result_types);
    for (size_t g = 0; g < groupby.size(); ++g) {
      if (groupby_handles[g] && result.n_groups) Assert(static_cast<DataType>(hy_column_data_type(groupby_handles[g])) == definitions[g].data_type, "AggregateHash: a gathered GROUP BY column has another type than its input column");
    }
    const uint64_t n_groups = result.n_groups;
    const RowID* rows = nullptr;   // the representative rows on the host: only where a GROUP BY column has to be read through them
    const auto host_rows = [&] {
      if (!rows) { row_ids->prefetch_to_host(n_groups); rows = row_ids->host_copy(); }
      return rows;
    };
    const auto resident_segment = [](DataType type, const std::shared_ptr<const DeviceColumnOwner>& owner, uint32_t chunk, ChunkOffset size) -> std::shared_ptr<AbstractSegment> {
      switch (type) {
        case DataType::Int: return std::make_shared<DeviceValueSegment<int32_t>>(owner, chunk, size);
        case DataType::Long: return std::make_shared<DeviceValueSegment<int64_t>>(owner, chunk, size);
        case DataType::Float: return std::make_shared<DeviceValueSegment<float>>(owner, chunk, size);
        default: return std::make_shared<DeviceValueSegment<double>>(owner, chunk, size);
      }
    };
    // String outputs made in HBM (device_string_results): a column of the input at the representative rows (a string GROUP BY column, ANY),
    // or the strings behind an aggregate's ranks (MIN / MAX).  nullptr: the host makes the column -- the switch is off, the column is not
    // wholly dictionary-encoded, or the library refused.
    const auto gathered_at_rows = [&](ColumnID column_id) -> std::shared_ptr<const DeviceStringResult> {
      std::shared_ptr<const Table> data_table;
      ColumnID data_column_id = column_id;
      if (!device_string_results() || !n_groups || !string_dictionary_column(input_table, column_id, data_table, data_column_id)) return nullptr;
      const auto column = device_column(input_table, column_id);
      const auto dictionary = device_string_dictionary(data_table, data_column_id);
      hy_column* made = nullptr;
      hy_string_dictionary* made_dictionary = nullptr;
      const auto status = hy_string_column_gather(column->handle, dictionary->handle, result.group_row_ids, n_groups, Chunk::DEFAULT_SIZE, &made, &made_dictionary);
      if (status == HY_ERR_UNSUPPORTED) return nullptr;
      check_status(status);
      return std::make_shared<const DeviceStringResult>(made, made_dictionary);
    };
    const auto strings_of_ranks = [&](ColumnID column_id, const hy_column* ranks) -> std::shared_ptr<const DeviceStringResult> {
      std::shared_ptr<const Table> data_table;
      ColumnID data_column_id = column_id;
      if (!device_string_results() || !n_groups || !string_dictionary_column(input_table, column_id, data_table, data_column_id)) return nullptr;
      if (hy_column_data_type(ranks) != HY_TYPE_INT) return nullptr;   // (int64 ranks the host made: device_string_ranking() is off)
      const auto dictionary = device_string_dictionary(data_table, data_column_id);
      hy_column* made = nullptr;
      hy_string_dictionary* made_dictionary = nullptr;
      const auto status = hy_string_ranks_gather(dictionary->handle, ranks, &made, &made_dictionary);
      if (status == HY_ERR_UNSUPPORTED) return nullptr;
      check_status(status);
      return std::make_shared<const DeviceStringResult>(made, made_dictionary);
    };
    std::vector<std::shared_ptr<const DeviceStringResult>> groupby_strings(_groupby.size()), aggregate_strings(specs.size());
    std::vector<std::vector<std::string>> rank_orders(specs.size());   // MIN / MAX on the host: the distinct strings of the column, in byte order
    for (size_t g = 0; g < _groupby.size(); ++g) if (!groupby_owners[g] && definitions[g].data_type == DataType::String) groupby_strings[g] = gathered_at_rows(_groupby[g]);
    for (size_t a = 0; a < specs.size(); ++a) {
      if (!string_aggregate(a)) continue;
      const bool any = _aggregates[a].function == WindowFunction::Any;
      aggregate_strings[a] = any ? gathered_at_rows(_aggregates[a].column_id) : strings_of_ranks(_aggregates[a].column_id, aggregate_handles[a]);
      if (aggregate_strings[a] || any) continue;
      std::shared_ptr<const Table> data_table;
      ColumnID data_column_id = _aggregates[a].column_id;
      Assert(string_dictionary_column(input_table, _aggregates[a].column_id, data_table, data_column_id) || !n_groups, "MIN / MAX over strings: unencoded string segments stay on the CPU path");
      for (ChunkID k = 0; n_groups && k < data_table->chunk_count(); ++k) {
        const auto& dictionary = static_cast<const DictionarySegment<std::string>&>(*data_table->get_chunk(k)->get_segment(data_column_id)).dictionary();
        rank_orders[a].insert(rank_orders[a].end(), dictionary.begin(), dictionary.end());
      }
      std::sort(rank_orders[a].begin(), rank_orders[a].end());
      rank_orders[a].erase(std::unique(rank_orders[a].begin(), rank_orders[a].end()), rank_orders[a].end());
    }
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (uint64_t begin = 0; begin < n_groups; begin += Chunk::DEFAULT_SIZE) {
      const auto chunk = static_cast<uint32_t>(begin / Chunk::DEFAULT_SIZE);
      const auto size = static_cast<ChunkOffset>(std::min<uint64_t>(Chunk::DEFAULT_SIZE, n_groups - begin));
      Segments segments;
      for (size_t g = 0; g < _groupby.size(); ++g) {
        const auto& definition = definitions[g];
        if (groupby_owners[g]) { segments.push_back(resident_segment(definition.data_type, groupby_owners[g], chunk, size)); continue; }
        if (groupby_strings[g]) { segments.push_back(std::make_shared<DeviceStringDictionarySegment>(groupby_strings[g], chunk, size)); continue; }
        std::vector<std::vector<AllTypeVariant>> cells;
        for (uint64_t r = begin; r < begin + size; ++r) cells.push_back({(*input.get_chunk(host_rows()[r].chunk_id)->get_segment(_groupby[g]))[host_rows()[r].chunk_offset]});
        switch (definition.data_type) {
          case DataType::Int: segments.push_back(make_value_segment<int32_t>(cells, ColumnID{0}, definition.nullable)); break;
          case DataType::Long: segments.push_back(make_value_segment<int64_t>(cells, ColumnID{0}, definition.nullable)); break;
          case DataType::Float: segments.push_back(make_value_segment<float>(cells, ColumnID{0}, definition.nullable)); break;
          case DataType::Double: segments.push_back(make_value_segment<double>(cells, ColumnID{0}, definition.nullable)); break;
          default: segments.push_back(make_value_segment<std::string>(cells, ColumnID{0}, definition.nullable)); break;
        }
      }
      for (size_t a = 0; a < specs.size(); ++a) {
        if (!string_aggregate(a)) { segments.push_back(resident_segment(definitions[_groupby.size() + a].data_type, aggregate_owners[a], chunk, size)); continue; }
        if (aggregate_strings[a]) { segments.push_back(std::make_shared<DeviceStringDictionarySegment>(aggregate_strings[a], chunk, size)); continue; }
        std::vector<std::vector<AllTypeVariant>> cells;
        if (_aggregates[a].function == WindowFunction::Any) {
          for (uint64_t r = begin; r < begin + size; ++r) cells.push_back({(*input.get_chunk(host_rows()[r].chunk_id)->get_segment(_aggregates[a].column_id))[host_rows()[r].chunk_offset]});
        } else {   // the chunk's ranks (int32 made on the device, int64 made on the host) read back, every rank its string
          const bool wide = static_cast<DataType>(hy_column_data_type(aggregate_handles[a])) == DataType::Long;
          std::vector<int64_t> ranks(size);
          std::vector<uint64_t> null_words((size_t{size} + 63) / 64, 0);
          check_status(hy_column_read_chunk(aggregate_handles[a], chunk, ranks.data(), null_words.data()));
          for (ChunkOffset r = 0; r < size; ++r) {
            const int64_t rank = wide ? ranks[r] : reinterpret_cast<const int32_t*>(ranks.data())[r];
            if ((null_words[r / 64] >> (r % 64)) & 1) cells.push_back({AllTypeVariant{NullValue{}}});
            else cells.push_back({AllTypeVariant{rank_orders[a].at(static_cast<size_t>(rank))}});
          }
        }
        segments.push_back(make_value_segment<std::string>(cells, ColumnID{0}, true));
      }
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    return std::make_shared<Table>(std::move(definitions), TableType::Data, std::move(chunks));
  }

 private:
  std::vector<AggregateDefinition> _aggregates;
  std::vector<ColumnID> _groupby;
};

// ---- TableScan(s) -> Projection -> AggregateHash of one data table in ONE pass (hy_scan_project_aggregate) --------------------------------
// What the adapter substitutes for the plan  GetTable -> [Validate ->] TableScan ... -> Projection -> AggregateHash  when every scan is a
// ColumnVsValue / Between / IsNull scan of a numeric column of the stored table and every aggregate a MIN / MAX / SUM / AVG / COUNT of an
// arithmetic expression over its columns (tpch_queries.cpp:60-80, 206-210: Q1, Q6).  Expressions are given in postfix order, like
// hy_expression:  l_extendedprice * (1 - l_discount)  =  column, literal 1, column, Subtraction, Multiplication.
enum class ArithmeticOperator : uint8_t { Addition, Subtraction, Multiplication, Division, Modulo };   // expression/arithmetic_expression.hpp:12
struct ExpressionNode {
  static ExpressionNode column(ColumnID id) { ExpressionNode n; n.kind = HY_EXPR_COLUMN; n.column_id = id; return n; }
  static ExpressionNode literal(AllTypeVariant v) { ExpressionNode n; n.kind = HY_EXPR_LITERAL; n.value = std::move(v); return n; }
  static ExpressionNode arithmetic(ArithmeticOperator op) { ExpressionNode n; n.kind = HY_EXPR_ARITHMETIC; n.op = op; return n; }
  uint32_t kind = HY_EXPR_COLUMN;
  ColumnID column_id = INVALID_COLUMN_ID;
  AllTypeVariant value;
  ArithmeticOperator op = ArithmeticOperator::Addition;
};
struct ScanPredicate {   // column <condition> value [AND value2]
  ColumnID column_id;
  PredicateCondition condition;
  AllTypeVariant value;
  std::optional<AllTypeVariant> value2;
};
struct ExpressionAggregate {   // WindowFunctionExpression over an arithmetic expression (no nodes: COUNT(*))
  WindowFunction function;
  std::vector<ExpressionNode> input;
};

class ScanProjectAggregate : public AbstractReadOnlyOperator {
 public:
  ScanProjectAggregate(std::shared_ptr<const AbstractOperator> in, std::vector<ScanPredicate> predicates, std::vector<ColumnID> groupby_column_ids, std::vector<ExpressionAggregate> aggregates)
      : AbstractReadOnlyOperator(std::move(in)), _predicates(std::move(predicates)), _groupby(std::move(groupby_column_ids)), _aggregates(std::move(aggregates)) {}
  const std::string& name() const override { static const std::string n = "ScanProjectAggregate"; return n; }
  // with a context, Validate is the pass's first filter (sql_pipeline_builder.hpp:55: every SQL-driven plan validates behind GetTable)
  void set_transaction_context(std::shared_ptr<TransactionContext> context) { _context = std::move(context); }

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto input = left_input_table();
    Assert(input->type() == TableType::Data, "ScanProjectAggregate reads a stored table: run the operator chain on reference tables.");
    std::vector<std::shared_ptr<DeviceColumn>> keep;
    std::vector<hy_filter> filters;
    if (_context) {
      keep.push_back(mvcc_column(input));
      hy_filter filter{};
      filter.column = keep.back()->handle;
      filter.predicate.condition = HY_FILTER_VALIDATE;
      filter.predicate.value.value_id = _context->transaction_id();
      filter.predicate.value2.value_id = _context->snapshot_commit_id();
      filter.predicate.column_is_nullable = _context->has_in_flight_delete() ? 0u : 1u;   // can_use_chunk_shortcut (validate.cpp:116-127)
      filters.push_back(filter);
    }
    for (const auto& predicate : _predicates) {
      const auto column_type = input->column_data_type(predicate.column_id);
      Assert(column_type != DataType::String, "ScanProjectAggregate: string predicates run as the operator chain.");
      keep.push_back(device_column(input, predicate.column_id));
      hy_filter filter{};
      filter.column = keep.back()->handle;
      filter.predicate.condition = static_cast<uint32_t>(predicate.condition);
      filter.predicate.column_is_nullable = input->column_is_nullable(predicate.column_id);
      if (predicate.condition != PredicateCondition::IsNull && predicate.condition != PredicateCondition::IsNotNull) {
        const hy_value first = to_hy_value(predicate.value), second = predicate.value2 ? to_hy_value(*predicate.value2) : hy_value{};
        hy_predicate cast{};
        const auto status = hy_predicate_cast(static_cast<uint32_t>(predicate.condition), static_cast<uint32_t>(column_type), static_cast<uint32_t>(data_type_from_all_type_variant(predicate.value)), &first,
                                              predicate.value2 ? static_cast<uint32_t>(data_type_from_all_type_variant(*predicate.value2)) : HY_TYPE_NULL, predicate.value2 ? &second : nullptr, &cast);
        Assert(status != HY_ERR_UNSUPPORTED, "ScanProjectAggregate: the literal has no lossless predicate cast -- run the operator chain.");
        check_status(status);
        filter.predicate.condition = cast.condition, filter.predicate.value_type = cast.value_type, filter.predicate.value = cast.value, filter.predicate.value2 = cast.value2;
      }
      filters.push_back(filter);
    }
    std::vector<const hy_column*> groupby;
    for (const auto id : _groupby) {
      keep.push_back(device_column(input, id, input->column_data_type(id) == DataType::String ? StringKeys::AggregateKeyNames : StringKeys::None));
      groupby.push_back(keep.back()->handle);
    }
    std::vector<hy_expression> expressions(_aggregates.size());
    std::vector<hy_fused_aggregate> specs(_aggregates.size());
    for (size_t a = 0; a < _aggregates.size(); ++a) {
      specs[a].function = static_cast<uint32_t>(_aggregates[a].function);
      const auto& nodes = _aggregates[a].input;
      if (nodes.empty()) { Assert(_aggregates[a].function == WindowFunction::Count, "Only COUNT may omit its argument."); continue; }
      Assert(nodes.size() <= HY_MAX_EXPRESSION_NODES, "ScanProjectAggregate: expression too long -- run the operator chain.");
      expressions[a].n_nodes = static_cast<uint32_t>(nodes.size());
      for (size_t k = 0; k < nodes.size(); ++k) {
        hy_expression_node& out = expressions[a].nodes[k];
        out.kind = nodes[k].kind;
        if (nodes[k].kind == HY_EXPR_COLUMN) {
          keep.push_back(device_column(input, nodes[k].column_id));
          out.column = keep.back()->handle;
        } else if (nodes[k].kind == HY_EXPR_LITERAL) {
          out.literal_type = static_cast<uint32_t>(data_type_from_all_type_variant(nodes[k].value));
          if (!variant_is_null(nodes[k].value)) out.literal = to_hy_value(nodes[k].value);
        } else {
          out.op = static_cast<uint32_t>(nodes[k].op);
        }
      }
      specs[a].input = &expressions[a];
    }
    const uint32_t capacity = static_cast<uint32_t>(input->row_count() + 1);
    std::vector<RowID> group_rows(capacity);
    std::vector<std::vector<uint64_t>> values(specs.size(), std::vector<uint64_t>(capacity));
    std::vector<std::vector<uint8_t>> nulls(specs.size(), std::vector<uint8_t>(capacity));
    std::vector<hy_aggregate_column> columns(std::max<size_t>(1, specs.size()));
    for (size_t a = 0; a < specs.size(); ++a) { columns[a].values = values[a].data(); columns[a].is_null = nulls[a].data(); }
    hy_aggregate_result result{};
    result.mem = HY_MEM_HOST;
    result.group_capacity = capacity;
    result.group_row_ids = reinterpret_cast<hy_row_id*>(group_rows.data());
    result.columns = columns.data();
    check_status(hy_scan_project_aggregate(filters.data(), static_cast<uint32_t>(filters.size()), groupby.data(), static_cast<uint32_t>(groupby.size()), specs.data(),
                                           static_cast<uint32_t>(specs.size()), &result));
    // output like AggregateHash's: GROUP BY values through the representative rows (rows of the stored table), then the aggregates
    TableColumnDefinitions definitions;
    for (const auto id : _groupby) definitions.push_back(input->column_definitions()[id]);
    static const char* names[] = {"MIN", "MAX", "SUM", "AVG", "COUNT", "COUNT DISTINCT", "STDDEV_SAMP", "ANY"};
    for (size_t a = 0; a < specs.size(); ++a) {
      const bool needs_null = _aggregates[a].function != WindowFunction::Count;
      definitions.push_back({std::string(names[static_cast<int>(_aggregates[a].function)]) + "(" + (_aggregates[a].input.empty() ? "*" : "expression " + std::to_string(a)) + ")",
                             static_cast<DataType>(columns[a].data_type), needs_null});
    }
    auto output = std::make_shared<Table>(definitions, TableType::Data, Chunk::DEFAULT_SIZE);
    for (uint32_t g = 0; g < result.n_groups; ++g) {
      std::vector<AllTypeVariant> row;
      for (const auto id : _groupby) row.push_back((*input->get_chunk(group_rows[g].chunk_id)->get_segment(id))[group_rows[g].chunk_offset]);
      for (size_t a = 0; a < specs.size(); ++a) {
        if (nulls[a][g]) { row.emplace_back(NullValue{}); continue; }
        switch (static_cast<DataType>(columns[a].data_type)) {
          case DataType::Int: row.emplace_back(reinterpret_cast<const int32_t*>(values[a].data())[g]); break;
          case DataType::Long: row.emplace_back(reinterpret_cast<const int64_t*>(values[a].data())[g]); break;
          case DataType::Float: row.emplace_back(reinterpret_cast<const float*>(values[a].data())[g]); break;
          default: row.emplace_back(reinterpret_cast<const double*>(values[a].data())[g]); break;
        }
      }
      output->append(std::move(row));
    }
    output->finalize();
    return output;
  }

 private:
  std::vector<ScanPredicate> _predicates;
  std::vector<ColumnID> _groupby;
  std::vector<ExpressionAggregate> _aggregates;
  std::shared_ptr<TransactionContext> _context;
};

// ---- a star join as one operator (hy_star_join_aggregate, csrc/plan.hip) ---------------------------------------------------------------
// fact JOIN dimension_1 ... JOIN dimension_k (Inner, one key each, in this order) -> GROUP BY columns of any of the tables -> aggregates
// over fact / dimension columns or over `left <op> right`: the subtree TableScan(s) -> JoinHash(es) -> Projection -> AggregateHash that
// Hyrise's optimizer produces for SSB, handed to the library as ONE call.  Inputs are stored tables; the output is AggregateHash's: the
// GROUP BY columns, then one column per aggregate.
struct StarDimension {
  std::shared_ptr<const AbstractOperator> table;
  ColumnID key;
  std::optional<ScanPredicate> filter;   // on a column of the dimension; none: the dimension is joined whole
  ColumnID fact_key;
};
struct StarColumn { size_t table; ColumnID column; };   // table 0 = the fact table, d + 1 = dimension d
struct StarAggregate {
  WindowFunction function;
  std::optional<StarColumn> left;                    // none: COUNT(*)
  std::optional<ArithmeticOperator> op;              // with `right`: the aggregate of  left <op> right
  std::optional<StarColumn> right;
};

class StarJoinAggregate : public AbstractReadOnlyOperator {
 public:
  StarJoinAggregate(std::shared_ptr<const AbstractOperator> fact, std::vector<StarDimension> dimensions, std::vector<StarColumn> groupby, std::vector<StarAggregate> aggregates)
      : AbstractReadOnlyOperator(std::move(fact)), _dimensions(std::move(dimensions)), _groupby(std::move(groupby)), _aggregates(std::move(aggregates)) {}
  const std::string& name() const override { static const std::string n = "StarJoinAggregate"; return n; }
  uint64_t joined_rows = 0;

 protected:
  std::shared_ptr<const Table> _on_execute() override {
    const auto fact = left_input_table();
    std::vector<std::shared_ptr<const Table>> tables{fact};
    for (const auto& dimension : _dimensions) tables.push_back(dimension.table->get_output());   // (executed by the caller, like every input)
    for (const auto& table : tables) Assert(table->type() == TableType::Data, "StarJoinAggregate reads stored tables.");
    std::vector<std::shared_ptr<DeviceColumn>> keep;
    auto column_of = [&](const StarColumn& c) -> const hy_column* {
      Assert(c.table < tables.size(), "StarJoinAggregate: no such table.");
      Assert(tables[c.table]->column_data_type(c.column) != DataType::String, "StarJoinAggregate: string columns run as the operator chain.");
      keep.push_back(device_column(tables[c.table], c.column));
      return keep.back()->handle;
    };
    std::vector<hy_star_dimension> dims(_dimensions.size());
    for (size_t d = 0; d < _dimensions.size(); ++d) {
      std::memset(&dims[d], 0, sizeof(dims[d]));
      dims[d].key = column_of({d + 1, _dimensions[d].key});
      dims[d].fact_key = column_of({0, _dimensions[d].fact_key});
      if (!_dimensions[d].filter) continue;
      const ScanPredicate& predicate = *_dimensions[d].filter;
      const auto column_type = tables[d + 1]->column_data_type(predicate.column_id);
      dims[d].filter_column = column_of({d + 1, predicate.column_id});
      dims[d].predicate.condition = static_cast<uint32_t>(predicate.condition);
      dims[d].predicate.column_is_nullable = tables[d + 1]->column_is_nullable(predicate.column_id);
      if (predicate.condition != PredicateCondition::IsNull && predicate.condition != PredicateCondition::IsNotNull) {
        const hy_value first = to_hy_value(predicate.value), second = predicate.value2 ? to_hy_value(*predicate.value2) : hy_value{};
        hy_predicate cast{};
        const auto status = hy_predicate_cast(static_cast<uint32_t>(predicate.condition), static_cast<uint32_t>(column_type), static_cast<uint32_t>(data_type_from_all_type_variant(predicate.value)), &first,
                                              predicate.value2 ? static_cast<uint32_t>(data_type_from_all_type_variant(*predicate.value2)) : HY_TYPE_NULL, predicate.value2 ? &second : nullptr, &cast);
        Assert(status != HY_ERR_UNSUPPORTED, "StarJoinAggregate: the literal has no lossless predicate cast -- run the operator chain.");
        check_status(status);
        dims[d].predicate.condition = cast.condition, dims[d].predicate.value_type = cast.value_type, dims[d].predicate.value = cast.value, dims[d].predicate.value2 = cast.value2;
      }
    }
    std::vector<hy_star_column> groupby(_groupby.size());
    for (size_t g = 0; g < _groupby.size(); ++g) groupby[g] = hy_star_column{static_cast<uint32_t>(_groupby[g].table), 0, column_of(_groupby[g])};
    // the caller's aggregates, then MIN of every GROUP BY column: the groups' representative rows are rows of an intermediate table
    std::vector<hy_star_aggregate> specs(_aggregates.size() + _groupby.size());
    for (size_t a = 0; a < _aggregates.size(); ++a) {
      std::memset(&specs[a], 0, sizeof(specs[a]));
      specs[a].function = static_cast<uint32_t>(_aggregates[a].function);
      specs[a].op = HY_STAR_NO_OP;
      if (!_aggregates[a].left) { Assert(_aggregates[a].function == WindowFunction::Count, "Only COUNT may omit its argument."); continue; }
      specs[a].left = hy_star_column{static_cast<uint32_t>(_aggregates[a].left->table), 0, column_of(*_aggregates[a].left)};
      if (_aggregates[a].op) {
        Assert(_aggregates[a].right.has_value(), "StarJoinAggregate: an expression needs two columns.");
        specs[a].op = static_cast<uint32_t>(*_aggregates[a].op);
        specs[a].right = hy_star_column{static_cast<uint32_t>(_aggregates[a].right->table), 0, column_of(*_aggregates[a].right)};
      }
    }
    for (size_t g = 0; g < _groupby.size(); ++g) {
      std::memset(&specs[_aggregates.size() + g], 0, sizeof(hy_star_aggregate));
      specs[_aggregates.size() + g].function = HY_AGG_MIN;
      specs[_aggregates.size() + g].op = HY_STAR_NO_OP;
      specs[_aggregates.size() + g].left = groupby[g];
    }
    Assert(specs.size() <= HY_MAX_STAR_AGGREGATES, "StarJoinAggregate: too many aggregates and GROUP BY columns for one call.");
    const uint32_t capacity = static_cast<uint32_t>(std::min<uint64_t>(fact->row_count() + 1, 1u << 20));
    std::vector<RowID> group_rows(capacity);
    std::vector<std::vector<uint64_t>> values(specs.size(), std::vector<uint64_t>(capacity));
    std::vector<std::vector<uint8_t>> nulls(specs.size(), std::vector<uint8_t>(capacity));
    std::vector<hy_aggregate_column> columns(std::max<size_t>(1, specs.size()));
    for (size_t a = 0; a < specs.size(); ++a) { columns[a].values = values[a].data(); columns[a].is_null = nulls[a].data(); }
    hy_aggregate_result result{};
    result.mem = HY_MEM_HOST;
    result.group_capacity = capacity;
    result.group_row_ids = reinterpret_cast<hy_row_id*>(group_rows.data());
    result.columns = columns.data();
    check_status(hy_star_join_aggregate(dims.data(), static_cast<uint32_t>(dims.size()), groupby.data(), static_cast<uint32_t>(groupby.size()), specs.data(), static_cast<uint32_t>(specs.size()),
                                        &result, &joined_rows));
    TableColumnDefinitions definitions;
    for (const auto& g : _groupby) definitions.push_back(tables[g.table]->column_definitions()[g.column]);
    static const char* names[] = {"MIN", "MAX", "SUM", "AVG", "COUNT", "COUNT DISTINCT", "STDDEV_SAMP", "ANY"};
    for (size_t a = 0; a < _aggregates.size(); ++a)
      definitions.push_back({std::string(names[static_cast<int>(_aggregates[a].function)]) + "(" + (_aggregates[a].left ? "expression " + std::to_string(a) : "*") + ")", static_cast<DataType>(columns[a].data_type),
                             _aggregates[a].function != WindowFunction::Count});
    auto cell = [&](size_t a, uint32_t g) -> AllTypeVariant {
      if (nulls[a][g]) return NullValue{};
      switch (static_cast<DataType>(columns[a].data_type)) {
        case DataType::Int: return reinterpret_cast<const int32_t*>(values[a].data())[g];
        case DataType::Long: return reinterpret_cast<const int64_t*>(values[a].data())[g];
        case DataType::Float: return reinterpret_cast<const float*>(values[a].data())[g];
        default: return reinterpret_cast<const double*>(values[a].data())[g];
      }
    };
    auto output = std::make_shared<Table>(definitions, TableType::Data, Chunk::DEFAULT_SIZE);
    for (uint32_t g = 0; g < result.n_groups; ++g) {
      std::vector<AllTypeVariant> row;
      for (size_t k = 0; k < _groupby.size(); ++k) row.push_back(cell(_aggregates.size() + k, g));
      for (size_t a = 0; a < _aggregates.size(); ++a) row.push_back(cell(a, g));
      output->append(std::move(row));
    }
    output->finalize();
    return output;
  }

 private:
  std::vector<StarDimension> _dimensions;
  std::vector<StarColumn> _groupby;
  std::vector<StarAggregate> _aggregates;
};

// ---- Projection (operators/projection.hpp, projection.cpp) ------------------------------------------------------------------------------
// A minimal expression tree (expression/*.hpp): what hy_projection_expression evaluates.  A predicate between a STRING column and string
// literals (binary, LIKE family, In / NotIn) becomes a column test, lowered through TableScan's own functions.
// Substr (FunctionExpression(Substring), expression_evaluator.cpp:1566-1642) is a Projection's column of its own, not a node of a program:
// SUBSTR(string column, literal, literal) becomes one hy_string_column_substr call; over anything else, or below another expression, a Fail.
enum class ExpressionType : uint8_t { Column, Value, Arithmetic, Predicate, IsNull, IsNotNull, And, Or, UnaryMinus, Case, Substr };
struct Expression {
  ExpressionType type;
  ColumnID column_id = 0;                      // Column
  AllTypeVariant value = NullValue{};          // Value
  ArithmeticOperator arithmetic_operator = ArithmeticOperator::Addition;
  PredicateCondition condition = PredicateCondition::Equals;
  std::vector<std::shared_ptr<const Expression>> arguments;   // Predicate: left, right (In / NotIn: left, then the list's elements)
  int32_t substr_start = 0, substr_length = 0;   // Substr: the two literals, Long ones cast to Int (expression_evaluator.cpp:1572-1578)
};
using ExpressionPtr = std::shared_ptr<const Expression>;
inline ExpressionPtr column_(ColumnID column_id) { auto e = std::make_shared<Expression>(); e->type = ExpressionType::Column; e->column_id = column_id; return e; }
inline ExpressionPtr value_(AllTypeVariant value) { auto e = std::make_shared<Expression>(); e->type = ExpressionType::Value; e->value = std::move(value); return e; }
inline ExpressionPtr null_() { return value_(NullValue{}); }
inline ExpressionPtr expression_of(ExpressionType type, std::vector<ExpressionPtr> arguments) {
  auto e = std::make_shared<Expression>(); e->type = type; e->arguments = std::move(arguments); return e;
}
inline ExpressionPtr arithmetic_(ArithmeticOperator op, ExpressionPtr l, ExpressionPtr r) {
  auto e = std::make_shared<Expression>(); e->type = ExpressionType::Arithmetic; e->arithmetic_operator = op; e->arguments = {std::move(l), std::move(r)}; return e;
}
inline ExpressionPtr predicate_(PredicateCondition condition, std::vector<ExpressionPtr> arguments) {
  auto e = std::make_shared<Expression>(); e->type = ExpressionType::Predicate; e->condition = condition; e->arguments = std::move(arguments); return e;
}
inline ExpressionPtr and_(ExpressionPtr l, ExpressionPtr r) { return expression_of(ExpressionType::And, {std::move(l), std::move(r)}); }
inline ExpressionPtr or_(ExpressionPtr l, ExpressionPtr r) { return expression_of(ExpressionType::Or, {std::move(l), std::move(r)}); }
inline ExpressionPtr is_null_(ExpressionPtr x) { return expression_of(ExpressionType::IsNull, {std::move(x)}); }
inline ExpressionPtr is_not_null_(ExpressionPtr x) { return expression_of(ExpressionType::IsNotNull, {std::move(x)}); }
inline ExpressionPtr unary_minus_(ExpressionPtr x) { return expression_of(ExpressionType::UnaryMinus, {std::move(x)}); }
inline ExpressionPtr substr_(ExpressionPtr string_column, int32_t start, int32_t length) {
  auto e = std::make_shared<Expression>(); e->type = ExpressionType::Substr; e->arguments = {std::move(string_column)}; e->substr_start = start; e->substr_length = length; return e;
}
// _evaluate_substring's loop body (expression_evaluator.cpp:1597-1638) in 64-bit arithmetic: what hy_string_column_substr computes per entry
inline std::string substr_of(const std::string& string, int32_t start, int32_t length) {
  if (length <= 0) return {};
  const auto n = static_cast<int64_t>(string.size());
  int64_t s = 0, l = length;
  if (start < 0) s = int64_t{start} + n;
  else if (start == 0) l -= 1;
  else s = int64_t{start} - 1;
  const auto e = std::min(s + l, n);
  s = std::max<int64_t>(s, 0);
  return s < n && e > s ? string.substr(static_cast<size_t>(s), static_cast<size_t>(e - s)) : std::string{};
}
inline ExpressionPtr case_(ExpressionPtr when, ExpressionPtr then, ExpressionPtr otherwise) { return expression_of(ExpressionType::Case, {std::move(when), std::move(then), std::move(otherwise)}); }

class Projection : public AbstractReadOnlyOperator {
 public:
  Projection(std::shared_ptr<const AbstractOperator> in, std::vector<ExpressionPtr> expressions, std::vector<std::string> names = {})
      : AbstractReadOnlyOperator(std::move(in)), _expressions(std::move(expressions)), _names(std::move(names)) {}
  const std::string& name() const override { static const std::string n = "Projection"; return n; }

 protected:
  // projection.cpp:56-240 in its three steps: forward unmodified columns, evaluate the others, build the output table
  std::shared_ptr<const Table> _on_execute() override {
    const auto in_table = left_input_table();
    const auto chunk_count = in_table->chunk_count();
    // ---- "ForwardUnmodifiedColumns" (projection.cpp:69-100): a PQPColumnExpression shares its segments, reference segments stay reference segments
    bool any_computed = false;
    for (const auto& e : _expressions) any_computed = any_computed || e->type != ExpressionType::Column;
    // ---- evaluate (projection.cpp:129-190: one ExpressionEvaluator per chunk; here: one hy_projection_expression per computed column)
    std::vector<std::shared_ptr<const DeviceColumnOwner>> owners(_expressions.size());
    std::vector<std::shared_ptr<const DeviceStringResult>> substrings(_expressions.size());   // SUBSTR, or a forwarded string column behind PosLists, made in HBM; without one, the host loops below
    TableColumnDefinitions definitions;
    for (size_t i = 0; i < _expressions.size(); ++i) {
      const auto& e = _expressions[i];
      const std::string name = i < _names.size() ? _names[i] : (e->type == ExpressionType::Column ? in_table->column_name(e->column_id) : "expression_" + std::to_string(i));
      if (e->type == ExpressionType::Column) {
        const auto type = in_table->column_data_type(e->column_id);
        definitions.push_back({name, type, in_table->column_is_nullable(e->column_id)});
        // ---- build (projection.cpp:192-236): the output is a data table when a column was computed; a forwarded REFERENCE segment cannot
        // live in it (:201-215 materialises it through the evaluator).  Numeric: the column itself as a one-node program -- hy_column_gather's
        // result with the input's chunk layout kept --, strings from the RowIDs on the host (below).
        if (any_computed && in_table->type() == TableType::References && type != DataType::String && chunk_count) owners[i] = evaluate(in_table, e);
        // A string column behind PosLists, wholly dictionary-encoded: one hy_string_column_materialize, the chunks DictionarySegments in HBM
        if (any_computed && in_table->type() == TableType::References && type == DataType::String && chunk_count) {
          substrings[i] = materialized_string_column(in_table, e->column_id);
          if (substrings[i]) definitions.back().nullable = true;   // (as the host loop below leaves it)
        }
        continue;
      }
      if (e->type == ExpressionType::Substr) {
        Assert(e->arguments.size() == 1 && is_string_column(*in_table, *e->arguments[0]), "Projection: SUBSTR takes a string column (SUBSTR of an expression: the stock evaluator)");
        substrings[i] = substring_column(in_table, e->arguments[0]->column_id, e->substr_start, e->substr_length);
        definitions.push_back({name, DataType::String, true});
        continue;
      }
      Assert(chunk_count > 0, "Projection: an expression over a table without chunks has no device column to read");
      owners[i] = evaluate(in_table, e);
      definitions.push_back({name, static_cast<DataType>(hy_column_data_type(owners[i]->handle)), true});   // (the evaluator's results carry a null vector)
    }
    const auto resident_segment = [](DataType type, const std::shared_ptr<const DeviceColumnOwner>& owner, uint32_t chunk, ChunkOffset size) -> std::shared_ptr<AbstractSegment> {
      switch (type) {
        case DataType::Int: return std::make_shared<DeviceValueSegment<int32_t>>(owner, chunk, size);
        case DataType::Long: return std::make_shared<DeviceValueSegment<int64_t>>(owner, chunk, size);
        case DataType::Float: return std::make_shared<DeviceValueSegment<float>>(owner, chunk, size);
        default: return std::make_shared<DeviceValueSegment<double>>(owner, chunk, size);
      }
    };
    std::vector<std::shared_ptr<Chunk>> chunks;
    for (ChunkID chunk_id = 0; chunk_id < chunk_count; ++chunk_id) {
      const auto chunk_in = in_table->get_chunk(chunk_id);
      Segments segments;
      for (size_t i = 0; i < _expressions.size(); ++i) {
        if (owners[i]) { segments.push_back(resident_segment(definitions[i].data_type, owners[i], chunk_id, chunk_in->size())); continue; }
        if (substrings[i]) { segments.push_back(std::make_shared<DeviceStringDictionarySegment>(substrings[i], chunk_id, chunk_in->size())); continue; }
        if (_expressions[i]->type == ExpressionType::Substr) {   // the host path: the same formula over the values, row by row
          const auto& e = *_expressions[i];
          const auto argument = chunk_in->get_segment(e.arguments[0]->column_id);
          std::vector<std::vector<AllTypeVariant>> cells;
          for (ChunkOffset r = 0; r < chunk_in->size(); ++r) {
            const auto value = (*argument)[r];
            if (variant_is_null(value)) cells.push_back({value});
            else cells.push_back({substr_of(std::get<std::string>(value), e.substr_start, e.substr_length)});
          }
          segments.push_back(make_value_segment<std::string>(cells, ColumnID{0}, true));
          continue;
        }
        const auto segment = chunk_in->get_segment(_expressions[i]->column_id);
        if (!any_computed || in_table->type() == TableType::Data) { segments.push_back(segment); continue; }   // shared
        std::vector<std::vector<AllTypeVariant>> cells;   // a string column behind a PosList, materialised from the RowIDs on the host
        for (ChunkOffset r = 0; r < chunk_in->size(); ++r) cells.push_back({(*segment)[r]});
        segments.push_back(make_value_segment<std::string>(cells, ColumnID{0}, true));
        definitions[i].nullable = true;
      }
      chunks.push_back(std::make_shared<Chunk>(std::move(segments)));
    }
    const auto type = any_computed ? TableType::Data : in_table->type();   // a projection that only forwards outputs a table of the input's type
    return std::make_shared<Table>(std::move(definitions), type, std::move(chunks));
  }

 private:
  friend class TableScan;   // (TableScan over a predicate expression lowers it with the functions below)
  struct Lowered {   // the program and everything its pointers name
    hy_projection_program program{};
    std::vector<std::shared_ptr<DeviceColumn>> columns;
    std::deque<std::vector<uint32_t>> words32;
    std::deque<std::vector<uint8_t>> bytes;
    std::deque<std::vector<uint64_t>> words64;
    std::deque<hy_in_list> lists;
  };

  static bool is_string_column(const Table& table, const Expression& e) { return e.type == ExpressionType::Column && table.column_data_type(e.column_id) == DataType::String; }

  static void push(Lowered& l, const hy_projection_node& node) {
    if (l.program.n_nodes >= HY_MAX_PROJECTION_NODES) Fail("Projection: the expression has more than HY_MAX_PROJECTION_NODES nodes");
    l.program.nodes[l.program.n_nodes++] = node;
  }

  static void lower(const std::shared_ptr<const Table>& in_table, const Expression& e, Lowered& l) {
    hy_projection_node node{};
    switch (e.type) {
      case ExpressionType::Column: {
        const auto column = device_column(in_table, e.column_id);
        uint32_t index = 0;
        while (index < l.columns.size() && l.columns[index]->handle != column->handle) ++index;
        if (index == l.columns.size()) {
          if (index >= HY_MAX_PROJECTION_COLUMNS) Fail("Projection: the expression reads more than HY_MAX_PROJECTION_COLUMNS columns");
          l.columns.push_back(column);
          l.program.columns[index] = column->handle;
          l.program.n_columns = index + 1;
        }
        node.kind = HY_PROJ_COLUMN;
        node.index = index;
        break;
      }
      case ExpressionType::Value:
        node.kind = HY_PROJ_LITERAL;
        node.literal_type = static_cast<uint32_t>(data_type_from_all_type_variant(e.value));
        if (e.value.index() >= 1 && e.value.index() <= 4) node.literal = to_hy_value(e.value);
        break;
      case ExpressionType::Substr: Fail("Projection: SUBSTR below another expression is not evaluated (string-valued nodes: the stock evaluator)");
      case ExpressionType::Predicate:
        if (is_string_column(*in_table, *e.arguments[0])) { lower_column_test(in_table, e, l); return; }
        if (e.condition == PredicateCondition::IsNull || e.condition == PredicateCondition::IsNotNull) {
          lower(in_table, *e.arguments[0], l);
          node.kind = e.condition == PredicateCondition::IsNull ? HY_PROJ_IS_NULL : HY_PROJ_IS_NOT_NULL;
          break;
        }
        Assert(e.arguments.size() == 2, "Projection: a numeric predicate is binary (Between, In: HY_ERR_UNSUPPORTED on this path)");
        lower(in_table, *e.arguments[0], l);
        lower(in_table, *e.arguments[1], l);
        node.kind = HY_PROJ_COMPARISON;
        node.op = static_cast<uint32_t>(e.condition);
        break;
      default: {
        if ((e.type == ExpressionType::IsNull || e.type == ExpressionType::IsNotNull) && is_string_column(*in_table, *e.arguments[0])) {   // string IS [NOT] NULL: a column test
          Expression test;
          test.type = ExpressionType::Predicate;
          test.condition = e.type == ExpressionType::IsNull ? PredicateCondition::IsNull : PredicateCondition::IsNotNull;
          test.arguments = e.arguments;
          lower_column_test(in_table, test, l);
          return;
        }
        for (const auto& argument : e.arguments) lower(in_table, *argument, l);
        switch (e.type) {
          case ExpressionType::Arithmetic: node.kind = HY_PROJ_ARITHMETIC; node.op = static_cast<uint32_t>(e.arithmetic_operator); break;
          case ExpressionType::IsNull: node.kind = HY_PROJ_IS_NULL; break;
          case ExpressionType::IsNotNull: node.kind = HY_PROJ_IS_NOT_NULL; break;
          case ExpressionType::And: node.kind = HY_PROJ_AND; break;
          case ExpressionType::Or: node.kind = HY_PROJ_OR; break;
          case ExpressionType::UnaryMinus: node.kind = HY_PROJ_UNARY_MINUS; break;
          default: node.kind = HY_PROJ_CASE; break;
        }
      }
    }
    push(l, node);
  }

  // string column <condition> 'literal' | LIKE 'pattern' | IN ('a', ...): the hy_predicate / hy_in_list TableScan makes for the same scan
  static void lower_column_test(const std::shared_ptr<const Table>& in_table, const Expression& e, Lowered& l) {
    const auto column_id = e.arguments[0]->column_id;
    if (l.program.n_tests >= HY_MAX_PROJECTION_TESTS) Fail("Projection: the expression has more than HY_MAX_PROJECTION_TESTS column tests");
    l.columns.push_back(device_column(in_table, column_id));   // (kept alive; not one of program.columns)
    hy_projection_test& test = l.program.tests[l.program.n_tests];
    test.column = l.columns.back()->handle;
    test.predicate.condition = static_cast<uint32_t>(e.condition);
    test.predicate.column_is_nullable = in_table->column_is_nullable(column_id);
    const auto literal = [&](size_t i) -> const AllTypeVariant& {
      Assert(e.arguments.size() > i && e.arguments[i]->type == ExpressionType::Value, "Projection: a string column is compared with literals");
      return e.arguments[i]->value;
    };
    const bool like = e.condition >= PredicateCondition::Like && e.condition <= PredicateCondition::NotLikeInsensitive;
    if (e.condition == PredicateCondition::In || e.condition == PredicateCondition::NotIn) {
      std::vector<std::string> strings;
      for (size_t i = 1; i < e.arguments.size(); ++i) {
        Assert(std::holds_alternative<std::string>(literal(i)), "Projection: IN over a string column takes string literals (NULL elements: the stock evaluator)");
        strings.push_back(std::get<std::string>(literal(i)));
      }
      l.words32.emplace_back();
      TableScan::resolve_string_list(in_table, column_id, strings, l.words32.back());
      hy_in_list list{};
      list.value_type = HY_TYPE_STRING;
      list.n_values = static_cast<uint32_t>(strings.size());
      list.negated = e.condition == PredicateCondition::NotIn;
      list.column_is_nullable = test.predicate.column_is_nullable;
      list.per_chunk_value_ids = l.words32.back().data();
      l.lists.push_back(list);
      test.in_list = &l.lists.back();
    } else if (like) {
      Assert(std::holds_alternative<std::string>(literal(1)), "Right parameter must be a string.");
      l.words64.emplace_back();
      l.words64.emplace_back();
      TableScan::find_matches_in_dictionaries(in_table, column_id, e.condition, literal(1), l.words64[l.words64.size() - 2], l.words64.back(), test.predicate);
    } else if (e.condition != PredicateCondition::IsNull && e.condition != PredicateCondition::IsNotNull) {
      Assert(data_type_from_all_type_variant(literal(1)) == DataType::String, "Cannot scan: column and value data type do not match.");
      std::optional<AllTypeVariant> second;
      if (is_between(e.condition)) second = literal(2);   // (the library refuses Between: the status reaches the caller as a Fail)
      l.words32.emplace_back();
      l.words32.emplace_back();
      l.bytes.emplace_back();
      TableScan::resolve_string_literal(in_table, column_id, e.condition, literal(1), second, l.words32[l.words32.size() - 2], l.words32.back(), l.bytes.back(), test.predicate);
    } else {
      test.predicate.value_type = HY_TYPE_STRING;
    }
    hy_projection_node node{};
    node.kind = HY_PROJ_COLUMN_TEST;
    node.index = l.program.n_tests++;
    push(l, node);
  }

  // SUBSTR(column, start, length) made in HBM: one hy_string_column_substr over the input's column -- a data column, or a reference column with
  // its PosLists where they are.  nullptr: the switch is off, the column is not wholly dictionary-encoded, or the library refused it.
  static std::shared_ptr<const DeviceStringResult> substring_column(const std::shared_ptr<const Table>& in_table, ColumnID column_id, int32_t start, int32_t length) {
    std::shared_ptr<const Table> data_table;
    ColumnID data_column_id = column_id;
    if (!device_string_results() || !string_dictionary_column(in_table, column_id, data_table, data_column_id)) return nullptr;
    const auto column = device_column(in_table, column_id);
    const auto dictionary = device_string_dictionary(data_table, data_column_id);
    hy_column* made = nullptr;
    hy_string_dictionary* made_dictionary = nullptr;
    const auto status = hy_string_column_substr(column->handle, dictionary->handle, start, length, &made, &made_dictionary);
    if (status == HY_ERR_UNSUPPORTED) return nullptr;
    check_status(status);
    return std::make_shared<const DeviceStringResult>(made, made_dictionary);
  }

  // A forwarded string column of a reference table made in HBM (projection.cpp:201-215 materialises it through the evaluator): one
  // hy_string_column_materialize over the reference column, its PosLists where they are.  nullptr: as substring_column.
  static std::shared_ptr<const DeviceStringResult> materialized_string_column(const std::shared_ptr<const Table>& in_table, ColumnID column_id) {
    std::shared_ptr<const Table> data_table;
    ColumnID data_column_id = column_id;
    if (!device_string_results() || !string_dictionary_column(in_table, column_id, data_table, data_column_id)) return nullptr;
    const auto column = device_column(in_table, column_id);
    const auto dictionary = device_string_dictionary(data_table, data_column_id);
    hy_column* made = nullptr;
    hy_string_dictionary* made_dictionary = nullptr;
    const auto status = hy_string_column_materialize(column->handle, dictionary->handle, &made, &made_dictionary);
    if (status == HY_ERR_UNSUPPORTED) return nullptr;
    check_status(status);
    return std::make_shared<const DeviceStringResult>(made, made_dictionary);
  }

  std::shared_ptr<const DeviceColumnOwner> evaluate(const std::shared_ptr<const Table>& in_table, const ExpressionPtr& e) const {
    Lowered l;
    lower(in_table, *e, l);
    hy_column* column = nullptr;
    check_status(hy_projection_expression(&l.program, &column));   // HY_ERR_UNSUPPORTED is a Fail: the mirror has no CPU operators
    return std::make_shared<const DeviceColumnOwner>(column);
  }

  std::vector<ExpressionPtr> _expressions;
  std::vector<std::string> _names;
};

// ---- TableScan over a predicate expression (table_scan.cpp:450-451 -> ExpressionEvaluator::evaluate_expression_to_pos_list) ---------------
// The predicate is lowered like a Projection's expression and handed to hy_table_scan_expression; the PosLists land where every other scan's
// do (DeviceScanOutput), and the output is assembled by the same code.  Answered on the host: a Value root (Int: non-zero keeps every row,
// zero and the NULL literal none; a Long, Float, Double or String literal at the root is a Fail, "Expression type cannot be evaluated to PosList").  BETWEEN on the spine -- the root and the nodes below nothing but AND / OR -- becomes two comparisons
// (rewrite_between_expression; over a string column it stays ONE column test with a Between condition, which the library takes there);
// anywhere else the library refuses it, and what the library refuses is a Fail.
inline bool TableScan::scan_expression(const std::shared_ptr<const Table>& in_table, hy_scan_result* result, std::vector<uint32_t>& counts, std::vector<uint8_t>& states) const {
  const auto chunk_count = in_table->chunk_count();
  const auto constant = [&](bool every_row) {
    for (ChunkID c = 0; c < chunk_count; ++c) {
      const bool excluded = std::find(excluded_chunk_ids.begin(), excluded_chunk_ids.end(), c) != excluded_chunk_ids.end();
      counts[c] = every_row && !excluded ? in_table->get_chunk(c)->size() : 0;
      states[c] = counts[c] ? HY_CHUNK_ALL_MATCH : HY_CHUNK_NONE_MATCH;
    }
    return false;
  };
  if (_predicate->type == ExpressionType::Value) {
    if (variant_is_null(_predicate->value)) return constant(false);
    Assert(std::holds_alternative<int32_t>(_predicate->value), "Expression type cannot be evaluated to PosList.");
    return constant(std::get<int32_t>(_predicate->value) != 0);
  }
  if (chunk_count == 0) return constant(false);   // (no rows to test, and no device column to describe)
  std::function<ExpressionPtr(const ExpressionPtr&)> spine = [&](const ExpressionPtr& e) -> ExpressionPtr {
    if (e->type == ExpressionType::And || e->type == ExpressionType::Or) return expression_of(e->type, {spine(e->arguments[0]), spine(e->arguments[1])});
    if (e->type == ExpressionType::Predicate && is_between(e->condition) && e->arguments.size() == 3 && !Projection::is_string_column(*in_table, *e->arguments[0])) {
      const bool lower_inclusive = e->condition == PredicateCondition::BetweenInclusive || e->condition == PredicateCondition::BetweenUpperExclusive;
      const bool upper_inclusive = e->condition == PredicateCondition::BetweenInclusive || e->condition == PredicateCondition::BetweenLowerExclusive;
      return and_(predicate_(lower_inclusive ? PredicateCondition::GreaterThanEquals : PredicateCondition::GreaterThan, {e->arguments[0], e->arguments[1]}),
                  predicate_(upper_inclusive ? PredicateCondition::LessThanEquals : PredicateCondition::LessThan, {e->arguments[0], e->arguments[2]}));
    }
    return e;
  };
  Projection::Lowered l;
  Projection::lower(in_table, *spine(_predicate), l);
  check_status(hy_table_scan_expression(&l.program, excluded_chunk_ids.data(), static_cast<uint32_t>(excluded_chunk_ids.size()), result));
  return true;
}

}  // namespace hyrise_amd

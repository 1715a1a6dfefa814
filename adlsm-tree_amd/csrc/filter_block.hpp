// adlsm-tree_amd/csrc/filter_block.hpp -- host C++ mirror of the reference's
// filter API (src/filter_block.hpp:13-73, src/murmur3_hash.hpp:9) on top of the
// gfx950 C-ABI in include/adl_bloom.h.
//
// Same class names, signatures and semantics as the reference, so
// src/sstable.cpp and test/filter_block_test.cpp compile against it unchanged.
// What differs underneath:
//   * FilterBlockWriter keeps its pending keys in a packed arena (bytes +
//     uint64 offsets) instead of vector<string>.  Keys2Block() closes a filter;
//     Final() builds every filter of the block in one pipelined segmented GPU
//     build (adl_bloom_build_segmented) straight into the block buffer, at the
//     byte offsets the reference's successive appends would give them.
//   * FilterBlockReader::Init uploads the block's bitmaps once into a
//     FilterCache arena (keyed by SSTable oid); IsKeyExists probes on the GPU.
//     Batched IsKeysExist() and the level multi-get (level_filter.hpp) are
//     the intended read paths (one launch per batch).
//   * Device failures surface as RC::DEVICE_ERROR; nothing throws.
#pragma once
#include <stdint.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "rc.hpp"

struct adl_bloom_filter_set;
struct adl_bloom_filter_cache;
struct adl_bloom_cache_ticket;
struct adl_bloom_stream;

namespace adl {

using namespace std;

/* Packed key batch: key i = bytes[offsets[i] .. offsets[i+1]). */
class KeyArena {
 public:
  KeyArena() : offsets_{0} {}
  void Add(string_view key) {
    bytes_.append(key.data(), key.size());
    offsets_.push_back(bytes_.size());
  }
  /* room for `keys` more keys of `bytes` bytes in all (no reallocation while they are added) */
  void Reserve(size_t keys, size_t bytes) {
    bytes_.reserve(bytes_.size() + bytes);
    offsets_.reserve(offsets_.size() + keys);
  }
  /* keys i < n = base[off[i] .. off[i+1] - trim): a packed run of records
   * whose last `trim` bytes are not part of the key (inner keys' seq + op);
   * every record must be at least `trim` bytes.  Space is reserved once. */
  void AddTrimmed(const char *base, const uint64_t *off, size_t n, size_t trim) {
    if (!n) return;
    bytes_.reserve(bytes_.size() + (size_t)(off[n] - off[0]) - n * trim);
    offsets_.reserve(offsets_.size() + n);
    for (size_t i = 0; i < n; ++i) {
      bytes_.append(base + off[i], (size_t)(off[i + 1] - off[i]) - trim);
      offsets_.push_back(bytes_.size());
    }
  }
  void Clear() {
    bytes_.clear();
    offsets_.assign(1, 0);
  }
  size_t size() const { return offsets_.size() - 1; }
  string_view key(size_t i) const {
    return string_view(bytes_).substr(offsets_[i], offsets_[i + 1] - offsets_[i]);
  }
  bool empty() const { return size() == 0; }
  const string &bytes() const { return bytes_; }
  const vector<uint64_t> &offsets() const { return offsets_; }

 private:
  string bytes_;
  vector<uint64_t> offsets_;
};

/* src/filter_block.hpp:13-20.  The first three members are the reference's;
 * the batched extensions after them have default implementations in terms of
 * those three, so a subclass written against the reference's FilterAlgorithm
 * (overriding only Keys2Block(vector<string>), IsKeyExists and FilterInfo)
 * compiles and works unchanged in FilterBlockWriter / FilterBlockReader.
 * BloomFilter overrides them with the batched GPU path. */
class FilterAlgorithm {
 public:
  virtual RC Keys2Block(const vector<string> &keys, string &result) = 0;
  virtual bool IsKeyExists(string_view key, string_view bitmap) = 0;
  virtual void FilterInfo(string &/*info*/) { /* NOTHING */ }
  /* batched extensions (defaults: unpack and call the reference methods) */
  virtual RC Keys2Block(const KeyArena &keys, string &result);
  /* Keys2Block for consecutive filters: filter f = keys [key_begin[f],
   * key_begin[f+1]); the bitmaps are appended to result back to back, as
   * successive Keys2Block calls would, filter f starting at starts[f].  The
   * default loops over Keys2Block.  adjacent_duplicates: a hint that many keys
   * equal their predecessor (versions of one user key in memtable order); the
   * result is the same either way, an implementation may skip such keys. */
  virtual RC Keys2Blocks(const KeyArena &keys, const vector<uint64_t> &key_begin, string &result,
                         vector<uint64_t> &starts, bool adjacent_duplicates = false);
  /* out[i] = IsKeyExists(key i, bitmap); the default loops over IsKeyExists */
  virtual RC IsKeysExist(const KeyArena &keys, string_view bitmap, vector<uint8_t> &out);
  virtual ~FilterAlgorithm() = default;
};

/* src/filter_block.hpp:22-34 */
class BloomFilter : public FilterAlgorithm {
 public:
  explicit BloomFilter(int bits_per_key);
  RC Keys2Block(const vector<string> &keys, string &result) override;
  bool IsKeyExists(string_view key, string_view bitmap) override;
  void FilterInfo(string &info) override;
  RC Keys2Block(const KeyArena &keys, string &result) override;
  RC Keys2Blocks(const KeyArena &keys, const vector<uint64_t> &key_begin, string &result,
                 vector<uint64_t> &starts, bool adjacent_duplicates = false) override;
  RC IsKeysExist(const KeyArena &keys, string_view bitmap, vector<uint8_t> &out) override;
  int bits_per_key() const { return bits_per_key_; }
  int num_probes() const { return k_; }
  ~BloomFilter() = default;

 private:
  int bits_per_key_;
  int k_;
};

class FilterCache;

/* A filter block built into a FilterCache's arena and not yet published
 * (adl_bloom_cache_ticket): FilterCache::Build makes it, Publish or Abandon
 * consume it.  Move-only; a ticket destroyed while it still holds a range
 * abandons it, so its cache must outlive it. */
class FilterCacheTicket {
 public:
  FilterCacheTicket() = default;
  ~FilterCacheTicket() { Reset(); }
  FilterCacheTicket(FilterCacheTicket &&o) noexcept : cache_(o.cache_), t_(o.t_) { o.t_ = nullptr; }
  FilterCacheTicket &operator=(FilterCacheTicket &&o) noexcept {
    if (this != &o) {
      Reset();
      cache_ = o.cache_;
      t_ = o.t_;
      o.t_ = nullptr;
    }
    return *this;
  }
  FilterCacheTicket(const FilterCacheTicket &) = delete;
  FilterCacheTicket &operator=(const FilterCacheTicket &) = delete;
  explicit operator bool() const { return t_ != nullptr; }

 private:
  friend class FilterCache;
  void Reset(); /* abandons */
  adl_bloom_filter_cache *cache_ = nullptr;
  adl_bloom_cache_ticket *t_ = nullptr;
};

/* src/filter_block.hpp:36-52 */
class FilterBlockWriter {
 public:
  explicit FilterBlockWriter(unique_ptr<FilterAlgorithm> &&method);
  RC Update(string_view key);
  /* Update for a packed run (KeyArena::AddTrimmed): n keys, one reservation */
  RC UpdateBatch(const char *base, const uint64_t *off, size_t n, size_t trim);
  RC Final(string &result);
  /* Final through the write-through path when the algorithm is the
   * BloomFilter: the block (the same bytes) is built straight into `cache`'s
   * arena and `t` holds it until FilterCache::Publish names its table; verify
   * re-probes every key first (FILTER_BLOCK_ERROR when one is missing).  A
   * cache-path failure that is not a filter error (no room in the arena, a
   * block larger than it) and any other FilterAlgorithm fall back to
   * Final(result) and leave `t` empty. */
  RC Final(string &result, FilterCache &cache, FilterCacheTicket &t, bool verify);
  RC Keys2Block();
  /* keys added since the last Final that equal the previous key of their filter */
  uint64_t adjacent_duplicates() const { return dups_; }
  /* Streamed build (adl_bloom_stream): Update / UpdateBatch collect keys in a
   * small host batch that is uploaded and hashed on the device whenever it
   * reaches ADL_BLOOM_STREAM_BATCH_KEYS keys (default 1048576); the writer keeps
   * no other copy of the keys, only the last one of the open filter (for
   * adjacent_duplicates).  Keys2Block flushes and cuts; Final flushes the
   * tail, builds every filter from the stored hash pairs and frames the block
   * on the host.  Block bytes, RCs and adjacent_duplicates() are those of the
   * ordinary writer.  Only valid while no key or filter is pending
   * (BAD_RECORD otherwise); ignored when the algorithm is not the BloomFilter.
   * Final through a FilterCache goes through FilterCache::BuildStream (the
   * block built from the stream straight into the arena, verify from the
   * pairs); its fallback to the ordinary build finishes from the same stream.
   * The default is off, or on with ADL_BLOOM_STREAM_BUILD=1. */
  RC SetStreaming(bool on);
  bool streaming() const { return streaming_ && bloom_; }

 private:
  struct StreamDeleter {
    void operator()(adl_bloom_stream *s) const;
  };
  void CountDuplicates(size_t from);
  RC FlushBatch();
  RC FinalStreamed(string &result);
  void Frame(const vector<uint64_t> &offsets, string &result);
  bool streaming_ = false;
  BloomFilter *bloom_ = nullptr;  /* method_ when it is the BloomFilter */
  unique_ptr<adl_bloom_stream, StreamDeleter> stream_;
  KeyArena batch_;               /* streaming: keys of the open filter not yet appended */
  string last_key_;              /* streaming: the last key appended to the open filter */
  bool have_last_ = false;
  uint64_t stream_keys_ = 0;     /* streaming: keys since the last Final */
  bool stream_cut_ = false;      /* streaming: a filter was closed since the last Final */
  size_t batch_limit_ = 1048576;  /* DESIGN.md section 5, streamed build */
  int stream_status_ = 0;        /* streaming: the first failed append's status, returned by Final */
  KeyArena keys_;              /* keys of every filter not yet built */
  vector<uint64_t> bounds_{0}; /* filter f = keys_ [bounds_[f], bounds_[f+1]) */
  uint64_t dups_ = 0;          /* adjacent duplicates among keys_ (CountDuplicates) */
  string buffer_;
  unique_ptr<FilterAlgorithm> method_;
};

/* Device-resident filter blocks of many SSTables in one HBM arena, keyed by
 * oid (the SSTable's SHA-256 file name), least recently used evicted first:
 * the filter side of DB::table_cache_ (src/db.hpp:96-97, LRUCache
 * src/cache.hpp:23-93).  C++ handle over adl_bloom_filter_cache (C-ABI);
 * thread-safe, and no lock is held while a probe runs on the device. */
class FilterCache {
 public:
  /* bits_per_key: kept for source compatibility; blocks of any bits_per_key
   * are accepted, each probed with the k of its own "bf:" info */
  FilterCache(uint64_t capacity_bytes, uint32_t max_tables, int bits_per_key = 10);
  ~FilterCache();
  FilterCache(const FilterCache &) = delete;
  FilterCache &operator=(const FilterCache &) = delete;
  RC status() const { return status_; } /* creation result */
  int bits_per_key() const { return bits_per_key_; }
  /* FilterBlockReader::Init's checks (FILTER_BLOCK_ERROR), then one upload */
  RC Put(string_view oid, string_view filter_block);
  bool Contains(string_view oid);
  bool Remove(string_view oid);
  /* Write-through (adl_bloom_filter_cache_build): the filter block of `keys`
   * (filter f = keys [key_begin[f], key_begin[f+1])) built straight into a
   * reserved range of the arena.  `block` receives the reference's block for
   * the file; `t` holds the range until Publish makes it the resident block
   * of table `oid` (no re-upload) or Abandon gives it back.  flags:
   * ADL_BLOOM_SKIP_ADJACENT_DUPLICATES, ADL_BLOOM_CACHE_VERIFY.  A build never
   * waits for room held by unpublished tickets (DEVICE_ERROR instead). */
  using Ticket = FilterCacheTicket;
  RC Build(const KeyArena &keys, const vector<uint64_t> &key_begin, int bits_per_key, uint32_t flags, string &block,
           Ticket &t);
  /* The same with a stream (adl_bloom_stream) as the key source
   * (adl_bloom_filter_cache_build_stream): the streamed writer's cache path. */
  RC BuildStream(adl_bloom_stream *stream, int bits_per_key, uint32_t flags, string &block, Ticket &t);
  RC Publish(Ticket &t, string_view oid);
  RC Abandon(Ticket &t);
  /* arena bytes in use (blocks, tickets' ranges) and cached tables */
  uint64_t bytes_used();
  uint32_t tables();
  /* One launch for the batch: out[i] = filter `filter` of table
   * oids[table[i]] may contain keys[i] (a table that is not cached answers 1,
   * "may be present"; *uncached counts those queries). */
  RC Probe(const vector<string_view> &oids, const vector<uint32_t> &table, const KeyArena &keys, int filter,
           vector<uint8_t> &out, uint64_t *uncached = nullptr);
  /* The same batch with each key given once: key i against the tables
   * oids[table[p]], p in [begin[i], begin[i+1]) (begin: keys.size() + 1
   * entries from 0, non-decreasing; begin.back() == table.size()).  out[p]
   * and *uncached are Probe's on the expanded pairs; the keys are uploaded
   * and hashed once each (one launch, adl_bloom_filter_cache_probe_fanout). */
  RC ProbeFanout(const vector<string_view> &oids, const vector<uint32_t> &begin, const vector<uint32_t> &table,
                 const KeyArena &keys, int filter, vector<uint8_t> &out, uint64_t *uncached = nullptr);
  /* Bulk probe of keys that are already on the DEVICE
   * (adl_bloom_filter_cache_probe_batch_device): d_out[i] (device, n bytes) is
   * Probe's answer for key i against table oids[d_table[i]] (device u32; an
   * index past the list answers 0), each table with the k of its own block,
   * through the tile-binned pipeline when the batch is large.  d_offsets
   * null: keys of key_stride bytes.  cached (optional): 1 per listed table
   * that was cached.  The workspace comes from ProbeBatchWorkspaceBytes for
   * the same list, n and stride (0 with offsets); DEVICE_ERROR if a table was
   * replaced by one of a larger k since (ask again).  Returns after the probe
   * has completed on `stream`. */
  uint64_t ProbeBatchWorkspaceBytes(const vector<string_view> &oids, uint64_t n, uint32_t key_stride);
  RC ProbeBatchDevice(const vector<string_view> &oids, int filter, const uint8_t *d_keys, const uint64_t *d_offsets,
                      uint64_t n, uint32_t key_stride, const uint32_t *d_table, uint8_t *d_out,
                      vector<uint8_t> *cached, void *d_workspace, uint64_t workspace_bytes, void *stream = nullptr);
  /* The process-wide cache FilterBlockReader::Init(string_view) keeps its
   * bitmaps in, for blocks of every bits_per_key (arena
   * ADL_BLOOM_READER_CACHE_BYTES, default 1 GiB); created on first use and
   * kept until exit.  (Shared(int) is the round-5 spelling: the same cache.) */
  static FilterCache *Shared();
  static FilterCache *Shared(int bits_per_key);
  /* the C-ABI handle (NULL when creation failed), for calls that take a cache */
  adl_bloom_filter_cache *handle() const { return h_; }

 private:
  adl_bloom_filter_cache *h_ = nullptr;
  int bits_per_key_;
  RC status_;
};

/* src/filter_block.hpp:54-73.  The bitmaps live in a FilterCache arena (one
 * upload per block, no allocation per Init); the reader keeps the caller's
 * view of the block, as the reference's does, and re-uploads it if the cache
 * evicted it. */
class FilterBlockReader {
 public:
  FilterBlockReader();
  ~FilterBlockReader();
  FilterBlockReader(const FilterBlockReader &) = delete;
  FilterBlockReader &operator=(const FilterBlockReader &) = delete;
  /* src/filter_block.hpp:57: the bitmaps go into FilterCache::Shared()
   * under an id private to this reader (removed by the destructor) */
  RC Init(string_view filter_block);
  /* the same, with the table's entry in `cache` under `oid`: every reader of
   * one SSTable (and a level multi-get over it) shares one device copy */
  RC Init(string_view filter_block, FilterCache &cache, string_view oid);
  bool IsKeyExists(int filter_block_num, string_view key);
  /* batched: out[i] = IsKeyExists(filter_block_num, key i), one launch */
  RC IsKeysExist(int filter_block_num, const KeyArena &keys, vector<uint8_t> &out);
  int filters_nums() const { return filters_nums_; }

 private:
  RC Parse(string_view filter_block);
  RC CreateFilterAlgorithm();
  RC Upload();
  RC Probe(int filter_block_num, const KeyArena &keys, vector<uint8_t> &out);
  void Release();

  int filters_nums_;
  int filters_offsets_offset_;
  string_view filters_offsets_;
  string_view filter_info_;
  string_view filter_blocks_;
  unique_ptr<FilterAlgorithm> method_;
  int bits_per_key_ = 0;
  FilterCache *cache_ = nullptr;               /* where the bitmaps are resident */
  string oid_;                                 /* their key in cache_ */
  bool own_oid_ = false;                       /* a private id: removed with the reader */
  std::mutex upload_mu_;                       /* guards the move to device_set_ */
  std::atomic<adl_bloom_filter_set *> device_set_{nullptr}; /* a copy of its own: blocks larger than
                                                   the shared arena, or evicted again and again */
};

/* src/murmur3_hash.hpp:9 -- computed on the GPU (adl_bloom_murmur3). */
uint32_t murmur3_hash(uint32_t seed, const char *data, size_t len);

}  // namespace adl

// adlsm-tree_amd/csrc/filter_cache_impl.hpp -- the filter cache's bookkeeping,
// shared by filter_cache.hip (put / probe) and cache_build.hip (write-through
// builds): the arena's free list, the LRU list, the entries in limbo.  See
// filter_cache.hip for the concurrency rules.
#pragma once
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "probe_server.hpp"

namespace adl_cache {
constexpr uint64_t kAlign = 256;
}  // namespace adl_cache

struct adl_bloom_filter_cache {
  enum State : uint8_t { kLive, kLoading, kDead };
  struct Entry {
    std::string oid;
    uint64_t base = 0, size = 0;  // arena range [base, base + size)
    std::vector<uint64_t> off;    // block-relative filter offsets (F+1)
    uint8_t k = 1;                // probes per key: from the block's own bits_per_key
    uint32_t pins = 0;            // probes (or the uploading put, or a build's ticket) using the range
    State state = kLive;
    bool ticket = false;          // loading, held by an unpublished write-through build (cache_build.hip)
  };
  using Iter = std::list<Entry>::iterator;
  std::mutex mu;
  std::condition_variable freed;  // a dead or loading entry gave back its range
  uint8_t *arena = nullptr;       // [ones][blocks...]
  uint64_t capacity = 0, used = 0;
  uint32_t max_tables = 0;
  std::list<Entry> lru;      // live entries, front = most recently used
  std::list<Entry> limbo;    // loading (pinned by their put or ticket) and dead (pinned by probes)
  std::unordered_map<std::string, Iter> index;  // live entries only
  std::map<uint64_t, uint64_t> free_;           // offset -> size, coalesced
  // the resident probe server of this cache's small batches (created on the
  // first one; srv_tried: do not retry a failed creation)
  adl_srv::Server *srv = nullptr;
  bool srv_tried = false;
  // after a kBusy (the server's wave found no room on the GPU for
  // adl_srv::kTimeout), small batches go straight to a launch until this
  // steady-clock time (ns), instead of each waiting out the timeout again
  std::atomic<int64_t> srv_backoff_until{0};
  // published puts so far (the server invalidates its caches before it reads
  // bits of a range that may have been written since it last did)
  std::atomic<uint64_t> epoch{1};
  // pinned 16-byte slots the verify results of device-variant builds are
  // copied into (cache_build.hip; allocated by the first such build, freed
  // with the cache)
  uint64_t *verify_slots = nullptr;
  std::vector<uint32_t> verify_free;

  bool alloc(uint64_t size, uint64_t &at) {
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second < size) continue;
      at = it->first;
      const uint64_t rest = it->second - size;
      free_.erase(it);
      if (rest) free_[at + size] = rest;
      used += size;
      return true;
    }
    return false;
  }
  void release(uint64_t at, uint64_t size) {
    used -= size;
    auto it = free_.emplace(at, size).first;
    auto nx = std::next(it);
    if (nx != free_.end() && it->first + it->second == nx->first) {
      it->second += nx->second;
      free_.erase(nx);
    }
    if (it != free_.begin()) {
      auto pv = std::prev(it);
      if (pv->first + pv->second == it->first) {
        pv->second += it->second;
        free_.erase(it);
      }
    }
  }
  // Take a live entry out of the index: its range is freed now, or -- while
  // probes hold it -- by the last of them (unpin).
  void retire(Iter it) {
    index.erase(it->oid);
    if (it->pins == 0) {
      release(it->base, it->size);
      lru.erase(it);
      freed.notify_all();
    } else {
      it->state = kDead;
      limbo.splice(limbo.end(), lru, it);
    }
  }
  void unpin(Iter it) {
    if (--it->pins == 0 && it->state == kDead) {
      release(it->base, it->size);
      limbo.erase(it);
      freed.notify_all();
    }
  }
  // put's step 4 (and a build's publish): the loading entry `mine` becomes the
  // live, most recently used block of `key`, replacing one cached under it.
  void publish(Iter mine, const std::string &key) {
    if (auto it = index.find(key); it != index.end()) retire(it->second);  // the block this one replaces
    mine->oid = key;
    mine->pins = 0;
    mine->ticket = false;
    mine->state = kLive;
    lru.splice(lru.begin(), limbo, mine);
    index[key] = lru.begin();
    epoch.fetch_add(1, std::memory_order_release);  // (under the lock: before any probe can resolve it)
    while (lru.size() > max_tables) retire(std::prev(lru.end()));
    freed.notify_all();  // a put waiting for room may evict this entry now
  }
};

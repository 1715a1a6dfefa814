// adlsm-tree_amd/csrc/filter_cache.hip -- device-resident filter cache keyed by
// SSTable oid, for batched multi-get probes.
//
// The reference keeps open SSTableReaders in an LRU cache keyed by oid
// (DB::table_cache_, src/db.hpp:96-97; LRUCache, src/cache.hpp:23-93); each
// reader holds its filter block as a view into the mmapped file
// (SSTableReader::ReadFilterBlock, src/sstable.cpp:179-209) and Get probes
// filter 0 one key at a time (src/sstable.cpp:238).  Here the filter blocks of
// many tables live in ONE device arena (capacity fixed at creation, sized for
// HBM), so a whole multi-get batch -- keys bound for many tables -- is one
// launch of the range-based multi-filter probe.
//
//  * put(oid, block): parses the trailer as FilterBlockReader::Init does
//    (src/filter_block.cpp:113-155, same FILTER_BLOCK_ERROR cases plus bounds
//    checks), uploads the bitmap region once, and inserts it as most recently
//    used; least recently used blocks are evicted until it fits (arena bytes)
//    and the table count is within max_tables (the reference's maxSize).
//  * probe(oids, per-query table index, keys): every referenced table is
//    looked up (and marked used); a query bound for a table that is not
//    cached answers 1 ("may be present": the caller reads the table), one
//    bound for a filter the block does not have answers 0, as
//    FilterBlockReader::IsKeyExists does (src/filter_block.cpp:174).
//  * build / publish (cache_build.hip): a table's filter block built by the
//    build kernels straight into a reserved range -- no upload at all -- and
//    published under the oid once the file is written; the bookkeeping both
//    files share is filter_cache_impl.hpp.
//  * Concurrency: one mutex per cache guards the index, the LRU list and the
//    arena's free list, and is held only for that bookkeeping -- never across
//    a copy or a kernel.  A probe pins the entries it resolved (a count per
//    entry) before it lets go of the lock; an entry evicted, replaced or
//    removed while pinned leaves the index at once but keeps its arena range
//    until the last probe using it unpins it.  A put reserves its range under
//    the lock, uploads without it, and publishes under it again; a put that
//    finds no room while pinned or uploading blocks hold the arena waits for
//    them (condition variable) instead of failing.  So probes never wait for
//    each other, and readers, like the reference's (src/db.cpp:166-172), take
//    no lock for the duration of a lookup.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <stdint.h>
#include <string.h>

#include <condition_variable>
#include <list>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "bloom_common.hpp"
#include "filter_block_format.hpp"
#include "filter_cache_impl.hpp"
#include "level_index_impl.hpp"
#include "probe_server.hpp"

namespace {

using adl_cache::kAlign;
constexpr uint64_t kOnesBytes = 16;  // an all-ones 16-byte filter: every probe hits
constexpr int64_t kServerBackoffNs = 1000000000;  // launched probes for 1 s after a starved server request

// FilterBlockReader::Init's trailer walk (src/filter_block.cpp:113-155, in
// filter_block_format.hpp): bitmaps region [0, offsets_start), filter f =
// [off_f, off_{f+1} or offsets_start).  Each block carries its own
// bits_per_key in its "bf:" info, and the reference builds its BloomFilter
// from it per block (CreateFilterAlgorithm, src/filter_block.cpp:158-170),
// so a level may mix tables written under different DBOptions::bits_per_key
// (src/options.hpp:24): the block's k is kept with its entry.
int parse_block(const uint8_t *b, uint64_t len, std::vector<uint64_t> &off, uint8_t &k) {
  adl_fmt::FilterBlockLayout lay;
  if (adl_fmt::parse_filter_block(b, len, lay)) return ADL_FILTER_BLOCK_ERROR;
  off = std::move(lay.off);
  k = (uint8_t)adl_host::num_probes(lay.bits_per_key);
  return ADL_OK;
}

// The calling thread's completion event of a mapped small-batch probe (timing
// off: it is only queried).
struct DoneEvent {
  hipEvent_t e = nullptr;
  bool tried = false;
  ~DoneEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  hipEvent_t get() {
    if (!tried) {
      tried = true;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    }
    return e;
  }
};
thread_local DoneEvent t_done;

// What a probe resolved under the cache's lock: per listed table the arena
// range of its filter (be[j], be[num_tables + j]), whether it is cached, its
// block's k, and the entries it pinned.  (Per-thread scratch: a single-key
// Get allocates nothing here.)
struct Resolved {
  std::vector<uint64_t> be;
  std::vector<uint8_t> cached, kt;
  std::vector<adl_bloom_filter_cache::Iter> pinned;
  std::string oid_key;
};
thread_local Resolved t_res;

// Per listed table, the arena range of its filter `filter` (the all-ones
// filter when the table is not cached, an empty range when it has no such
// filter) and its block's k, its entry pinned and marked used.
void resolve_tables(adl_bloom_filter_cache *c, const char *const *oids, const uint64_t *oid_lens,
                    uint32_t num_tables, uint32_t filter, Resolved &r) {
  r.be.assign(2 * (size_t)num_tables, 0);
  r.cached.assign(num_tables, 0);
  r.kt.assign(num_tables, 1);
  r.pinned.reserve(num_tables);  // (no entry is counted and then not listed)
  std::lock_guard<std::mutex> g(c->mu);
  for (uint32_t j = 0; j < num_tables; ++j) {
    r.oid_key.assign(oids[j], oid_lens[j]);
    auto it = c->index.find(r.oid_key);
    if (it == c->index.end()) {
      r.be[j] = 0;
      r.be[num_tables + j] = kOnesBytes;
      continue;
    }
    r.cached[j] = 1;
    adl_bloom_filter_cache::Iter e = it->second;
    r.kt[j] = e->k;
    c->lru.splice(c->lru.begin(), c->lru, e);
    ++e->pins;
    r.pinned.push_back(e);
    const uint64_t nf = e->off.size() - 1;
    r.be[j] = r.be[num_tables + j] = e->base;
    if (filter < nf) {
      r.be[j] = e->base + e->off[filter];
      r.be[num_tables + j] = e->base + e->off[filter + 1];
    }
  }
}

// Owns the pins resolve_tables takes into `r` (the thread's scratch: nothing
// is allocated per call) and gives them back when it goes out of scope, on
// every path (a range retired meanwhile is freed by its last unpin).  The
// kernels and copies that read the pinned ranges must be complete by then, so
// the scope of one ends after its call's last synchronize or watch_answers.
class PinScope {
 public:
  PinScope(adl_bloom_filter_cache *c, Resolved &r) : c_(c), r_(r) { r_.pinned.clear(); }
  PinScope(const PinScope &) = delete;
  PinScope &operator=(const PinScope &) = delete;
  ~PinScope() {
    std::lock_guard<std::mutex> g(c_->mu);
    for (auto e : r_.pinned) c_->unpin(e);
    r_.pinned.clear();
  }

 private:
  adl_bloom_filter_cache *c_;
  Resolved &r_;
};

// resolve_tables on the tables of the given levels (null: an empty level), in
// order, as one oid list of num_tables entries.
void resolve_levels(adl_bloom_filter_cache *c, adl_bloom_level *const *levels, size_t num_levels, uint32_t num_tables,
                    uint32_t filter, Resolved &r) {
  std::vector<const char *> op;
  std::vector<uint64_t> ol;
  op.reserve(num_tables);
  ol.reserve(num_tables);
  for (size_t l = 0; l < num_levels; ++l) {
    if (!levels[l]) continue;
    for (const std::string &oid : levels[l]->oids) {
      op.push_back(oid.data());
      ol.push_back(oid.size());
    }
  }
  resolve_tables(c, op.data(), ol.data(), num_tables, filter, r);
}

// The resolved tables' range table (begin[], then end[]) and k table, as every
// cached probe stages them after its keys and ids.
struct TableBlock {
  uint64_t o_be, o_k;
  TableBlock(adl_host::StagePlan &p, const Resolved &r) : o_be(p.take(r.be.size() * 8)), o_k(p.take(r.kt.size())) {}
  void fill(uint8_t *hbuf, const Resolved &r) const {
    memcpy(hbuf + o_be, r.be.data(), r.be.size() * 8);
    if (!r.kt.empty()) memcpy(hbuf + o_k, r.kt.data(), r.kt.size());
  }
  const uint64_t *begin(const uint8_t *dbuf) const { return reinterpret_cast<const uint64_t *>(dbuf + o_be); }
  const uint8_t *k(const uint8_t *dbuf) const { return dbuf + o_k; }
};

// Waits for a mapped small batch by watching its n answers arrive (each is
// written once, 0 or 1, over a 0xFF sentinel, by the probe kernel's one store
// per query after all its reads), then for the launch's completion event.
// true: both seen (rc may have become ADL_ERR_DEVICE); false: 2 ms passed, the
// caller synchronizes the stream.
bool watch_answers(const volatile uint8_t *ans, uint64_t n, hipEvent_t done, int &rc) {
  const auto t0 = std::chrono::steady_clock::now();
  auto late = [&] { return std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2); };
  uint64_t i = 0;
  for (;;) {
    while (i < n && ans[i] != 0xff) ++i;
    if (i == n || late()) break;
    __builtin_ia32_pause();
  }
  if (i != n) return false;
  // every answer is in: now the launch itself
  const bool fault = adl_host::g_test_faults.take(ADL_TEST_FAULT_CACHE_COMPLETION) >= 0;
  for (;;) {
    const hipError_t q = fault ? hipErrorLaunchFailure : hipEventQuery(done);
    if (q == hipSuccess) return true;
    if (q != hipErrorNotReady) {
      rc = ADL_ERR_DEVICE;
      return false;
    }
    if (late()) return false;
    __builtin_ia32_pause();
  }
}

// A single-key Get asks the cache's resident server: no launch.  Its answers
// arrive, in h_out, after all its reads of the pinned ranges.  ask(server,
// arena epoch) posts the request (adl_srv::probe or adl_srv::probe_fan).
// adl_srv::kBusy: not served -- the request is not eligible, the server is
// switched off, missing or backing off, or no answer came in adl_srv::kTimeout
// (a healthy GPU with no room for the server's wave) -- and the caller probes
// by a launch, the ranges still pinned.
template <class Ask>
int ask_server(adl_bloom_filter_cache *c, bool eligible, Ask &&ask) {
  if (!eligible || !adl_host::knobs().probe_server) return adl_srv::kBusy;
  const int64_t now_ns =
      std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  if (now_ns < c->srv_backoff_until.load(std::memory_order_relaxed)) return adl_srv::kBusy;
  adl_srv::Server *srv = nullptr;
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->srv_tried) {
      c->srv_tried = true;
      c->srv = adl_srv::create();
    }
    srv = c->srv;
  }
  if (!srv) return adl_srv::kBusy;
  int rc = ask(srv, c->epoch.load(std::memory_order_acquire));
  if (rc == ADL_OK && adl_host::g_test_faults.take(ADL_TEST_FAULT_CACHE_COMPLETION) >= 0) rc = ADL_ERR_DEVICE;
  if (rc == adl_srv::kBusy) c->srv_backoff_until.store(now_ns + kServerBackoffNs, std::memory_order_relaxed);
  return rc;
}

// Up to adl_srv::kMaxQ queries, each with its own key, in one server request.
int serve_resident(adl_bloom_filter_cache *c, const Resolved &res, uint32_t num_tables, const uint8_t *h_keys,
                   const uint64_t *h_offsets, uint64_t n, uint32_t key_stride, const uint32_t *h_table,
                   uint8_t *h_out) {
  const uint64_t kbytes = h_offsets ? h_offsets[n] - h_offsets[0] : n * (uint64_t)key_stride;
  return ask_server(c, adl_srv::eligible(n, kbytes), [&](adl_srv::Server *srv, uint64_t epoch) {
    uint64_t rng[2 * adl_srv::kMaxQ];
    uint8_t kq[adl_srv::kMaxQ];
    const uint64_t a0 = reinterpret_cast<uint64_t>(c->arena);
    for (uint64_t i = 0; i < n; ++i) {
      rng[2 * i] = a0 + res.be[h_table[i]];
      rng[2 * i + 1] = a0 + res.be[num_tables + h_table[i]];
      kq[i] = res.kt[h_table[i]];
    }
    return adl_srv::probe(srv, h_keys, h_offsets, key_stride, n, rng, kq, epoch, h_out);
  });
}

// ONE key against every resolved table (0 .. num_tables-1), in one server
// request of the fan form: up to adl_srv::kFanTables tables, a key of up to
// adl_srv::kFanKeyBytes bytes.
int serve_resident_key(adl_bloom_filter_cache *c, const Resolved &res, uint32_t num_tables, const uint8_t *h_key,
                       uint64_t key_len, uint8_t *h_out) {
  return ask_server(c, adl_srv::eligible_fan(num_tables, key_len), [&](adl_srv::Server *srv, uint64_t epoch) {
    uint64_t rng[2 * adl_srv::kFanTables];
    const uint64_t a0 = reinterpret_cast<uint64_t>(c->arena);
    for (uint32_t t = 0; t < num_tables; ++t) {
      rng[2 * t] = a0 + res.be[t];
      rng[2 * t + 1] = a0 + res.be[num_tables + t];
    }
    return adl_srv::probe_fan(srv, h_key, key_len, num_tables, rng, res.kt.data(), epoch, h_out);
  });
}

// The body of a batch that answers a byte per query: the plan's sections up
// to o_out are the upload, the n answers follow at o_out.  A small batch (a
// single-key Get) is handed over in the thread's mapped buffer: the kernel
// reads it and writes its answers there directly; a larger one is staged, sent
// in one H2D and its answers fetched in one D2H.  fill(hbuf) places the
// upload, launch(dbuf, done) enqueues the probe on `st`.
//
// A mapped small batch is waited for by watching its answers arrive (each is
// written once, 0 or 1, over a 0xFF sentinel, by the probe kernel's one store
// per query after all its reads) instead of a stream synchronize.  Its
// completion event rides on the probe's dispatch packet, and the call returns
// only once that has fired too, so a fault after the answers landed is still
// this call's error.  Both waits fall back to the synchronize after 2 ms (or
// with ADL_BLOOM_SPIN=0).  On return the kernel and the copies are done; the
// answers are in h_out when the status is ADL_OK.
template <class Fill, class Launch>
int run_answer_batch(const adl_host::StagePlan &plan, uint64_t o_out, uint64_t n, hipStream_t st, Fill &&fill,
                     Launch &&launch, uint8_t *h_out) {
  adl_host::Staging &sg = adl_host::t_stage;
  uint8_t *hbuf = adl_host::t_mapped.get(plan.end), *dbuf = adl_host::t_mapped.dev;
  const bool mapped = hbuf != nullptr;
  int rc = ADL_OK;
  if (!mapped) {
    rc = sg.reserve(plan.end, plan.end);
    hbuf = sg.host;
    dbuf = sg.dev;
  }
  const bool spin = mapped && n <= 4096 && adl_host::knobs().spin;
  if (rc == ADL_OK) {
    fill(hbuf);
    if (spin) memset(hbuf + o_out, 0xff, n);
    if (!mapped && hipMemcpyAsync(dbuf, hbuf, o_out, hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
  }
  hipEvent_t done = spin && rc == ADL_OK ? t_done.get() : nullptr;
  if (rc == ADL_OK) rc = launch(dbuf, done);
  if (rc == ADL_OK && !mapped && hipMemcpyAsync(hbuf + o_out, dbuf + o_out, n, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = ADL_ERR_DEVICE;
  const bool finished = done && watch_answers(hbuf + o_out, n, done, rc);
  if (!finished && hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
  if (rc == ADL_OK) memcpy(h_out, hbuf + o_out, n);
  return rc;
}

// The results of a multi-get, fetched from the thread's staging pair: the
// area [o_counts, o_end) starts with the counts and what has a fixed size;
// from o_payload on it holds lists whose lengths the counts give.  A small
// area comes back in one copy; a larger one first learns the counts.
// counted(piece) reads the counts from sg.host and names the list pieces they
// call for, piece(at, bytes); it runs once the counts are in, whichever way
// the area came.  rc: the status so far (the stream is synchronized whatever
// it is).  On return the kernels and the copies are done.
template <class Counted>
int fetch_count_first(adl_host::Staging &sg, uint64_t o_counts, uint64_t o_payload, uint64_t o_end, hipStream_t st,
                      int rc, Counted &&counted) {
  const bool one_copy = o_end - o_counts <= (256u << 10);
  if (rc == ADL_OK && hipMemcpyAsync(sg.host + o_counts, sg.dev + o_counts, (one_copy ? o_end : o_payload) - o_counts,
                                     hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = ADL_ERR_DEVICE;
  if (hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
  if (rc != ADL_OK) return rc;
  bool second = false;
  counted([&](uint64_t at, uint64_t bytes) {
    if (one_copy || !bytes) return;
    second = true;
    if (rc == ADL_OK && hipMemcpyAsync(sg.host + at, sg.dev + at, bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = ADL_ERR_DEVICE;
  });
  if (second && hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
  return rc;
}

// The launched fan-out probe of resolved tables: keys (once each), their
// offsets, the begin array, the table ids and the range and k tables up, one
// fan-out launch, a byte per pair down.
int launch_fanout(adl_bloom_filter_cache *c, const Resolved &res, uint32_t num_tables, const uint8_t *h_keys,
                  const uint64_t *h_offsets, uint64_t num_keys, uint32_t key_stride, const uint32_t *h_pair_begin,
                  const uint32_t *h_pair_table, uint64_t np, uint8_t *h_out, hipStream_t st) {
  adl_host::StagePlan plan;
  const adl_host::KeyBlock kb(plan, h_offsets, num_keys, key_stride);
  const uint64_t o_pb = plan.take((num_keys + 1) * 4);
  const uint64_t o_pt = plan.take(np * 4);
  const TableBlock tb(plan, res);
  const uint64_t o_out = plan.take(np);
  return run_answer_batch(
      plan, o_out, np, st,
      [&](uint8_t *hbuf) {
        kb.fill(hbuf, h_keys, h_offsets);
        memcpy(hbuf + o_pb, h_pair_begin, (num_keys + 1) * 4);
        memcpy(hbuf + o_pt, h_pair_table, np * 4);
        tb.fill(hbuf, res);
      },
      [&](uint8_t *dbuf, hipEvent_t done) {
        return adl_host::adl_probe_fanout_device_ev(
            dbuf, kb.offsets(dbuf), num_keys, key_stride, reinterpret_cast<const uint32_t *>(dbuf + o_pb),
            reinterpret_cast<const uint32_t *>(dbuf + o_pt), np, num_tables, c->arena, tb.begin(dbuf),
            tb.begin(dbuf) + num_tables, tb.k(dbuf), dbuf + o_out, st, done);
      },
      h_out);
}

// 0, 1, 2, ...: the candidate list of a one-key fan-out over every listed
// table (per-thread, grown once).
thread_local std::vector<uint32_t> t_iota;

// One key against every resolved table (0 .. num_tables-1, >= 1), h_out[t] its
// answer: one request of the fan form to the resident server, or -- more
// tables or a longer key than that takes, or the server not serving -- the
// launched fan-out probe of one key with all the tables as its list.
int probe_key_resolved(adl_bloom_filter_cache *c, const Resolved &res, uint32_t num_tables, const uint8_t *h_key,
                       uint64_t key_len, uint8_t *h_out, hipStream_t st) {
  int rc = serve_resident_key(c, res, num_tables, h_key, key_len, h_out);
  if (rc != adl_srv::kBusy) return rc;
  while (t_iota.size() < num_tables) t_iota.push_back((uint32_t)t_iota.size());
  static const uint8_t no_bytes[1] = {0};  // (an empty key still has an address)
  const uint64_t off[2] = {0, key_len};
  const uint32_t pb[2] = {0, num_tables};
  return launch_fanout(c, res, num_tables, h_key ? h_key : no_bytes, off, 1, 0, pb, t_iota.data(), num_tables, h_out,
                       st);
}

}  // namespace

extern "C" {

int adl_bloom_filter_cache_create(uint64_t capacity_bytes, uint32_t max_tables, int32_t bits_per_key,
                                  adl_bloom_filter_cache **out) {
  if (!out || bits_per_key < 0 || max_tables == 0 || capacity_bytes == 0) return ADL_ERR_INVALID_ARG;
  *out = nullptr;
  try {
    auto *c = new adl_bloom_filter_cache;
    c->capacity = adl_host::round_up(capacity_bytes, kAlign);
    c->max_tables = max_tables;
    if (hipMalloc((void **)&c->arena, c->capacity + kAlign) != hipSuccess) {
      (void)hipGetLastError();
      delete c;
      return ADL_ERR_OUT_OF_MEMORY;
    }
    hipStream_t st = adl_host::sync_stream(nullptr);
    if (hipMemsetAsync(c->arena, 0xff, kOnesBytes, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipFree(c->arena);
      delete c;
      return ADL_ERR_DEVICE;
    }
    c->free_[kAlign] = c->capacity;  // blocks after the all-ones filter
    *out = c;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// No call on the cache may be running or start once this is called.
int adl_bloom_filter_cache_destroy(adl_bloom_filter_cache *c) {
  if (!c) return ADL_OK;
  adl_srv::destroy(c->srv);  // stops its kernel before the arena goes
  if (c->verify_slots) (void)hipHostFree(c->verify_slots);
  (void)hipFree(c->arena);
  delete c;
  return ADL_OK;
}

int adl_bloom_filter_cache_put(adl_bloom_filter_cache *c, const char *oid, uint64_t oid_len,
                               const uint8_t *h_block, uint64_t block_len) {
  if (!c || !oid || !h_block) return ADL_ERR_INVALID_ARG;
  try {
    std::vector<uint64_t> off;
    uint8_t k = 1;
    if (int rc = parse_block(h_block, block_len, off, k)) return rc;
    const uint64_t bytes = off.back();  // the bitmap region
    const uint64_t size = adl_host::round_up(bytes + 1, kAlign);
    const std::string key(oid, oid_len);
    adl_bloom_filter_cache::Iter mine;
    {
      std::unique_lock<std::mutex> g(c->mu);
      if (size > c->capacity) return ADL_ERR_OUT_OF_MEMORY;
      // 1. room: the table count (LRUCache's maxSize) and the arena bytes.  A
      //    block being replaced (LRUCache::Put of a cached key) stays visible to
      //    probes until the new one is published.
      const size_t replacing = c->index.count(key);
      while (c->lru.size() - replacing >= c->max_tables) c->retire(std::prev(c->lru.end()));
      uint64_t at = 0;
      while (!c->alloc(size, at)) {
        if (!c->lru.empty()) {
          c->retire(std::prev(c->lru.end()));
        } else if (!c->limbo.empty()) {
          c->freed.wait(g);  // pinned or uploading blocks hold the rest of the arena
        } else {
          return ADL_ERR_OUT_OF_MEMORY;  // cannot happen: an empty arena fits any size <= capacity
        }
      }
      // 2. reserve the range, pinned by this put while it uploads
      adl_bloom_filter_cache::Entry e;
      e.oid = key;
      e.base = at;
      e.size = size;
      e.off = std::move(off);
      e.k = k;
      e.pins = 1;
      e.state = adl_bloom_filter_cache::kLoading;
      mine = c->limbo.insert(c->limbo.end(), std::move(e));
    }
    // 3. upload without the lock
    hipStream_t st = adl_host::sync_stream(nullptr);
    const bool ok = !bytes || (hipMemcpyAsync(c->arena + mine->base, h_block, bytes, hipMemcpyHostToDevice, st) ==
                                   hipSuccess &&
                               hipStreamSynchronize(st) == hipSuccess);
    // 4. publish as most recently used (or give the range back)
    std::lock_guard<std::mutex> g(c->mu);
    if (!ok) {
      mine->state = adl_bloom_filter_cache::kDead;
      c->unpin(mine);
      return ADL_ERR_DEVICE;
    }
    c->publish(mine, key);
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_contains(adl_bloom_filter_cache *c, const char *oid, uint64_t oid_len) {
  if (!c || !oid) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->index.find(std::string(oid, oid_len));
  if (it == c->index.end()) return 0;
  c->lru.splice(c->lru.begin(), c->lru, it->second);  // LRUCache::Get marks it used
  return 1;
}

int adl_bloom_filter_cache_remove(adl_bloom_filter_cache *c, const char *oid, uint64_t oid_len) {
  if (!c || !oid) return 0;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->index.find(std::string(oid, oid_len));
  if (it == c->index.end()) return 0;
  c->retire(it->second);
  return 1;
}

int adl_bloom_filter_cache_stats(adl_bloom_filter_cache *c, uint32_t *tables, uint64_t *bytes_used) {
  if (!c) return ADL_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (tables) *tables = (uint32_t)c->lru.size();
  if (bytes_used) *bytes_used = c->used;
  return ADL_OK;
}

int adl_bloom_filter_cache_probe(adl_bloom_filter_cache *c, const char *const *oids, const uint64_t *oid_lens,
                                 uint32_t num_tables, uint32_t filter, const uint8_t *h_keys,
                                 const uint64_t *h_offsets, uint64_t n, uint32_t key_stride,
                                 const uint32_t *h_table, uint8_t *h_out, uint64_t *h_uncached, void *stream) {
  if (!c || (num_tables && (!oids || !oid_lens))) return ADL_ERR_INVALID_ARG;
  if (h_uncached) *h_uncached = 0;
  if (n == 0) return ADL_OK;
  if (!h_keys || !h_table || !h_out || (!h_offsets && key_stride == 0)) return ADL_ERR_INVALID_ARG;
  try {
    for (uint64_t i = 0; i < n; ++i)
      if (h_table[i] >= num_tables) return ADL_ERR_INVALID_ARG;
    hipStream_t st = adl_host::sync_stream(stream);
    // 1. under the lock: the listed tables' ranges and k, pinned and marked
    //    used, until this call is done with them
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_tables(c, oids, oid_lens, num_tables, filter, res);
    uint64_t uncached = 0;
    for (uint64_t i = 0; i < n; ++i) uncached += !res.cached[h_table[i]];
    // 2. a single-key Get: the resident server (its answer is in h_out when
    //    this call returns, the pins given back on the way out)
    int rc = serve_resident(c, res, num_tables, h_keys, h_offsets, n, key_stride, h_table, h_out);
    if (rc == adl_srv::kBusy) {
      // 3. without the lock: keys, offsets, table ids and the range and k
      //    tables up, one probe launch, a byte per query down
      adl_host::StagePlan plan;
      const adl_host::KeyBlock kb(plan, h_offsets, n, key_stride);
      const uint64_t o_fid = plan.take(n * 4);
      const TableBlock tb(plan, res);
      const uint64_t o_out = plan.take(n);
      rc = run_answer_batch(
          plan, o_out, n, st,
          [&](uint8_t *hbuf) {
            kb.fill(hbuf, h_keys, h_offsets);
            memcpy(hbuf + o_fid, h_table, n * 4);
            tb.fill(hbuf, res);
          },
          [&](uint8_t *dbuf, hipEvent_t done) {
            return adl_host::adl_probe_ranges_device_ev(
                dbuf, kb.offsets(dbuf), n, key_stride, reinterpret_cast<const uint32_t *>(dbuf + o_fid), num_tables,
                c->arena, tb.begin(dbuf), tb.begin(dbuf) + num_tables, tb.k(dbuf), dbuf + o_out, st, done);
          },
          h_out);
    }
    if (rc) return rc;
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

uint64_t adl_bloom_filter_cache_probe_batch_workspace_bytes(adl_bloom_filter_cache *c, const char *const *oids,
                                                            const uint64_t *oid_lens, uint32_t num_tables, uint64_t n,
                                                            uint32_t key_stride) {
  if (!c || (num_tables && (!oids || !oid_lens))) return 0;
  try {
    uint32_t max_k = 1;  // (an uncached table is the all-ones filter with k = 1)
    {
      std::lock_guard<std::mutex> g(c->mu);
      std::string key;
      for (uint32_t j = 0; j < num_tables; ++j) {
        key.assign(oids[j], oid_lens[j]);
        auto it = c->index.find(key);
        if (it != c->index.end()) max_k = std::max<uint32_t>(max_k, it->second->k);
      }
    }
    return adl_bloom_probe_batch_k_workspace_bytes(n, num_tables, max_k, key_stride);
  } catch (...) {
    return 0;
  }
}

// The bulk probe of device keys: the listed tables resolved and pinned as by
// every cached probe, their range and k tables staged and uploaded, and
// adl_bloom_probe_batch_k_device over the arena with max_k the largest k
// resolved.  The stream is idle when the pins are given back, on every path.
int adl_bloom_filter_cache_probe_batch_device(adl_bloom_filter_cache *c, const char *const *oids,
                                              const uint64_t *oid_lens, uint32_t num_tables, uint32_t filter,
                                              const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                              uint32_t key_stride, const uint32_t *d_table, uint8_t *d_out,
                                              uint8_t *h_cached, void *d_workspace, uint64_t workspace_bytes,
                                              void *stream) {
  if (!c || (num_tables && (!oids || !oid_lens))) return ADL_ERR_INVALID_ARG;
  if (n && (!d_keys || !d_table || !d_out || (!d_offsets && key_stride == 0))) return ADL_ERR_INVALID_ARG;
  try {
    hipStream_t st = (hipStream_t)stream;  // (the caller's keys are ordered on it)
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_tables(c, oids, oid_lens, num_tables, filter, res);
    if (h_cached && num_tables) memcpy(h_cached, res.cached.data(), num_tables);
    if (n == 0) return ADL_OK;
    uint32_t max_k = 1;
    for (uint8_t k : res.kt) max_k = std::max<uint32_t>(max_k, k);
    adl_host::StagePlan plan;
    const TableBlock tb(plan, res);
    adl_host::Staging &sg = adl_host::t_stage;
    plan.take(1);  // (a list of no tables still has an address)
    if (int rc = sg.reserve(plan.end, plan.end)) return rc;
    tb.fill(sg.host, res);
    if (hipMemcpyAsync(sg.dev, sg.host, plan.end, hipMemcpyHostToDevice, st) != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return ADL_ERR_DEVICE;
    }
    // (a short workspace is refused before the pipeline's first launch: d_out is not written)
    const int rc = adl_bloom_probe_batch_k_device(d_keys, d_offsets, n, key_stride, d_table, num_tables, c->arena,
                                                  tb.begin(sg.dev), tb.begin(sg.dev) + num_tables, tb.k(sg.dev),
                                                  max_k, d_out, d_workspace, workspace_bytes, st);
    if (hipStreamSynchronize(st) != hipSuccess) return ADL_ERR_DEVICE;
    return rc;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_probe_fanout(adl_bloom_filter_cache *c, const char *const *oids, const uint64_t *oid_lens,
                                        uint32_t num_tables, uint32_t filter, const uint8_t *h_keys,
                                        const uint64_t *h_offsets, uint64_t num_keys, uint32_t key_stride,
                                        const uint32_t *h_pair_begin, const uint32_t *h_pair_table, uint8_t *h_out,
                                        uint64_t *h_uncached, void *stream) {
  if (!c || (num_tables && (!oids || !oid_lens))) return ADL_ERR_INVALID_ARG;
  if (h_uncached) *h_uncached = 0;
  if (num_keys == 0) return ADL_OK;
  if (!h_keys || !h_pair_begin || (!h_offsets && key_stride == 0)) return ADL_ERR_INVALID_ARG;
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;
  try {
    if (h_pair_begin[0] != 0) return ADL_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < num_keys; ++i)
      if (h_pair_begin[i + 1] < h_pair_begin[i]) return ADL_ERR_INVALID_ARG;
    const uint64_t np = h_pair_begin[num_keys];
    if (np == 0) return ADL_OK;
    if (!h_pair_table || !h_out) return ADL_ERR_INVALID_ARG;
    for (uint64_t p = 0; p < np; ++p)
      if (h_pair_table[p] >= num_tables) return ADL_ERR_INVALID_ARG;
    // A Get's worth of pairs: expanded, so that adl_bloom_filter_cache_probe
    // (the resident server) serves it as before.
    if (np <= adl_srv::kMaxQ) {
      std::string kbytes;
      uint64_t koff[adl_srv::kMaxQ + 1] = {0};
      uint64_t p = 0;
      for (uint64_t i = 0; i < num_keys && p < np; ++i) {
        const uint64_t o0 = h_offsets ? h_offsets[i] : i * key_stride;
        const uint64_t len = h_offsets ? h_offsets[i + 1] - o0 : key_stride;
        for (; p < h_pair_begin[i + 1]; ++p) {
          kbytes.append(reinterpret_cast<const char *>(h_keys) + o0, len);
          koff[p + 1] = kbytes.size();
        }
      }
      kbytes.push_back('\0');  // (a batch of empty keys still has an address)
      return adl_bloom_filter_cache_probe(c, oids, oid_lens, num_tables, filter,
                                          reinterpret_cast<const uint8_t *>(kbytes.data()), koff, np, 0, h_pair_table,
                                          h_out, h_uncached, stream);
    }
    hipStream_t st = adl_host::sync_stream(stream);
    // 1. under the lock: the listed tables' ranges and k, pinned and marked used
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_tables(c, oids, oid_lens, num_tables, filter, res);
    uint64_t uncached = 0;
    for (uint64_t p = 0; p < np; ++p) uncached += !res.cached[h_pair_table[p]];
    // 2. without the lock: one fan-out launch
    const int rc = launch_fanout(c, res, num_tables, h_keys, h_offsets, num_keys, key_stride, h_pair_begin,
                                 h_pair_table, np, h_out, st);
    if (rc) return rc;
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_probe_key(adl_bloom_filter_cache *c, const char *const *oids, const uint64_t *oid_lens,
                                     uint32_t num_tables, uint32_t filter, const uint8_t *h_key, uint64_t key_len,
                                     uint8_t *h_out, uint64_t *h_uncached, void *stream) {
  if (!c || (num_tables && (!oids || !oid_lens))) return ADL_ERR_INVALID_ARG;
  if (h_uncached) *h_uncached = 0;
  if (num_tables == 0) return ADL_OK;
  if (!h_out || (key_len && !h_key)) return ADL_ERR_INVALID_ARG;
  try {
    hipStream_t st = adl_host::sync_stream(stream);
    // under the lock: the listed tables' ranges and k, pinned and marked used,
    // until this call is done with them
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_tables(c, oids, oid_lens, num_tables, filter, res);
    if (int rc = probe_key_resolved(c, res, num_tables, h_key, key_len, h_out, st)) return rc;
    uint64_t uncached = 0;
    for (uint32_t t = 0; t < num_tables; ++t) uncached += !res.cached[t];
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// The level multi-get over a resident index (level_index.hip): keys and
// offsets up, selection + expansion + fan-out probe on the device, the begin
// entries, table indices and answers down.  The level's tables are resolved
// and pinned exactly as adl_bloom_filter_cache_probe_fanout resolves its oid
// list, so the answers are that call's on the same lists.
int adl_bloom_level_multiget(adl_bloom_level *lv, adl_bloom_filter_cache *c, uint32_t filter, const uint8_t *h_keys,
                             const uint64_t *h_offsets, uint64_t num_keys, uint32_t key_stride, int64_t seq,
                             uint32_t *h_pair_begin, uint32_t *h_pair_table, uint8_t *h_out, uint64_t pair_capacity,
                             uint64_t *num_pairs, uint64_t *h_uncached, void *stream) {
  if (!lv || !c || !num_pairs || !h_pair_begin) return ADL_ERR_INVALID_ARG;
  *num_pairs = 0;
  if (h_uncached) *h_uncached = 0;
  h_pair_begin[0] = 0;
  if (num_keys == 0) return ADL_OK;
  const uint32_t num_tables = lv->ix.num_tables;
  if (!h_keys || (!h_offsets && key_stride == 0) || (pair_capacity && (!h_pair_table || !h_out)))
    return ADL_ERR_INVALID_ARG;
  if (num_tables && lv->oids.size() != num_tables) return ADL_ERR_INVALID_ARG;  // created without oids
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;
  try {
    hipStream_t st = adl_host::sync_stream(stream);
    const uint64_t cap = std::min<uint64_t>(pair_capacity, 0xffffffffull);
    // 1. under the lock: the level's tables' ranges and k, pinned and marked used
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_levels(c, &lv, 1, num_tables, filter, res);
    // 2. without the lock: keys, offsets and the range and k tables in one H2D;
    //    selection (three launches) and the fan-out probe; then the results:
    //    num_pairs, the begin array | the table ids and answers | scratch
    const uint64_t wsb = adl_bloom_level_candidates_workspace_bytes(num_keys);
    adl_host::StagePlan plan;
    const adl_host::KeyBlock kb(plan, h_offsets, num_keys, key_stride);
    const TableBlock tb(plan, res);
    const uint64_t o_np = plan.take(8);  // the end of the upload
    const uint64_t o_pb = plan.take((num_keys + 1) * 4);
    const uint64_t o_pt = plan.take(cap * 4);
    const uint64_t o_out = plan.take(cap);
    const uint64_t o_ws = plan.take(wsb);  // the end of what the host buffer holds
    adl_host::Staging &sg = adl_host::t_stage;
    int rc = sg.reserve(o_ws, plan.end);
    uint8_t *hbuf = sg.host, *dbuf = sg.dev;
    if (rc == ADL_OK) {
      kb.fill(hbuf, h_keys, h_offsets);
      tb.fill(hbuf, res);
      if (hipMemcpyAsync(dbuf, hbuf, o_np, hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    }
    uint32_t *d_pb = reinterpret_cast<uint32_t *>(dbuf + o_pb), *d_pt = reinterpret_cast<uint32_t *>(dbuf + o_pt);
    if (rc == ADL_OK)
      rc = adl_host::level_select_device(lv, dbuf, kb.offsets(dbuf), num_keys, key_stride, seq, d_pb, d_pt, cap,
                                         reinterpret_cast<uint64_t *>(dbuf + o_np), dbuf + o_ws, wsb, st);
    if (rc == ADL_OK && cap)  // (the kernel stops at cap pairs whatever pair_begin says)
      rc = adl_host::adl_probe_fanout_device_ev(dbuf, kb.offsets(dbuf), num_keys, key_stride, d_pb, d_pt, cap,
                                                num_tables, c->arena, tb.begin(dbuf), tb.begin(dbuf) + num_tables,
                                                tb.k(dbuf), dbuf + o_out, st, nullptr);
    uint64_t np = 0;
    rc = fetch_count_first(sg, o_np, o_pt, o_ws, st, rc, [&](auto piece) {
      memcpy(&np, hbuf + o_np, 8);
      const uint64_t have = std::min(np, cap);
      piece(o_pt, have * 4);
      piece(o_out, have);
    });
    // 3. the kernels and the copies are done: report (the uncached pairs are
    //    counted where the ids arrived, before anything is copied out: a large
    //    copy leaves neither side in the CPU's caches)
    if (rc) return rc;
    uint64_t uncached = 0;
    const uint32_t *pt = reinterpret_cast<const uint32_t *>(hbuf + o_pt);
    if (np <= cap)
      for (uint64_t p = 0; p < np; ++p) uncached += !res.cached[pt[p]];
    *num_pairs = np;
    if (np > 0xffffffffull) return ADL_ERR_TOO_LARGE;
    memcpy(h_pair_begin, hbuf + o_pb, (num_keys + 1) * 4);
    if (np > pair_capacity) return ADL_ERR_WORKSPACE;
    if (np) {
      memcpy(h_pair_table, pt, np * 4);
      memcpy(h_out, hbuf + o_out, np);
    }
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// The revision multi-get (revision_index.hip): keys and offsets up; selection
// over every level, expansion, the fan-out probe and the compaction of the
// hits on the device; the hit lists down.  The tables of all levels are
// resolved and pinned in ONE pass over the concatenated oid list (global id =
// table_base[level] + table), so the answers are adl_bloom_level_multiget's,
// level by level.  The candidate pairs stay in device scratch.
int adl_bloom_revision_multiget(adl_bloom_revision *rev, adl_bloom_filter_cache *c, uint32_t filter,
                                const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                                uint32_t key_stride, int64_t seq, uint32_t *h_hit_begin, uint32_t *h_hit_table,
                                uint64_t hit_capacity, uint64_t *num_hits, uint64_t pair_capacity,
                                uint64_t *num_pairs, uint64_t *h_uncached, void *stream) {
  if (!rev || !c || !num_hits || !num_pairs || !h_hit_begin) return ADL_ERR_INVALID_ARG;
  *num_hits = *num_pairs = 0;
  if (h_uncached) *h_uncached = 0;
  if (num_keys == 0) {
    h_hit_begin[0] = 0;
    return ADL_OK;
  }
  if (!h_keys || (!h_offsets && key_stride == 0) || (hit_capacity && !h_hit_table)) return ADL_ERR_INVALID_ARG;
  const uint32_t num_tables = rev->table_base.back();
  for (adl_bloom_level *lv : rev->levels)
    if (lv && lv->ix.num_tables && lv->oids.size() != lv->ix.num_tables) return ADL_ERR_INVALID_ARG;  // no oids
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;
  try {
    hipStream_t st = adl_host::sync_stream(stream);
    const uint64_t worst = std::min<uint64_t>(num_keys * (uint64_t)rev->longest, 0xffffffffull);
    const uint64_t cap = pair_capacity ? std::min<uint64_t>(pair_capacity, 0xffffffffull) : worst;
    const uint64_t hcap = std::min(hit_capacity, cap);  // (no more hits than pairs)
    // 1. under the lock: every level's tables' ranges and k, pinned and marked used
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_levels(c, rev->levels.data(), rev->levels.size(), num_tables, filter, res);
    // 2. without the lock: keys, offsets and the range and k tables in one H2D;
    //    selection (three launches), probe + hit count, scan, compaction; then
    //    the results: num_pairs and num_hits, the hit begin array | the hits |
    //    the candidate pairs and scratch, on the device only
    const uint64_t wsc = adl_bloom_revision_candidates_workspace_bytes(rev, num_keys);
    const uint64_t wsh = adl_bloom_probe_fanout_hits_workspace_bytes(num_keys, cap);
    adl_host::StagePlan plan;
    const adl_host::KeyBlock kb(plan, h_offsets, num_keys, key_stride);
    const TableBlock tb(plan, res);
    const uint64_t o_np = plan.take(16);  // the end of the upload: num_pairs, num_hits
    const uint64_t o_hb = plan.take((num_keys + 1) * 4);
    const uint64_t o_ht = plan.take(hcap * 4);
    const uint64_t o_pb = plan.take((num_keys + 1) * 4);  // the end of what comes back
    const uint64_t o_pt = plan.take(cap * 4);
    const uint64_t o_wsc = plan.take(wsc);
    const uint64_t o_wsh = plan.take(wsh);
    adl_host::Staging &sg = adl_host::t_stage;
    int rc = sg.reserve(o_pb, plan.end);
    uint8_t *hbuf = sg.host, *dbuf = sg.dev;
    if (rc == ADL_OK) {
      kb.fill(hbuf, h_keys, h_offsets);
      tb.fill(hbuf, res);
      if (hipMemcpyAsync(dbuf, hbuf, o_np, hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    }
    uint32_t *d_pb = reinterpret_cast<uint32_t *>(dbuf + o_pb), *d_pt = reinterpret_cast<uint32_t *>(dbuf + o_pt);
    if (rc == ADL_OK)
      rc = adl_host::revision_select_device(rev, dbuf, kb.offsets(dbuf), num_keys, key_stride, seq, d_pb, d_pt, cap,
                                            reinterpret_cast<uint64_t *>(dbuf + o_np), dbuf + o_wsc, wsc, st);
    if (rc == ADL_OK)  // (the kernels stop at cap pairs whatever pair_begin says)
      rc = adl_host::probe_fanout_hits_device(dbuf, kb.offsets(dbuf), num_keys, key_stride, d_pb, d_pt, cap,
                                              num_tables, c->arena, tb.begin(dbuf), tb.begin(dbuf) + num_tables, 10,
                                              tb.k(dbuf), reinterpret_cast<uint32_t *>(dbuf + o_hb),
                                              reinterpret_cast<uint32_t *>(dbuf + o_ht), hcap,
                                              reinterpret_cast<uint64_t *>(dbuf + o_np + 8), dbuf + o_wsh, wsh, st);
    uint64_t np = 0, nh = 0;
    rc = fetch_count_first(sg, o_np, o_ht, o_pb, st, rc, [&](auto piece) {
      memcpy(&np, hbuf + o_np, 8);
      memcpy(&nh, hbuf + o_np + 8, 8);
      if (np <= cap && nh <= hcap) piece(o_ht, nh * 4);
    });
    // 3. the kernels and the copies are done: report (the uncached hits are
    //    counted where the ids arrived, before anything is copied out)
    if (rc) return rc;
    uint64_t uncached = 0;
    const uint32_t *ht = reinterpret_cast<const uint32_t *>(hbuf + o_ht);
    if (np <= cap && nh <= hcap)
      for (uint64_t p = 0; p < nh; ++p) uncached += !res.cached[ht[p]];
    *num_pairs = np;
    if (np > 0xffffffffull) return ADL_ERR_TOO_LARGE;
    if (np > cap) return ADL_ERR_WORKSPACE;  // (the hits of the first cap pairs only: nothing else is reported)
    *num_hits = nh;
    memcpy(h_hit_begin, hbuf + o_hb, (num_keys + 1) * 4);
    if (nh > hit_capacity) return ADL_ERR_WORKSPACE;
    if (nh) memcpy(h_hit_table, ht, nh * 4);
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// The revision multi-get for ONE key -- DB::Get's filter stage.  The key's
// candidate tables are selected in the levels' host indices (no device copy of
// the revision is made or used), ONLY their oids are resolved and pinned (a
// Get does not walk the revision's whole oid list under the cache's mutex),
// one request of the fan form asks the resident server about all of them, and
// the survivors are compacted here.  Per-thread scratch: nothing is allocated
// per call once it has grown.
int adl_bloom_revision_get(adl_bloom_revision *rev, adl_bloom_filter_cache *c, uint32_t filter, const uint8_t *h_key,
                           uint64_t key_len, int64_t seq, uint32_t *h_hit_table, uint32_t hit_capacity,
                           uint32_t *num_hits, uint32_t *num_candidates, uint32_t *h_uncached, void *stream) {
  if (!rev || !c || !num_hits || (key_len && !h_key) || (hit_capacity && !h_hit_table)) return ADL_ERR_INVALID_ARG;
  *num_hits = 0;
  if (num_candidates) *num_candidates = 0;
  if (h_uncached) *h_uncached = 0;
  for (adl_bloom_level *lv : rev->levels)
    if (lv && lv->ix.num_tables && lv->oids.size() != lv->ix.num_tables) return ADL_ERR_INVALID_ARG;  // no oids
  try {
    struct Scratch {
      std::vector<uint32_t> cand;
      std::vector<const char *> op;
      std::vector<uint64_t> ol;
      std::vector<uint8_t> ans;
    };
    thread_local Scratch sc;
    // 1. selection on the host (no key has more candidates than rev->longest)
    if (sc.cand.size() < rev->longest) sc.cand.resize(rev->longest);
    uint32_t n = 0;
    if (int rc = adl_bloom_revision_candidates_host(rev, h_key, key_len, seq, sc.cand.data(), (uint32_t)sc.cand.size(),
                                                    &n))
      return rc;
    if (num_candidates) *num_candidates = n;
    if (n == 0) return ADL_OK;
    // 2. the candidates' oids (a global id's level: the last base not above it)
    sc.op.resize(n);
    sc.ol.resize(n);
    sc.ans.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      const size_t l = std::upper_bound(rev->table_base.begin(), rev->table_base.end(), sc.cand[i]) -
                       rev->table_base.begin() - 1;
      const std::string &oid = rev->levels[l]->oids[sc.cand[i] - rev->table_base[l]];
      sc.op[i] = oid.data();
      sc.ol[i] = oid.size();
    }
    hipStream_t st = adl_host::sync_stream(stream);
    // 3. under the lock: their ranges and k, pinned and marked used; then one request
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_tables(c, sc.op.data(), sc.ol.data(), n, filter, res);
    if (int rc = probe_key_resolved(c, res, n, h_key, key_len, sc.ans.data(), st)) return rc;
    // 4. the survivors, in visiting order
    uint32_t nh = 0, uncached = 0;
    for (uint32_t i = 0; i < n; ++i) nh += sc.ans[i] != 0;
    *num_hits = nh;
    if (nh > hit_capacity) return ADL_ERR_WORKSPACE;
    nh = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (!sc.ans[i]) continue;
      h_hit_table[nh++] = sc.cand[i];
      uncached += !res.cached[i];
    }
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// The revision multi-get that returns a read plan (read_plan.hip): the pieces
// of adl_bloom_revision_multiget in the same order, then the hits grouped by
// table on the device.  The key-major hit arrays stay in device scratch beside
// the candidate pairs, sized for as many hits as pairs, so the grouping is
// never short of room there and both totals are exact whatever the caller's
// capacities are; what comes back is the counts, then the groups and entries
// they call for.
int adl_bloom_revision_read_plan(adl_bloom_revision *rev, adl_bloom_filter_cache *c, uint32_t filter,
                                 const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t num_keys,
                                 uint32_t key_stride, int64_t seq, uint32_t *h_group_table, uint32_t *h_group_begin,
                                 uint64_t group_capacity, uint64_t *num_groups, uint32_t *h_entry_key,
                                 uint64_t entry_capacity, uint64_t *num_hits, uint64_t pair_capacity,
                                 uint64_t *num_pairs, uint64_t *h_uncached, void *stream) {
  if (!rev || !c || !num_groups || !num_hits || !num_pairs || !h_group_begin) return ADL_ERR_INVALID_ARG;
  *num_groups = *num_hits = *num_pairs = 0;
  if (h_uncached) *h_uncached = 0;
  if (num_keys == 0) {
    h_group_begin[0] = 0;
    return ADL_OK;
  }
  if (!h_keys || (!h_offsets && key_stride == 0) || (group_capacity && !h_group_table) ||
      (entry_capacity && !h_entry_key))
    return ADL_ERR_INVALID_ARG;
  const uint32_t num_tables = rev->table_base.back();
  for (adl_bloom_level *lv : rev->levels)
    if (lv && lv->ix.num_tables && lv->oids.size() != lv->ix.num_tables) return ADL_ERR_INVALID_ARG;  // no oids
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;
  try {
    hipStream_t st = adl_host::sync_stream(stream);
    const uint64_t worst = std::min<uint64_t>(num_keys * (uint64_t)rev->longest, 0xffffffffull);
    const uint64_t cap = pair_capacity ? std::min<uint64_t>(pair_capacity, 0xffffffffull) : worst;
    const uint64_t gcap = std::min<uint64_t>(num_tables, cap);  // (no more groups than tables, or than hits)
    const uint64_t ecap = std::min(entry_capacity, cap);        // what the host buffer may have to hold
    // 1. under the lock: every level's tables' ranges and k, pinned and marked used
    Resolved &res = t_res;
    PinScope pins(c, res);
    resolve_levels(c, rev->levels.data(), rev->levels.size(), num_tables, filter, res);
    // 2. without the lock: keys, offsets and the range and k tables in one H2D;
    //    selection, probe + hit count, scan, compaction, grouping; then the
    //    results: num_pairs, num_hits, H and G | the group arrays | the entries
    //    | the hit lists, the candidate pairs and scratch, on the device only
    const uint64_t wsc = adl_bloom_revision_candidates_workspace_bytes(rev, num_keys);
    const uint64_t wsh = adl_bloom_probe_fanout_hits_workspace_bytes(num_keys, cap);
    const uint64_t wsg = adl_bloom_hits_by_table_workspace_bytes(num_keys, cap, num_tables);
    adl_host::StagePlan plan;
    const adl_host::KeyBlock kb(plan, h_offsets, num_keys, key_stride);
    const TableBlock tb(plan, res);
    const uint64_t o_np = plan.take(32);  // the end of the upload
    const uint64_t o_gb = plan.take((gcap + 1) * 4);
    const uint64_t o_gt = plan.take(gcap * 4);
    const uint64_t o_ek = plan.take(cap * 4);
    const uint64_t o_back = o_ek + adl_host::round_up(ecap * 4, 256);  // the end of what comes back
    const uint64_t o_hb = plan.take((num_keys + 1) * 4);
    const uint64_t o_ht = plan.take(cap * 4);
    const uint64_t o_pb = plan.take((num_keys + 1) * 4);
    const uint64_t o_pt = plan.take(cap * 4);
    const uint64_t o_wsc = plan.take(wsc);
    const uint64_t o_wsh = plan.take(wsh);
    const uint64_t o_wsg = plan.take(wsg);
    // the group arrays of a revision of a few thousand tables ride with the counts
    const bool groups_fixed = gcap * 8 <= (64u << 10);
    adl_host::Staging &sg = adl_host::t_stage;
    int rc = sg.reserve(o_back, plan.end);
    uint8_t *hbuf = sg.host, *dbuf = sg.dev;
    if (rc == ADL_OK) {
      kb.fill(hbuf, h_keys, h_offsets);
      tb.fill(hbuf, res);
      if (hipMemcpyAsync(dbuf, hbuf, o_np, hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    }
    auto d32 = [&](uint64_t at) { return reinterpret_cast<uint32_t *>(dbuf + at); };
    if (rc == ADL_OK)
      rc = adl_host::revision_select_device(rev, dbuf, kb.offsets(dbuf), num_keys, key_stride, seq, d32(o_pb),
                                            d32(o_pt), cap, reinterpret_cast<uint64_t *>(dbuf + o_np), dbuf + o_wsc,
                                            wsc, st);
    if (rc == ADL_OK)  // (the kernels stop at cap pairs whatever pair_begin says)
      rc = adl_host::probe_fanout_hits_device(dbuf, kb.offsets(dbuf), num_keys, key_stride, d32(o_pb), d32(o_pt), cap,
                                              num_tables, c->arena, tb.begin(dbuf), tb.begin(dbuf) + num_tables, 10,
                                              tb.k(dbuf), d32(o_hb), d32(o_ht), cap,
                                              reinterpret_cast<uint64_t *>(dbuf + o_np + 8), dbuf + o_wsh, wsh, st);
    if (rc == ADL_OK)
      rc = adl_host::hits_by_table_device(d32(o_hb), d32(o_ht), num_keys, num_tables, d32(o_gt), d32(o_gb), gcap,
                                          d32(o_ek), cap, reinterpret_cast<uint64_t *>(dbuf + o_np + 16),
                                          dbuf + o_wsg, wsg, st);
    uint64_t np = 0, nh = 0, ng = 0;
    auto fits = [&] { return np <= cap && nh <= entry_capacity && ng <= group_capacity; };
    rc = fetch_count_first(sg, o_np, groups_fixed ? o_ek : o_gb, o_back, st, rc, [&](auto piece) {
      memcpy(&np, hbuf + o_np, 8);
      memcpy(&nh, hbuf + o_np + 16, 8);
      memcpy(&ng, hbuf + o_np + 24, 8);
      if (!fits()) return;
      if (!groups_fixed) {
        piece(o_gb, (ng + 1) * 4);
        piece(o_gt, ng * 4);
      }
      piece(o_ek, nh * 4);
    });
    // 3. the kernels and the copies are done: report
    if (rc) return rc;
    *num_pairs = np;
    if (np > 0xffffffffull) return ADL_ERR_TOO_LARGE;
    if (np > cap) return ADL_ERR_WORKSPACE;  // (the hits of the first cap pairs only: nothing else is reported)
    *num_hits = nh;
    *num_groups = ng;
    if (!fits()) return ADL_ERR_WORKSPACE;
    const uint32_t *gb = reinterpret_cast<const uint32_t *>(hbuf + o_gb);
    const uint32_t *gt = reinterpret_cast<const uint32_t *>(hbuf + o_gt);
    uint64_t uncached = 0;
    for (uint64_t g = 0; g < ng; ++g)
      if (!res.cached[gt[g]]) uncached += gb[g + 1] - gb[g];
    memcpy(h_group_begin, gb, (ng + 1) * 4);
    if (ng) memcpy(h_group_table, gt, ng * 4);
    if (nh) memcpy(h_entry_key, hbuf + o_ek, nh * 4);
    if (h_uncached) *h_uncached = uncached;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

}  // extern "C"

// adlsm-tree_amd/csrc/level_filter.cpp -- Level::Get's filter stage, batched
// (see level_filter.hpp).
#include "level_filter.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "adl_bloom.h"
#include "level_index_core.hpp"

namespace adl {

namespace {

using adl_level::Decode;
using adl_level::Decoded;
using adl_level::Less;

}  // namespace

bool InnerKeyLess(string_view a, string_view b) { return Less(Decode(a), Decode(b)); }

bool LookupLess(string_view user_key, int64_t seq, string_view inner_key) {
  return Less(Decoded{user_key, seq, 0 /* OP_PUT */}, Decode(inner_key));
}

bool InnerLessLookup(string_view inner_key, string_view user_key, int64_t seq) {
  return Less(Decode(inner_key), Decoded{user_key, seq, 0});
}

/* src/revision.cpp:281-287:
 *   if ((mk < min_inner_key && mk.user_key_ != min_inner_key.user_key_) ||
 *       max_inner_key < mk) continue; */
bool TableCoversKey(const TableRange &t, string_view user_key, int64_t seq) {
  const Decoded mn = Decode(t.min_inner_key);
  if (LookupLess(user_key, seq, t.min_inner_key) && user_key != mn.user) return false;
  if (InnerLessLookup(t.max_inner_key, user_key, seq)) return false;
  return true;
}

void LevelCandidates(const vector<TableRange> &tables, const vector<string_view> &user_keys, int64_t seq,
                     vector<uint32_t> &begin, vector<uint32_t> &table) {
  const size_t K = user_keys.size(), T = tables.size();
  begin.assign(K + 1, 0);
  table.clear();
  // The per-call form of a LevelIndex: the region index (level_index_core.hpp)
  // built for this one batch and looked up once.  A caller that asks about the
  // same level again keeps a LevelIndex instead.
  vector<string_view> mins(T), maxs(T);
  for (size_t t = 0; t < T; ++t) {
    mins[t] = tables[t].min_inner_key;
    maxs[t] = tables[t].max_inner_key;
  }
  adl_level::Index ix;
  adl_level::Sweep sw;
  // The region lists hold sum(active tables per region) entries: for heavily
  // overlapping tables (L0, wide ranges) that is O(T^2) whatever K is.  When it
  // would exceed the K x T range tests of a direct scan (or the index's
  // limits), scan directly: the same predicate, in the same visiting order,
  // decided before any list is built.  The index lists a table at its own max
  // boundary even where this seq drops it there, so the count can be up to T
  // entries above what this one lookup needs and a borderline level may take
  // the other algorithm; the output is the same either way.
  if (!adl_level::Prepare(mins.data(), maxs.data(), T, ix, sw) || sw.total > (uint64_t)K * T ||
      !adl_level::Finish(sw, ~0ull, ix)) {
    for (size_t i = 0; i < K; ++i) {
      const string_view u = user_keys[i];
      for (size_t r = T; r-- > 0;) {
        const uint32_t t = sw.asc[r];
        const Decoded &mn = sw.mn[t], &mx = sw.mx[t];
        if (sw.never(t) || u < mn.user) continue;
        if (u < mx.user || (u == mx.user && !Less(mx, Decoded{mx.user, seq, 0}))) table.push_back(t);
      }
      begin[i + 1] = (uint32_t)table.size();
    }
    return;
  }
  adl_level::Lookup(ix, K, [&](size_t i) { return user_keys[i]; }, seq, begin.data(), table);
}

namespace {

/* ADL_BLOOM_LEVEL_FANOUT, read once per process: 1 (default)
 * probes each key once against its candidate list (FilterCache::ProbeFanout)
 * where that saves at least kFanoutMinSavedBytes of upload, 2 always, 0 never
 * (the (key, table) pairs as independent queries, FilterCache::Probe). */
int LevelFanout() {
  static const int mode = [] {
    const char *e = getenv("ADL_BLOOM_LEVEL_FANOUT");
    return e && *e ? (int)strtoul(e, nullptr, 10) : 1;
  }();
  return mode;
}

/* The measured crossover: the fan-out call costs 1.4 us more
 * than the pair call on a 1 000-key batch with one candidate per key, and
 * gains with the bytes it does not stage and send.  1 000 16-byte keys with
 * 1.9 candidates each (17 KB saved) lost 3 us of 37, with 3.4 each (54 KB
 * saved) won 6 us of 51; 65 536 keys tie at one candidate each and win from
 * 1.3 (224 KB saved). */
constexpr int64_t kFanoutMinSavedBytes = 32 << 10;

/* ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS, read once per process: the
 * batch size from which LevelMultiGetFilter(cache, LevelIndex, ...) selects on
 * the device; 0 = never.  The default is the measured crossover (DESIGN.md §5,
 * "Resident level index"): the device path costs 40-60 us up to a few thousand
 * keys, so on 16-table levels it loses 12-16 us to the host copy at 1 000 keys
 * and 2-11 us at 2 000, wins on every level measured at 3 000 (by 1-11 us) and
 * at 4 000 (7-23 us), and is 3-4x faster at 65 536. */
constexpr uint64_t kLevelDeviceMinKeys = 3000;

uint64_t LevelDeviceMinKeys() {
  static const uint64_t v = [] {
    const char *e = getenv("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS");
    return e && *e ? (uint64_t)strtoull(e, nullptr, 10) : kLevelDeviceMinKeys;
  }();
  return v;
}

/* The batch size from which RevisionMultiGetFilter makes the one device call,
 * by the number of non-empty levels; 0 = never.  ADL_BLOOM_REVISION_DEVICE_
 * MIN_KEYS, or else ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS, where the environment
 * sets one (read once per process), holds for every revision.
 * The defaults are the measured crossovers ("Revision
 * multi-get"; profiles/revision/crossover_summary.txt): the smallest measured
 * batch from which the single call won on absent-key batches AND on batches
 * whose every pair is a hit, its worst case (all the pairs come back, as they
 * do per level).  One level: the call loses 3-32 us up to 2 000 keys and 9 us
 * on all-hit batches at 4 000, loses 2 us on them at 8 000 and wins 19-47 us
 * at 16 000.  Two: loses 3-13 us up to
 * 1 000 keys on all-hit batches, wins 29-46 us at 2 000.  Three: loses 5 us
 * at 500, wins 21-42 us at 1 000 (four levels were not measured and take
 * three's).  Five: loses 8 us at 250, wins 14-46 us at 500. */
uint64_t RevisionDeviceMinKeys(size_t live_levels) {
  static const int64_t env = [] {
    for (const char *name : {"ADL_BLOOM_REVISION_DEVICE_MIN_KEYS", "ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS"}) {
      const char *e = getenv(name);
      if (e && *e) return (int64_t)strtoull(e, nullptr, 10);
    }
    return (int64_t)-1;
  }();
  if (env >= 0) return (uint64_t)env;
  return live_levels <= 1 ? 16000 : live_levels == 2 ? 2000 : live_levels <= 4 ? 1000 : 500;
}

/* The batch size from which RevisionReadPlanFilter makes the one device call
 * (adl_bloom_revision_read_plan); 0 = never.  The environment's threshold, as
 * RevisionDeviceMinKeys reads it, holds here too.  Otherwise never below that
 * function's crossover, and never below the measured floor for the revision's
 * number of tables ("Read plan"; profiles/read_plan/summary.txt):
 * the smallest measured batch from which the call did not lose to
 * RevisionMultiGetFilter + GroupHitsByTable by more than the run-to-run spread
 * on absent-key batches (next to no hits: the grouping's launches buy nothing)
 * and won on batches whose every pair is a hit.  Up to 256 tables the sort is
 * one pass and the grouping four launches: it loses 10 us on absent batches at
 * 1 000 keys, ties at 3 000 (6 us, inside the spread) and wins from there (11
 * and 31 us on absent, 82 to 2 400 us on all-hit batches).  Beyond 256 tables
 * it is ten launches or more: absent batches lose 17-23 us up to 16 000 keys
 * and tie at 65 536, where all-hit batches win 2.1 ms (47 and 480 us at 3 000
 * and 16 000, which this floor forgoes rather than tax hit-free batches). */
uint64_t ReadPlanDeviceMinKeys(size_t live_levels, uint32_t num_tables) {
  const uint64_t rev = RevisionDeviceMinKeys(live_levels);
  static const bool forced = [] {
    for (const char *name : {"ADL_BLOOM_REVISION_DEVICE_MIN_KEYS", "ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS"}) {
      const char *e = getenv(name);
      if (e && *e) return true;
    }
    return false;
  }();
  if (forced || rev == 0) return rev;
  return std::max<uint64_t>(rev, num_tables <= 256 ? 3000 : 65536);
}

RC FromStatus(int status) {
  if (status == ADL_OK) return OK;
  if (status == ADL_FILTER_BLOCK_ERROR) return FILTER_BLOCK_ERROR;
  if (status == ADL_ERR_TOO_LARGE) return OUT_OF_RANGE;
  return DEVICE_ERROR;
}

size_t KeyBytes(const vector<string_view> &user_keys) {
  size_t bytes = 0;
  for (string_view k : user_keys) bytes += k.size();
  return bytes;
}

/* The batch's keys, each once, packed into `batch` for upload (key_bytes = KeyBytes(user_keys)). */
void PackKeys(const vector<string_view> &user_keys, size_t key_bytes, KeyArena &batch) {
  batch.Reserve(user_keys.size(), key_bytes);
  for (string_view k : user_keys) batch.Add(k);
}

/* The result capacities of a device multi-get.  No key has more candidates
 * than its level's longest list, but one wide region must not size every
 * batch's buffers (here and, pinned, in the library) for K x longest: `first`,
 * room for twice the mean list per key, and then the exact size, which the
 * call reports (ADL_ERR_WORKSPACE with np > pcap or nh > hcap), where a batch
 * needs more -- never beyond `worst`.  call(pcap, hcap) makes the call with
 * those pair and hit capacities and sets np and nh; returns its last status. */
template <class Call>
int CallWithGrownCapacity(uint64_t first, uint64_t worst, uint64_t &np, uint64_t &nh, Call &&call) {
  uint64_t pcap = std::min(worst, first), hcap = pcap;
  int st = ADL_OK;
  for (int attempt = 0; attempt < 3; ++attempt) {
    st = call(pcap, hcap);
    if (st != ADL_ERR_WORKSPACE || np > worst) break;
    if (np > pcap) pcap = np;
    else if (nh > hcap) hcap = nh;
    else break;
  }
  return st;
}

/* The probes of a selected batch: out.begin / out.table are key i's candidates;
 * fills out.maybe and out.uncached. */
RC ProbeSelected(FilterCache &cache, const vector<string_view> &oids, const vector<string_view> &user_keys,
                 MultiGetFilterResult &out) {
  const size_t K = user_keys.size();
  // SSTableReader::Get probes the user key (src/sstable.cpp:238).  Upload per
  // path: a batch of pairs carries key bytes + an 8-byte offset + a table id
  // per PAIR; the fan-out batch carries key bytes + offset + a begin entry
  // per KEY and a table id per pair.
  size_t key_bytes = 0, pair_bytes = 0;
  for (size_t i = 0; i < K; ++i) {
    key_bytes += user_keys[i].size();
    pair_bytes += (size_t)(out.begin[i + 1] - out.begin[i]) * user_keys[i].size();
  }
  const int64_t saved = (int64_t)(pair_bytes + 8 * out.table.size()) - (int64_t)(key_bytes + 12 * K + 4);
  const int mode = LevelFanout();
  KeyArena batch;
  if (mode >= 2 || (mode == 1 && saved >= kFanoutMinSavedBytes)) {
    // each key once, probed against its candidate list (out.begin / out.table
    // as they are): uploaded and hashed once per key instead of once per pair
    PackKeys(user_keys, key_bytes, batch);
    return cache.ProbeFanout(oids, out.begin, out.table, batch, 0, out.maybe, &out.uncached);
  }
  // the probe batch: pair p = (key, table)
  batch.Reserve(out.table.size(), pair_bytes);
  for (size_t i = 0; i < K; ++i)
    for (uint32_t c = out.begin[i]; c < out.begin[i + 1]; ++c) batch.Add(user_keys[i]);
  return cache.Probe(oids, out.table, batch, 0, out.maybe, &out.uncached);
}

}  // namespace

RC LevelMultiGetFilter(FilterCache &cache, const vector<TableRange> &tables, const vector<string_view> &user_keys,
                       int64_t seq, MultiGetFilterResult &out) {
  out = MultiGetFilterResult{};
  LevelCandidates(tables, user_keys, seq, out.begin, out.table);
  const size_t T = tables.size();
  vector<string_view> oids(T);
  for (size_t t = 0; t < T; ++t) oids[t] = tables[t].oid;
  return ProbeSelected(cache, oids, user_keys, out);
}

LevelIndex::LevelIndex(const vector<TableRange> &tables, uint64_t max_index_bytes)
    : ix_(new adl_level::Index), tables_(tables), max_index_bytes_(max_index_bytes) {
  const size_t T = tables_.size();
  vector<string_view> mins(T), maxs(T);
  oid_views_.resize(T);
  for (size_t t = 0; t < T; ++t) {
    oid_views_[t] = tables_[t].oid;
    mins[t] = tables_[t].min_inner_key;
    maxs[t] = tables_[t].max_inner_key;
  }
  status_ = adl_level::Build(mins.data(), maxs.data(), T,
                             max_index_bytes ? max_index_bytes : adl_level::kDefaultIndexBytes, *ix_)
                ? OK
                : OUT_OF_RANGE;
}

LevelIndex::~LevelIndex() { (void)adl_bloom_level_destroy(h_); }

uint32_t LevelIndex::longest_list() const { return ix_->longest; }

uint32_t LevelIndex::mean_list() const {
  const uint64_t regions = 2ull * ix_->num_boundaries + 1;
  return (uint32_t)((ix_->rlist.size() + regions - 1) / regions);
}

adl_bloom_level *LevelIndex::handle() {
  std::call_once(handle_once_, [this] {
    if (status_) {
      device_status_ = status_;
      return;
    }
    const size_t T = tables_.size();
    vector<const char *> op(T), mn(T), mx(T);
    vector<uint64_t> ol(T), ml(T), xl(T);
    for (size_t t = 0; t < T; ++t) {
      op[t] = tables_[t].oid.data();
      ol[t] = tables_[t].oid.size();
      mn[t] = tables_[t].min_inner_key.data();
      ml[t] = tables_[t].min_inner_key.size();
      mx[t] = tables_[t].max_inner_key.data();
      xl[t] = tables_[t].max_inner_key.size();
    }
    device_status_ = FromStatus(adl_bloom_level_create(op.data(), ol.data(), mn.data(), ml.data(), mx.data(),
                                                       xl.data(), (uint32_t)T, max_index_bytes_, &h_));
  });
  return h_;
}

void LevelIndex::Candidates(const vector<string_view> &user_keys, int64_t seq, vector<uint32_t> &begin,
                            vector<uint32_t> &table) const {
  const size_t K = user_keys.size();
  begin.assign(K + 1, 0);
  table.clear();
  if (status_) return;
  adl_level::Lookup(*ix_, K, [&](size_t i) { return user_keys[i]; }, seq, begin.data(), table);
}

RC LevelMultiGetFilter(FilterCache &cache, LevelIndex &level, const vector<string_view> &user_keys, int64_t seq,
                       MultiGetFilterResult &out) {
  out = MultiGetFilterResult{};
  if (level.status()) return level.status();
  const size_t K = user_keys.size();
  const uint64_t min_keys = LevelDeviceMinKeys();
  if (min_keys == 0 || K < min_keys) {
    // the call above without its per-call index build
    level.Candidates(user_keys, seq, out.begin, out.table);
    return ProbeSelected(cache, level.oids(), user_keys, out);
  }
  adl_bloom_level *lv = level.handle();
  if (!lv) return level.device_status();
  if (!cache.handle()) return cache.status();
  // keys up, lists and answers down: selection, expansion and the probes on
  // the device.
  KeyArena batch;
  PackKeys(user_keys, KeyBytes(user_keys), batch);
  const uint64_t worst = std::min<uint64_t>((uint64_t)K * level.longest_list(), 0xffffffffull);
  out.begin.assign(K + 1, 0);
  uint64_t np = 0, nh = 0;
  const int st = CallWithGrownCapacity(2ull * K * level.mean_list() + 1024, worst, np, nh, [&](uint64_t cap, uint64_t) {
    out.table.resize(cap);
    out.maybe.resize(cap);
    return adl_bloom_level_multiget(lv, cache.handle(), 0, reinterpret_cast<const uint8_t *>(batch.bytes().data()),
                                    batch.offsets().data(), K, 0, seq, out.begin.data(), out.table.data(),
                                    out.maybe.data(), cap, &np, &out.uncached, nullptr);
  });
  if (st != ADL_OK) {
    out = MultiGetFilterResult{};
    return FromStatus(st);
  }
  out.table.resize(np);
  out.maybe.resize(np);
  return OK;
}

RevisionIndex::RevisionIndex(const vector<LevelIndex *> &levels) : levels_(levels) {
  table_base_.assign(levels_.size() + 1, 0);
  if (levels_.size() > ADL_BLOOM_MAX_LEVELS) {
    status_ = BAD_REVISION;
    return;
  }
  uint64_t longest = 0, tables = 0;
  for (size_t l = 0; l < levels_.size(); ++l) {
    const LevelIndex *lv = levels_[l];
    if (lv && lv->status()) {
      status_ = lv->status();
      return;
    }
    tables += lv ? lv->tables() : 0;
    longest += lv && lv->tables() ? lv->longest_list() : 0;
    table_base_[l + 1] = (uint32_t)tables;
  }
  if (tables >= adl_level::kTableMask || longest >= (1u << 24)) status_ = OUT_OF_RANGE;
  longest_ = (uint32_t)longest;
}

RevisionIndex::~RevisionIndex() { (void)adl_bloom_revision_destroy(h_); }

adl_bloom_revision *RevisionIndex::handle() {
  std::call_once(handle_once_, [this] {
    if (status_) {
      device_status_ = status_;
      return;
    }
    vector<adl_bloom_level *> hs(levels_.size(), nullptr);
    for (size_t l = 0; l < levels_.size(); ++l) {
      if (!levels_[l] || levels_[l]->tables() == 0) continue;
      hs[l] = levels_[l]->handle();
      if (!hs[l]) {
        device_status_ = levels_[l]->device_status();
        return;
      }
    }
    device_status_ = FromStatus(adl_bloom_revision_create(hs.data(), (uint32_t)hs.size(), &h_));
  });
  return h_;
}

void RevisionIndex::Candidates(const vector<string_view> &user_keys, int64_t seq, vector<uint32_t> &begin,
                               vector<uint32_t> &table) const {
  const size_t K = user_keys.size(), L = levels_.size();
  begin.assign(K + 1, 0);
  table.clear();
  if (status_) return;
  vector<vector<uint32_t>> lb(L), lt(L);
  for (size_t l = 0; l < L; ++l)
    if (levels_[l] && levels_[l]->tables()) levels_[l]->Candidates(user_keys, seq, lb[l], lt[l]);
  for (size_t i = 0; i < K; ++i) {
    for (size_t l = 0; l < L; ++l) {
      if (lb[l].empty()) continue;
      for (uint32_t p = lb[l][i]; p < lb[l][i + 1]; ++p) table.push_back(table_base_[l] + lt[l][p]);
    }
    begin[i + 1] = (uint32_t)table.size();
  }
}

RC RevisionMultiGetFilter(FilterCache &cache, RevisionIndex &rev, const vector<string_view> &user_keys, int64_t seq,
                          RevisionMultiGetResult &out) {
  out = RevisionMultiGetResult{};
  if (rev.status()) return rev.status();
  const size_t K = user_keys.size(), L = rev.levels();
  const vector<uint32_t> &base = rev.table_base();
  out.begin.assign(K + 1, 0);
  auto fill_levels = [&] {
    out.level.resize(out.table.size());
    for (size_t p = 0; p < out.table.size(); ++p)
      out.level[p] = (uint8_t)(std::upper_bound(base.begin(), base.end(), out.table[p]) - base.begin() - 1);
  };
  size_t live = 0;
  for (size_t l = 0; l < L; ++l) live += rev.level(l) && rev.level(l)->tables();
  const uint64_t min_keys = RevisionDeviceMinKeys(live);
  if (min_keys == 0 || K < min_keys) {
    // one level multi-get per level, then the pass that keeps the hits
    vector<MultiGetFilterResult> per(L);
    for (size_t l = 0; l < L; ++l) {
      LevelIndex *lv = rev.level(l);
      if (!lv || lv->tables() == 0) continue;
      if (RC rc = LevelMultiGetFilter(cache, *lv, user_keys, seq, per[l])) {
        out = RevisionMultiGetResult{};
        return rc;
      }
    }
    for (size_t i = 0; i < K; ++i) {
      for (size_t l = 0; l < L; ++l) {
        const MultiGetFilterResult &r = per[l];
        if (r.begin.empty()) continue;
        for (uint32_t p = r.begin[i]; p < r.begin[i + 1]; ++p)
          if (r.maybe[p]) out.table.push_back(base[l] + r.table[p]);
      }
      out.begin[i + 1] = (uint32_t)out.table.size();
    }
    // a table that is not cached answers 1 for every pair: its pairs are all hits
    for (size_t l = 0; l < L; ++l) out.uncached += per[l].uncached;
    fill_levels();
    return OK;
  }
  adl_bloom_revision *h = rev.handle();
  if (!h) return rev.device_status();
  if (!cache.handle()) return cache.status();
  // (packed and sized here, not through PackKeys and CallWithGrownCapacity:
  // with them this function's all-hit batches of 65 536 keys measured 3-7 %
  // slower)
  size_t key_bytes = 0;
  for (string_view k : user_keys) key_bytes += k.size();
  KeyArena batch;
  batch.Reserve(K, key_bytes);
  for (string_view k : user_keys) batch.Add(k);
  // Scratch for twice the mean lists per key first, as the level overload
  // sizes its buffers, and the exact sizes, which the call reports, where a
  // batch needs more.
  const uint64_t worst = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)K * rev.longest_list(), 0xffffffffull));
  uint64_t mean = 0;
  for (size_t l = 0; l < L; ++l)
    if (rev.level(l) && rev.level(l)->tables()) mean += rev.level(l)->mean_list();
  uint64_t pcap = std::min<uint64_t>(worst, 2ull * K * mean + 1024), hcap = pcap;
  uint64_t np = 0, nh = 0;
  int st = ADL_OK;
  for (int attempt = 0; attempt < 3; ++attempt) {
    out.table.resize(hcap);
    st = adl_bloom_revision_multiget(h, cache.handle(), 0, reinterpret_cast<const uint8_t *>(batch.bytes().data()),
                                     batch.offsets().data(), K, 0, seq, out.begin.data(), out.table.data(), hcap,
                                     &nh, pcap, &np, &out.uncached, nullptr);
    if (st != ADL_ERR_WORKSPACE || np > worst) break;
    if (np > pcap) pcap = np;
    else if (nh > hcap) hcap = nh;
    else break;
  }
  if (st != ADL_OK) {
    out = RevisionMultiGetResult{};
    return FromStatus(st);
  }
  out.table.resize(nh);
  fill_levels();
  return OK;
}

RC RevisionGetFilter(FilterCache &cache, RevisionIndex &rev, string_view user_key, int64_t seq,
                     RevisionGetResult &out) {
  out.table.clear();
  out.level.clear();
  out.candidates = out.uncached = 0;
  if (rev.status()) return rev.status();
  adl_bloom_revision *h = rev.handle();
  if (!h) return rev.device_status();
  if (!cache.handle()) return cache.status();
  const vector<uint32_t> &base = rev.table_base();
  // no key has more candidates, so no call comes back short of room
  out.table.resize(rev.longest_list());
  uint32_t nh = 0;
  const int st = adl_bloom_revision_get(h, cache.handle(), 0, reinterpret_cast<const uint8_t *>(user_key.data()),
                                        user_key.size(), seq, out.table.data(), (uint32_t)out.table.size(), &nh,
                                        &out.candidates, &out.uncached, nullptr);
  if (st != ADL_OK) {
    out.table.clear();
    return FromStatus(st);
  }
  out.table.resize(nh);
  out.level.resize(nh);
  for (uint32_t p = 0; p < nh; ++p)
    out.level[p] = (uint8_t)(std::upper_bound(base.begin(), base.end(), out.table[p]) - base.begin() - 1);
  return OK;
}

namespace {

/* group_level and level_begin of a plan whose group_table is set */
void FillPlanLevels(const vector<uint32_t> &base, RevisionReadPlan &out) {
  const size_t G = out.group_table.size(), L = base.size() - 1;
  out.group_level.resize(G);
  out.level_begin.assign(L + 1, 0);
  for (size_t g = 0; g < G; ++g) {
    const size_t l = std::upper_bound(base.begin(), base.end(), out.group_table[g]) - base.begin() - 1;
    out.group_level[g] = (uint8_t)l;
    ++out.level_begin[l + 1];
  }
  for (size_t l = 0; l < L; ++l) out.level_begin[l + 1] += out.level_begin[l];
}

}  // namespace

void GroupHitsByTable(const RevisionMultiGetResult &hits, const vector<uint32_t> &table_base, RevisionReadPlan &out) {
  out = RevisionReadPlan{};
  out.uncached = hits.uncached;
  const size_t K = hits.begin.empty() ? 0 : hits.begin.size() - 1, H = hits.table.size();
  // a counting sort on the table id: the hits per table, the tables that have
  // any (ascending) with their first entry, then the keys placed in batch order
  vector<uint32_t> at(table_base.back() + 1, 0);
  for (uint32_t t : hits.table) ++at[t + 1];
  uint32_t run = 0;
  for (size_t t = 0; t + 1 < at.size(); ++t) {
    const uint32_t n = at[t + 1];
    if (n) {
      out.group_table.push_back((uint32_t)t);
      out.group_begin.push_back(run);
    }
    at[t] = run;
    run += n;
  }
  out.group_begin.push_back(run);
  out.key.resize(H);
  for (size_t i = 0; i < K; ++i)
    for (uint32_t p = hits.begin[i]; p < hits.begin[i + 1]; ++p) out.key[at[hits.table[p]]++] = (uint32_t)i;
  FillPlanLevels(table_base, out);
}

RC RevisionReadPlanFilter(FilterCache &cache, RevisionIndex &rev, const vector<string_view> &user_keys, int64_t seq,
                          RevisionReadPlan &out) {
  out = RevisionReadPlan{};
  if (rev.status()) return rev.status();
  const size_t K = user_keys.size(), L = rev.levels();
  size_t live = 0;
  for (size_t l = 0; l < L; ++l) live += rev.level(l) && rev.level(l)->tables();
  const uint64_t min_keys = ReadPlanDeviceMinKeys(live, rev.table_base().back());
  if (min_keys == 0 || K < min_keys) {
    RevisionMultiGetResult hits;
    if (RC rc = RevisionMultiGetFilter(cache, rev, user_keys, seq, hits)) return rc;
    GroupHitsByTable(hits, rev.table_base(), out);
    return OK;
  }
  adl_bloom_revision *h = rev.handle();
  if (!h) return rev.device_status();
  if (!cache.handle()) return cache.status();
  size_t key_bytes = 0;
  for (string_view k : user_keys) key_bytes += k.size();
  KeyArena batch;
  batch.Reserve(K, key_bytes);
  for (string_view k : user_keys) batch.Add(k);
  // Capacities as RevisionMultiGetFilter sizes them: twice the mean lists per
  // key first, then the exact sizes the call reports.  No more groups than
  // tables.
  const uint64_t worst = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)K * rev.longest_list(), 0xffffffffull));
  uint64_t mean = 0;
  for (size_t l = 0; l < L; ++l)
    if (rev.level(l) && rev.level(l)->tables()) mean += rev.level(l)->mean_list();
  uint64_t pcap = std::min<uint64_t>(worst, 2ull * K * mean + 1024), ecap = pcap;
  const uint64_t gcap = rev.table_base().back();
  uint64_t np = 0, nh = 0, ng = 0;
  int st = ADL_OK;
  out.group_table.resize(gcap);
  out.group_begin.resize(gcap + 1);
  for (int attempt = 0; attempt < 3; ++attempt) {
    out.key.resize(ecap);
    st = adl_bloom_revision_read_plan(h, cache.handle(), 0, reinterpret_cast<const uint8_t *>(batch.bytes().data()),
                                      batch.offsets().data(), K, 0, seq, out.group_table.data(),
                                      out.group_begin.data(), gcap, &ng, out.key.data(), ecap, &nh, pcap, &np,
                                      &out.uncached, nullptr);
    if (st != ADL_ERR_WORKSPACE || np > worst) break;
    if (np > pcap) pcap = np;
    else if (nh > ecap) ecap = nh;
    else break;
  }
  if (st != ADL_OK) {
    out = RevisionReadPlan{};
    return FromStatus(st);
  }
  out.group_table.resize(ng);
  out.group_begin.resize(ng + 1);
  out.key.resize(nh);
  FillPlanLevels(rev.table_base(), out);
  return OK;
}

}  // namespace adl

namespace {

/* The test hooks' arguments: tables [t0, t1) of (pointer, length) arrays (no
 * oids), keys [i0, i1) as views, and a result copied out to the caller's
 * arrays (the number of pairs, or -1 when cap is too small). */
std::vector<adl::TableRange> HookTables(const char *const *mins, const uint64_t *min_lens, const char *const *maxs,
                                        const uint64_t *max_lens, uint32_t t0, uint32_t t1) {
  std::vector<adl::TableRange> tabs(t1 - t0);
  for (uint32_t t = t0; t < t1; ++t) {
    tabs[t - t0].min_inner_key.assign(mins[t], min_lens[t]);
    tabs[t - t0].max_inner_key.assign(maxs[t], max_lens[t]);
  }
  return tabs;
}

std::vector<std::string_view> HookKeys(const char *const *keys, const uint64_t *key_lens, uint32_t i0, uint32_t i1) {
  std::vector<std::string_view> ks(i1 - i0);
  for (uint32_t i = i0; i < i1; ++i) ks[i - i0] = std::string_view(keys[i], key_lens[i]);
  return ks;
}

int64_t HookResult(const std::vector<uint32_t> &b, const std::vector<uint32_t> &tb, uint32_t *begin, uint32_t *table,
                   uint64_t cap) {
  if (tb.size() > cap) return -1;
  std::copy(b.begin(), b.end(), begin);
  std::copy(tb.begin(), tb.end(), table);
  return (int64_t)tb.size();
}

}  // namespace

/* Test hook (tests/test_revision_cpu.py): one LevelIndex per level over its
 * tables, a RevisionIndex over them, and its host Candidates for one batch.
 * Level l's tables are [table_begin[l], table_begin[l+1]) of mins / maxs; a
 * level with skip[l] != 0 is handed over as nullptr.  begin: K+1 entries,
 * table: up to cap global ids.  Returns the number of pairs, -1 when cap is
 * too small, -2 when an index was not built. */
extern "C" int64_t adl_revision_index_candidates(const char *const *mins, const uint64_t *min_lens,
                                                 const char *const *maxs, const uint64_t *max_lens,
                                                 const uint32_t *table_begin, const uint8_t *skip, uint32_t L,
                                                 const char *const *keys, const uint64_t *key_lens, uint32_t K,
                                                 int64_t seq, uint32_t *begin, uint32_t *table, uint64_t cap) {
  std::vector<std::unique_ptr<adl::LevelIndex>> own(L);
  std::vector<adl::LevelIndex *> lv(L, nullptr);
  for (uint32_t l = 0; l < L; ++l) {
    if (skip && skip[l]) continue;
    own[l] = std::make_unique<adl::LevelIndex>(
        HookTables(mins, min_lens, maxs, max_lens, table_begin[l], table_begin[l + 1]));
    lv[l] = own[l].get();
  }
  adl::RevisionIndex rev(lv);
  if (rev.status()) return -2;
  std::vector<uint32_t> b, tb;
  rev.Candidates(HookKeys(keys, key_lens, 0, K), seq, b, tb);
  return HookResult(b, tb, begin, table, cap);
}

/* Test hook (tests/test_read_plan_cpu.py): GroupHitsByTable on a key-major
 * result handed over as arrays (hit_begin: K+1 entries; table_base: L+1).
 * group_table / group_level: up to group_cap entries, group_begin: one more;
 * key: hit_begin[K] entries; level_begin: L+1.  Returns the number of groups,
 * or -1 when group_cap is too small. */
extern "C" int64_t adl_revision_group_hits(const uint32_t *hit_begin, const uint32_t *hit_table, uint32_t K,
                                           const uint32_t *table_base, uint32_t L, uint32_t *group_table,
                                           uint8_t *group_level, uint32_t *group_begin, uint64_t group_cap,
                                           uint32_t *key, uint32_t *level_begin) {
  adl::RevisionMultiGetResult hits;
  hits.begin.assign(hit_begin, hit_begin + K + 1);
  hits.table.assign(hit_table, hit_table + hit_begin[K]);
  adl::RevisionReadPlan plan;
  adl::GroupHitsByTable(hits, std::vector<uint32_t>(table_base, table_base + L + 1), plan);
  if (plan.group_table.size() > group_cap) return -1;
  std::copy(plan.group_table.begin(), plan.group_table.end(), group_table);
  std::copy(plan.group_level.begin(), plan.group_level.end(), group_level);
  std::copy(plan.group_begin.begin(), plan.group_begin.end(), group_begin);
  std::copy(plan.key.begin(), plan.key.end(), key);
  std::copy(plan.level_begin.begin(), plan.level_begin.end(), level_begin);
  return (int64_t)plan.group_table.size();
}

/* Test hook (tests/test_level_cpu.py): LevelCandidates over tables and keys
 * handed over as (pointer, length) arrays; begin: K+1 entries, table: up to
 * cap entries.  Returns the number of pairs, or -1 when cap is too small. */
extern "C" int64_t adl_level_candidates(const char *const *mins, const uint64_t *min_lens, const char *const *maxs,
                                        const uint64_t *max_lens, uint32_t T, const char *const *keys,
                                        const uint64_t *key_lens, uint32_t K, int64_t seq, uint32_t *begin,
                                        uint32_t *table, uint64_t cap) {
  std::vector<uint32_t> b, tb;
  adl::LevelCandidates(HookTables(mins, min_lens, maxs, max_lens, 0, T), HookKeys(keys, key_lens, 0, K), seq, b, tb);
  return HookResult(b, tb, begin, table, cap);
}

/* Test hook (tests/test_level_index_cpu.py): ONE LevelIndex over the tables,
 * then `batches` host lookups in it, batch b = keys [key_begin[b],
 * key_begin[b+1]) at seqs[b].  begin: one entry per key and one more per
 * batch, batch b's starting at key_begin[b] + b and counting from 0; table:
 * the lists of all batches back to back, up to cap entries.  Returns the
 * number of pairs, -1 when cap is too small, -2 when the index was not built. */
extern "C" int64_t adl_level_index_candidates(const char *const *mins, const uint64_t *min_lens,
                                              const char *const *maxs, const uint64_t *max_lens, uint32_t T,
                                              uint64_t max_index_bytes, const char *const *keys,
                                              const uint64_t *key_lens, const uint32_t *key_begin, uint32_t batches,
                                              const int64_t *seqs, uint32_t *begin, uint32_t *table, uint64_t cap) {
  adl::LevelIndex index(HookTables(mins, min_lens, maxs, max_lens, 0, T), max_index_bytes);
  if (index.status()) return -2;
  uint64_t total = 0;
  for (uint32_t b = 0; b < batches; ++b) {
    std::vector<uint32_t> bg, tb;
    index.Candidates(HookKeys(keys, key_lens, key_begin[b], key_begin[b + 1]), seqs[b], bg, tb);
    const int64_t n = HookResult(bg, tb, begin + key_begin[b] + b, table + total, cap - total);
    if (n < 0) return -1;
    total += (uint64_t)n;
  }
  return (int64_t)total;
}

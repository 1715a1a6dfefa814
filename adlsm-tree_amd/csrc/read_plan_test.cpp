// adlsm-tree_amd/csrc/read_plan_test.cpp -- revision multi-gets that return a
// read plan (the hits grouped by table on the device) against the key-major
// multi-get grouped on the host, for tests/.  Needs a GPU.
//
//   read_plan_test device | host
//     A revision of three levels -- 12 overlapping tables (bits_per_key 10, 3,
//     16 in turn, one table not cached), 40 disjoint tables, and 12 overlapping
//     tables again over the same user keys -- asked with batches of 300 and of
//     3 000 keys at four sequence numbers.  `device` sets
//     ADL_BLOOM_REVISION_DEVICE_MIN_KEYS to 1 (every batch is the single
//     adl_bloom_revision_read_plan call), `host` to 0 (never).  Every plan must
//     equal GroupHitsByTable(RevisionMultiGetFilter(...)) and be well formed
//     (tables ascending, keys ascending within a group, level_begin matching
//     table_base).  Exit 0 = all equal.
//
//   read_plan_test --race
//     Four threads call RevisionReadPlanFilter (the device call) on one
//     revision and cache at once, each at its own sequence numbers; every plan
//     must equal the one made sequentially beforehand.  Exit 0 = all equal.
//
//   read_plan_test --bench <levels> <tables> <keys>[,<keys>...] [<bottom_tables> [absent|present]]
//     revision_test --bench's revision and batches.  Timed in one process, the
//     repetitions interleaved: RevisionMultiGetFilter followed by
//     GroupHitsByTable on the host, and one RevisionReadPlanFilter call, both
//     forced onto the device (ADL_BLOOM_REVISION_DEVICE_MIN_KEYS=1).  One JSON
//     line per batch: median, min and max of both in ms, the host grouping's
//     share, and the pair, hit and group counts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "filter_block.hpp"
#include "level_filter.hpp"

namespace {

using namespace adl;

int g_digits = 12;  // "user" + 12 digits: 16 bytes (--bench: 9 digits)

std::string UserKey(uint64_t i) {
  char b[32];
  snprintf(b, sizeof(b), "user%0*llu", g_digits, (unsigned long long)i);
  return b;
}

std::string Inner(const std::string &user, int64_t seq, char op = '\0') {
  std::string k = user;
  k.append(reinterpret_cast<const char *>(&seq), 8);
  k.push_back(op);
  return k;
}

// table t holds user keys [t stride, t stride + span), bits_per_key bpk[t % nb]
bool MakeLevel(FilterCache &cache, int T, uint64_t stride, uint64_t span, const int *bpk, int nb,
               const std::string &tag, int skip_table, std::vector<TableRange> &tables) {
  for (int t = 0; t < T; ++t) {
    FilterBlockWriter w(std::make_unique<BloomFilter>(bpk[t % nb]));
    const uint64_t lo = (uint64_t)t * stride, hi = lo + span;
    for (uint64_t i = lo; i < hi; ++i) w.Update(UserKey(i));
    std::string block;
    if (w.Final(block)) return false;
    tables.push_back(TableRange{tag + "-" + std::to_string(t), Inner(UserKey(lo), (int64_t)lo),
                                Inner(UserKey(hi - 1), (int64_t)hi - 1, (char)(t & 1))});
    if (t != skip_table && cache.Put(tables.back().oid, block)) return false;
  }
  return true;
}

bool SamePlan(const RevisionReadPlan &a, const RevisionReadPlan &b) {
  return a.group_table == b.group_table && a.group_level == b.group_level && a.group_begin == b.group_begin &&
         a.key == b.key && a.level_begin == b.level_begin && a.uncached == b.uncached;
}

// tables ascending, begins ascending and closed by the hit total, keys ascending
// within a group, level_begin cutting the groups where table_base cuts the ids
bool WellFormed(const RevisionReadPlan &p, const std::vector<uint32_t> &base, size_t K) {
  const size_t G = p.group_table.size(), L = base.size() - 1;
  if (p.group_begin.size() != G + 1 || p.group_level.size() != G || p.level_begin.size() != L + 1) return false;
  if (p.group_begin.front() != 0 || p.group_begin.back() != p.key.size() || p.level_begin.back() != G) return false;
  for (size_t g = 0; g < G; ++g) {
    if (g && p.group_table[g] <= p.group_table[g - 1]) return false;
    if (p.group_begin[g + 1] <= p.group_begin[g]) return false;
    for (uint32_t e = p.group_begin[g]; e < p.group_begin[g + 1]; ++e)
      if (p.key[e] >= K || (e > p.group_begin[g] && p.key[e] <= p.key[e - 1])) return false;
    const uint8_t l = p.group_level[g];
    if (p.group_table[g] < base[l] || p.group_table[g] >= base[l + 1]) return false;
    if (g < p.level_begin[l] || g >= p.level_begin[l + 1]) return false;
  }
  return true;
}

struct ThreeLevels {
  FilterCache cache{64ull << 20, 256};
  std::vector<TableRange> l0, l1, l2;
  std::unique_ptr<LevelIndex> i0, i1, i2;
  std::unique_ptr<RevisionIndex> rev;
  static constexpr uint64_t kKeySpace = 500 * 11 + 2000;
  bool Make() {
    static const int kBpk[3] = {10, 3, 16};
    if (cache.status()) return false;
    if (!MakeLevel(cache, 12, 500, 2000, kBpk, 3, "l0", 5, l0)) return false;
    if (!MakeLevel(cache, 40, 190, 190, kBpk, 1, "l1", -1, l1)) return false;
    if (!MakeLevel(cache, 12, 500, 2000, kBpk + 1, 2, "l2", -1, l2)) return false;
    i0 = std::make_unique<LevelIndex>(l0);
    i1 = std::make_unique<LevelIndex>(l1);
    i2 = std::make_unique<LevelIndex>(l2);
    rev = std::make_unique<RevisionIndex>(std::vector<LevelIndex *>{i0.get(), i1.get(), i2.get()});
    return !rev->status() && rev->table_base().back() == 64;
  }
};

std::vector<std::string> Batch(size_t K, uint64_t seed, const std::vector<TableRange> &l0) {
  std::vector<std::string> q;
  uint64_t s = seed + K;
  for (size_t i = 0; i < K; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t r = s >> 17;
    std::string k = UserKey(r % (ThreeLevels::kKeySpace + 100));
    if (i % 3 == 2) k.back() = '#';                  // absent, inside the ranges
    else if (i % 11 == 10) k.replace(0, 4, "zzzz");  // beyond every table
    else if (i % 7 == 6) {                           // a table's max user key
      const TableRange &t = l0[r % l0.size()];
      k = t.max_inner_key.substr(0, t.max_inner_key.size() - 9);
    }
    q.push_back(std::move(k));
  }
  return q;
}

const int64_t kSeqs[4] = {INT64_MAX, 1999, 2499, 100};

int Check(bool device) {
  setenv("ADL_BLOOM_REVISION_DEVICE_MIN_KEYS", device ? "1" : "0", 1);
  ThreeLevels w;
  if (!w.Make()) return 1;
  int failures = 0;
  size_t hits = 0, groups = 0;
  for (size_t K : {300u, 3000u}) {
    const std::vector<std::string> q = Batch(K, 0x5EED, w.l0);
    std::vector<std::string_view> qv(q.begin(), q.end());
    for (int64_t seq : kSeqs) {
      RevisionMultiGetResult key_major;
      RevisionReadPlan want, got;
      const RC rc_w = RevisionMultiGetFilter(w.cache, *w.rev, qv, seq, key_major);
      GroupHitsByTable(key_major, w.rev->table_base(), want);
      const RC rc_g = RevisionReadPlanFilter(w.cache, *w.rev, qv, seq, got);
      if (rc_w != OK || rc_g != OK || !SamePlan(want, got) || !WellFormed(got, w.rev->table_base(), K)) {
        ++failures;
        fprintf(stderr, "MISMATCH K=%zu seq=%lld: rc %d / %d, hits %zu / %zu, groups %zu / %zu, uncached %llu / %llu\n",
                K, (long long)seq, (int)rc_w, (int)rc_g, want.key.size(), got.key.size(), want.group_table.size(),
                got.group_table.size(), (unsigned long long)want.uncached, (unsigned long long)got.uncached);
      }
      hits += got.key.size();
      groups += got.group_table.size();
    }
  }
  printf("%s: %zu hits, %zu groups, %d mismatches\n", device ? "device" : "host", hits, groups, failures);
  return failures || hits == 0 || groups == 0 ? 1 : 0;
}

int Race() {
  setenv("ADL_BLOOM_REVISION_DEVICE_MIN_KEYS", "1", 1);
  constexpr int kThreads = 4, kRounds = 6;
  ThreeLevels w;
  if (!w.Make()) return 1;
  const size_t kKeys[2] = {3000, 300};
  std::vector<std::string> q[2];
  std::vector<std::string_view> qv[2];
  RevisionReadPlan want[2][4];
  size_t hits = 0;
  for (int b = 0; b < 2; ++b) {
    q[b] = Batch(kKeys[b], 0xACE, w.l0);
    qv[b].assign(q[b].begin(), q[b].end());
    for (int j = 0; j < 4; ++j) {
      if (RevisionReadPlanFilter(w.cache, *w.rev, qv[b], kSeqs[j], want[b][j]) != OK) return 1;
      if (!WellFormed(want[b][j], w.rev->table_base(), kKeys[b])) return 1;
      hits += want[b][j].key.size();
    }
  }
  std::atomic<int> ready{0}, bad{0};
  std::atomic<bool> go{false};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      ++ready;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      for (int r = 0; r < kRounds; ++r) {
        const int b = r & 1, j = (t + r) & 3;
        RevisionReadPlan got;
        const RC rc = RevisionReadPlanFilter(w.cache, *w.rev, qv[b], kSeqs[j], got);
        if (rc != OK || !SamePlan(got, want[b][j])) {
          ++bad;
          fprintf(stderr, "MISMATCH thread %d round %d K=%zu seq=%lld: rc %d, hits %zu / %zu\n", t, r, kKeys[b],
                  (long long)kSeqs[j], (int)rc, got.key.size(), want[b][j].key.size());
        }
      }
    });
  while (ready.load() < kThreads) std::this_thread::yield();
  go.store(true, std::memory_order_release);
  for (std::thread &x : th) x.join();
  printf("%d threads, %d calls each, %zu hits, %d mismatches\n", kThreads, kRounds, hits, bad.load());
  return bad.load() || hits == 0 ? 1 : 0;
}

struct Stat {
  double med, lo, hi;
};

Stat Summary(std::vector<double> &ms) {
  std::sort(ms.begin(), ms.end());
  return Stat{ms[ms.size() / 2], ms.front(), ms.back()};
}

double Ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// One batch against the revision, both ways, interleaved; one JSON line.
int BenchBatch(FilterCache &cache, RevisionIndex &rev, int L, int T, int bottom, uint64_t key_space, size_t keys,
               bool present) {
  std::vector<std::string> q;
  uint64_t s = 11 + keys;
  for (size_t i = 0; i < keys; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    q.push_back(UserKey((s >> 17) % key_space) + (present ? "" : "#"));
  }
  std::vector<std::string_view> qv(q.begin(), q.end());
  RevisionMultiGetResult hits;
  RevisionReadPlan a, b;
  std::vector<double> ms_host, ms_group, ms_plan;
  const int reps = keys > 10000 ? 30 : 200;
  for (int i = 0; i < reps + 5; ++i) {  // interleaved: a drift of the machine meets both alike
    auto t0 = std::chrono::steady_clock::now();
    if (RevisionMultiGetFilter(cache, rev, qv, INT64_MAX, hits) != OK) return 1;
    auto t1 = std::chrono::steady_clock::now();
    GroupHitsByTable(hits, rev.table_base(), a);
    auto t2 = std::chrono::steady_clock::now();
    if (RevisionReadPlanFilter(cache, rev, qv, INT64_MAX, b) != OK) return 1;
    auto t3 = std::chrono::steady_clock::now();
    if (i >= 5) {
      ms_host.push_back(Ms(t0, t2));
      ms_group.push_back(Ms(t1, t2));
      ms_plan.push_back(Ms(t2, t3));
    }
  }
  if (!SamePlan(a, b)) return 1;
  const Stat sh = Summary(ms_host), sg = Summary(ms_group), sp = Summary(ms_plan);
  printf("{\"levels\": %d, \"tables\": %d, \"bottom_tables\": %d, \"num_tables\": %u, \"keys\": %zu, \"batch\": \"%s\", "
         "\"hits\": %zu, \"groups\": %zu, \"multiget_then_host_ms\": %.4f, \"multiget_then_host_min\": %.4f, "
         "\"multiget_then_host_max\": %.4f, \"host_grouping_ms\": %.4f, \"read_plan_ms\": %.4f, "
         "\"read_plan_min\": %.4f, \"read_plan_max\": %.4f}\n",
         L, T, bottom, rev.table_base().back(), keys, present ? "present" : "absent", b.key.size(),
         b.group_table.size(), sh.med, sh.lo, sh.hi, sg.med, sp.med, sp.lo, sp.hi);
  fflush(stdout);
  return 0;
}

int Bench(int L, int T, const std::vector<size_t> &key_counts, int bottom, const std::string &only) {
  g_digits = 9;
  setenv("ADL_BLOOM_REVISION_DEVICE_MIN_KEYS", "1", 1);
  static const int kBpk[1] = {10};
  FilterCache cache(2ull << 30, 1 << 16);
  if (cache.status()) return 1;
  const uint64_t stride = 50000, span = 200000, key_space = stride * (T - 1) + span;
  std::vector<std::vector<TableRange>> tabs(L);
  std::vector<std::unique_ptr<LevelIndex>> idx;
  std::vector<LevelIndex *> lv;
  for (int l = 0; l < L; ++l) {
    const bool cut = bottom && l == L - 1;
    const uint64_t w = cut ? (key_space + bottom - 1) / bottom : 0;
    if (!MakeLevel(cache, cut ? bottom : T, cut ? w : stride, cut ? w : span, kBpk, 1, "L" + std::to_string(l), -1,
                   tabs[l]))
      return 1;
    idx.push_back(std::make_unique<LevelIndex>(tabs[l]));
    if (idx.back()->status()) return 1;
    lv.push_back(idx.back().get());
  }
  RevisionIndex rev(lv);
  if (rev.status()) return 1;
  for (size_t keys : key_counts)
    for (bool present : {false, true}) {
      if (!only.empty() && only != (present ? "present" : "absent")) continue;
      if (int rc = BenchBatch(cache, rev, L, T, bottom, key_space, keys, present)) return rc;
    }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (argc >= 5 && argc <= 7 && mode == "--bench") {
    std::vector<size_t> key_counts;
    for (const char *p = argv[4]; *p;) {
      char *end;
      key_counts.push_back((size_t)strtoull(p, &end, 10));
      if (end == p) return 2;
      p = *end == ',' ? end + 1 : end;
    }
    return Bench(atoi(argv[2]), atoi(argv[3]), key_counts, argc > 5 ? atoi(argv[5]) : 0, argc > 6 ? argv[6] : "");
  }
  if (argc == 2 && mode == "--race") return Race();
  if (argc == 2 && (mode == "device" || mode == "host")) return Check(mode == "device");
  fprintf(stderr, "usage: read_plan_test device | host | --race | --bench <levels> <tables> <keys>[,<keys>...] "
                  "[<bottom_tables> [absent|present]]\n");
  return 2;
}

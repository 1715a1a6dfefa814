// adlsm-tree_amd/csrc/level_index_test.cpp -- level multi-gets over a resident
// LevelIndex against the per-call selection, for tests/.  Needs a GPU.
//
//   level_index_test
//     Three levels -- 12 overlapping tables (bits_per_key 10, 3, 16 in turn, up
//     to four candidates per key, one table not cached), 2 000 disjoint tables,
//     and the 12 overlapping ones beside 200 disjoint tables that no key falls
//     into (the mean region list is far shorter than the batch's lists, so the
//     device path's first buffers are too small and it asks again with the
//     exact size) -- each asked with batches of 300 and of 3 000 keys at three
//     sequence numbers (above every table's max seq, equal to one, below
//     most).  ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS is set to 1 000 unless the
//     environment sets it, so the small batches take the host copy of the
//     index and the large ones the device path.  Every result of
//     LevelMultiGetFilter(cache, index, ...) must equal
//     LevelMultiGetFilter(cache, tables, ...) on the same input: begin,
//     table, maybe and uncached.  Exit 0 = all equal.
//
//   level_index_test --race
//     Eight threads share ONE freshly made LevelIndex (the 12 overlapping
//     tables) and are released together; the first call of each is a 3 000-key
//     batch on the device path, so handle()'s call_once and the upload of the
//     device copy race.  Each thread then alternates 3 000-key and 300-key
//     batches at its own sequence numbers, and every MultiGetFilterResult must
//     equal the one LevelMultiGetFilter(cache, tables, ...) gave on one thread
//     beforehand.  Exit 0 = all equal.
//
//   level_index_test --bench <tables> <stride> <span> <keys>
//     level_fanout_test --bench's level and batch, timed three ways in one
//     process, one after the other: LevelMultiGetFilter(cache, index, ...),
//     LevelMultiGetFilter(cache, tables, ...) (the per-call selection) and
//     LevelCandidates alone (its selection share).  One JSON line; run with
//     ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS=0 / =1 for the host-copy / the device
//     path of the index.
//
//   level_index_test --bench-readpath <keys>
//     The same three timings on readpath_test --bench's level and queries: 16
//     tables, 13-14-byte user keys, about 3.2 candidates per key, every third
//     key absent, every eleventh beyond the level.
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

int g_digits = 12;  // "user" + 12 digits: 16 bytes (--bench-readpath: 9 digits, readpath_test's keys)

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

struct TestLevel {
  std::vector<TableRange> tables;
  uint64_t key_space = 0;
};

// table t holds user keys [base + t stride, base + t stride + span), bits_per_key bpk[t % nb]
bool MakeLevel(FilterCache &cache, int T, uint64_t stride, uint64_t span, const int *bpk, int nb, const char *tag,
               int skip_table, TestLevel &lv, uint64_t base = 0) {
  for (int t = 0; t < T; ++t) {
    FilterBlockWriter w(std::make_unique<BloomFilter>(bpk[t % nb]));
    const uint64_t lo = base + (uint64_t)t * stride, hi = lo + span;
    for (uint64_t i = lo; i < hi; ++i) w.Update(UserKey(i));
    std::string block;
    if (w.Final(block)) return false;
    // max op 1 on every other table: at seq == max seq those are gone at their max key
    lv.tables.push_back(TableRange{std::string(tag) + "-" + std::to_string(t), Inner(UserKey(lo), (int64_t)lo),
                                   Inner(UserKey(hi - 1), (int64_t)hi - 1, (char)(t & 1))});
    if (t != skip_table && cache.Put(lv.tables.back().oid, block)) return false;
  }
  lv.key_space = base + stride * (T - 1) + span;
  return true;
}

double Median(std::vector<double> &ms) {
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

int Bench(int T, uint64_t stride, uint64_t span, size_t keys, bool readpath) {
  if (readpath) g_digits = 9;
  static const int kBpk[1] = {10};
  FilterCache cache(1ull << 30, 4096);
  if (cache.status()) return 1;
  TestLevel lv;
  if (!MakeLevel(cache, T, stride, span, kBpk, 1, "bench", -1, lv)) return 1;
  std::vector<std::string> q;
  uint64_t s = 11 + keys;
  for (size_t i = 0; i < keys; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t r = s >> 17;
    if (readpath && i % 3 == 2) q.push_back(UserKey(r % lv.key_space) + "#");  // absent, inside the ranges
    else if (readpath && i % 11 == 10) q.push_back("zzz" + std::to_string(r));  // beyond every table
    else q.push_back(UserKey(r % lv.key_space));
  }
  std::vector<std::string_view> qv(q.begin(), q.end());
  const auto t_build = std::chrono::steady_clock::now();
  LevelIndex index(lv.tables);
  const double build_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count();
  if (index.status()) return 1;
  MultiGetFilterResult r, ri;
  std::vector<uint32_t> b, tb;
  std::vector<double> ms_tables, ms_sel, ms_index;
  const int reps = keys > 10000 ? 30 : 200;
  // one loop per variant: each runs with its own buffers warm, as a caller's would be
  auto timed = [&](std::vector<double> &ms, auto &&call) {
    for (int i = 0; i < reps + 5; ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      if (!call()) return false;
      if (i >= 5) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    return true;
  };
  if (!timed(ms_index, [&] { return LevelMultiGetFilter(cache, index, qv, INT64_MAX, ri) == OK; })) return 1;
  if (!timed(ms_tables, [&] { return LevelMultiGetFilter(cache, lv.tables, qv, INT64_MAX, r) == OK; })) return 1;
  if (!timed(ms_sel, [&] {
        LevelCandidates(lv.tables, qv, INT64_MAX, b, tb);
        return true;
      }))
    return 1;
  if (r.begin != ri.begin || r.table != ri.table || r.maybe != ri.maybe) return 1;
  const char *e = getenv("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS");
  printf("{\"tables\": %d, \"stride\": %llu, \"span\": %llu, \"keys\": %zu, \"pairs_probed\": %zu, "
         "\"device_min_keys\": \"%s\", \"index_build_ms\": %.4f, \"per_call_tables_ms\": %.4f, "
         "\"level_candidates_ms\": %.4f, \"index_ms\": %.4f}\n",
         T, (unsigned long long)stride, (unsigned long long)span, keys, r.table.size(), e ? e : "default", build_ms,
         Median(ms_tables), Median(ms_sel), Median(ms_index));
  return 0;
}

int failures = 0;

void Compare(const char *what, size_t K, int64_t seq, RC rc_a, const MultiGetFilterResult &a, RC rc_b,
             const MultiGetFilterResult &b) {
  const bool same = rc_a == OK && rc_b == OK && a.begin == b.begin && a.table == b.table && a.maybe == b.maybe &&
                    a.uncached == b.uncached;
  if (!same) {
    ++failures;
    fprintf(stderr, "MISMATCH %s K=%zu seq=%lld: rc %d / %d, pairs %zu / %zu, uncached %llu / %llu\n", what, K,
            (long long)seq, (int)rc_a, (int)rc_b, a.table.size(), b.table.size(), (unsigned long long)a.uncached,
            (unsigned long long)b.uncached);
  }
}

int Check() {
  setenv("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "1000", 0);
  FilterCache cache(64ull << 20, 4096);
  if (cache.status()) return 1;
  static const int kBpk[3] = {10, 3, 16};
  TestLevel overlap, disjoint, skewed;
  if (!MakeLevel(cache, 12, 500, 2000, kBpk, 3, "ovl", 5, overlap)) return 1;
  if (!MakeLevel(cache, 2000, 64, 64, kBpk, 1, "dis", -1, disjoint)) return 1;
  if (!MakeLevel(cache, 200, 64, 64, kBpk, 1, "far", -1, skewed, 1000000)) return 1;
  skewed.tables.insert(skewed.tables.end(), overlap.tables.begin(), overlap.tables.end());
  skewed.key_space = overlap.key_space;  // every key among the overlapping tables
  size_t pairs = 0, hits = 0;
  for (const TestLevel *lv : {&overlap, &disjoint, &skewed}) {
    LevelIndex index(lv->tables);
    if (index.status()) return 1;
    for (size_t K : {300u, 3000u}) {
      std::vector<std::string> q;
      uint64_t s = 0x1EE7 + K;
      for (size_t i = 0; i < K; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t r = s >> 17;
        std::string k = UserKey(r % (lv->key_space + 100));
        if (i % 3 == 2) k.back() = '#';                     // absent, inside the ranges
        else if (i % 11 == 10) k.replace(0, 4, "zzzz");     // beyond every table
        else if (i % 7 == 6) {                              // a table's max user key
          const TableRange &t = lv->tables[r % lv->tables.size()];
          k = t.max_inner_key.substr(0, t.max_inner_key.size() - 9);
        }
        q.push_back(std::move(k));
      }
      std::vector<std::string_view> qv(q.begin(), q.end());
      // table 0's max seq is its span - 1 (op 0), table 1's stride + span - 1 (op 1)
      const int64_t span = lv == &disjoint ? 64 : 2000, stride = lv == &disjoint ? 64 : 500;
      for (int64_t seq : {INT64_MAX, span - 1, stride + span - 1, (int64_t)100}) {
        MultiGetFilterResult want, got;
        const RC rc_w = LevelMultiGetFilter(cache, lv->tables, qv, seq, want);
        const RC rc_g = LevelMultiGetFilter(cache, index, qv, seq, got);
        Compare(lv == &overlap ? "overlapping" : lv == &disjoint ? "disjoint" : "skewed", K, seq, rc_w, want, rc_g, got);
        pairs += want.table.size();
        for (uint8_t m : want.maybe) hits += m;
      }
    }
  }
  printf("%zu pairs, %zu maybe, %d mismatches\n", pairs, hits, failures);
  return failures || pairs == 0 || hits == 0 || hits == pairs ? 1 : 0;
}

// Eight threads whose first call on a shared, never used LevelIndex is the
// device path.
int Race() {
  setenv("ADL_BLOOM_LEVEL_DEVICE_MIN_KEYS", "1000", 0);
  constexpr int kThreads = 8, kRounds = 6;
  FilterCache cache(64ull << 20, 4096);
  if (cache.status()) return 1;
  static const int kBpk[3] = {10, 3, 16};
  TestLevel overlap;
  if (!MakeLevel(cache, 12, 500, 2000, kBpk, 3, "ovl", 5, overlap)) return 1;
  // the batches and what they have to give, made on this thread without an index
  const size_t kKeys[2] = {3000, 300};
  const int64_t kSeqs[4] = {INT64_MAX, 1999, 2499, 100};
  std::vector<std::string> q[2];
  std::vector<std::string_view> qv[2];
  MultiGetFilterResult want[2][4];
  size_t pairs = 0, hits = 0;
  for (int b = 0; b < 2; ++b) {
    uint64_t s = 0xACE + kKeys[b];
    for (size_t i = 0; i < kKeys[b]; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t r = s >> 17;
      std::string k = UserKey(r % (overlap.key_space + 100));
      if (i % 3 == 2) k.back() = '#';
      else if (i % 7 == 6) {
        const TableRange &t = overlap.tables[r % overlap.tables.size()];
        k = t.max_inner_key.substr(0, t.max_inner_key.size() - 9);
      }
      q[b].push_back(std::move(k));
    }
    qv[b].assign(q[b].begin(), q[b].end());
    for (int j = 0; j < 4; ++j) {
      if (LevelMultiGetFilter(cache, overlap.tables, qv[b], kSeqs[j], want[b][j]) != OK) return 1;
      pairs += want[b][j].table.size();
      for (uint8_t m : want[b][j].maybe) hits += m;
    }
  }
  LevelIndex index(overlap.tables);  // no call on it before the threads start
  if (index.status()) return 1;
  std::atomic<int> ready{0}, bad{0};
  std::atomic<bool> go{false};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      ++ready;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      for (int r = 0; r < kRounds; ++r) {
        const int b = r & 1, j = (t + r) & 3;  // round 0: 3 000 keys, the device path
        MultiGetFilterResult got;
        const RC rc = LevelMultiGetFilter(cache, index, qv[b], kSeqs[j], got);
        const MultiGetFilterResult &w = want[b][j];
        if (rc != OK || got.begin != w.begin || got.table != w.table || got.maybe != w.maybe ||
            got.uncached != w.uncached) {
          ++bad;
          fprintf(stderr, "MISMATCH thread %d round %d K=%zu seq=%lld: rc %d, pairs %zu / %zu\n", t, r, kKeys[b],
                  (long long)kSeqs[j], (int)rc, got.table.size(), w.table.size());
        }
      }
    });
  while (ready.load() < kThreads) std::this_thread::yield();
  go.store(true, std::memory_order_release);
  for (std::thread &x : th) x.join();
  printf("%d threads, %d calls each, %zu pairs, %zu maybe, %d mismatches\n", kThreads, kRounds, pairs, hits,
         bad.load());
  return bad.load() || pairs == 0 || hits == 0 || hits == pairs ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 6 && std::string(argv[1]) == "--bench")
    return Bench(atoi(argv[2]), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10),
                 (size_t)strtoull(argv[5], nullptr, 10), false);
  if (argc == 3 && std::string(argv[1]) == "--bench-readpath")
    return Bench(16, 50000, 200000, (size_t)strtoull(argv[2], nullptr, 10), true);
  if (argc == 2 && std::string(argv[1]) == "--race") return Race();
  if (argc != 1) {
    fprintf(stderr,
            "usage: level_index_test | --race | --bench <tables> <stride> <span> <keys> | --bench-readpath <keys>\n");
    return 2;
  }
  return Check();
}

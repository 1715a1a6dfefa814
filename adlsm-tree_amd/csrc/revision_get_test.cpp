// adlsm-tree_amd/csrc/revision_get_test.cpp -- the single-key revision Get
// (RevisionGetFilter: one request to the cache's resident probe server for all
// of a key's candidate tables) against RevisionMultiGetFilter asked about the
// same key alone, for tests/.  Needs a GPU.
//
//   revision_get_test
//     A revision of five levels -- 12 overlapping tables (bits_per_key 10, 3,
//     16 in turn, one table not cached), an empty level, a missing one
//     (nullptr), 2 000 disjoint tables, and 30 tables that overlap up to
//     thirtyfold over the low user keys (a key there has more than
//     ADL_BLOOM_GET_MAX_TABLES candidates, so its Get is a launched probe;
//     the keys above them stay within one server request).  Four threads, each
//     with 400 keys of its own -- present, absent inside the ranges, beyond
//     every table, tables' max user keys, one of 120 bytes -- at four sequence
//     numbers: every RevisionGetFilter result must equal the one-key
//     RevisionMultiGetFilter's (the per-level loop).  Exit 0 = all equal, and
//     Gets of both kinds (served by the resident server, launched) were made.
//
//   revision_get_test --bench <levels> <tables> <key_bytes> <absent|present> [<calls>]
//     <levels> levels of readpath_test --bench's shape (<tables> tables of
//     200 000 user keys each, the tables overlapping fourfold; user keys of
//     <key_bytes> >= 13 bytes).  <calls> (default 2 000) Gets of distinct keys
//     each way -- RevisionGetFilter, and RevisionMultiGetFilter with one key
//     (one server round trip per level, or a launch) -- in blocks of 100 that
//     alternate, in one process.  One JSON line: median and p99 per call of
//     both in us, the candidates per key, and how many of the Gets the
//     resident server answered (adl_bloom_probe_server_phases) and how many
//     server kernels were launched meanwhile.
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

#include "adl_bloom.h"
#include "filter_block.hpp"
#include "level_filter.hpp"

namespace {

using namespace adl;

int g_digits = 12;  // "user" + 12 digits: 16 bytes

std::string UserKey(uint64_t i) {
  char b[160];
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
    // max op 1 on every other table: at seq == max seq those are gone at their max key
    tables.push_back(TableRange{tag + "-" + std::to_string(t), Inner(UserKey(lo), (int64_t)lo),
                                Inner(UserKey(hi - 1), (int64_t)hi - 1, (char)(t & 1))});
    if (t != skip_table && cache.Put(tables.back().oid, block)) return false;
  }
  return true;
}

uint64_t Served() {
  uint64_t n = 0;
  (void)adl_bloom_probe_server_phases(&n, nullptr, nullptr, 0);
  return n;
}

int Check() {
  constexpr int kThreads = 4, kKeys = 400;
  FilterCache cache(64ull << 20, 4096);
  if (cache.status()) return 1;
  static const int kBpk[3] = {10, 3, 16};
  std::vector<TableRange> l0, l3, l4, none;
  if (!MakeLevel(cache, 12, 500, 2000, kBpk, 3, "l0", 5, l0)) return 1;
  if (!MakeLevel(cache, 2000, 4, 4, kBpk, 1, "l3", -1, l3)) return 1;
  if (!MakeLevel(cache, 30, 50, 2000, kBpk + 1, 2, "l4", -1, l4)) return 1;
  LevelIndex i0(l0), i1(none), i3(l3), i4(l4);
  RevisionIndex rev({&i0, &i1, nullptr, &i3, &i4});
  if (rev.status() || rev.table_base().back() != 2042) return 1;
  const uint64_t key_space = 500 * 11 + 2000;
  const int64_t kSeqs[4] = {INT64_MAX, 1999, 2499, 100};  // table 0's max seq is 1999 (op 0), table 1's 2499 (op 1)
  std::atomic<int> bad{0};
  std::atomic<uint64_t> hits{0}, cands{0}, wide{0}, narrow{0};
  const uint64_t served0 = Served();
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      uint64_t s = 0x6E7 + 977 * t;
      RevisionGetResult got;  // kept across the calls
      for (int i = 0; i < kKeys; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t r = s >> 17;
        std::string k = UserKey(r % (key_space + 100));
        if (i % 3 == 2) k.back() = '#';                  // absent, inside the ranges
        else if (i % 11 == 10) k.replace(0, 4, "zzzz");  // beyond every table
        else if (i % 7 == 6) {                           // a table's max user key
          const TableRange &tr = (i % 2 ? l0 : l4)[r % (i % 2 ? l0 : l4).size()];
          k = tr.max_inner_key.substr(0, tr.max_inner_key.size() - 9);
        } else if (i % 13 == 12) k = UserKey(r % 100) + std::string(104, 'x');  // 120 bytes, inside the ranges
        const std::vector<std::string_view> one{k};
        const int64_t seq = kSeqs[(i + t) & 3];
        RevisionMultiGetResult want;
        const RC rc_w = RevisionMultiGetFilter(cache, rev, one, seq, want);
        const RC rc_g = RevisionGetFilter(cache, rev, k, seq, got);
        if (rc_w != OK || rc_g != OK || want.table != got.table || want.level != got.level ||
            want.uncached != got.uncached || got.candidates < got.table.size()) {
          ++bad;
          fprintf(stderr, "MISMATCH thread %d key %d (%zu bytes) seq=%lld: rc %d / %d, hits %zu / %zu, uncached %llu / %u\n",
                  t, i, k.size(), (long long)seq, (int)rc_w, (int)rc_g, want.table.size(), got.table.size(),
                  (unsigned long long)want.uncached, got.uncached);
        }
        hits += got.table.size();
        cands += got.candidates;
        const bool fits = got.candidates <= ADL_BLOOM_GET_MAX_TABLES && k.size() <= ADL_BLOOM_GET_MAX_KEY_BYTES;
        if (got.candidates) ++(fits ? narrow : wide);
      }
    });
  for (std::thread &x : th) x.join();
  const uint64_t served = Served() - served0;
  printf("%d threads, %d keys each, %llu candidates, %llu hits, %llu Gets within one server request, %llu beyond, "
         "%llu requests served, %d mismatches\n",
         kThreads, kKeys, (unsigned long long)cands.load(), (unsigned long long)hits.load(),
         (unsigned long long)narrow.load(), (unsigned long long)wide.load(), (unsigned long long)served, bad.load());
  return bad.load() || hits == 0 || hits == cands || narrow == 0 || wide == 0 || served < narrow ? 1 : 0;
}

double Pct(std::vector<double> &v, double p) {
  std::sort(v.begin(), v.end());
  return v[std::min(v.size() - 1, (size_t)(p * (double)v.size()))];
}

int Bench(int L, int T, int key_bytes, bool present, int calls) {
  if (key_bytes < 13 || key_bytes > 150 || L < 1 || T < 1 || calls < 100) return 2;
  g_digits = key_bytes - 4;
  static const int kBpk[1] = {10};
  FilterCache cache(2ull << 30, 1 << 16);
  if (cache.status()) return 1;
  const uint64_t stride = 50000, span = 200000, key_space = stride * (T - 1) + span;
  std::vector<std::vector<TableRange>> tabs(L);
  std::vector<std::unique_ptr<LevelIndex>> idx;
  std::vector<LevelIndex *> lv;
  for (int l = 0; l < L; ++l) {
    if (!MakeLevel(cache, T, stride, span, kBpk, 1, "L" + std::to_string(l), -1, tabs[l])) return 1;
    idx.push_back(std::make_unique<LevelIndex>(tabs[l]));
    if (idx.back()->status()) return 1;
    lv.push_back(idx.back().get());
  }
  RevisionIndex rev(lv);
  if (rev.status()) return 1;
  std::vector<std::string> q;
  uint64_t s = 11 + calls;
  for (int i = 0; i < calls + 100; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    std::string k = UserKey((s >> 17) % key_space);
    if (!present) k.back() = '#';
    q.push_back(std::move(k));
  }
  RevisionGetResult g;
  RevisionMultiGetResult m;
  std::vector<std::string_view> one(1);
  std::vector<double> us_get, us_loop;
  uint64_t cands = 0, hits = 0, served_get = 0, served_loop = 0, launches0 = 0, launches1 = 0;
  (void)adl_bloom_probe_server_launches(&launches0);
  // blocks of 100 calls, the two ways alternating: a drift of the machine meets both alike
  for (int b = -1; b * 100 < calls; ++b) {  // (block -1: warm-up, not recorded)
    const int i0 = b < 0 ? calls : b * 100;
    const uint64_t s0 = Served();
    for (int i = i0; i < i0 + 100; ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      if (RevisionGetFilter(cache, rev, q[i], INT64_MAX, g) != OK) return 1;
      const auto t1 = std::chrono::steady_clock::now();
      if (b >= 0) us_get.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      if (b >= 0) cands += g.candidates, hits += g.table.size();
    }
    const uint64_t s1 = Served();
    for (int i = i0; i < i0 + 100; ++i) {
      one[0] = q[i];
      const auto t0 = std::chrono::steady_clock::now();
      if (RevisionMultiGetFilter(cache, rev, one, INT64_MAX, m) != OK) return 1;
      const auto t1 = std::chrono::steady_clock::now();
      if (b >= 0) us_loop.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
    }
    if (b >= 0) served_get += s1 - s0, served_loop += Served() - s1;
    // the two ways agree (on the block's last key)
    if (RevisionGetFilter(cache, rev, q[i0 + 99], INT64_MAX, g) != OK || g.table != m.table) return 1;
  }
  (void)adl_bloom_probe_server_launches(&launches1);
  const double gm = Pct(us_get, 0.5), g99 = Pct(us_get, 0.99), lm = Pct(us_loop, 0.5), l99 = Pct(us_loop, 0.99);
  printf("{\"levels\": %d, \"tables\": %d, \"key_bytes\": %d, \"keys\": \"%s\", \"calls\": %zu, "
         "\"candidates_per_key\": %.2f, \"hits_per_key\": %.2f, \"get_us\": %.2f, \"get_p99_us\": %.2f, "
         "\"per_level_us\": %.2f, \"per_level_p99_us\": %.2f, \"get_requests_served\": %llu, "
         "\"per_level_requests_served\": %llu, \"server_launches\": %llu}\n",
         L, T, key_bytes, present ? "present" : "absent", us_get.size(), (double)cands / (double)us_get.size(),
         (double)hits / (double)us_get.size(), gm, g99, lm, l99, (unsigned long long)served_get,
         (unsigned long long)served_loop, (unsigned long long)(launches1 - launches0));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if ((argc == 6 || argc == 7) && std::string(argv[1]) == "--bench") {
    const std::string kind = argv[5];
    if (kind != "absent" && kind != "present") return 2;
    return Bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), kind == "present", argc == 7 ? atoi(argv[6]) : 2000);
  }
  if (argc != 1) {
    fprintf(stderr, "usage: revision_get_test | --bench <levels> <tables> <key_bytes> <absent|present> [<calls>]\n");
    return 2;
  }
  return Check();
}

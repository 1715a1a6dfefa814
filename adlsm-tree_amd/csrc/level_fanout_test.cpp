// adlsm-tree_amd/csrc/level_fanout_test.cpp -- one level multi-get over a small
// level of overlapping tables, for tests/ to check against the oracle.  Needs
// a GPU.
//
//   level_fanout_test <outdir>
//     Builds 12 SSTable filter blocks of 2 000 16-byte user keys each
//     (FilterBlockWriter; table t holds keys [500 t, 500 t + 2000), so up to
//     four tables cover a key; bits_per_key cycles through 10, 3 and 16),
//     caches them in a FilterCache and runs ONE LevelMultiGetFilter over 3 000
//     queries (members, absent keys inside the ranges, keys beyond every
//     table).  LevelMultiGetFilter hands each key over once with its candidate
//     list (FilterCache::ProbeFanout; forced with ADL_BLOOM_LEVEL_FANOUT=2),
//     or, with ADL_BLOOM_LEVEL_FANOUT=0, one query per (key, table) pair: the
//     files written are the same either way.
//     Writes tables.txt, table_<t>.blk, queries.txt and multiget.txt in the
//     formats readpath_test writes.  Exit 0 = the multi-get ran.
//
//   level_fanout_test --bench <tables> <stride> <span> <keys>
//     Median time of a level multi-get of <keys> member keys over <tables>
//     tables, table t holding user keys [t stride, t stride + span): about
//     span / stride candidates per key (stride == span: exactly one).  One
//     JSON line; run with ADL_BLOOM_LEVEL_FANOUT=2 and =0 for the A/B of the
//     two probe paths at a given fan-out.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "filter_block.hpp"
#include "level_filter.hpp"

namespace {

using namespace adl;

std::string UserKey(uint64_t i) {
  char b[32];
  snprintf(b, sizeof(b), "user%012llu", (unsigned long long)i);  // 16 bytes
  return b;
}

std::string Inner(const std::string &user, int64_t seq) {
  std::string k = user;
  k.append(reinterpret_cast<const char *>(&seq), 8);
  k.push_back('\0');  // OP_PUT
  return k;
}

bool WriteFile(const std::string &path, const std::string &data) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
  return fclose(f) == 0 && ok;
}

std::string Hex(const std::string &s) {
  static const char *d = "0123456789abcdef";
  std::string h;
  for (unsigned char c : s) {
    h.push_back(d[c >> 4]);
    h.push_back(d[c & 15]);
  }
  return h;
}

// Median time of one LevelMultiGetFilter over `keys` member keys of a level of
// T tables (bits_per_key 10), table t holding [t * stride, t * stride + span):
// every key has about span / stride candidates (1 when stride == span).
int Bench(int T, uint64_t stride, uint64_t span, size_t keys) {
  std::vector<TableRange> tables;
  FilterCache cache(1ull << 30, 1024);
  if (cache.status()) return 1;
  for (int t = 0; t < T; ++t) {
    FilterBlockWriter w(std::make_unique<BloomFilter>(10));
    const uint64_t lo = (uint64_t)t * stride, hi = lo + span;
    for (uint64_t i = lo; i < hi; ++i) w.Update(UserKey(i));
    std::string block;
    if (w.Final(block)) return 1;
    tables.push_back(TableRange{"bench-" + std::to_string(t), Inner(UserKey(lo), (int64_t)lo),
                                Inner(UserKey(hi - 1), (int64_t)hi - 1)});
    if (cache.Put(tables.back().oid, block)) return 1;
  }
  const uint64_t key_space = stride * (T - 1) + span;
  std::vector<std::string> q;
  uint64_t s = 11 + keys;
  for (size_t i = 0; i < keys; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    q.push_back(UserKey((s >> 17) % key_space));
  }
  std::vector<std::string_view> qv(q.begin(), q.end());
  MultiGetFilterResult r;
  std::vector<double> ms;
  const int reps = keys > 10000 ? 30 : 200;
  for (int i = 0; i < reps + 5; ++i) {
    const auto t0 = std::chrono::steady_clock::now();
    if (LevelMultiGetFilter(cache, tables, qv, INT64_MAX, r)) return 1;
    if (i >= 5) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"tables\": %d, \"stride\": %llu, \"span\": %llu, \"keys\": %zu, \"pairs_probed\": %zu, "
         "\"median_ms\": %.4f, \"p90_ms\": %.4f}\n",
         T, (unsigned long long)stride, (unsigned long long)span, keys, r.table.size(), ms[ms.size() / 2],
         ms[ms.size() * 9 / 10]);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 6 && std::string(argv[1]) == "--bench")
    return Bench(atoi(argv[2]), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10),
                 (size_t)strtoull(argv[5], nullptr, 10));
  if (argc < 2) {
    fprintf(stderr, "usage: level_fanout_test <outdir> | --bench <tables> <stride> <span> <keys>\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int T = 12;
  const uint64_t stride = 500, span = 2000;
  static const int kBpk[3] = {10, 3, 16};
  std::vector<TableRange> tables;
  std::vector<std::string> blocks;
  for (int t = 0; t < T; ++t) {
    FilterBlockWriter w(std::make_unique<BloomFilter>(kBpk[t % 3]));
    const uint64_t lo = (uint64_t)t * stride, hi = lo + span;
    for (uint64_t i = lo; i < hi; ++i) w.Update(UserKey(i));
    std::string block;
    if (RC rc = w.Final(block)) {
      fprintf(stderr, "build failed: %s\n", std::string(strrc(rc)).c_str());
      return 1;
    }
    char oid[80];
    snprintf(oid, sizeof(oid), "%064x", 0xF000 + t);  // stands in for the SHA-256 hex
    tables.push_back(TableRange{oid, Inner(UserKey(lo), (int64_t)lo), Inner(UserKey(hi - 1), (int64_t)hi - 1)});
    blocks.push_back(std::move(block));
  }
  const uint64_t key_space = stride * (T - 1) + span + 200;
  std::vector<std::string> q;
  uint64_t s = 0xFA2007;
  for (size_t i = 0; i < 3000; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t r = s >> 17;
    std::string k = UserKey(r % key_space);
    if (i % 3 == 2) k.back() = '#';  // absent, inside the ranges
    else if (i % 11 == 10) k.replace(0, 4, "zzzz");  // beyond every table
    q.push_back(std::move(k));
  }
  std::vector<std::string_view> qv(q.begin(), q.end());

  FilterCache cache(16ull << 20, 64);
  if (cache.status()) return 1;
  for (int t = 0; t < T; ++t)
    if (RC rc = cache.Put(tables[t].oid, blocks[t])) {
      fprintf(stderr, "put failed: %s\n", std::string(strrc(rc)).c_str());
      return 1;
    }
  MultiGetFilterResult got;
  if (RC rc = LevelMultiGetFilter(cache, tables, qv, INT64_MAX, got); rc || got.uncached) {
    fprintf(stderr, "multi-get failed: %s, %llu uncached\n", std::string(strrc(rc)).c_str(),
            (unsigned long long)got.uncached);
    return 1;
  }
  std::string tables_txt, q_txt, mg_txt;
  for (int t = 0; t < T; ++t) {
    if (!WriteFile(dir + "/table_" + std::to_string(t) + ".blk", blocks[t])) return 1;
    tables_txt += tables[t].oid + " " + Hex(tables[t].min_inner_key) + " " + Hex(tables[t].max_inner_key) + "\n";
  }
  for (const auto &k : q) q_txt += Hex(k) + "\n";
  for (size_t i = 0; i < q.size(); ++i) {
    mg_txt += std::to_string(i);
    for (uint32_t p = got.begin[i]; p < got.begin[i + 1]; ++p)
      mg_txt += " " + std::to_string(got.table[p]) + ":" + std::to_string(got.maybe[p]);
    mg_txt += "\n";
  }
  if (!WriteFile(dir + "/tables.txt", tables_txt) || !WriteFile(dir + "/queries.txt", q_txt) ||
      !WriteFile(dir + "/multiget.txt", mg_txt))
    return 1;
  printf("%d tables, %zu queries, %zu pairs\n", T, q.size(), got.table.size());
  return 0;
}

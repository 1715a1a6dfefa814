// adlsm-tree_amd/csrc/write_through_test.cpp -- SSTableWriter with a filter
// cache (SetFilterCache): the memtable of the reference's test/sstable_test.cpp
// (BuildSSTable :9-27) flushed with the filter block built straight into the
// cache arena and published under the file's oid.  Needs a GPU.
//
//   write_through_test <dir>   prints "oid <hex>" and, when every check held,
//                              "write_through_test: all passed" (exit 0)
//
// Checks: the file and the oid are the same with and without a cache (Final
// and BeginFinal / EndFinal, with and without verification); the table is
// resident right after Final with no Put; a level multi-get over it reports
// nothing uncached and answers as a FilterBlockReader on the block read back
// from the file; a sink failing in Finish and a non-BloomFilter algorithm
// leave the cache alone.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "level_filter.hpp"
#include "sstable_writer.hpp"

namespace {

using namespace adl;

struct Entry {
  std::string user_key;
  int64_t seq;
  int op;
  std::string value;
};

/* MemKey::operator< (src/keys.cpp:61-74) */
bool MemLess(const Entry &a, const Entry &b) {
  const int c = a.user_key.compare(b.user_key);
  if (c) return c < 0;
  if (a.seq != b.seq) return a.seq > b.seq;
  return a.op > b.op;
}

/* MemKey::ToKey (src/keys.cpp:76-84) */
std::string InnerKey(const Entry &e) {
  std::string k = e.user_key;
  k.append(reinterpret_cast<const char *>(&e.seq), 8);
  k.push_back((char)e.op);
  return k;
}

std::vector<Entry> Memtable() {
  std::vector<Entry> v;
  for (int i = 0; i < 10000; ++i) v.push_back({"key" + std::to_string(i), i, 0, "value" + std::to_string(i)});
  std::sort(v.begin(), v.end(), MemLess);
  return v;
}

/* a sink whose rename fails: everything was appended, the file never stands */
class FailingSink : public StringSink {
 public:
  RC Finish(string_view) override { return IO_ERROR; }
};

/* a FilterAlgorithm written against the reference's interface only: one byte
 * per filter, the XOR of its keys' first bytes */
class XorFilter : public FilterAlgorithm {
 public:
  RC Keys2Block(const vector<string> &keys, string &result) override {
    char x = 0;
    for (const auto &k : keys) x ^= k.empty() ? 0 : k[0];
    result.push_back(x);
    return OK;
  }
  bool IsKeyExists(string_view, string_view) override { return true; }
  void FilterInfo(string &info) override { info.append("xr"); }
};

int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

enum Mode { kFinal, kBeginEnd };

/* the memtable through a writer; returns the writer's status */
RC Write(const std::vector<Entry> &mem, SSTableWriter &w, Mode mode, std::string &oid) {
  for (const auto &e : mem)
    if (RC rc = w.Add(InnerKey(e), e.value); rc) return rc;
  unsigned char d[32];
  RC rc = OK;
  if (mode == kFinal) {
    rc = w.Final(d);
  } else {
    if ((rc = w.BeginFinal())) return rc;
    rc = w.EndFinal(d);
  }
  if (rc == OK) oid = Sha256Hex(d);
  return rc;
}

int Load32(const std::string &s, size_t at) {
  int v;
  memcpy(&v, s.data() + at, 4);
  return v;
}

/* the filter block of an SSTable: footer -> meta block, whose one entry
 * "filter" holds the block's handle (src/sstable.cpp:60-75) */
std::string FilterBlockOf(const std::string &file) {
  const size_t foot = file.size() - FooterBlockWriter::footer_size;
  const int meta_off = Load32(file, foot);
  const size_t handle = (size_t)meta_off + 12 + 6;  // shared, non-shared, value length, "filter"
  return file.substr((size_t)Load32(file, handle), (size_t)Load32(file, handle + 4));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dir>\n", argv[0]);
    return 2;
  }
  const auto mem = Memtable();

  // the file as it is written today
  StringSink plain;
  std::string oid0;
  {
    SSTableWriter w(&plain, 10);
    CHECK(Write(mem, w, kFinal, oid0) == OK);
  }
  printf("oid %s\n", oid0.c_str());
  CHECK(oid0.rfind("15c52c56", 0) == 0);

  FilterCache cache(64ull << 20, 64);
  CHECK(cache.status() == OK);
  if (g_failed) return 1;

  // 1. through the cache: the same file, the table resident with no Put
  for (int verify = 0; verify < 2; ++verify)
    for (Mode mode : {kFinal, kBeginEnd}) {
      cache.Remove(oid0);
      const uint64_t used0 = cache.bytes_used();
      StringSink sink;
      SSTableWriter w(&sink, 10);
      w.SetFilterCache(&cache, verify != 0);
      std::string oid;
      CHECK(Write(mem, w, mode, oid) == OK);
      CHECK(oid == oid0);
      CHECK(sink.data() == plain.data());
      CHECK(cache.Contains(oid0));
      CHECK(cache.tables() == 1 && cache.bytes_used() > used0);
    }

  // 2. a level multi-get over that one table against a reader of the block in the file
  {
    std::vector<std::string> users;
    for (const auto &e : mem) users.push_back(e.user_key);
    for (int i = 0; i < 10000; ++i) users.push_back("key5000x" + std::to_string(i));  // strangers inside the range
    std::vector<string_view> views(users.begin(), users.end());
    const std::vector<TableRange> level{{oid0, InnerKey(mem.front()), InnerKey(mem.back())}};
    MultiGetFilterResult res;
    CHECK(LevelMultiGetFilter(cache, level, views, INT64_MAX, res) == OK);
    CHECK(res.uncached == 0);
    const std::string block = FilterBlockOf(plain.data());
    FilterBlockReader reader;
    CHECK(reader.Init(block) == OK);
    KeyArena arena;
    for (const auto &u : users) arena.Add(u);
    std::vector<uint8_t> want;
    CHECK(reader.IsKeysExist(0, arena, want) == OK);
    uint64_t pairs = 0, hits = 0, bad = 0;
    for (size_t i = 0; i + 1 < res.begin.size(); ++i)
      for (uint32_t p = res.begin[i]; p < res.begin[i + 1]; ++p) {
        ++pairs;
        hits += res.maybe[p];
        bad += res.maybe[p] != want[i];
      }
    CHECK(pairs >= 19000);  // every key but the range's ends is a candidate of the table
    CHECK(bad == 0);
    CHECK(hits + 2 >= mem.size() && hits < pairs);
    printf("multi-get: %llu pairs, %llu hits, %llu mismatches, %llu uncached\n", (unsigned long long)pairs,
           (unsigned long long)hits, (unsigned long long)bad, (unsigned long long)res.uncached);
  }

  // 3. the file write fails in Finish: the table is not cached, its range is given back
  for (Mode mode : {kFinal, kBeginEnd}) {
    cache.Remove(oid0);
    const uint64_t used0 = cache.bytes_used();
    FailingSink sink;
    SSTableWriter w(&sink, 10);
    w.SetFilterCache(&cache, true);
    std::string oid;
    CHECK(Write(mem, w, mode, oid) == IO_ERROR);
    CHECK(!cache.Contains(oid0));
    CHECK(cache.tables() == 0 && cache.bytes_used() == used0);
  }

  // 4. a writer dropped between BeginFinal and EndFinal gives its range back too
  {
    const uint64_t used0 = cache.bytes_used();
    {
      StringSink sink;
      SSTableWriter w(&sink, 10);
      w.SetFilterCache(&cache);
      for (const auto &e : mem) CHECK(w.Add(InnerKey(e), e.value) == OK);
      CHECK(w.BeginFinal() == OK);
    }
    CHECK(cache.tables() == 0 && cache.bytes_used() == used0);
  }

  // 5. another FilterAlgorithm: the same file as without a cache, nothing published
  {
    StringSink a, b;
    std::string oid_a, oid_b;
    SSTableWriter wa(&a, std::make_unique<XorFilter>());
    CHECK(Write(mem, wa, kFinal, oid_a) == OK);
    const uint64_t used0 = cache.bytes_used();
    SSTableWriter wb(&b, std::make_unique<XorFilter>());
    wb.SetFilterCache(&cache, true);
    CHECK(Write(mem, wb, kFinal, oid_b) == OK);
    CHECK(oid_a == oid_b && a.data() == b.data() && oid_a != oid0);
    CHECK(!cache.Contains(oid_b) && cache.tables() == 0 && cache.bytes_used() == used0);
  }

  // 6. an arena too small for the block: the ordinary build, the same file, nothing cached
  {
    FilterCache tiny(4096, 4);
    CHECK(tiny.status() == OK);
    StringSink sink;
    SSTableWriter w(&sink, 10);
    w.SetFilterCache(&tiny);
    std::string oid;
    CHECK(Write(mem, w, kFinal, oid) == OK);
    CHECK(oid == oid0 && sink.data() == plain.data());
    CHECK(!tiny.Contains(oid0) && tiny.bytes_used() == 0);
  }

  if (g_failed) {
    fprintf(stderr, "write_through_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("write_through_test: all passed\n");
  return 0;
}

// adlsm-tree_amd/csrc/asan_test.cpp -- host sanitizer run (make asan) over the
// code that parses and frames untrusted bytes, as the reference builds every
// target with -fsanitize=address (CMakeLists.txt:5,13).  Runs on a CPU: no
// path here reaches the device.
//
//   1. The filter-block trailer walk (filter_block_format.hpp, used by
//      FilterBlockReader::Init and the device filter cache): every truncation
//      of valid blocks, every single-byte change of their trailers, and
//      hand-made hostile trailers (offsets past the end, negative and huge
//      counts, info_len 1..len, filters over 2^31 bits), each parsed from a
//      heap buffer of exactly its length, so any read outside it is caught.
//      Malformed blocks also go through FilterBlockReader::Init, which must
//      answer FILTER_BLOCK_ERROR before touching the device.
//   2. A FilterAlgorithm written against the reference's interface
//      (src/filter_block.hpp:13-20: only Keys2Block(vector<string>),
//      IsKeyExists and FilterInfo) driving FilterBlockWriter and
//      SSTableWriter: the block and the SSTable framing (BlockWriter, footer,
//      SHA-256) end to end, and the block read back.
// Exit 0 = all checks passed and the sanitizers reported nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "filter_block.hpp"
#include "level_filter.hpp"
#include "filter_block_format.hpp"
#include "sstable_writer.hpp"

namespace {

using namespace adl;

int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

void Put32(std::string &s, int32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); }

// FilterBlockWriter::Final's layout (src/filter_block.cpp:77-102) around
// arbitrary bitmaps
std::string Frame(const std::vector<std::string> &bitmaps, int32_t bpk) {
  std::string b;
  std::vector<int32_t> off;
  for (const auto &m : bitmaps) {
    off.push_back((int32_t)b.size());
    b += m;
  }
  const int32_t start = (int32_t)b.size();
  for (int32_t o : off) Put32(b, o);
  Put32(b, start);
  Put32(b, (int32_t)off.size());
  b += "bf:";
  Put32(b, bpk);
  Put32(b, 7);
  return b;
}

// parse from a heap copy of exactly len bytes
int ParseExact(const std::string &blk, size_t len, adl_fmt::FilterBlockLayout &lay) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[len ? len : 1]);
  memcpy(buf.get(), blk.data(), len);
  return adl_fmt::parse_filter_block(buf.get(), len, lay);
}

void ReaderRejects(const std::string &blk) {
  std::unique_ptr<char[]> buf(new char[blk.size() ? blk.size() : 1]);
  memcpy(buf.get(), blk.data(), blk.size());
  FilterBlockReader r;
  CHECK(r.Init(std::string_view(buf.get(), blk.size())) == FILTER_BLOCK_ERROR);
  CHECK(!r.IsKeyExists(0, "k"));
}

void ParserChecks() {
  std::vector<std::string> valid = {
      Frame({}, 10),
      Frame({std::string(17, '\x5a')}, 10),
      Frame({std::string(27, '\x01'), std::string(7, '\x00'), std::string(1007, '\xff')}, 10),
      Frame({std::string(7, '\0'), std::string(7, '\0'), std::string(7, '\0'), std::string(7, '\0')}, 0),
  };
  for (const auto &v : valid) {
    adl_fmt::FilterBlockLayout lay;
    CHECK(ParseExact(v, v.size(), lay) == 0);
    CHECK(lay.bits_per_key == 10 || lay.bits_per_key == 0);
    CHECK(lay.off.size() == (size_t)lay.num_filters + 1);
    CHECK(lay.off.back() == (uint64_t)lay.offsets_start);
    // every truncation, from the front and from the back
    for (size_t len = 0; len < v.size(); ++len) {
      ParseExact(v, len, lay);
      std::string tail = v.substr(v.size() - len);
      ParseExact(tail, tail.size(), lay);
    }
    // every single-byte change of the trailer (4F + 19 bytes)
    const size_t trailer = 4 * lay.off.size() + 15;
    for (size_t i = v.size() - std::min(v.size(), trailer); i < v.size(); ++i)
      for (int x : {0x00, 0x01, 0x7f, 0x80, 0xff}) {
        std::string m = v;
        m[i] = (char)x;
        adl_fmt::FilterBlockLayout l2;
        if (ParseExact(m, m.size(), l2) == 0) {
          // accepted: the layout must lie inside the block
          CHECK(l2.offsets_start >= 0 && (uint64_t)l2.offsets_start <= m.size());
          for (size_t f = 0; f + 1 < l2.off.size(); ++f) CHECK(l2.off[f] <= l2.off[f + 1]);
        } else {
          ReaderRejects(m);
        }
      }
  }
  // hostile trailers
  struct Case {
    int32_t start, nf, info_len;
    const char *what;
  } cases[] = {
      {0x7fffffff, 1, 7, "offsets_start past the end"},
      {-4, 1, 7, "negative offsets_start"},
      {0, 0x40000000, 7, "huge filter count"},
      {0, -1, 7, "negative filter count"},
      {0, 1, 0x7ffffff0, "info_len past the front"},
      {0, 1, 0, "zero info_len"},
      {0, 1, 2, "info shorter than bf:<bpk>"},
  };
  for (const auto &c : cases) {
    std::string b(64, '\0');
    Put32(b, c.start);
    Put32(b, c.nf);
    b += "bf:";
    Put32(b, 10);
    Put32(b, c.info_len);
    adl_fmt::FilterBlockLayout lay;
    const int rc = ParseExact(b, b.size(), lay);
    if (rc == 0) fprintf(stderr, "accepted: %s\n", c.what);
    CHECK(rc == adl_fmt::kFilterBlockError);
    ReaderRejects(b);
  }
  // a filter of more than 2^31 bits cannot be probed with the reference's int m
  {
    const std::string b = Frame({std::string((1u << 28) + 1, '\0')}, 10);  // 2^31 + 8 bits
    adl_fmt::FilterBlockLayout lay;
    CHECK(adl_fmt::parse_filter_block(reinterpret_cast<const uint8_t *>(b.data()), b.size(), lay) ==
          adl_fmt::kFilterBlockError);
    const std::string ok = Frame({std::string((1u << 28) - 1, '\0')}, 10);  // 2^31 - 8 bits: accepted
    CHECK(adl_fmt::parse_filter_block(reinterpret_cast<const uint8_t *>(ok.data()), ok.size(), lay) == 0);
  }
  // info_len of every size up to the whole block
  std::string v = Frame({std::string(40, '\x11')}, 10);
  for (int32_t il = -2; il < (int32_t)v.size() + 2; ++il) {
    std::string m = v;
    memcpy(&m[m.size() - 4], &il, 4);
    adl_fmt::FilterBlockLayout lay;
    ParseExact(m, m.size(), lay);
  }
}

// A filter written against the reference's FilterAlgorithm only: one byte
// per key (the key's length), no GPU.  Exercises the default batched
// extensions of the mirror.
class LengthFilter : public FilterAlgorithm {
 public:
  RC Keys2Block(const vector<string> &keys, string &result) override {
    for (const auto &k : keys) result.push_back((char)k.size());
    result.push_back('\x7f');
    return OK;
  }
  bool IsKeyExists(string_view key, string_view bitmap) override {
    return bitmap.find((char)key.size()) != string_view::npos;
  }
  void FilterInfo(string &info) override {
    info.append("bf:");
    Put32(info, 3);
  }
};

void WriterChecks() {
  FilterBlockWriter w(std::make_unique<LengthFilter>());
  for (int f = 0; f < 5; ++f) {
    for (int i = 0; i < 10 * f; ++i) w.Update(std::string(i % 9 + 1, 'k'));
    w.Keys2Block();
  }
  std::string block;
  CHECK(w.Final(block) == OK);
  adl_fmt::FilterBlockLayout lay;
  CHECK(ParseExact(block, block.size(), lay) == 0);
  CHECK(lay.num_filters == 5 && lay.bits_per_key == 3);
  for (int f = 0; f < 5; ++f) CHECK(lay.off[f + 1] - lay.off[f] == (uint64_t)(10 * f + 1));

  // SSTableWriter framing over a memtable-shaped run (sstable.cpp's Add/Final)
  StringSink sink;
  SSTableWriter t(&sink, std::make_unique<LengthFilter>());
  for (int i = 0; i < 5000; ++i) {
    char k[32];
    const int n = snprintf(k, sizeof(k), "key%06d", i);
    std::string inner(k, n);
    const int64_t seq = i;
    inner.append(reinterpret_cast<const char *>(&seq), 8);
    inner.push_back('\0');
    CHECK(t.Add(inner, std::string(i % 300, 'v')) == OK);
  }
  unsigned char sha[32];
  CHECK(t.Final(sha) == OK);
  const std::string &file = sink.data();
  CHECK((int)file.size() == t.GetFileSize());
  CHECK(file.size() > 18 && (unsigned char)file[file.size() - 2] == 0x12 &&
        (unsigned char)file[file.size() - 1] == 0x34);  // footer magic (src/footer_block.cpp:24-25)

  // The streamed writer's host batch (SetStreaming): keys and trimmed packed
  // runs, empty keys and repeats, counted as the ordinary writer counts them.
  // Fewer keys than a flush carries, and no Keys2Block / Final: nothing here
  // reaches the device (a stream allocates nothing before its first append).
  FilterBlockWriter plain(std::make_unique<BloomFilter>(10)), streamed(std::make_unique<BloomFilter>(10));
  CHECK(plain.SetStreaming(false) == OK);
  CHECK(streamed.SetStreaming(true) == OK && streamed.streaming());
  std::string run;
  std::vector<uint64_t> off{0};
  for (int i = 0; i < 300; ++i) {
    run += std::string((i / 3) % 7, (char)('a' + (i / 3) % 5)) + "123456789";  // 9 bytes to trim; runs of 3 equal keys
    off.push_back(run.size());
  }
  for (FilterBlockWriter *fw : {&plain, &streamed}) {
    for (const char *k : {"", "", "a", "a", "b", ""}) CHECK(fw->Update(k) == OK);
    CHECK(fw->UpdateBatch(run.data(), off.data(), 300, 9) == OK);
    CHECK(fw->Update(std::string((299 / 3) % 7, (char)('a' + (299 / 3) % 5))) == OK);  // equals the run's last key
  }
  CHECK(streamed.adjacent_duplicates() == plain.adjacent_duplicates() && plain.adjacent_duplicates() >= 200);
  CHECK(streamed.SetStreaming(false) == BAD_RECORD);  // keys are pending
}

// The level index builder and its host lookup (level_index_core.hpp through
// LevelIndex and LevelCandidates): empty levels, empty and repeated keys,
// tables whose max sorts before their min, inner keys without a suffix, a
// budget that refuses the index.  Every lookup equals TableCoversKey on every
// table, in LevelCandidates' order.
void LevelIndexChecks() {
  auto inner = [](const std::string &user, int64_t seq, char op) {
    std::string k = user;
    k.append(reinterpret_cast<const char *>(&seq), 8);
    k.push_back(op);
    return k;
  };
  const std::vector<std::string> users = {"", "a", "ab", std::string("ab\0", 3), "b", std::string(40, 'p'),
                                          std::string(40, 'p') + "\x80", "\x7f\x10", "\x80\x01", "\xff"};
  uint64_t s = 0x5A17;
  auto rnd = [&](uint64_t n) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (s >> 33) % n;
  };
  for (int round = 0; round < 40; ++round) {
    std::vector<TableRange> tabs(round == 0 ? 0 : 1 + rnd(12));
    for (auto &t : tabs) {
      const std::string &a = users[rnd(users.size())], &b = users[rnd(users.size())];
      t.oid = "t";
      t.min_inner_key = rnd(5) ? inner(a, (int64_t)rnd(4), (char)rnd(2)) : a.substr(0, 8);
      t.max_inner_key = rnd(5) ? inner(b, (int64_t)rnd(4), (char)rnd(2)) : b.substr(0, 8);
    }
    LevelIndex index(tabs);
    CHECK(index.status() == OK);
    std::vector<std::string> keys(users);
    keys.push_back(std::string(300, 'z'));
    keys.push_back("a" + std::string(1, '\0'));
    std::vector<std::string_view> kv(keys.begin(), keys.end());
    for (int64_t seq : {(int64_t)0, (int64_t)2, INT64_MAX}) {
      std::vector<uint32_t> b1, t1, b2, t2;
      index.Candidates(kv, seq, b1, t1);
      LevelCandidates(tabs, kv, seq, b2, t2);
      CHECK(b1 == b2 && t1 == t2);
      for (size_t i = 0; i < kv.size(); ++i) {
        size_t covered = 0;
        for (const auto &t : tabs) covered += TableCoversKey(t, kv[i], seq);
        CHECK(b1[i + 1] - b1[i] == covered);
      }
    }
  }
  // 64 mutually overlapping tables: a 4 KiB budget refuses the index
  std::vector<TableRange> wide(64);
  for (int t = 0; t < 64; ++t) {
    wide[t].min_inner_key = inner("u" + std::to_string(100 + t), 1, 0);
    wide[t].max_inner_key = inner("v" + std::to_string(100 + t), 1, 0);
  }
  CHECK(LevelIndex(wide, 4096).status() == OUT_OF_RANGE);
  CHECK(LevelIndex(wide).status() == OK && LevelIndex(wide).longest_list() == 64);
  // A revision's host lookup: the levels' lists back to back as global ids; a
  // missing and a table-less level are skipped; nine levels are refused.
  std::vector<TableRange> one(1), none;
  one[0].min_inner_key = inner("u120", 1, 0);
  one[0].max_inner_key = inner("v101", 1, 0);
  LevelIndex lw(wide), l1(one), l0(none);
  RevisionIndex rev({&l1, nullptr, &l0, &lw, &l1});
  CHECK(rev.status() == OK && rev.longest_list() == 66);
  CHECK((rev.table_base() == std::vector<uint32_t>{0, 1, 1, 1, 65, 66}));
  const std::vector<std::string> keys = {"u130", "", "v100", "zz"};
  const std::vector<std::string_view> kv(keys.begin(), keys.end());
  std::vector<uint32_t> b, t, bw, tw, b1, t1;
  rev.Candidates(kv, INT64_MAX, b, t);
  lw.Candidates(kv, INT64_MAX, bw, tw);
  l1.Candidates(kv, INT64_MAX, b1, t1);
  CHECK(b.size() == 5 && b[4] == t.size() && t.size() == tw.size() + 2 * t1.size());
  // (four keys on `wide`: its lists outgrow 4 x 64 range tests, so LevelCandidates scans the tables directly)
  std::vector<uint32_t> bd, td;
  LevelCandidates(wide, kv, INT64_MAX, bd, td);
  CHECK(bd == bw && td == tw);
  for (size_t i = 0; i < kv.size(); ++i) {
    std::vector<uint32_t> want(t1.begin() + b1[i], t1.begin() + b1[i + 1]);
    for (uint32_t p = bw[i]; p < bw[i + 1]; ++p) want.push_back(1 + tw[p]);
    for (uint32_t p = b1[i]; p < b1[i + 1]; ++p) want.push_back(65 + t1[p]);
    CHECK(want == std::vector<uint32_t>(t.begin() + b[i], t.begin() + b[i + 1]));
  }
  CHECK(b[1] - b[0] == 33 && b[2] == b[1]);  // "u130": tables u100..u130 of `wide`, and `one` twice
  CHECK(RevisionIndex(std::vector<LevelIndex *>(9, &l1)).status() == BAD_REVISION);
}

}  // namespace

int main() {
  ParserChecks();
  WriterChecks();
  LevelIndexChecks();
  printf("asan_test: %d failed checks\n", g_fail);
  return g_fail ? 1 : 0;
}

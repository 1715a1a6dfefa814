// adlsm-tree_amd/csrc/test_memtables.hpp -- the memtables of the reference's
// test/sstable_test.cpp (BuildSSTable :9-27, BuildSSTable2 :29-43) and one with
// several versions per user key, in memtable order, for the test binaries
// (sstable_test.cpp, stream_build_test.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace {

struct Entry {
  std::string user_key;
  int64_t seq;
  int op;  // OP_PUT = 0, OP_DELETE = 1 (src/keys.hpp:10-13)
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

std::vector<Entry> Memtable(int which) {
  std::vector<Entry> v;
  if (which == 3) {
    // 1-5 versions of each of 4 000 user keys (puts and deletes): in memtable
    // order a user key's versions are adjacent filter keys
    int64_t seq = 0;
    for (int j = 0; j < 4000; ++j)
      for (int r = 0; r <= (j * 7) % 5; ++r, ++seq)
        v.push_back({"user" + std::to_string(j), seq, seq % 3 == 2 ? 1 : 0, "v" + std::to_string(seq)});
  }
  for (int i = 0; which != 3 && i < 10000; ++i) {
    if (which == 1)
      v.push_back({"key" + std::to_string(i), i, 0, "value" + std::to_string(i)});
    else
      v.push_back({"key" + std::to_string(i / 2), i, i % 2 ? 1 : 0, "value" + std::to_string(i / 2)});
  }
  std::sort(v.begin(), v.end(), MemLess);
  return v;
}

}  // namespace

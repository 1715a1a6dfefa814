// oracle/ref_filter_block_harness.cpp -- TEST INFRASTRUCTURE ONLY.
// C-ABI shim over the reference's own, unmodified src/filter_block.cpp
// (BloomFilter, FilterBlockWriter, FilterBlockReader), compiled in place with
// src/murmur3_hash.cpp and src/encode.cpp by oracle/Makefile into
// oracle/_ref/libref_filter_block.so.  The reference's headers come in by
// include path; <spdlog/...> resolves to oracle/spdlog_stand_in (a logger
// that discards everything).  src/monitor_logger.cpp is not compiled, so the
// two MonitorLogger members filter_block.cpp needs are defined here.
//
// The reference's reader trusts the block: for some malformed trailers it
// reads outside it, and for an empty filter range it divides by zero.  The
// reader entry points below work on a private copy of the block with 64 zero
// bytes on both sides, and answer kRefOutside / kRefDivZero instead of calling
// into the reference where it would do either.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "filter_block.hpp"    // reference src/filter_block.hpp
#include "monitor_logger.hpp"  // reference src/monitor_logger.hpp

namespace adl {
MonitorLogger::MonitorLogger() : logger(std::make_shared<spdlog::logger>("ref")) {}
MonitorLogger &MonitorLogger::Logger() {
  static MonitorLogger l;
  return l;
}
}  // namespace adl

namespace {

constexpr int kRefOutside = -1;  // the reference would read outside the block
constexpr int kRefDivZero = -2;  // the reference would compute h % 0 (an empty bitmap)
constexpr size_t kSlack = 64;

inline std::string_view key_at(const char *keys, const uint64_t *offsets, uint64_t i) {
  return {keys + offsets[i], (size_t)(offsets[i + 1] - offsets[i])};
}

inline int32_t rd32(const std::string &buf, int64_t at) {  // at: offset in the block
  int32_t v;
  memcpy(&v, buf.data() + kSlack + at, 4);
  return v;
}

// A reader over a private, padded copy of the block.
struct Reader {
  std::string buf;
  int64_t len = 0;
  adl::FilterBlockReader r;
  int rc = kRefOutside;
  int32_t nf = 0, offsets_start = 0;

  Reader(const char *block, uint64_t n) : buf(kSlack, '\0'), len((int64_t)n) {
    buf.append(block, n);
    buf.append(kSlack, '\0');
    // The one unbounded read of Init (src/filter_block.cpp:143): walk the
    // trailer as Init does up to there.  Where an earlier check of Init's
    // fails, Init returns before that read and is safe to call.
    bool reaches = false;
    if (len >= 4) {
      const int64_t info_len_off = len - 4;
      const int32_t info_len = rd32(buf, info_len_off);
      if (!(info_len > info_len_off || info_len <= 0)) {
        const int64_t info_off = info_len_off - info_len;
        const bool bf = buf[kSlack + info_off] == 'b' && (info_len < 2 || buf[kSlack + info_off + 1] == 'f');
        if (bf && info_len >= 2 && info_off >= 4 && info_off - 4 >= 4) {
          nf = rd32(buf, info_off - 4);
          offsets_start = rd32(buf, info_off - 8);
          reaches = offsets_start >= 0;  // (negative: Init returns at :139)
        }
      }
    }
    if (reaches && (int64_t)offsets_start + 4 > len) return;  // rc = kRefOutside
    rc = (int)r.Init(std::string_view(buf.data() + kSlack, (size_t)len));
  }

  // 0/1, kRefOutside or kRefDivZero; only after rc == OK
  int exists(int32_t id, std::string_view key) {
    if (id < 0) return kRefOutside;  // filters_offsets_[negative]
    if (id < nf) {
      // the reads of src/filter_block.cpp:175-180 and the range :183
      const int64_t a = (int64_t)offsets_start + 4ll * id;
      if (a + 4 > len) return kRefOutside;
      const int64_t o1 = rd32(buf, a);
      int64_t o2 = offsets_start;
      if (id + 1 != nf) {
        if (a + 8 > len) return kRefOutside;
        o2 = rd32(buf, a + 4);
      }
      if (o1 < 0 || o2 > len || o1 > o2) return kRefOutside;
      if (o1 == o2) return kRefDivZero;
    }
    return r.IsKeyExists(id, key) ? 1 : 0;
  }
};

}  // namespace

extern "C" {

int ref_code_outside(void) { return kRefOutside; }
int ref_code_div_zero(void) { return kRefDivZero; }

// BloomFilter(bpk).Keys2Block over keys [offsets[i], offsets[i+1]); the bitmap's length, or -1 when it exceeds cap
int64_t ref_keys2block(int bpk, const char *keys, const uint64_t *offsets, uint64_t n, char *out, uint64_t cap) {
  std::vector<std::string> v;
  v.reserve(n);
  for (uint64_t i = 0; i < n; i++) v.emplace_back(key_at(keys, offsets, i));
  std::string result;
  adl::BloomFilter(bpk).Keys2Block(v, result);
  if (result.size() > cap) return -1;
  memcpy(out, result.data(), result.size());
  return (int64_t)result.size();
}

int ref_is_key_exists(int bpk, const char *key, uint64_t len, const char *bitmap, uint64_t bytes) {
  if (bytes == 0) return kRefDivZero;
  return adl::BloomFilter(bpk).IsKeyExists({key, (size_t)len}, {bitmap, (size_t)bytes}) ? 1 : 0;
}

int ref_is_key_exists_batch(int bpk, const char *keys, const uint64_t *offsets, uint64_t n, const char *bitmap,
                            uint64_t bytes, uint8_t *out) {
  if (bytes == 0) return kRefDivZero;
  adl::BloomFilter bf(bpk);
  for (uint64_t i = 0; i < n; i++) out[i] = bf.IsKeyExists(key_at(keys, offsets, i), {bitmap, (size_t)bytes}) ? 1 : 0;
  return 0;
}

// FilterBlockWriter driven as the reference's SSTableWriter and test/filter_block_test.cpp drive it:
// Update per key, Keys2Block() at each filter boundary (a filter of zero keys too), then Final.
int64_t ref_filter_block_build(int bpk, const char *keys, const uint64_t *offsets, const uint64_t *filter_key_counts,
                               uint32_t F, char *out, uint64_t cap) {
  adl::FilterBlockWriter w(std::make_unique<adl::BloomFilter>(bpk));
  uint64_t i = 0;
  for (uint32_t f = 0; f < F; f++) {
    for (uint64_t e = i + filter_key_counts[f]; i < e; i++) w.Update(key_at(keys, offsets, i));
    w.Keys2Block();
  }
  std::string result;
  w.Final(result);
  if (result.size() > cap) return -1;
  memcpy(out, result.data(), result.size());
  return (int64_t)result.size();
}

// FilterBlockReader::Init's RC, or kRefOutside
int ref_reader_init(const char *block, uint64_t len) { return Reader(block, len).rc; }

// 0/1; kRefOutside / kRefDivZero; 1000 + RC when Init fails
int ref_reader_is_key_exists(const char *block, uint64_t len, int32_t filter_id, const char *key, uint64_t key_len) {
  Reader rd(block, len);
  if (rd.rc == kRefOutside) return kRefOutside;
  if (rd.rc != 0) return 1000 + rd.rc;
  return rd.exists(filter_id, {key, (size_t)key_len});
}

// The same for query i = (filter_ids[i], key i) with one Init; out[i] as above.  Returns Init's RC or kRefOutside.
int ref_reader_is_key_exists_batch(const char *block, uint64_t len, const int32_t *filter_ids, const char *keys,
                                   const uint64_t *offsets, uint64_t n, int8_t *out) {
  Reader rd(block, len);
  if (rd.rc != 0) return rd.rc;
  for (uint64_t i = 0; i < n; i++) out[i] = (int8_t)rd.exists(filter_ids[i], key_at(keys, offsets, i));
  return 0;
}

}  // extern "C"

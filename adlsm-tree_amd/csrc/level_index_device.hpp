// adlsm-tree_amd/csrc/level_index_device.hpp -- the device pieces the level
// kernels (level_index.hip) and the revision kernels (revision_index.hip)
// share: a level's device view, the key view, the 16-byte prefix, the boundary
// comparison, the search of a key's region and its candidate count at `seq`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "level_index_core.hpp"

namespace adl_level_dev {

using adl_level::kGoneAtMaxFlag;
using adl_level::kTableMask;

constexpr int kBlockL = 256;              // as the fan-out probe's workgroups
constexpr uint32_t kLdsBoundaries = 512;  // boundary prefixes staged in LDS up to this many (8 KiB)

struct LevelDev {
  const uint64_t *pref;   // NB x (hi, lo)
  const uint8_t *bbytes;
  const uint32_t *boff;   // NB + 1
  const uint32_t *rbeg;   // 2 NB + 2
  const uint32_t *rlist;
  const int64_t *mx_seq;
  const uint8_t *mx_op;
  uint32_t nb;
};

struct KeySet {
  const uint8_t *keys;
  const uint64_t *offs;  // null: fixed stride
  uint32_t stride;
  __device__ __forceinline__ const uint8_t *at(uint64_t i, uint32_t &len) const {
    if (offs) {
      const uint64_t o0 = offs[i];
      len = (uint32_t)(offs[i + 1] - o0);
      return keys + o0;
    }
    len = stride;
    return keys + i * stride;
  }
};

// The first 16 bytes, zero padded, as two big-endian words.  Byte loads (any
// alignment), and UNSIGNED bytes: the order is memcmp's.
__device__ __forceinline__ void prefix_of(const uint8_t *__restrict__ p, uint32_t len, uint64_t &hi, uint64_t &lo) {
  hi = lo = 0;
  const uint32_t n = len < 16 ? len : 16;
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t b = p[j];
    if (j < 8) hi |= b << (56 - 8 * j);
    else lo |= b << (56 - 8 * (j - 8));
  }
}

// boundary i against the key (memcmp order, then length): < 0, 0, > 0.  Equal
// padded prefixes say only that the first min(16, both lengths) bytes agree
// ("ab" and "ab\0" tie), so a tie goes on to the bytes after them and then to
// the lengths.
__device__ __forceinline__ int boundary_cmp(const LevelDev &lv, uint32_t i, uint64_t bhi, uint64_t blo,
                                            const uint8_t *__restrict__ key, uint32_t klen, uint64_t khi,
                                            uint64_t klo) {
  if (bhi != khi) return bhi < khi ? -1 : 1;
  if (blo != klo) return blo < klo ? -1 : 1;
  const uint32_t b0 = lv.boff[i], blen = lv.boff[i + 1] - b0;
  const uint32_t n = blen < klen ? blen : klen;
  const uint8_t *__restrict__ b = lv.bbytes + b0;
  for (uint32_t j = n < 16 ? n : 16; j < n; ++j) {
    const uint32_t x = b[j], y = key[j];
    if (x != y) return x < y ? -1 : 1;
  }
  return blen == klen ? 0 : (blen < klen ? -1 : 1);
}

__device__ __forceinline__ bool entry_gone(const LevelDev &lv, uint32_t e, int64_t seq) {
  if (!(e & kGoneAtMaxFlag)) return false;
  const uint32_t t = e & kTableMask;
  const int64_t ms = lv.mx_seq[t];
  return ms > seq || (ms == seq && lv.mx_op[t] > 0);
}

// The region of a key: the lower bound among the boundaries (the first that is
// not < key), 2 lo for the gap before it, 2 lo + 1 when the key equals it.
// lds_pref: the level's prefixes are staged in spref (nb <= kLdsBoundaries).
__device__ __forceinline__ uint32_t locate_region(const LevelDev &lv, const uint64_t *spref, bool lds_pref,
                                                  const uint8_t *__restrict__ key, uint32_t klen, uint64_t khi,
                                                  uint64_t klo) {
  uint32_t lo = 0, n = lv.nb;
  while (n) {
    const uint32_t h = n >> 1, m = lo + h;
    const uint64_t bhi = lds_pref ? spref[2 * m] : lv.pref[2 * m];
    const uint64_t blo = lds_pref ? spref[2 * m + 1] : lv.pref[2 * m + 1];
    if (boundary_cmp(lv, m, bhi, blo, key, klen, khi, klo) < 0) {
      lo = m + 1;
      n -= h + 1;
    } else {
      n = h;
    }
  }
  uint32_t r = 2 * lo;
  if (lo < lv.nb) {
    const uint64_t bhi = lds_pref ? spref[2 * lo] : lv.pref[2 * lo];
    const uint64_t blo = lds_pref ? spref[2 * lo + 1] : lv.pref[2 * lo + 1];
    if (boundary_cmp(lv, lo, bhi, blo, key, klen, khi, klo) == 0) r = 2 * lo + 1;
  }
  return r;
}

// The candidates region r lists at `seq`.
__device__ __forceinline__ uint32_t region_count(const LevelDev &lv, uint32_t r, int64_t seq) {
  const uint32_t l0 = lv.rbeg[r], l1 = lv.rbeg[r + 1];
  uint32_t cnt = l1 - l0;
  if (r & 1)  // only a point region lists tables at their own max user key
    for (uint32_t p = l0; p < l1; ++p) cnt -= entry_gone(lv, lv.rlist[p], seq);
  return cnt;
}

}  // namespace adl_level_dev

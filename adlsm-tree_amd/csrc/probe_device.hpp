// adlsm-tree_amd/csrc/probe_device.hpp -- the device pieces every direct
// probe kernel shares (bloom_probe.hip's probe kernels, cache_build.hip's
// verify kernel): the bit reads of one query, the per-filter divisor table in
// LDS and the lookup of a filter's range, divisor and probe count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bloom_common.hpp"

namespace adl_dev {

constexpr int kBlockP = 256;

constexpr uint32_t kLdsFilters = 4096;   // per-filter divisor table kept in LDS up to this many

// The k bitmap reads of one query, one at a time with the reference's stop at
// the first clear bit (src/filter_block.cpp:54-59).  Issuing 2-8 reads per
// round (so they overlap) measured slower: the probe is bound by random HBM
// reads, so the fewest reads win.
__device__ __forceinline__ uint8_t probe_bits(const uint8_t *__restrict__ bm, uint32_t h1, uint32_t h2,
                                              uint32_t k, const FastMod &mod) {
  for (uint32_t j = 0; j < k; ++j) {
    const uint32_t p = fastmod(h1 + j * h2, mod);
    if (!((bm[p >> 3] >> (p & 7)) & 1u)) return 0;
  }
  return 1;
}

// Each filter has its own divisor m = 8 * bitmap bytes, and -- when kf is
// given -- its own probe count kf[f] (blocks written with different
// bits_per_key: the reference reads bpk per block, src/filter_block.cpp:158-170).
// The magic-multiply constants and k of up to kLdsFilters filters are built
// once per workgroup into LDS (dynamic, 8 B per filter), beyond that per query.
struct ModLds {
  uint32_t magic, shift_k;  // shift | k << 8
};

// The workgroup's share of building the table (nf <= kLdsFilters); a barrier
// must follow before filter_lookup reads it.
__device__ __forceinline__ void mod_table_fill(ModLds *lmod, uint32_t nf, uint32_t k,
                                               const uint8_t *__restrict__ kf,
                                               const uint64_t *__restrict__ boff,
                                               const uint64_t *__restrict__ bend) {
  for (uint32_t f = threadIdx.x; f < nf; f += kBlockP) {
    // an empty range (m = 0: a filter the table does not have) and a filter
    // of 2^31 bits or more answer 0 below and need no divisor
    const uint64_t bytes = (bend ? bend[f] : boff[f + 1]) - boff[f];
    const uint32_t m = bytes <= 0x0fffffffull ? (uint32_t)(bytes * 8) : 0u;
    const FastMod fm = m ? fastmod_for(m) : FastMod{};
    lmod[f] = ModLds{fm.magic, fm.shift | (kf ? (uint32_t)kf[f] : k) << 8};
  }
}

// Filter f's bitmap start, divisor and probe count.  false: the query answers
// 0 (f >= nf, an empty filter, or one of 2^31 bits or more, outside the
// reference's int m, src/filter_block.cpp:50).
__device__ __forceinline__ bool filter_lookup(uint32_t f, uint32_t nf, bool lds_tab, const ModLds *lmod, uint32_t k,
                                              const uint8_t *__restrict__ kf, const uint64_t *__restrict__ boff,
                                              const uint64_t *__restrict__ bend, uint64_t &b0, FastMod &mod,
                                              uint32_t &kq) {
  if (f >= nf) return false;
  b0 = boff[f];
  const uint64_t b1 = bend ? bend[f] : boff[f + 1];
  const uint32_t m = b1 - b0 <= 0x0fffffffull ? (uint32_t)((b1 - b0) * 8) : 0u;
  if (m == 0) return false;
  if (lds_tab) {
    const ModLds e = lmod[f];
    mod = FastMod{m, e.magic, e.shift_k & 0xFFu, 0u};
    kq = e.shift_k >> 8;
  } else {
    mod = fastmod_for(m);
    kq = kf ? (uint32_t)kf[f] : k;
  }
  return true;
}

}  // namespace adl_dev

namespace adl_host {

// Grid-stride launches: enough workgroups to cover n, at most blocks_per_cu
// per CU (the multi-filter probe amortises a per-workgroup table over many
// queries, so it asks for a persistent-sized grid).
inline uint32_t grid_for(uint64_t n, int block, uint32_t blocks_per_cu = 64) {
  return (uint32_t)std::max<uint64_t>(
      1, std::min<uint64_t>((n + block - 1) / block, (uint64_t)device_cus() * blocks_per_cu));
}

template <class F>
int dispatch_keys(const uint8_t *d_keys, const uint64_t *d_offsets, uint32_t key_stride, F &&fn) {
  if (d_offsets) return fn(adl_dev::KeysVar{d_keys, d_offsets});
  if (key_stride == 16 && reinterpret_cast<uintptr_t>(d_keys) % 16 == 0)
    return fn(adl_dev::Keys16{reinterpret_cast<const uint4 *>(d_keys)});
  return fn(adl_dev::KeysStride{d_keys, key_stride});
}

}  // namespace adl_host

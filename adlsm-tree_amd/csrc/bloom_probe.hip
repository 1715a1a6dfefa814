// adlsm-tree_amd/csrc/bloom_probe.hip -- MI355X (gfx950) batched bloom probe,
// batched murmur3 and the device-side synthetic key generators.
//
// Probe replaces BloomFilter::IsKeyExists (reference src/filter_block.cpp:49-62)
// for a batch: m = bitmap_bytes*8 (:50), the same h1 + j*h2 positions as the
// build, "absent" at the first clear bit (:54-59).  One query per lane; the key
// load is coalesced, the k bitmap reads are random byte loads that stop at the
// first clear bit (the same early exit as the reference), issued a few at a
// time so that independent reads overlap.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "bloom_common.hpp"
#include "level_index_impl.hpp"
#include "probe_device.hpp"

using namespace adl_dev;
using adl_host::dispatch_keys;
using adl_host::grid_for;

namespace {

// (probe_bits, the per-filter divisor table and filter_lookup: probe_device.hpp)

template <class Keys>
__global__ __launch_bounds__(kBlockP) void bloom_probe_kernel(Keys keys, uint64_t n, uint32_t k,
                                                              FastMod mod,
                                                              const uint8_t *__restrict__ bitmap,
                                                              uint8_t *__restrict__ out) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlockP + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlockP) {
    uint32_t h1, h2;
    keys.hash(i, h1, h2);
    out[i] = probe_bits(bitmap, h1, h2, k, mod);
  }
}

// Multi-filter probe: query i against filter fid[i] (or uniform_f).  Each
// filter has its own divisor m = 8 * bitmap bytes, and -- when kf is given --
// its own probe count kf[f] (blocks written with different bits_per_key: the
// reference reads bpk per block, src/filter_block.cpp:158-170).  The
// magic-multiply constants and k of up to kLdsFilters filters are built once
// per workgroup into LDS (dynamic, 8 B per filter), beyond that per query
// (mod_table_fill / filter_lookup, probe_device.hpp).
template <class Keys>
__global__ __launch_bounds__(kBlockP) void bloom_probe_multi_kernel(
    Keys keys, uint64_t n, uint32_t k, const uint8_t *__restrict__ kf, const uint32_t *__restrict__ fid,
    uint32_t uniform_f, uint32_t nf, const uint8_t *__restrict__ bitmaps, const uint64_t *__restrict__ boff,
    const uint64_t *__restrict__ bend, uint8_t *__restrict__ out) {
  // filter f = bitmaps[boff[f], bend[f]), or [boff[f], boff[f+1]) when bend is null
  extern __shared__ ModLds lmod[];
  const bool lds_tab = nf <= kLdsFilters;
  if (lds_tab) {
    mod_table_fill(lmod, nf, k, kf, boff, bend);
    __syncthreads();
  }
  for (uint64_t i = blockIdx.x * (uint64_t)kBlockP + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlockP) {
    const uint32_t f = fid ? fid[i] : uniform_f;  // fid == nullptr: every query -> uniform_f
    uint8_t hit = 0;
    uint64_t b0;
    FastMod mod;
    uint32_t kq;
    if (filter_lookup(f, nf, lds_tab, lmod, k, kf, boff, bend, b0, mod, kq)) {
      uint32_t h1, h2;
      keys.hash(i, h1, h2);
      hit = probe_bits(bitmaps + b0, h1, h2, kq, mod);
    }
    out[i] = hit;
  }
}

// Fan-out probe: key i against each filter of its own list, pair_filter
// [pair_begin[i], pair_begin[i+1]) (CSR, pair_begin[0] = 0), out[p] per pair in
// pair order -- Level::Get's shape (src/revision.cpp:265-310: one lookup key,
// every table of the level whose range covers it).  The hash pair of a key is
// the same for all its filters (only m, k and the bitmap differ), so a
// workgroup takes 256 keys at a time, lane t hashes key kb+t ONCE into LDS,
// and the lanes then stride over the block's pairs, one pair per lane per
// round whatever the fan-out of single keys is: pair_filter loads and out
// stores are coalesced, and a key with 700 candidates is spread over the
// workgroup instead of serialising one lane.  The owner of pair p is found by
// an upper-bound search of the block's begin entries in LDS (8 steps); keys
// without candidates are never hashed and never found.  Every answer equals
// bloom_probe_multi_kernel's on the expanded pairs (the same table, lookup and
// bit reads).  np bounds the pair ids should pair_begin hold anything larger.
template <class Keys>
__global__ __launch_bounds__(kBlockP) void bloom_probe_fanout_kernel(
    Keys keys, uint64_t nkeys, const uint32_t *__restrict__ pair_begin, const uint32_t *__restrict__ pair_filter,
    uint32_t np, uint32_t k, const uint8_t *__restrict__ kf, uint32_t nf, const uint8_t *__restrict__ bitmaps,
    const uint64_t *__restrict__ boff, const uint64_t *__restrict__ bend, uint8_t *__restrict__ out) {
  extern __shared__ ModLds lmod[];
  __shared__ uint32_t sh1[kBlockP], sh2[kBlockP], spb[kBlockP + 1];
  const bool lds_tab = nf <= kLdsFilters;
  if (lds_tab) mod_table_fill(lmod, nf, k, kf, boff, bend);  // (the first barrier below covers it)
  const uint32_t t = threadIdx.x;
  const uint64_t nblk = (nkeys + kBlockP - 1) / kBlockP;
  for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t kb = blk * kBlockP;
    const uint32_t nk = (uint32_t)(nkeys - kb < (uint64_t)kBlockP ? nkeys - kb : (uint64_t)kBlockP);
    if (t < nk) {
      const uint32_t b = pair_begin[kb + t], e = pair_begin[kb + t + 1];
      spb[t] = b;
      if (t == nk - 1) spb[nk] = e;
      // (hashing every key, so that the key loads need not wait for the begin
      // entries, measured the same on 1 000-key batches)
      if (e > b) {
        uint32_t h1, h2;
        keys.hash(kb + t, h1, h2);
        sh1[t] = h1;
        sh2[t] = h2;
      }
    }
    __syncthreads();
    const uint32_t p1 = spb[nk] < np ? spb[nk] : np;
    for (uint64_t p = (uint64_t)spb[0] + t; p < p1; p += kBlockP) {
      // the first j in [1, nk] with spb[j] > p (spb[nk] > p): key j - 1 owns p
      uint32_t lo = 1, hi = nk;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (spb[mid] > (uint32_t)p) hi = mid; else lo = mid + 1;
      }
      uint8_t hit = 0;
      uint64_t b0;
      FastMod mod;
      uint32_t kq;
      if (filter_lookup(pair_filter[p], nf, lds_tab, lmod, k, kf, boff, bend, b0, mod, kq))
        hit = probe_bits(bitmaps + b0, sh1[lo - 1], sh2[lo - 1], kq, mod);
      out[p] = hit;
    }
    __syncthreads();  // the next block of keys reuses sh1 / sh2 / spb
  }
}

// The fan-out probe that also counts: the same 256 keys per workgroup, hashes
// in LDS and lanes striding over the block's pairs, but the answer bytes go to
// scratch (ans[p]) and what comes out is hits[i], the number of pairs of key i
// answered 1 (counted in LDS), and one hit total per block of keys.  Every
// answer is bloom_probe_fanout_kernel's.  (A kernel of its own, not a flag on
// that one: the answer path of the level multi-get keeps its code and its
// registers as measured.)
template <class Keys>
__global__ __launch_bounds__(kBlockP) void bloom_probe_fanout_count_kernel(
    Keys keys, uint64_t nkeys, const uint32_t *__restrict__ pair_begin, const uint32_t *__restrict__ pair_filter,
    uint32_t np, uint32_t k, const uint8_t *__restrict__ kf, uint32_t nf, const uint8_t *__restrict__ bitmaps,
    const uint64_t *__restrict__ boff, const uint64_t *__restrict__ bend, uint8_t *__restrict__ ans,
    uint32_t *__restrict__ hits, uint64_t *__restrict__ block_total) {
  extern __shared__ ModLds lmod[];
  __shared__ uint32_t sh1[kBlockP], sh2[kBlockP], spb[kBlockP + 1], shits[kBlockP];
  __shared__ uint32_t scratch[kBlockP / kWave + 1];
  const bool lds_tab = nf <= kLdsFilters;
  if (lds_tab) mod_table_fill(lmod, nf, k, kf, boff, bend);  // (the first barrier below covers it)
  const uint32_t t = threadIdx.x;
  const uint64_t nblk = (nkeys + kBlockP - 1) / kBlockP;
  for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t kb = blk * kBlockP;
    const uint32_t nk = (uint32_t)(nkeys - kb < (uint64_t)kBlockP ? nkeys - kb : (uint64_t)kBlockP);
    shits[t] = 0;
    if (t < nk) {
      const uint32_t b = pair_begin[kb + t], e = pair_begin[kb + t + 1];
      spb[t] = b;
      if (t == nk - 1) spb[nk] = e;
      if (e > b) {
        uint32_t h1, h2;
        keys.hash(kb + t, h1, h2);
        sh1[t] = h1;
        sh2[t] = h2;
      }
    }
    __syncthreads();
    const uint32_t p1 = spb[nk] < np ? spb[nk] : np;
    for (uint64_t p = (uint64_t)spb[0] + t; p < p1; p += kBlockP) {
      // the first j in [1, nk] with spb[j] > p (spb[nk] > p): key j - 1 owns p
      uint32_t lo = 1, hi = nk;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (spb[mid] > (uint32_t)p) hi = mid; else lo = mid + 1;
      }
      uint8_t hit = 0;
      uint64_t b0;
      FastMod mod;
      uint32_t kq;
      if (filter_lookup(pair_filter[p], nf, lds_tab, lmod, k, kf, boff, bend, b0, mod, kq))
        hit = probe_bits(bitmaps + b0, sh1[lo - 1], sh2[lo - 1], kq, mod);
      ans[p] = hit;
      if (hit) atomicAdd(&shits[lo - 1], 1u);  // (LDS, within the workgroup: a count, no order hangs on it)
    }
    __syncthreads();
    const uint32_t mine = t < nk ? shits[t] : 0u;
    if (t < nk) hits[kb + t] = mine;
    uint32_t total;
    (void)block_excl_scan<kBlockP>(mine, scratch, &total);  // (its barriers: sh1 / sh2 / spb / shits are free again)
    if (t == 0) block_total[blk] = total;
  }
}

// Workgroup b owns the pairs of keys [256 b, 256 b + 256): hit_begin of its
// keys from their hit counts and the block's offset, then a stable stream
// compaction of its pairs in rounds of 256 -- a lane per pair, the hit flags
// scanned over the workgroup (block_excl_scan: wave scans, no atomic), so the
// hits keep pair order.  Entries at hit_capacity and beyond are not written.
__global__ __launch_bounds__(kBlockP) void fanout_compact_kernel(
    uint64_t nkeys, const uint32_t *__restrict__ pair_begin, const uint32_t *__restrict__ pair_filter, uint32_t np,
    const uint8_t *__restrict__ ans, const uint32_t *__restrict__ hits, const uint64_t *__restrict__ block_off,
    uint32_t *__restrict__ hit_begin, uint32_t *__restrict__ hit_filter, uint64_t hit_capacity) {
  __shared__ uint32_t scratch[kBlockP / kWave + 1];
  const uint32_t t = threadIdx.x;
  const uint64_t kb = blockIdx.x * (uint64_t)kBlockP;
  const uint64_t i = kb + t;
  const uint32_t nk = (uint32_t)(nkeys - kb < (uint64_t)kBlockP ? nkeys - kb : (uint64_t)kBlockP);
  const uint32_t cnt = i < nkeys ? hits[i] : 0u;
  uint32_t btotal;
  const uint32_t excl = block_excl_scan<kBlockP>(cnt, scratch, &btotal);
  const uint64_t base = block_off[blockIdx.x];
  if (i < nkeys) {
    hit_begin[i] = (uint32_t)(base + excl);
    if (i == nkeys - 1) hit_begin[nkeys] = (uint32_t)(base + excl + cnt);
  }
  if (btotal == 0) return;  // (uniform)
  const uint32_t pe = pair_begin[kb + nk];
  const uint64_t p0 = pair_begin[kb], p1 = pe < np ? pe : np;
  uint64_t w = base;
  for (uint64_t r = p0; r < p1; r += kBlockP) {
    const uint64_t p = r + t;
    const bool hit = p < p1 && ans[p];
    uint32_t rtotal;
    const uint32_t at = block_excl_scan<kBlockP>(hit ? 1u : 0u, scratch, &rtotal);
    if (hit && w + at < hit_capacity) hit_filter[w + at] = pair_filter[p];
    w += rtotal;
  }
}

template <class Keys>
__global__ __launch_bounds__(kBlockP) void murmur3_batch_kernel(Keys keys, uint64_t n,
                                                                uint32_t *__restrict__ out) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlockP + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlockP) {
    uint32_t a, b;
    keys.hash(i, a, b);
    out[2 * i] = a;
    out[2 * i + 1] = b;
  }
}

// Arbitrary seeds (the key views hash with the filter's two seeds).
__global__ __launch_bounds__(kBlockP) void murmur3_seeded_kernel(const uint8_t *__restrict__ keys,
                                                                 const uint64_t *__restrict__ offs,
                                                                 uint32_t stride, uint64_t n,
                                                                 uint32_t sa, uint32_t sb,
                                                                 uint32_t *__restrict__ out) {
  for (uint64_t i = blockIdx.x * (uint64_t)kBlockP + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlockP) {
    const uint64_t o0 = offs ? offs[i] : i * stride;
    const uint32_t len = offs ? (uint32_t)(offs[i + 1] - o0) : stride;
    uint32_t a, b;
    hash_bytes(keys + o0, len, sa, sb, a, b);
    out[2 * i] = a;
    out[2 * i + 1] = b;
  }
}

// ---------------------------------------------------------------- synthetic data
__device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t call /* 1-based */) {
  uint64_t z = seed + call * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void synth_keys16_kernel(uint4 *__restrict__ out, uint64_t seed,
                                                           uint64_t skip, uint64_t n) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t c = 2 * (skip + i);
    const uint64_t a = splitmix_at(seed, c + 1), b = splitmix_at(seed, c + 2);
    out[i] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  }
}

__global__ __launch_bounds__(256) void synth_probe_kernel(uint4 *__restrict__ keys, uint32_t *__restrict__ fid,
                                                          uint8_t *__restrict__ member, uint64_t seed, uint64_t q0,
                                                          uint64_t n, uint32_t tables, uint64_t tseed0,
                                                          uint64_t per_table) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t c = 4 * (q0 + i);
    const uint64_t r0 = splitmix_at(seed, c + 1), r1 = splitmix_at(seed, c + 2);
    const uint32_t t = (uint32_t)(r0 % tables);
    uint64_t a, b;
    const bool ins = (r1 & 1) && per_table;
    if (ins) {
      const uint64_t j = (r1 >> 1) % per_table;
      a = splitmix_at(tseed0 + t, 2 * j + 1);
      b = splitmix_at(tseed0 + t, 2 * j + 2);
    } else {
      a = splitmix_at(seed, c + 3);
      b = splitmix_at(seed, c + 4);
    }
    keys[i] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    fid[i] = t;
    if (member) member[i] = ins;
  }
}

constexpr int kZipfR = 249;  // lengths 8 .. 256

// Inverse-CDF table of Zipf(s) on [1, kZipfR] in 53-bit fixed point: r is the
// first rank with x < thr[r-1], x = a SplitMix64 output >> 11.  Built on the
// host (zipf_table), so the device and the oracle's restatement
// (oracle_synth_varlen_lengths) draw identical lengths from the same stream.
struct ZipfTable {
  uint64_t thr[kZipfR];
};

__global__ __launch_bounds__(256) void synth_lengths_kernel(uint32_t *__restrict__ len, uint64_t seed,
                                                            uint64_t n, ZipfTable zt) {
  const uint64_t lseed = seed ^ 0xD1B54A32D192ED03ull;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t x = splitmix_at(lseed, i + 1) >> 11;
    int lo = 0, hi = kZipfR - 1;  // first r with x < thr[r]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (x < zt.thr[mid]) hi = mid; else lo = mid + 1;
    }
    len[i] = 8u + (uint32_t)lo;
  }
}

// cdf(r) = sum_{i<=r} i^-s / sum_{i<=R} i^-s in double; thr = ceil(cdf * 2^53),
// so x < thr  <=>  x * 2^-53 < cdf  for every 53-bit integer x
ZipfTable zipf_table(double s) {
  ZipfTable z{};
  double cdf[kZipfR], acc = 0;
  for (int r = 1; r <= kZipfR; ++r) {
    acc += pow((double)r, -s);
    cdf[r - 1] = acc;
  }
  for (int r = 0; r < kZipfR; ++r) z.thr[r] = (uint64_t)ceil(cdf[r] / acc * 9007199254740992.0);
  return z;
}

__global__ __launch_bounds__(256) void synth_fill_kernel(uint64_t *__restrict__ out, uint64_t seed,
                                                         uint64_t words) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256)
    out[i] = splitmix_at(seed, i + 1);
}

}  // namespace

extern "C" {

int adl_bloom_probe_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                           uint32_t key_stride, int32_t bits_per_key, const uint8_t *d_bitmap,
                           uint64_t bitmap_bytes, uint8_t *d_out, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_bitmap || !d_out || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  if (!d_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  if (bitmap_bytes == 0) return ADL_ERR_INVALID_ARG;  // h % 0 is undefined in the reference
  if (bitmap_bytes * 8 > 0x7fffffffull) return ADL_ERR_TOO_LARGE;
  const uint32_t k = (uint32_t)adl_host::num_probes(bits_per_key);
  const FastMod mod = adl_host::make_fastmod((uint32_t)(bitmap_bytes * 8));
  hipStream_t st = (hipStream_t)stream;
  return dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
    hipLaunchKernelGGL(bloom_probe_kernel<decltype(keys)>, dim3(grid_for(n, kBlockP)), dim3(kBlockP), 0,
                       st, keys, n, k, mod, d_bitmap, d_out);
    ADL_HIP_TRY(hipGetLastError());
    return ADL_OK;
  });
}

}  // extern "C"

namespace {
// fid == nullptr sends every query to filter `uniform_f`.
int probe_multi(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                const uint32_t *d_filter_id, uint32_t uniform_f, uint32_t num_filters,
                const uint8_t *d_bitmaps, const uint64_t *d_bitmap_off, int32_t bits_per_key,
                uint8_t *d_out, hipStream_t st, const uint64_t *d_bitmap_end = nullptr,
                hipEvent_t done = nullptr, const uint8_t *d_k = nullptr) {
  if (num_filters && (!d_bitmaps || !d_bitmap_off)) return ADL_ERR_INVALID_ARG;
  if (!d_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  const uint32_t k = (uint32_t)adl_host::num_probes(bits_per_key);
  return dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
    const size_t lds = num_filters <= kLdsFilters ? (size_t)num_filters * sizeof(ModLds) : 0;
    // `done` rides on the dispatch packet itself (no marker packet after it)
    hipExtLaunchKernelGGL(bloom_probe_multi_kernel<decltype(keys)>, dim3(grid_for(n, kBlockP, 8)),
                          dim3(kBlockP), lds, st, nullptr, done, 0, keys, n, k, d_k, d_filter_id,
                          uniform_f, num_filters, d_bitmaps, d_bitmap_off, d_bitmap_end, d_out);
    ADL_HIP_TRY(hipGetLastError());
    return ADL_OK;
  });
}
// One workgroup per 256 keys, at most 8 per CU (the rest by grid stride).
int probe_fanout(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys, uint32_t key_stride,
                 const uint32_t *d_pair_begin, const uint32_t *d_pair_filter, uint64_t num_pairs,
                 uint32_t num_filters, const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                 int32_t bits_per_key, const uint8_t *d_k, uint8_t *d_out, hipStream_t st, hipEvent_t done) {
  if (num_keys == 0 || num_pairs == 0) return ADL_OK;
  if (!d_keys || !d_pair_begin || !d_pair_filter || !d_out || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  if (num_filters && (!d_bitmaps || !d_begin)) return ADL_ERR_INVALID_ARG;
  if (!d_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  if (num_pairs > 0xffffffffull) return ADL_ERR_TOO_LARGE;  // pair_begin is u32
  const uint32_t k = (uint32_t)adl_host::num_probes(bits_per_key);
  return dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
    const size_t lds = num_filters <= kLdsFilters ? (size_t)num_filters * sizeof(ModLds) : 0;
    hipExtLaunchKernelGGL(bloom_probe_fanout_kernel<decltype(keys)>, dim3(grid_for(num_keys, kBlockP, 8)),
                          dim3(kBlockP), lds, st, nullptr, done, 0, keys, num_keys, d_pair_begin, d_pair_filter,
                          (uint32_t)num_pairs, k, d_k, num_filters, d_bitmaps, d_begin, d_end, d_out);
    ADL_HIP_TRY(hipGetLastError());
    return ADL_OK;
  });
}
uint64_t hits_ws_layout(uint64_t num_keys, uint64_t num_pairs, uint64_t &o_hits, uint64_t &o_btot, uint64_t &o_boff) {
  const uint64_t nblk = (num_keys + kBlockP - 1) / kBlockP;
  o_hits = adl_host::round_up(num_pairs, 256);  // after the answer bytes
  o_btot = o_hits + adl_host::round_up(num_keys * 4, 256);
  o_boff = o_btot + adl_host::round_up(nblk * 8, 256);
  return o_boff + adl_host::round_up(nblk * 8, 256) + 256;
}
}  // namespace

// Probe + hit count, the scan of the block totals, the compaction: three
// launches whatever the batch holds.
int adl_host::probe_fanout_hits_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                       uint32_t key_stride, const uint32_t *d_pair_begin,
                                       const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
                                       const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                                       int32_t bits_per_key, const uint8_t *d_k, uint32_t *d_hit_begin,
                                       uint32_t *d_hit_filter, uint64_t hit_capacity, uint64_t *d_num_hits,
                                       void *d_workspace, uint64_t workspace_bytes, hipStream_t st) {
  if (!d_hit_begin || !d_num_hits) return ADL_ERR_INVALID_ARG;
  if (num_keys >= 0xffffffffull || num_pairs > 0xffffffffull) return ADL_ERR_TOO_LARGE;  // the begin arrays are u32
  if (num_keys == 0 || num_pairs == 0) {
    ADL_HIP_TRY(hipMemsetAsync(d_hit_begin, 0, (num_keys + 1) * 4, st));
    ADL_HIP_TRY(hipMemsetAsync(d_num_hits, 0, 8, st));
    return ADL_OK;
  }
  if (!d_keys || !d_pair_begin || !d_pair_filter || bits_per_key < 0 || !d_workspace) return ADL_ERR_INVALID_ARG;
  if (hit_capacity && !d_hit_filter) return ADL_ERR_INVALID_ARG;
  if (num_filters && (!d_bitmaps || !d_begin)) return ADL_ERR_INVALID_ARG;
  if (!d_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(d_workspace) % 256) return ADL_ERR_INVALID_ARG;
  uint64_t o_hits, o_btot, o_boff;
  if (workspace_bytes < hits_ws_layout(num_keys, num_pairs, o_hits, o_btot, o_boff)) return ADL_ERR_WORKSPACE;
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  uint8_t *ans = ws;
  uint32_t *hits = reinterpret_cast<uint32_t *>(ws + o_hits);
  uint64_t *btot = reinterpret_cast<uint64_t *>(ws + o_btot), *boff = reinterpret_cast<uint64_t *>(ws + o_boff);
  const uint64_t nblk = (num_keys + kBlockP - 1) / kBlockP;
  const uint32_t k = (uint32_t)adl_host::num_probes(bits_per_key);
  int rc = dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
    const size_t lds = num_filters <= kLdsFilters ? (size_t)num_filters * sizeof(ModLds) : 0;
    hipLaunchKernelGGL(bloom_probe_fanout_count_kernel<decltype(keys)>, dim3(grid_for(num_keys, kBlockP, 8)),
                       dim3(kBlockP), lds, st, keys, num_keys, d_pair_begin, d_pair_filter, (uint32_t)num_pairs, k,
                       d_k, num_filters, d_bitmaps, d_begin, d_end, ans, hits, btot);
    ADL_HIP_TRY(hipGetLastError());
    return ADL_OK;
  });
  if (rc) return rc;
  if ((rc = adl_host::level_scan_launch(btot, nblk, boff, d_num_hits, st))) return rc;
  hipLaunchKernelGGL(fanout_compact_kernel, dim3((uint32_t)nblk), dim3(kBlockP), 0, st, num_keys, d_pair_begin,
                     d_pair_filter, (uint32_t)num_pairs, ans, hits, boff, d_hit_begin, d_hit_filter, hit_capacity);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

extern "C" uint64_t adl_bloom_probe_fanout_hits_workspace_bytes(uint64_t num_keys, uint64_t num_pairs) {
  uint64_t a, b, c;
  return hits_ws_layout(num_keys, num_pairs, a, b, c);
}

extern "C" int adl_bloom_probe_fanout_hits_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                                  uint32_t key_stride, const uint32_t *d_pair_begin,
                                                  const uint32_t *d_pair_filter, uint64_t num_pairs,
                                                  uint32_t num_filters, const uint8_t *d_bitmaps,
                                                  const uint64_t *d_begin, const uint64_t *d_end,
                                                  int32_t bits_per_key, uint32_t *d_hit_begin,
                                                  uint32_t *d_hit_filter, uint64_t hit_capacity,
                                                  uint64_t *d_num_hits, void *d_workspace, uint64_t workspace_bytes,
                                                  void *stream) {
  return adl_host::probe_fanout_hits_device(d_keys, d_offsets, num_keys, key_stride, d_pair_begin, d_pair_filter,
                                            num_pairs, num_filters, d_bitmaps, d_begin, d_end, bits_per_key, nullptr,
                                            d_hit_begin, d_hit_filter, hit_capacity, d_num_hits, d_workspace,
                                            workspace_bytes, (hipStream_t)stream);
}

// adl_bloom_probe_fanout_device with a probe count per filter (d_k[f]), whose
// launch also completes `done` (the filter cache, as adl_probe_ranges_device_ev).
int adl_host::adl_probe_fanout_device_ev(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                         uint32_t key_stride, const uint32_t *d_pair_begin,
                                         const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
                                         const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                                         const uint8_t *d_k, uint8_t *d_out, hipStream_t st, hipEvent_t done) {
  if (num_keys && num_pairs && num_filters && !d_k) return ADL_ERR_INVALID_ARG;
  return probe_fanout(d_keys, d_offsets, num_keys, key_stride, d_pair_begin, d_pair_filter, num_pairs, num_filters,
                      d_bitmaps, d_begin, d_end, 10, d_k, d_out, st, done);
}

extern "C" int adl_bloom_probe_fanout_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                                             uint32_t key_stride, const uint32_t *d_pair_begin,
                                             const uint32_t *d_pair_filter, uint64_t num_pairs,
                                             uint32_t num_filters, const uint8_t *d_bitmaps,
                                             const uint64_t *d_begin, const uint64_t *d_end, int32_t bits_per_key,
                                             uint8_t *d_out, void *stream) {
  return probe_fanout(d_keys, d_offsets, num_keys, key_stride, d_pair_begin, d_pair_filter, num_pairs, num_filters,
                      d_bitmaps, d_begin, d_end, bits_per_key, nullptr, d_out, (hipStream_t)stream, nullptr);
}

// adl_bloom_probe_ranges_device with a probe count per filter (d_k[f]), whose
// launch also completes `done` (the filter cache's small batches wait on it;
// see filter_cache.hip).
int adl_host::adl_probe_ranges_device_ev(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                               const uint32_t *d_filter_id, uint32_t num_filters, const uint8_t *d_bitmaps,
                               const uint64_t *d_begin, const uint64_t *d_end, const uint8_t *d_k, uint8_t *d_out,
                               hipStream_t st, hipEvent_t done) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_filter_id || !d_out || (num_filters && !d_k)) return ADL_ERR_INVALID_ARG;
  if (num_filters && !d_end) return ADL_ERR_INVALID_ARG;
  return probe_multi(d_keys, d_offsets, n, key_stride, d_filter_id, 0, num_filters, d_bitmaps, d_begin, 10, d_out,
                     st, d_end, done, d_k);
}

// The direct kernel with a probe count per filter over offsets (d_end null)
// or ranges: what a batch of adl_bloom_probe_batch_k_device that does not take
// the binned pipeline runs.
int adl_host::adl_probe_multi_k_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                       uint32_t key_stride, const uint32_t *d_filter_id, uint32_t num_filters,
                                       const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
                                       const uint8_t *d_k, uint8_t *d_out, hipStream_t st) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_filter_id || !d_out || (num_filters && !d_k)) return ADL_ERR_INVALID_ARG;
  return probe_multi(d_keys, d_offsets, n, key_stride, d_filter_id, 0, num_filters, d_bitmaps, d_begin, 10, d_out,
                     st, d_end, nullptr, d_k);
}

extern "C" int adl_bloom_probe_ranges_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                             uint32_t key_stride, const uint32_t *d_filter_id,
                                             uint32_t num_filters, const uint8_t *d_bitmaps,
                                             const uint64_t *d_begin, const uint64_t *d_end,
                                             int32_t bits_per_key, uint8_t *d_out, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_filter_id || !d_out || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  if (num_filters && !d_end) return ADL_ERR_INVALID_ARG;
  return probe_multi(d_keys, d_offsets, n, key_stride, d_filter_id, 0, num_filters, d_bitmaps, d_begin,
                     bits_per_key, d_out, (hipStream_t)stream, d_end);
}

namespace {

// The end of a staged host-pointer probe whose launch returned rc: its n
// answers come from sg.dev + o_out through the front of the host buffer (the
// upload is done with it) to h_out.  The stream is idle on return.
int fetch_answers(adl_host::Staging &sg, uint64_t o_out, uint64_t n, hipStream_t st, int rc, uint8_t *h_out) {
  if (rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (hipMemcpyAsync(sg.host, sg.dev + o_out, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return ADL_ERR_DEVICE;
  memcpy(h_out, sg.host, n);
  return ADL_OK;
}

}  // namespace

extern "C" {

int adl_bloom_probe_multi_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                 uint32_t key_stride, const uint32_t *d_filter_id,
                                 uint32_t num_filters, const uint8_t *d_bitmaps,
                                 const uint64_t *d_bitmap_off, int32_t bits_per_key,
                                 uint8_t *d_out, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_filter_id || !d_out || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  return probe_multi(d_keys, d_offsets, n, key_stride, d_filter_id, 0, num_filters, d_bitmaps,
                     d_bitmap_off, bits_per_key, d_out, (hipStream_t)stream);
}

int adl_bloom_probe(const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                    uint32_t key_stride, int32_t bits_per_key, const uint8_t *h_bitmap,
                    uint64_t bitmap_bytes, uint8_t *h_out, void *stream) {
  if (n == 0) return ADL_OK;
  if (!h_keys || !h_bitmap || !h_out) return ADL_ERR_INVALID_ARG;
  if (!h_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  hipStream_t st = adl_host::sync_stream(stream);
  adl_host::StagePlan plan;
  const adl_host::KeyBlock kb(plan, h_offsets, n, key_stride);
  const uint64_t o_bm = plan.take(bitmap_bytes);
  const uint64_t o_out = plan.take(n);  // the end of the upload
  adl_host::Staging &sg = adl_host::t_stage;
  int rc = sg.reserve(o_out, plan.end);
  if (rc) return rc;
  kb.fill(sg.host, h_keys, h_offsets);
  memcpy(sg.host + o_bm, h_bitmap, bitmap_bytes);
  if (hipMemcpyAsync(sg.dev, sg.host, o_out, hipMemcpyHostToDevice, st) != hipSuccess) return ADL_ERR_DEVICE;
  rc = adl_bloom_probe_device(sg.dev, kb.offsets(sg.dev), n, key_stride, bits_per_key, sg.dev + o_bm, bitmap_bytes,
                              sg.dev + o_out, st);
  return fetch_answers(sg, o_out, n, st, rc, h_out);
}

int adl_bloom_murmur3_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                             uint32_t key_stride, uint32_t seed_a, uint32_t seed_b,
                             uint32_t *d_out, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_out || (!d_offsets && key_stride == 0)) return ADL_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (seed_a == kSeed1 && seed_b == kSeed2) {
    return dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
      hipLaunchKernelGGL(murmur3_batch_kernel<decltype(keys)>, dim3(grid_for(n, kBlockP)),
                         dim3(kBlockP), 0, st, keys, n, d_out);
      ADL_HIP_TRY(hipGetLastError());
      return ADL_OK;
    });
  }
  hipLaunchKernelGGL(murmur3_seeded_kernel, dim3(grid_for(n, kBlockP)), dim3(kBlockP), 0, st, d_keys,
                     d_offsets, key_stride, n, seed_a, seed_b, d_out);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

int adl_bloom_murmur3(uint32_t seed, const void *data, uint64_t len, uint32_t *h_out) {
  if (!h_out || (len && !data) || len > 0xffffffffull) return ADL_ERR_INVALID_ARG;
  const uint64_t o_out = adl_host::round_up(len + 16, 256);
  adl_host::Staging &sg = adl_host::t_stage;
  int rc = sg.reserve(o_out + 16, o_out + 16);
  if (rc) return rc;
  if (len) memcpy(sg.host, data, len);
  hipStream_t st = adl_host::sync_stream(nullptr);
  if (len && hipMemcpyAsync(sg.dev, sg.host, len, hipMemcpyHostToDevice, st) != hipSuccess) return ADL_ERR_DEVICE;
  hipLaunchKernelGGL(murmur3_seeded_kernel, dim3(1), dim3(kBlockP), 0, st, sg.dev, (const uint64_t *)nullptr,
                     (uint32_t)len, 1ull, seed, seed, reinterpret_cast<uint32_t *>(sg.dev + o_out));
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(sg.host + o_out, sg.dev + o_out, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return ADL_ERR_DEVICE;
  memcpy(h_out, sg.host + o_out, 4);
  return ADL_OK;
}

int adl_synth_keys16_device(uint8_t *d_out, uint64_t seed, uint64_t skip, uint64_t n, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 16) return ADL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(synth_keys16_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4 *>(d_out), seed, skip, n);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

int adl_synth_varlen_lengths_device(uint32_t *d_lengths, uint64_t seed, uint64_t n, double zipf_s,
                                    void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_lengths) return ADL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(synth_lengths_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     d_lengths, seed, n, zipf_table(zipf_s));
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

int adl_synth_varlen_fill_device(uint8_t *d_out, uint64_t seed, uint64_t total_bytes, void *stream) {
  if (total_bytes == 0) return ADL_OK;
  if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 8) return ADL_ERR_INVALID_ARG;
  const uint64_t words = (total_bytes + 7) / 8;  // caller allocates round_up(total_bytes, 8)
  hipLaunchKernelGGL(synth_fill_kernel, dim3(grid_for(words, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint64_t *>(d_out), seed, words);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

int adl_synth_probe_queries_device(uint8_t *d_keys, uint32_t *d_filter_id, uint8_t *d_member,
                                   uint64_t seed, uint64_t q0, uint64_t n, uint32_t num_tables,
                                   uint64_t table_seed0, uint64_t keys_per_table, void *stream) {
  if (n == 0) return ADL_OK;
  if (!d_keys || !d_filter_id || num_tables == 0 || reinterpret_cast<uintptr_t>(d_keys) % 16)
    return ADL_ERR_INVALID_ARG;
  hipLaunchKernelGGL(synth_probe_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<uint4 *>(d_keys), d_filter_id, d_member, seed, q0, n, num_tables,
                     table_seed0, keys_per_table);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

}  // extern "C"

// ====================================================================== filter sets
struct adl_bloom_filter_set {
  uint8_t *d_bitmaps = nullptr;
  uint64_t *d_off = nullptr;
  uint32_t nf = 0;
  int32_t bpk = 0;
};

extern "C" {

int adl_bloom_filter_set_create(const uint8_t *h_bitmaps, const uint64_t *h_bitmap_off,
                                uint32_t num_filters, int32_t bits_per_key,
                                adl_bloom_filter_set **out) {
  if (!out || !h_bitmap_off || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  *out = nullptr;
  const uint64_t total = h_bitmap_off[num_filters];
  for (uint32_t f = 0; f < num_filters; ++f) {
    if (h_bitmap_off[f + 1] < h_bitmap_off[f]) return ADL_ERR_INVALID_ARG;
    // m = 8 * bytes must stay a u32 the probe can reduce by (the reference's
    // int m, src/filter_block.cpp:50; adl_bloom_probe_device rejects the same)
    if ((h_bitmap_off[f + 1] - h_bitmap_off[f]) * 8 > 0x7fffffffull) return ADL_ERR_TOO_LARGE;
  }
  if (total && !h_bitmaps) return ADL_ERR_INVALID_ARG;
  auto *s = new (std::nothrow) adl_bloom_filter_set;
  if (!s) return ADL_ERR_OUT_OF_MEMORY;
  s->nf = num_filters;
  s->bpk = bits_per_key;
  int rc = ADL_OK;
  if (hipMalloc((void **)&s->d_bitmaps, total + 16) != hipSuccess ||
      hipMalloc((void **)&s->d_off, (num_filters + 1) * sizeof(uint64_t)) != hipSuccess) {
    rc = ADL_ERR_OUT_OF_MEMORY;
  } else if ((total && hipMemcpy(s->d_bitmaps, h_bitmaps, total, hipMemcpyHostToDevice) != hipSuccess) ||
             hipMemcpy(s->d_off, h_bitmap_off, (num_filters + 1) * sizeof(uint64_t),
                       hipMemcpyHostToDevice) != hipSuccess) {
    rc = ADL_ERR_DEVICE;
  }
  if (rc) {
    adl_bloom_filter_set_destroy(s);
    return rc;
  }
  *out = s;
  return ADL_OK;
}

int adl_bloom_filter_set_probe(const adl_bloom_filter_set *set, const uint8_t *h_keys,
                               const uint64_t *h_offsets, uint64_t n, uint32_t key_stride,
                               const uint32_t *h_filter_id, uint32_t filter, uint8_t *h_out,
                               void *stream) {
  if (!set) return ADL_ERR_INVALID_ARG;
  if (n == 0) return ADL_OK;
  if (!h_keys || !h_out || (!h_offsets && key_stride == 0)) return ADL_ERR_INVALID_ARG;
  hipStream_t st = adl_host::sync_stream(stream);
  adl_host::StagePlan plan;
  const adl_host::KeyBlock kb(plan, h_offsets, n, key_stride);
  const uint64_t o_fid = plan.take(h_filter_id ? n * 4 : 0);
  const uint64_t o_out = plan.take(n);  // the end of the upload
  adl_host::Staging &sg = adl_host::t_stage;
  int rc = sg.reserve(o_out, plan.end);
  if (rc) return rc;
  kb.fill(sg.host, h_keys, h_offsets);
  if (h_filter_id) memcpy(sg.host + o_fid, h_filter_id, n * 4);
  if (hipMemcpyAsync(sg.dev, sg.host, o_out, hipMemcpyHostToDevice, st) != hipSuccess) return ADL_ERR_DEVICE;
  rc = probe_multi(sg.dev, kb.offsets(sg.dev), n, key_stride,
                   h_filter_id ? reinterpret_cast<uint32_t *>(sg.dev + o_fid) : nullptr, filter, set->nf,
                   set->d_bitmaps, set->d_off, set->bpk, sg.dev + o_out, st);
  return fetch_answers(sg, o_out, n, st, rc, h_out);
}

int adl_bloom_filter_set_device_view(const adl_bloom_filter_set *set, const uint8_t **d_bitmaps,
                                     const uint64_t **d_bitmap_off, uint32_t *num_filters) {
  if (!set) return ADL_ERR_INVALID_ARG;
  if (d_bitmaps) *d_bitmaps = set->d_bitmaps;
  if (d_bitmap_off) *d_bitmap_off = set->d_off;
  if (num_filters) *num_filters = set->nf;
  return ADL_OK;
}

int adl_bloom_filter_set_destroy(adl_bloom_filter_set *set) {
  if (!set) return ADL_OK;
  int rc = ADL_OK;
  if (set->d_bitmaps && hipFree(set->d_bitmaps) != hipSuccess) rc = ADL_ERR_DEVICE;
  if (set->d_off && hipFree(set->d_off) != hipSuccess) rc = ADL_ERR_DEVICE;
  delete set;
  return rc;
}

}  // extern "C"

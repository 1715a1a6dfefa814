// adlsm-tree_amd/csrc/hash_run.hpp -- both murmur hashes of a run of keys that
// are not aligned 16-byte keys, hashed from LDS in length order.  The one run
// hasher: hash_var_kernel (bloom_build.hip) writes at the sorted slot in pass
// A's chunk grid, hash_run_pairs_kernel (hash_pairs.hip) at the key's index for
// a streamed build's appends and the binned probe's queries.
//
// A wave hashes 64 keys in lockstep, so it costs as much as its longest key;
// keys sorted by exact length within a run of S keys give waves of nearly
// equal keys.  One workgroup of BLK threads per run:
//   load   the run's offsets and its key bytes -- whole 16-byte blocks from the
//          block holding the run's first byte, up to run_stage_bytes<S>() --
//          every load in flight before the first is used (clamped indices:
//          unconditional, countable waits), so the run costs one memory round
//          trip and each byte is read from HBM once, in memory order;
//   sort   the keys counted into kRunBins exact-length bins in LDS and the
//          bytes staged there; wave 0 scans the bins; each key's (start,
//          length) is scattered to its length-sorted slot;
//   hash   wave w takes groups of 64 sorted slots, longest first, each lane one
//          key from LDS (hash_lds: both seeds, alignbyte words).  A key past
//          the staged bytes, one of 64 KiB or more, or one 4 GiB or more past
//          the run's first block is hashed from global memory (hash_bytes);
//          the latter two keep their index in the run instead of their start;
//   out    out(sorted slot, index in the run, h1, h2).  The index costs a
//          uint16_t per slot of LDS and exists only for an output that asks
//          for it (Out::kByIndex).
// Workgroups are small (256 threads), two per CU, so one workgroup's sort and
// staging overlap the other's hashing; no barrier waits for the slowest group
// (a workgroup ends when its last wave does).
//
// Read contracts (include/adl_bloom.h):
//   ReadWholeBlocks  the key buffer is 16-byte aligned; up to 15 bytes past the
//          run's last key are read, never a block the key bytes do not touch.
//   ReadExactBytes   any alignment, no byte outside the batch's keys is read:
//          the batch's keys are the byte range [off(0), off(n)).  A staged
//          block inside that range holds only bytes of this batch's keys and is
//          loaded whole.  The block the range starts in and the one it ends in
//          may reach outside it: of those two only the bytes inside the range
//          are loaded, one at a time, by threads 0..31.  A run of empty keys
//          loads nothing.
// hash_bytes reads a key's own bytes only, under either contract.
//
// Measured (the build, Zipf lengths): hashing in sorted order straight from
// global memory, lanes reading scattered keys, L2 missed each key line ~3.7
// times, 1.4 GB fetched for 0.4 GB of keys; hence the staging.  Longest groups
// go first because the longest group alone sets the workgroup's end: the waves
// start on it and the short groups fill in behind.  A queue handing each free
// wave the next group measured the same; splitting the longest groups between
// two waves by seed was slower.
#pragma once
#include <type_traits>

#include "bloom_common.hpp"

namespace adl_dev {

constexpr uint32_t kRunBins = 512;  // exact key length 0..510; 511 = longer

// LDS staging of a run's key bytes: 48 bytes per key (mean var-len key ~40 B)
template <uint32_t S>
constexpr uint32_t run_stage_bytes() {
  return S * 48;
}

// dynamic LDS of a kernel that calls hash_run<S, ...>
template <uint32_t S>
constexpr size_t run_lds_bytes(bool with_index) {
  return kRunBins * 4 + S * 4 + S * 2 + (with_index ? S * 2 : 0) + run_stage_bytes<S>() + 16;  // + hash_lds's read slack
}

struct ReadWholeBlocks {};
struct ReadExactBytes {
  uint64_t n;  // keys in the batch
};

// Diagnostics hook: operator()(i) is called after phase i = 0..4 (loaded;
// counted and staged; bins scanned; slots scattered; this wave's groups
// hashed); no_hash() makes the run store (start, length | 1) instead of hashes.
struct RunNoHook {
  __device__ __forceinline__ void operator()(int) const {}
  __device__ __forceinline__ static constexpr bool no_hash() { return false; }
};

// Output at the key's own index in the run: out[ix] = (h1, h2), pairs in key
// order (hash_run_pairs_kernel, hash_pairs.hip).
struct PairsByIndex {
  uint2 *out;
  static constexpr bool kByIndex = true;
  __device__ __forceinline__ void operator()(uint32_t, uint32_t ix, uint32_t h1, uint32_t h2) const {
    out[ix] = make_uint2(h1, h2);
  }
};

// Keys [first, first + cnt) of `keys` (anything with `keys` and off(i)),
// 0 < cnt <= S, by the whole workgroup.
template <uint32_t S, int BLK, class Keys, class Read, class Out, class Hook = RunNoHook>
__device__ __forceinline__ void hash_run(const Keys &keys, uint64_t first, uint32_t cnt, Read read, Out out,
                                         Hook hook = {}) {
  constexpr bool kExact = std::is_same_v<Read, ReadExactBytes>;
  constexpr bool kIdx = Out::kByIndex;
  constexpr uint32_t kStage = run_stage_bytes<S>();
  static_assert(kRunBins == 1u << 9 && kRunBins % kWave == 0, "a key's sort word is rank << 9 | bin");
  static_assert(S % BLK == 0, "whole rounds of keys per thread");
  static_assert(S % 8 == 0, "the stage is 16-byte aligned with and without the index array");
  static_assert(kStage % (16 * BLK) == 0, "the staging loads cover kStage in whole rounds of 16 B per thread");
  static_assert(S <= 65536 && run_lds_bytes<S>(kIdx) <= 160 * 1024, "the uint16_t index in the run; a CU's LDS");
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  uint32_t *bins = lds;                                        // kRunBins
  uint32_t *s_rel = lds + kRunBins;                            // key start - b16 (far keys: index in the run), by sorted slot
  uint16_t *s_len = reinterpret_cast<uint16_t *>(s_rel + S);   // length (0xffff: a far key, hashed from global memory)
  uint16_t *s_idx = s_len + S;                                 // index in the run (kIdx only)
  uint32_t *stage = reinterpret_cast<uint32_t *>(s_len + (kIdx ? 2 * S : S));
  constexpr int KPT = S / BLK;
  constexpr int VPT = kStage / 16 / BLK;
  constexpr uint32_t NW = BLK / kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  // Byte offsets from keys.keys, signed: under ReadExactBytes the run's first
  // block, b16, may start up to 15 bytes before the buffer.  (Every address is
  // keys.keys + offset: an integer cast back to a pointer turns the global
  // loads into flat ones, which also wait on the LDS counter.)
  const int64_t mis = kExact ? (int64_t)(reinterpret_cast<uintptr_t>(keys.keys) & 15u) : 0;
  const int64_t rb = (int64_t)keys.off(first), re = (int64_t)keys.off(first + cnt);
  const int64_t b16 = ((rb + mis) & ~(int64_t)15) - mis;
  // staged: bytes [b16, b16 + sbytes), nv whole blocks, each holding a byte of the run
  const uint32_t sbytes = (kExact && re == rb) ? 0u : (uint32_t)min((re - b16 + 15) & ~(int64_t)15, (int64_t)kStage);
  const uint32_t nv = sbytes / 16;
  // blocks [vb, ve) are loaded whole; under ReadExactBytes block 0 and block
  // nv - 1 may reach outside the batch's range [lo, hi)
  int64_t lo = 0, hi = 0;
  uint32_t vb = 0, ve = nv;
  if constexpr (kExact) {
    lo = (int64_t)keys.off(0), hi = (int64_t)keys.off(read.n);
    vb = b16 < lo ? 1u : 0u;
    ve = (nv && b16 + 16ll * nv > hi) ? nv - 1u : nv;
  }

  for (uint32_t i = tid; i < kRunBins; i += BLK) bins[i] = 0;
  uint64_t o0[KPT], o1[KPT];
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const uint32_t idx = min((uint32_t)(tid + i * BLK), cnt - 1u);
    o0[i] = keys.off(first + idx);
    o1[i] = keys.off(first + idx + 1);
  }
  u32x4_t v[VPT];  // (the ext-vector type: an array of uint4 held across the barrier goes to scratch)
  if (vb < ve) {   // a run of empty keys has no byte to stage (and maybe none to read)
    const u32x4_t *src = reinterpret_cast<const u32x4_t *>(keys.keys + b16);
#pragma unroll
    for (int i = 0; i < VPT; ++i) v[i] = src[min(max((uint32_t)(tid + i * BLK), vb), ve - 1u)];
  }
  // edge: threads 0..15 take the bytes of block 0, threads 16..31 those of
  // block nv - 1, where that block is not loaded whole; only bytes inside the
  // batch's range
  uint32_t edge_at = ~0u, edge_byte = 0;
  if constexpr (kExact) {
    if (tid < 32 && nv) {
      const uint32_t blk = tid < 16 ? 0u : nv - 1u;
      const bool partial = tid < 16 ? vb != 0u : (ve < nv && !(nv == 1u && vb != 0u));
      const int64_t a = b16 + 16ll * blk + (tid & 15);
      if (partial && a >= lo && a < hi) {
        edge_at = 16u * blk + (tid & 15);
        edge_byte = keys.keys[a];
      }
    }
  }
  __syncthreads();
  hook(0);
  // ---- sort the run's keys by length
  uint32_t rk[KPT];
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    rk[i] = ~0u;
    if (tid + i * BLK < cnt) {
      const uint32_t c = (uint32_t)min(o1[i] - o0[i], (uint64_t)(kRunBins - 1));
      rk[i] = (atomicAdd(&bins[c], 1u) << 9) | c;
    }
  }
  {
    u32x4_t *dst = reinterpret_cast<u32x4_t *>(stage);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const uint32_t j = tid + i * BLK;
      if (j >= vb && j < ve) dst[j] = v[i];
    }
    if (kExact && edge_at != ~0u) reinterpret_cast<uint8_t *>(stage)[edge_at] = (uint8_t)edge_byte;
  }
  __syncthreads();
  hook(1);
  if (wave == 0) {  // exclusive scan of the bins, 8 per lane
    constexpr int PER = kRunBins / kWave;
    uint32_t bv[PER], t = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) bv[j] = bins[lane * PER + j], t += bv[j];
    uint32_t run = wave_incl_scan(t, lane) - t;
#pragma unroll
    for (int j = 0; j < PER; ++j) bins[lane * PER + j] = run, run += bv[j];
  }
  __syncthreads();
  hook(2);
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    if (rk[i] != ~0u) {
      const uint32_t slot = bins[rk[i] & (kRunBins - 1)] + (rk[i] >> 9);
      const uint64_t len = o1[i] - o0[i], rel = (uint64_t)((int64_t)o0[i] - b16);
      const bool near = len < 0xffffu && rel < 0xffffffffull;
      s_rel[slot] = near ? (uint32_t)rel : tid + i * BLK;
      s_len[slot] = near ? (uint16_t)len : (uint16_t)0xffffu;
      if constexpr (kIdx) s_idx[slot] = (uint16_t)(tid + i * BLK);
    }
  }
  __syncthreads();
  hook(3);
  // ---- hash, group g = 64 sorted slots, longest groups first
  const uint32_t groups = (cnt + kWave - 1) / kWave;
  for (uint32_t gi = wave; gi < groups; gi += NW) {
    const uint32_t s = (groups - 1 - gi) * kWave + lane;
    if (s >= cnt) continue;
    uint32_t len = s_len[s];
    const uint32_t r = s_rel[s];
    uint32_t ix = 0, h1, h2;
    if constexpr (kIdx) ix = s_idx[s];
    if (hook.no_hash()) {
      out(s, ix, r, len | 1u);
      continue;
    }
    if (len < 0xffffu && (uint64_t)r + len <= sbytes) {
      hash_lds(stage, r, len, h1, h2);
    } else {
      int64_t k0 = b16 + r;
      if (len == 0xffffu) {
        k0 = (int64_t)keys.off(first + r);
        len = (uint32_t)(keys.off(first + r + 1) - (uint64_t)k0);
      }
      hash_bytes(keys.keys + k0, len, kSeed1, kSeed2, h1, h2);
    }
    out(s, ix, h1, h2);
  }
  hook(4);
}

}  // namespace adl_dev

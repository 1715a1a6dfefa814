// adlsm-tree_amd/csrc/bloom_common.hpp -- shared host/device plumbing of
// libadlbloom.so: status handling, key-set views, block scans.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/adl_bloom.h"
#include "murmur3_device.hpp"

// ADL_BLOOM_DEBUG=1: the HIP error behind a failed call goes to stderr
#define ADL_HIP_TRY(expr)                                                                    \
  do {                                                                                       \
    hipError_t adl_e_ = (expr);                                                              \
    if (adl_e_ != hipSuccess) {                                                              \
      if (getenv("ADL_BLOOM_DEBUG"))                                                         \
        fprintf(stderr, "adl_bloom: %s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(adl_e_)); \
      return adl_e_ == hipErrorOutOfMemory ? ADL_ERR_OUT_OF_MEMORY : ADL_ERR_DEVICE;         \
    }                                                                                        \
  } while (0)

namespace adl_dev {

constexpr int kWave = 64;

// ---------------------------------------------------------------- key views
// Fixed 16-byte keys, 16-byte aligned: one global_load_dwordx4 per key, so a
// wave reads 1 KiB contiguous.
struct Keys16 {
  const uint4 *keys;
  __device__ __forceinline__ void hash(uint64_t i, uint32_t &h1, uint32_t &h2) const {
    hash16(keys[i], h1, h2);
  }
  // key i == key i-1 (i > 0)
  __device__ __forceinline__ bool same_as_prev(uint64_t i) const {
    const uint4 a = keys[i], b = keys[i - 1];
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
  }
};

// Fixed stride (any stride, any alignment).
struct KeysStride {
  const uint8_t *keys;
  uint32_t stride;
  __device__ __forceinline__ uint64_t off(uint64_t i) const { return i * stride; }  // key i's first byte
  __device__ __forceinline__ void hash(uint64_t i, uint32_t &h1, uint32_t &h2) const {
    hash_bytes(keys + i * stride, stride, kSeed1, kSeed2, h1, h2);
  }
  __device__ __forceinline__ bool same_as_prev(uint64_t i) const {
    const uint8_t *a = keys + i * stride, *b = a - stride;
    for (uint32_t j = 0; j < stride; ++j)
      if (a[j] != b[j]) return false;
    return true;
  }
};

// Variable length: key i = keys[offs[i] .. offs[i+1]).
struct KeysVar {
  const uint8_t *keys;
  const uint64_t *offs;
  __device__ __forceinline__ uint64_t off(uint64_t i) const { return offs[i]; }
  __device__ __forceinline__ void hash(uint64_t i, uint32_t &h1, uint32_t &h2) const {
    const uint64_t o0 = offs[i], o1 = offs[i + 1];
    hash_bytes(keys + o0, (uint32_t)(o1 - o0), kSeed1, kSeed2, h1, h2);
  }
  __device__ __forceinline__ bool same_as_prev(uint64_t i) const {
    const uint64_t p0 = offs[i - 1], o0 = offs[i], o1 = offs[i + 1];
    if (o1 - o0 != o0 - p0) return false;
    for (uint64_t j = 0; j < o1 - o0; ++j)
      if (keys[o0 + j] != keys[p0 + j]) return false;
    return true;
  }
};

// The (h1, h2) pairs of a streamed build (stream_build.hip), pair i of key i,
// as a key view of the generic pass A (bloom_build.hip: any k, adjacent-
// duplicate skipping) and of the construction check (cache_build.hip).  Equal
// pairs give equal positions, so skipping a key whose pair equals its
// predecessor's leaves the bitmap as skipping an equal key does, and needs no
// key bytes.
struct KeysPair {
  const uint2 *h;
  __device__ __forceinline__ void hash(uint64_t i, uint32_t &h1, uint32_t &h2) const {
    const uint2 v = h[i];
    h1 = v.x;
    h2 = v.y;
  }
  __device__ __forceinline__ bool same_as_prev(uint64_t i) const {
    const uint2 a = h[i], b = h[i - 1];
    return a.x == b.x && a.y == b.y;
  }
};

// ---------------------------------------------------------------- nt access
// Non-temporal 16-byte load/store (global_*_dwordx4 ... nt): streamed data that
// should not displace what the next kernel re-reads from L2 / Infinity Cache.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 load_nt(const uint4 *p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void store_nt(uint4 *p, uint4 v) {
  const u32x4_t x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4_t *>(p));
}

// ---------------------------------------------------------------- scans
// Inclusive wave64 scan by DPP (row shifts inside 16-lane rows, then the
// row broadcasts 15 and 31): about 6 VALU steps instead of 6 ds_bpermute round
// trips through the LDS.  Lanes a DPP source does not cover read 0.
__device__ __forceinline__ uint32_t row16_incl_scan(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int /*lane*/) {
  v = row16_incl_scan(v);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

// Exclusive scan of one value per thread over the block.  `scratch` holds
// BLOCK/64 + 1 words of LDS.  Returns the exclusive prefix; *total = sum.
template <int BLOCK>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *scratch, uint32_t *total) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  constexpr int NW = BLOCK / kWave;
  const uint32_t incl = wave_incl_scan(v, lane);
  if (lane == kWave - 1) scratch[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    uint32_t w = lane < NW ? scratch[lane] : 0u;
    uint32_t wi = wave_incl_scan(w, lane);
    if (lane < NW) scratch[lane] = wi - w;
    if (lane == NW - 1) scratch[NW] = wi;
  }
  __syncthreads();
  const uint32_t r = scratch[wave] + incl - v;
  *total = scratch[NW];
  __syncthreads();  // scratch may be reused right after
  return r;
}

// In-place exclusive scan of an LDS array a[0..N), N <= BLOCK * 4 entries per
// thread; returns the total.  Each thread owns a contiguous run.
template <int BLOCK>
__device__ __forceinline__ uint32_t block_excl_scan_array(uint32_t *a, uint32_t N, uint32_t *scratch) {
  const uint32_t per = (N + BLOCK - 1) / BLOCK;
  const uint32_t beg = threadIdx.x * per;
  const uint32_t end = beg + per < N ? beg + per : N;
  uint32_t s = 0;
  for (uint32_t i = beg; i < end; ++i) s += a[i];
  uint32_t total;
  uint32_t run = block_excl_scan<BLOCK>(s, scratch, &total);
  for (uint32_t i = beg; i < end; ++i) {
    const uint32_t v = a[i];
    a[i] = run;
    run += v;
  }
  __syncthreads();
  return total;
}

// The same in-place exclusive scan with one barrier instead of four: every
// wave scans its threads' run sums, publishes its total, and after the one
// barrier each wave adds up the totals of the waves before it itself.  When
// each thread owns at most one entry (N <= BLOCK), entry i is written and
// later read back by thread i only, so no barrier follows; otherwise one does.
template <int BLOCK>
__device__ __forceinline__ uint32_t block_excl_scan_array_1b(uint32_t *a, uint32_t N, uint32_t *scratch) {
  constexpr int NW = BLOCK / kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t per = (N + BLOCK - 1) / BLOCK;
  const uint32_t beg = tid * per;
  const uint32_t end = beg + per < N ? beg + per : N;
  uint32_t v = 0;
  for (uint32_t i = beg; i < end; ++i) v += a[i];
  const uint32_t incl = wave_incl_scan(v, lane);
  if (lane == kWave - 1) scratch[wave] = incl;
  __syncthreads();
  // the totals of waves 0..wave-1: lane i < NW <= 16 holds wave i's, scanned
  // inside the first 16-lane row; wave w reads lane w-1, the total lane NW-1
  static_assert(NW <= 16, "wave totals scanned inside one DPP row");
  const uint32_t wt = lane < NW ? scratch[lane] : 0u;
  const uint32_t wi = row16_incl_scan(wt);
  const uint32_t before = wave ? __builtin_amdgcn_readlane(wi, wave - 1) : 0u;
  const uint32_t all = __builtin_amdgcn_readlane(wi, NW - 1);
  uint32_t run = before + incl - v;
  for (uint32_t i = beg; i < end; ++i) {
    const uint32_t x = a[i];
    a[i] = run;
    run += x;
  }
  if (per > 1) __syncthreads();
  return all;
}

}  // namespace adl_dev

namespace adl_host {

// The measured crossover of the binned probe for keys that are not 16-byte
// keys (profiles/probe_varlen/): slower than the direct kernel at
// 2^20 queries, at least 18 % faster from 2^22 on.
constexpr uint64_t kProbeBatchVarMinDefault = 1ull << 22;

// The largest max_k at which the binned probe with a probe count per filter
// takes a batch.  A binned query costs k_f entries whether it is a member or
// not, while the direct kernel stops at the first clear bit: at 2^24 queries
// over 256 filters of 1 M keys the pipeline beat the direct kernel on an
// all-member and on an all-absent batch at max_k = 2 only; from 6 on it won
// the member batch (x 0.39-0.52) and lost the absent one (x 1.07-1.31)
// (profiles/probe_batch_k/).  At 10^8 queries it won both kinds
// at every max_k from 6 on: a caller with such batches sets the knob to 30.
constexpr uint32_t kProbeBatchMaxKDefault = 2;

// Tuning and test switches, read from the environment once per
// process.  adl_bloom_reload_knobs() reads them again (tests, between calls:
// no call of the library may be running).
struct Knobs {
  uint32_t tile_log2 = 0;         // ADL_BLOOM_TILE_LOG2: pass-B tile bits (10..20; 0: the plan's choice)
  uint32_t chunk_keys = 0;        // ADL_BLOOM_CHUNK_KEYS: cap on pass A's keys per chunk (tests; 0: the plan's own)
  uint32_t claim = 3;             // ADL_BLOOM_CLAIM: 0 off, 1 wherever the share test passes, 2 forced, 3 auto
  uint32_t claim_cap = 0;         // ADL_BLOOM_CLAIM_CAP: claim region cap, percent of k*C (0: the LDS left)
  bool hash_dedup = true;         // ADL_BLOOM_HASH_DEDUP: pass A skips repeated hash pairs
  // ADL_BLOOM_STREAM_HASH_DEDUP: the same table in a streamed finish (stream_build.hip): 0 off, 1 on,
  // 2 (default) on when every key of the stream came as a 16-byte key, as the builds from keys have it
  uint32_t stream_hash_dedup = 2;
  bool spin = true;               // ADL_BLOOM_SPIN: small cache probes watch their mapped answers
  bool probe_server = true;       // ADL_BLOOM_PROBE_SERVER: cache batches of <= 8 queries go to the server
  uint64_t server_idle_us = 2000;   // ADL_BLOOM_SERVER_IDLE_US
  uint64_t server_life_us = 1000000;  // ADL_BLOOM_SERVER_LIFE_US
  uint64_t pipe_mb = 128;         // ADL_BLOOM_PIPE_MB: keys per group of the pipelined host build
  // ADL_BLOOM_BUILD_QUEUES: when the build passes take their items from work
  // queues instead of the static order: 0 never, 1 while a probe server
  // exists, 2 while a server kernel is resident (its alive word), 3 always.
  // ADL_BLOOM_BUILD_QUEUE_PASSES: which passes (bit 0 pass A, bit 1 pass B).
  uint32_t build_queues = 2;
  uint32_t build_queue_passes = 3;
  bool server_invalidate = false;  // ADL_BLOOM_SERVER_INVALIDATE: the server invalidates its caches at every request
  // ADL_BLOOM_PROBE_BATCH_VAR_MIN: the smallest batch of keys that are not
  // 16-byte keys (offsets, or a stride other than 16) that takes the binned
  // probe pipeline (probe_binned.hip).  0: never; 1 .. 2^20 mean 2^20 (the
  // pipeline's own floor).  Not set: kProbeBatchVarMinDefault.
  uint64_t probe_batch_var_min = kProbeBatchVarMinDefault;
  // ADL_BLOOM_PROBE_BATCH_MAX_K: a batch with a probe count per filter
  // (adl_bloom_probe_batch_k_device) whose max_k is above this stays on the
  // direct kernel.  Not set: kProbeBatchMaxKDefault.
  uint32_t probe_batch_max_k = kProbeBatchMaxKDefault;
  bool debug = false;            // ADL_BLOOM_DEBUG: the plan and failing HIP calls to stderr
  uint32_t exp = 0, pb_exp = 0;   // ADL_BLOOM_EXP / ADL_PB_EXP: diagnostics build (make stamps) only

  void load() {
    auto u64 = [](const char *name, uint64_t dflt) -> uint64_t {
      const char *e = getenv(name);
      return e && *e ? strtoull(e, nullptr, 10) : dflt;
    };
    *this = Knobs{};
    tile_log2 = (uint32_t)u64("ADL_BLOOM_TILE_LOG2", 0);
    chunk_keys = (uint32_t)std::min<uint64_t>(u64("ADL_BLOOM_CHUNK_KEYS", 0), 1u << 20);
    claim = (uint32_t)u64("ADL_BLOOM_CLAIM", 3);
    claim_cap = (uint32_t)u64("ADL_BLOOM_CLAIM_CAP", 0);
    hash_dedup = u64("ADL_BLOOM_HASH_DEDUP", 1) != 0;
    stream_hash_dedup = (uint32_t)u64("ADL_BLOOM_STREAM_HASH_DEDUP", 2);
    spin = u64("ADL_BLOOM_SPIN", 1) != 0;
    probe_server = u64("ADL_BLOOM_PROBE_SERVER", 1) != 0;
    server_idle_us = u64("ADL_BLOOM_SERVER_IDLE_US", 2000);
    server_life_us = u64("ADL_BLOOM_SERVER_LIFE_US", 1000000);
    pipe_mb = u64("ADL_BLOOM_PIPE_MB", 128);
    build_queues = (uint32_t)u64("ADL_BLOOM_BUILD_QUEUES", 2);
    build_queue_passes = (uint32_t)u64("ADL_BLOOM_BUILD_QUEUE_PASSES", 3);
    server_invalidate = u64("ADL_BLOOM_SERVER_INVALIDATE", 0) != 0;
    probe_batch_var_min = u64("ADL_BLOOM_PROBE_BATCH_VAR_MIN", kProbeBatchVarMinDefault);
    if (probe_batch_var_min) probe_batch_var_min = std::max<uint64_t>(probe_batch_var_min, 1ull << 20);
    probe_batch_max_k = (uint32_t)std::min<uint64_t>(u64("ADL_BLOOM_PROBE_BATCH_MAX_K", kProbeBatchMaxKDefault), 30);
    debug = u64("ADL_BLOOM_DEBUG", 0) != 0;
#ifdef ADL_BLOOM_STAMPS
    exp = (uint32_t)u64("ADL_BLOOM_EXP", 0);
    pb_exp = (uint32_t)u64("ADL_PB_EXP", 0);
#endif
  }
};

inline Knobs g_knobs;
inline std::once_flag g_knobs_once;

inline const Knobs &knobs() {
  std::call_once(g_knobs_once, [] { g_knobs.load(); });
  return g_knobs;
}

inline void reload_knobs() {
  (void)knobs();
  g_knobs.load();
}

// Host-side magic numbers for adl_dev::fastmod (see murmur3_device.hpp).
inline adl_dev::FastMod make_fastmod(uint32_t m) {
  adl_dev::FastMod f{};
  f.m = m;
  uint32_t l = 0;
  while ((1ull << l) < m) ++l;  // ceil(log2 m); m >= 2 (m = 8 * bitmap bytes >= 56)
  f.magic = (uint32_t)((((1ull << 32) * ((1ull << l) - m)) / m) + 1ull);
  f.shift = l - 1;
  return f;
}

// Compute units of the current device (256 on MI355X), queried once.
inline uint32_t device_cus() {
  static std::once_flag once;
  static uint32_t cus = 256;
  std::call_once(once, [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = (uint32_t)v;
  });
  return cus;
}

inline int num_probes(int32_t bpk) {
  int k = (int)(bpk * 0.69);  // src/filter_block.cpp:44
  if (k < 1) k = 1;
  if (k > 30) k = 30;
  return k;
}

inline uint64_t bitmap_bytes(uint64_t n, int32_t bpk) {
  if (bpk < 0) return 0;
  const uint64_t bytes = n * (uint64_t)bpk + 7;
  if (n > 0x7fffffffull || bytes * 8 > 0x7fffffffull) return 0;
  return bytes;
}

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Host memory the device can DMA directly (hipHostMalloc'd / registered).
inline bool is_pinned(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: clear the sticky error
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// Per-thread staging for the synchronous host-pointer entry points: a pinned
// host buffer (so every copy is a stream-ordered DMA; pageable hipMemcpyAsync
// is not used anywhere) and a device buffer, both grown on demand and reused.
// One per thread keeps the C-ABI re-entrant without locks.
struct Staging {
  uint8_t *host = nullptr;
  uint64_t hcap = 0;
  uint8_t *dev = nullptr;
  uint64_t dcap = 0;
  ~Staging() {
    if (host) (void)hipHostFree(host);
    if (dev) (void)hipFree(dev);
  }
  int reserve(uint64_t hbytes, uint64_t dbytes) {
    if (hbytes > hcap) {
      if (host) (void)hipHostFree(host);
      host = nullptr;
      hcap = 0;
      const uint64_t want = round_up(hbytes + (hbytes >> 3), 1 << 16);
      if (hipHostMalloc((void **)&host, want, hipHostMallocDefault) != hipSuccess) return ADL_ERR_OUT_OF_MEMORY;
      hcap = want;
    }
    if (dbytes > dcap) {
      if (dev) (void)hipFree(dev);
      dev = nullptr;
      dcap = 0;
      const uint64_t want = round_up(dbytes + (dbytes >> 3), 1 << 16);
      if (hipMalloc((void **)&dev, want) != hipSuccess) return ADL_ERR_OUT_OF_MEMORY;
      dcap = want;
    }
    return ADL_OK;
  }
};

inline thread_local Staging t_stage;

// The layout of a staging buffer (or a workspace, or a blob uploaded once):
// sections handed out one after another, each starting 256-byte aligned.
// `end` is where the next one would start: the bytes an upload of everything
// placed so far moves, and at last the size to reserve.
struct StagePlan {
  uint64_t end = 0;
  uint64_t take(uint64_t bytes) {
    const uint64_t at = end;
    end += round_up(bytes, 256);
    return at;
  }
};

// The key block every host-pointer entry point stages first, at offset 0 of a
// plan with nothing placed yet: the key bytes (+16: a kernel's wide loads of
// the last key stay inside the section), then the n + 1 offsets (no section
// for a fixed stride).
struct KeyBlock {
  uint64_t key_bytes, off_bytes, o_offs;
  KeyBlock(StagePlan &p, const uint64_t *h_offsets, uint64_t n, uint32_t key_stride)
      : key_bytes(h_offsets ? h_offsets[n] : n * (uint64_t)key_stride), off_bytes(h_offsets ? (n + 1) * 8 : 0) {
    p.take(key_bytes + 16);
    o_offs = p.take(off_bytes);
  }
  void fill(uint8_t *hbuf, const uint8_t *h_keys, const uint64_t *h_offsets) const {
    if (key_bytes) memcpy(hbuf, h_keys, key_bytes);
    if (off_bytes) memcpy(hbuf + o_offs, h_offsets, off_bytes);
  }
  // the device offsets of a buffer laid out by the plan (null: fixed stride)
  const uint64_t *offsets(const uint8_t *dbuf) const {
    return off_bytes ? reinterpret_cast<const uint64_t *>(dbuf + o_offs) : nullptr;
  }
};

// Per-thread small pinned buffer mapped into the device's address space
// (coherent): a small synchronous probe hands the kernel its keys and table
// ids where they are and has it write the answers back there, so a lookup is
// one launch and one stream sync, with no H2D / D2H copy commands.
struct MappedStage {
  static constexpr uint64_t kMax = 64 << 10;
  uint8_t *host = nullptr;
  uint8_t *dev = nullptr;
  bool tried = false;
  ~MappedStage() {
    if (host) (void)hipHostFree(host);
  }
  // nullptr if unavailable or bytes > kMax (the caller then stages and copies)
  uint8_t *get(uint64_t bytes) {
    if (bytes > kMax) return nullptr;
    if (!tried) {
      tried = true;
      void *d = nullptr;
      if (hipHostMalloc((void **)&host, kMax, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
          hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
        if (host) (void)hipHostFree(host);
        host = nullptr;
        (void)hipGetLastError();
        return nullptr;
      }
      dev = static_cast<uint8_t *>(d);
    }
    return host;
  }
};

inline thread_local MappedStage t_mapped;

// The stream a synchronous host-pointer entry point runs on: the caller's, or
// for stream == NULL a non-blocking stream of the calling thread (created on
// first use).  The legacy null stream would order every thread's calls one
// after the other on the device; these calls only touch their own staging
// buffers, so nothing is lost by not ordering them with the null stream.
struct ThreadStream {
  hipStream_t s = nullptr;
  bool tried = false;
  ~ThreadStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  hipStream_t get() {
    if (!tried) {
      tried = true;
      if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    }
    return s;
  }
};

inline thread_local ThreadStream t_stream;

inline hipStream_t sync_stream(void *stream) { return stream ? (hipStream_t)stream : t_stream.get(); }

// Small host -> device uploads in stream order from pinned memory (a build's
// filter descriptors): a ring of slots per thread, each reused only after its
// previous copy has completed.
//
// An outgrown slot buffer is kept until the thread ends, not freed where it
// is replaced: hipHostFree waits for every stream of the device, and so for a
// resident probe server's kernel (probe_server.hip).  A build beside Gets
// whose descriptors outgrew a slot stood still there until the server's kernel
// and its queued successor had idled out or reached their life limits
// (tests/test_gpu_claim.py, test_build_queue_selection_default_mode: 120 s
// when it ran with the idle limit at 60 s).  A slot at least doubles, so the buffers it has
// retired add up to less than the one in use.
struct UploadRing {
  static constexpr int kSlots = 4;
  uint8_t *host[kSlots] = {};
  uint64_t cap[kSlots] = {};
  hipEvent_t ev[kSlots] = {};
  bool used[kSlots] = {};
  int next = 0;
  std::vector<uint8_t *> retired;
  ~UploadRing() {
    for (int s = 0; s < kSlots; ++s) {
      if (used[s]) (void)hipEventSynchronize(ev[s]);
      if (ev[s]) (void)hipEventDestroy(ev[s]);
      if (host[s]) (void)hipHostFree(host[s]);
    }
    for (uint8_t *h : retired) (void)hipHostFree(h);
  }
  // The next slot, free and at least `bytes` long: the caller fills *h and
  // sends it with commit().  (A slot taken and not committed is simply reused.)
  int begin(uint64_t bytes, uint8_t **h) {
    const int s = next;
    if (!ev[s]) ADL_HIP_TRY(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
    if (used[s]) ADL_HIP_TRY(hipEventSynchronize(ev[s]));
    used[s] = false;
    if (bytes > cap[s]) {
      if (host[s]) retired.push_back(host[s]);  // (its last copy has completed: the event above)
      host[s] = nullptr;
      const uint64_t want = round_up(std::max(bytes, 2 * cap[s]), 1 << 16);
      cap[s] = 0;
      ADL_HIP_TRY(hipHostMalloc((void **)&host[s], want, hipHostMallocDefault));
      cap[s] = want;
    }
    *h = host[s];
    return ADL_OK;
  }
  // The first `bytes` of the slot begin() gave go to dst in stream order.
  int commit(void *dst, uint64_t bytes, hipStream_t st) {
    const int s = next;
    next = (next + 1) % kSlots;
    ADL_HIP_TRY(hipMemcpyAsync(dst, host[s], bytes, hipMemcpyHostToDevice, st));
    ADL_HIP_TRY(hipEventRecord(ev[s], st));
    used[s] = true;
    return ADL_OK;
  }
  int upload(void *dst, const void *src, uint64_t bytes, hipStream_t st) {
    uint8_t *h = nullptr;
    if (int rc = begin(bytes, &h)) return rc;
    memcpy(h, src, bytes);
    return commit(dst, bytes, st);
  }
};

inline thread_local UploadRing t_upload;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device
// (the whole 160 KiB of a CU; each launch asks for what it uses), not on every
// launch.
template <auto Kern>
int lds_limit() {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  ADL_HIP_TRY(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return ADL_OK;
  ADL_HIP_TRY(hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  done.fetch_or(bit, std::memory_order_acq_rel);
  return ADL_OK;
}

// Library-internal (bloom_probe.hip): adl_bloom_probe_ranges_device whose
// kernel launch also completes `done`.
__attribute__((visibility("hidden"))) int adl_probe_ranges_device_ev(
    const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride, const uint32_t *d_filter_id,
    uint32_t num_filters, const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
    const uint8_t *d_k, uint8_t *d_out, hipStream_t st, hipEvent_t done);

// Library-internal (bloom_probe.hip): the direct multi-filter probe with a
// probe count per filter (d_k[f]); d_end null: filter f ends at d_begin[f + 1].
__attribute__((visibility("hidden"))) int adl_probe_multi_k_device(
    const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride, const uint32_t *d_filter_id,
    uint32_t num_filters, const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end,
    const uint8_t *d_k, uint8_t *d_out, hipStream_t st);

// The same for adl_bloom_probe_fanout_device (d_k[f]: filter f's probe count).
__attribute__((visibility("hidden"))) int adl_probe_fanout_device_ev(
    const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys, uint32_t key_stride,
    const uint32_t *d_pair_begin, const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
    const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end, const uint8_t *d_k, uint8_t *d_out,
    hipStream_t st, hipEvent_t done);

// Library-internal (filter_block_device.hip): adl_bloom_filter_block_build_device
// with the segmented build's flags; in_place builds a one-filter block
// straight into d_block (no staging, no pack, no trailer on the device).
__attribute__((visibility("hidden"))) int adl_filter_block_build_into(
    const uint8_t *d_keys, const uint64_t *d_offsets, uint32_t key_stride, const uint64_t *key_begin,
    uint32_t num_filters, int32_t bits_per_key, uint8_t *d_block, uint64_t block_bytes, uint32_t flags, bool in_place,
    void *d_workspace, uint64_t workspace_bytes, hipStream_t st);

// Library-internal (bloom_build.hip): adl_bloom_build_segmented_device_ex over
// the (h1, h2) pairs of a streamed build (stream_build.hip), pair i (a uint2)
// at d_pairs[i], instead of keys.
__attribute__((visibility("hidden"))) int adl_build_pairs_device(
    const void *d_pairs, const uint64_t *key_begin, uint32_t num_filters, int32_t bits_per_key, uint8_t *d_bitmaps,
    const uint64_t *bitmap_off, uint32_t flags, bool hash_dedup, void *d_workspace, uint64_t workspace_bytes,
    hipStream_t st);

// Library-internal (hash_pairs.hip): both hashes of n keys of any shape, pair i
// (a uint2) at out[i].  whole: d_keys is 16-byte aligned and may be read in
// whole 16-byte blocks; otherwise no byte outside the n keys is read.
__attribute__((visibility("hidden"))) int hash_pairs_device(const uint8_t *d_keys, const uint64_t *d_offsets,
                                                            uint32_t key_stride, uint64_t n, bool whole, uint2 *out,
                                                            hipStream_t st);

// Library-internal (filter_block_device.hip): adl_filter_block_build_into over
// a streamed build's pairs instead of keys.
__attribute__((visibility("hidden"))) int adl_filter_block_build_into_pairs(
    const void *d_pairs, bool hash_dedup, const uint64_t *key_begin, uint32_t num_filters, int32_t bits_per_key,
    uint8_t *d_block, uint64_t block_bytes, uint32_t flags, bool in_place, void *d_workspace,
    uint64_t workspace_bytes, hipStream_t st);

// Library-internal (stream_build.hip), for a build that reads a stream's pair
// store itself (cache_build.hip).  stream_acquire: `st` waits for the object's
// appends (and earlier finishes); *d_pairs is the store, key_begin the bounds
// of adl_bloom_stream_counts, *hash_dedup whether a finish would use pass A's
// repeated-pair table.  stream_release: what was enqueued on `st` since counts
// as a finish of the object.
__attribute__((visibility("hidden"))) int stream_acquire(adl_bloom_stream *s, hipStream_t st, const void **d_pairs,
                                                         std::vector<uint64_t> &key_begin, bool *hash_dedup);
__attribute__((visibility("hidden"))) int stream_release(adl_bloom_stream *s, hipStream_t st);

// adl_bloom_test_fault's armed sites (-1: off).  take() disarms and returns the
// argument, so an armed fault fires once.
struct TestFaults {
  std::atomic<int64_t> site[4] = {-1, -1, -1, -1};
  int64_t take(int s) {
    if (site[s].load(std::memory_order_relaxed) < 0) return -1;
    return site[s].exchange(-1);
  }
};
inline TestFaults g_test_faults;

// ADL_TEST_FAULT_SERVER_SEQ: the sequence number the calling thread's next
// probe-server request continues its slot from (-1: none).  Per thread, since
// a slot belongs to the thread that posts into it: a preset armed by one
// thread is not taken by another thread's request.  probe_server.hip takes it.
inline thread_local int64_t t_server_seq_preset = -1;

}  // namespace adl_host

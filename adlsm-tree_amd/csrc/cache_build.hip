// adlsm-tree_amd/csrc/cache_build.hip -- write-through filter cache: a
// table's filter block built straight into the cache arena, and the
// construction check that goes with it.
//
// The write side (SSTableWriter::Final -> FilterBlockWriter::Final,
// src/sstable.cpp:58) builds a table's filters on the GPU, downloads the block
// for the file and used to drop the device copy; the read side got the same
// bytes back only when a reader opened the table and put them
// (SSTableReader::ReadFilterBlock, src/sstable.cpp:179-209): one more H2D of
// the whole bitmap, and until then every multi-get bound for the new table --
// a freshly flushed L0 table, the one lookups hit most -- answered "not
// cached, read the table".  Here the build's destination IS a reserved range
// of the arena:
//
//  * build: reserves the range as put does (a pinned kLoading entry in limbo,
//    marked `ticket`), builds the filters there -- a one-filter block in place,
//    a multi-filter block through aligned staging and the pack kernel
//    (filter_block_device.hip) -- and brings the block back for the file: the
//    bitmap region by one D2H, the trailer framed on the host.
//  * publish(ticket, oid): once the file is written and its SHA-256 known,
//    put's step 4 under the lock.  abandon(ticket) gives the range back.
//  * build_stream: the same with an adl_bloom_stream as the key source
//    (stream_build.hip): nothing to upload, the filters are built from the
//    stream's hash pairs.
//  * bloom_verify_kernel: every build key (or pair) probed again against the bitmap it
//    went into (the "probe what you inserted" check of storage engines; one
//    streaming pass).  With ADL_BLOOM_CACHE_VERIFY a block with a missing key
//    never goes resident.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "bloom_common.hpp"
#include "filter_cache_impl.hpp"
#include "probe_device.hpp"

using namespace adl_dev;
using adl_cache::kAlign;

namespace {

constexpr uint32_t kKnownFlags = ADL_BLOOM_SKIP_ADJACENT_DUPLICATES | ADL_BLOOM_CACHE_VERIFY;
constexpr uint32_t kVerifySlots = 256;  // outstanding verified device-variant tickets per cache

// The filter of key i: the f with kb[f] <= i < kb[f + 1], by an upper-bound
// search (empty filters -- equal entries -- are passed over); nf when the key
// lies outside [kb[0], kb[nf]).
template <class P>
__device__ __forceinline__ uint32_t key_filter(P kb, uint32_t nf, uint64_t i) {
  uint32_t lo = 0, hi = nf + 1;  // the first j with kb[j] > i, or nf + 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (kb[mid] > i) hi = mid; else lo = mid + 1;
  }
  return lo >= 1 && lo <= nf ? lo - 1 : nf;
}

// Construction check: key i against the filter it was built into, lane per
// key, the probe kernels' own hash, divisor table, lookup and bit reads
// (probe_device.hpp), so a key is "missing" exactly when a probe would answer
// 0 for it.  The divisor table of up to kLdsFilters filters sits in LDS as in
// bloom_probe_multi_kernel, and behind it key_begin when its nf + 1 entries
// fit the same budget once more (the kernel then reads global memory only for
// keys and bits).  Misses are counted per wave -- ballot and popcount over the
// 64 lanes, then one atomic add and one atomic min by the wave's first missing
// lane -- so a correct build, the common case, issues no atomic at all.  Keys
// outside every filter's range were not built and are not checked.
template <class Keys>
__global__ __launch_bounds__(kBlockP) void bloom_verify_kernel(
    Keys keys, uint64_t n, uint32_t k, const uint64_t *__restrict__ key_begin, uint32_t nf,
    const uint8_t *__restrict__ bitmaps, const uint64_t *__restrict__ boff, const uint64_t *__restrict__ bend,
    unsigned long long *__restrict__ result) {
  extern __shared__ ModLds lmod[];
  const bool lds_tab = nf <= kLdsFilters;
  const bool lds_kb = nf + 1 <= kLdsFilters;                  // (implies lds_tab)
  uint64_t *lkb = reinterpret_cast<uint64_t *>(lmod + nf);   // 8-byte entries before it: aligned
  if (lds_tab) {
    mod_table_fill(lmod, nf, k, nullptr, boff, bend);
    if (lds_kb)
      for (uint32_t f = threadIdx.x; f <= nf; f += kBlockP) lkb[f] = key_begin[f];
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & (kWave - 1);
  // whole waves enter every round (the ballot needs all 64 lanes)
  for (uint64_t base = blockIdx.x * (uint64_t)kBlockP; base < n; base += (uint64_t)gridDim.x * kBlockP) {
    const uint64_t i = base + threadIdx.x;
    bool miss = false;
    if (i < n) {
      const uint32_t f = lds_kb ? key_filter(lkb, nf, i) : key_filter(key_begin, nf, i);
      if (f < nf) {
        miss = true;  // an empty filter or one of 2^31 bits or more: the probe answers 0
        uint64_t b0;
        FastMod mod;
        uint32_t kq;
        if (filter_lookup(f, nf, lds_tab, lmod, k, nullptr, boff, bend, b0, mod, kq)) {
          uint32_t h1, h2;
          keys.hash(i, h1, h2);
          miss = !probe_bits(bitmaps + b0, h1, h2, kq, mod);
        }
      }
    }
    const unsigned long long mask = __ballot(miss);
    if (miss && lane == (uint32_t)__ffsll(mask) - 1u) {  // the wave's lowest missing key
      atomicAdd(&result[0], (unsigned long long)__popcll(mask));
      atomicMin(&result[1], (unsigned long long)i);
    }
  }
}

// adl_bloom_test_fault(ADL_TEST_FAULT_CACHE_BUILD_CORRUPT): clears the first
// non-zero byte of a bitmap (one workgroup walking it 256 bytes at a time).
__global__ __launch_bounds__(256) void cache_corrupt_kernel(uint8_t *__restrict__ bm, uint64_t bytes) {
  __shared__ uint32_t found;
  for (uint64_t base = 0; base < bytes; base += 256) {
    if (threadIdx.x == 0) found = 256;
    __syncthreads();
    const uint64_t i = base + threadIdx.x;
    if (i < bytes && bm[i]) atomicMin(&found, threadIdx.x);
    __syncthreads();
    const uint32_t first = found;
    if (first < 256) {  // (the same for every thread)
      if (threadIdx.x == first) bm[i] = 0;
      return;
    }
    __syncthreads();  // `found` is reset by the next round
  }
}

// The block FilterBlockWriter::Final frames (src/filter_block.cpp:77-102):
// off[f] = packed offset of filter f, off[F] = offsets_start.
struct BlockPlan {
  std::vector<uint64_t> off;
  uint64_t block_bytes = 0;
  uint64_t region() const { return off.back(); }
};

int plan_block(const uint64_t *key_begin, uint32_t nf, int32_t bpk, BlockPlan &P) {
  if (!key_begin || bpk < 0) return ADL_ERR_INVALID_ARG;
  P.off.assign((size_t)nf + 1, 0);
  for (uint32_t f = 0; f < nf; ++f) {
    if (key_begin[f + 1] < key_begin[f]) return ADL_ERR_INVALID_ARG;
    const uint64_t b = adl_host::bitmap_bytes(key_begin[f + 1] - key_begin[f], bpk);
    if (!b) return ADL_ERR_TOO_LARGE;
    P.off[f + 1] = P.off[f] + b;
  }
  P.block_bytes = P.region() + 4ull * nf + 4 + 4 + 7 + 4;
  if (P.block_bytes > 0x7fffffffull) return ADL_ERR_TOO_LARGE;  // the reference's int offsets
  return ADL_OK;
}

void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }  // (Append32 of the mirror: native-endian)

// i32 offsets[F], i32 offsets_start, i32 F, "bf:" + i32 bpk, i32 7 behind the bitmaps.
void frame_trailer(uint8_t *h_block, const BlockPlan &P, uint32_t nf, int32_t bpk) {
  uint8_t *p = h_block + P.region();
  for (uint32_t f = 0; f < nf; ++f, p += 4) put32(p, (uint32_t)P.off[f]);
  put32(p, (uint32_t)P.region());
  put32(p + 4, nf);
  memcpy(p + 8, "bf:", 3);
  put32(p + 11, (uint32_t)bpk);
  put32(p + 15, 7u);
}

// Device bytes of a build: [key_begin and filter offsets for the verify
// kernel][its result][the block build's workspace], each 256-byte aligned.
uint64_t aux_bytes(uint32_t nf) { return adl_host::round_up(2 * ((uint64_t)nf + 1) * 8, 256); }

using Cache = adl_bloom_filter_cache;

// Could `size` bytes be found if every block that is not an unpublished
// ticket's gave its range back?  (Live blocks can be evicted, blocks pinned by
// probes or being uploaded by a put are given back by calls that are running;
// a ticket's range only by its holder, who may be this very thread.)
bool fits_without_tickets(Cache *c, uint64_t size) {
  std::vector<std::pair<uint64_t, uint64_t>> r(c->free_.begin(), c->free_.end());
  for (const Cache::Entry &e : c->lru) r.emplace_back(e.base, e.size);
  for (const Cache::Entry &e : c->limbo)
    if (!e.ticket) r.emplace_back(e.base, e.size);
  std::sort(r.begin(), r.end());
  uint64_t at = 0, len = 0;
  for (const auto &x : r) {
    if (len && at + len == x.first) {
      len += x.second;
    } else {
      at = x.first;
      len = x.second;
    }
    if (len >= size) return true;
  }
  return false;
}

// put's steps 1 and 2 for a build: room in the arena (least recently used
// blocks evicted for it), the range reserved as a pinned loading entry in
// limbo.  The table count is enforced when the block is published.  Never
// waits for room that only unpublished tickets hold: ADL_ERR_OUT_OF_MEMORY,
// with nothing evicted.
int reserve_range(Cache *c, uint64_t size, std::vector<uint64_t> &&off, uint8_t k, Cache::Iter &mine) {
  std::unique_lock<std::mutex> g(c->mu);
  if (size > c->capacity || !fits_without_tickets(c, size)) return ADL_ERR_OUT_OF_MEMORY;
  uint64_t at = 0;
  while (!c->alloc(size, at)) {
    if (!c->lru.empty()) {
      c->retire(std::prev(c->lru.end()));
      continue;
    }
    bool running = false;  // a probe's pins or a put's upload: a call that will end
    for (const Cache::Entry &e : c->limbo) running |= !e.ticket;
    if (!running) return ADL_ERR_OUT_OF_MEMORY;  // (tickets taken while this call waited)
    c->freed.wait(g);
  }
  Cache::Entry e;
  e.base = at;
  e.size = size;
  e.off = std::move(off);
  e.k = k;
  e.pins = 1;
  e.state = Cache::kLoading;
  e.ticket = true;
  mine = c->limbo.insert(c->limbo.end(), std::move(e));
  return ADL_OK;
}

void release_range(Cache *c, Cache::Iter mine, int32_t slot = -1) {
  std::lock_guard<std::mutex> g(c->mu);
  if (slot >= 0) c->verify_free.push_back((uint32_t)slot);
  mine->state = Cache::kDead;
  c->unpin(mine);  // frees the range and wakes calls waiting for room
}

void report_missing(uint64_t missing, uint64_t first) {
  if (adl_host::knobs().debug)
    fprintf(stderr, "adl_bloom: cache build verify: %llu keys missing from their filter, the first is key %llu\n",
            (unsigned long long)missing, (unsigned long long)first);
}

int verify_launch(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                  const uint64_t *d_key_begin, uint32_t nf, const uint8_t *d_bitmaps, const uint64_t *d_begin,
                  const uint64_t *d_end, int32_t bpk, uint64_t *d_result, hipStream_t st) {
  ADL_HIP_TRY(hipMemsetAsync(d_result, 0, 8, st));
  ADL_HIP_TRY(hipMemsetAsync(d_result + 1, 0xff, 8, st));
  if (n == 0 || nf == 0) return ADL_OK;
  const uint32_t k = (uint32_t)adl_host::num_probes(bpk);
  return adl_host::dispatch_keys(d_keys, d_offsets, key_stride, [&](auto keys) -> int {
    size_t lds = 0;
    if (nf <= kLdsFilters) lds = (size_t)nf * sizeof(ModLds) + (nf + 1 <= kLdsFilters ? ((size_t)nf + 1) * 8 : 0);
    hipLaunchKernelGGL(bloom_verify_kernel<decltype(keys)>, dim3(adl_host::grid_for(n, kBlockP, 8)), dim3(kBlockP),
                       lds, st, keys, n, k, d_key_begin, nf, d_bitmaps, d_begin, d_end,
                       reinterpret_cast<unsigned long long *>(d_result));
    ADL_HIP_TRY(hipGetLastError());
    return ADL_OK;
  });
}

// The same check from a streamed build's hash pairs (pair i of key i): the
// keys are gone, and a pair is all the probe takes from a key.
int verify_launch_pairs(const uint2 *d_pairs, uint64_t n, const uint64_t *d_key_begin, uint32_t nf,
                        const uint8_t *d_bitmaps, const uint64_t *d_begin, int32_t bpk, uint64_t *d_result,
                        hipStream_t st) {
  ADL_HIP_TRY(hipMemsetAsync(d_result, 0, 8, st));
  ADL_HIP_TRY(hipMemsetAsync(d_result + 1, 0xff, 8, st));
  if (n == 0 || nf == 0) return ADL_OK;
  const uint32_t k = (uint32_t)adl_host::num_probes(bpk);
  size_t lds = 0;
  if (nf <= kLdsFilters) lds = (size_t)nf * sizeof(ModLds) + (nf + 1 <= kLdsFilters ? ((size_t)nf + 1) * 8 : 0);
  hipLaunchKernelGGL(bloom_verify_kernel<KeysPair>, dim3(adl_host::grid_for(n, kBlockP, 8)), dim3(kBlockP), lds, st,
                     KeysPair{d_pairs}, n, k, d_key_begin, nf, d_bitmaps, d_begin, (const uint64_t *)nullptr,
                     reinterpret_cast<unsigned long long *>(d_result));
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

// What a build's filters are built from: device keys, or (d_pairs set) a
// streamed build's hash pairs.
struct BuildSource {
  const uint8_t *d_keys = nullptr;
  const uint64_t *d_offsets = nullptr;
  uint32_t key_stride = 0;
  bool from_pairs = false;
  const uint2 *d_pairs = nullptr;  // (may be NULL when the stream holds no key)
  bool pair_dedup = false;         // pairs: pass A's repeated-pair table
};

// Everything a build enqueues on `st`: the filters into the arena range of
// `mine`, the test fault, the verify pass (result to d_result) and the D2H of
// the bitmap region into h_dst (pinned, or NULL).  key_begin: HOST, relative
// to d_keys / d_offsets.  d_ws: 256-byte aligned.
int enqueue_build(Cache *c, Cache::Iter mine, const BlockPlan &P, const BuildSource &src, const uint64_t *key_begin,
                  uint32_t nf, int32_t bpk, uint32_t flags, uint8_t *d_ws, uint64_t ws_bytes, uint64_t **d_result,
                  uint8_t *h_dst, hipStream_t st) {
  uint8_t *range = c->arena + mine->base;
  uint64_t *d_aux = reinterpret_cast<uint64_t *>(d_ws);
  *d_result = reinterpret_cast<uint64_t *>(d_ws + aux_bytes(nf));
  uint8_t *bws = d_ws + aux_bytes(nf) + 256;
  if (ws_bytes < aux_bytes(nf) + 256) return ADL_ERR_WORKSPACE;
  const int brc = src.from_pairs
                      ? adl_host::adl_filter_block_build_into_pairs(src.d_pairs, src.pair_dedup, key_begin, nf, bpk, range,
                                                                    mine->size, flags & ADL_BLOOM_SKIP_ADJACENT_DUPLICATES,
                                                                    true, bws, ws_bytes - aux_bytes(nf) - 256, st)
                      : adl_host::adl_filter_block_build_into(src.d_keys, src.d_offsets, src.key_stride, key_begin, nf, bpk,
                                                              range, mine->size, flags & ADL_BLOOM_SKIP_ADJACENT_DUPLICATES,
                                                              true, bws, ws_bytes - aux_bytes(nf) - 256, st);
  if (brc) return brc;
  if (adl_host::g_test_faults.take(ADL_TEST_FAULT_CACHE_BUILD_CORRUPT) >= 0 && P.off[1] > P.off[0]) {
    hipLaunchKernelGGL(cache_corrupt_kernel, dim3(1), dim3(256), 0, st, range, P.off[1]);
    ADL_HIP_TRY(hipGetLastError());
  }
  if (flags & ADL_BLOOM_CACHE_VERIFY) {
    std::vector<uint64_t> aux(key_begin, key_begin + nf + 1);
    aux.insert(aux.end(), P.off.begin(), P.off.end());
    if (int rc = adl_host::t_upload.upload(d_aux, aux.data(), aux.size() * 8, st)) return rc;
    const int vrc = src.from_pairs
                        ? verify_launch_pairs(src.d_pairs, key_begin[nf], d_aux, nf, range, d_aux + nf + 1, bpk, *d_result, st)
                        : verify_launch(src.d_keys, src.d_offsets, key_begin[nf], src.key_stride, d_aux, nf, range,
                                        d_aux + nf + 1, nullptr, bpk, *d_result, st);
    if (vrc) return vrc;
  }
  if (h_dst && P.region()) ADL_HIP_TRY(hipMemcpyAsync(h_dst, range, P.region(), hipMemcpyDeviceToHost, st));
  return ADL_OK;
}

}  // namespace

struct adl_bloom_cache_ticket {
  adl_bloom_filter_cache::Iter it;
  hipEvent_t done = nullptr;  // device variant: the end of the build's work on the caller's stream
  int32_t slot = -1;          // device variant with ADL_BLOOM_CACHE_VERIFY: its pinned result slot
};

extern "C" {

uint64_t adl_bloom_filter_cache_build_workspace_bytes(const uint64_t *key_begin, uint32_t num_filters,
                                                      int32_t bits_per_key) {
  try {
    BlockPlan P;
    if (plan_block(key_begin, num_filters, bits_per_key, P)) return 0;
    const uint64_t b = adl_bloom_filter_block_workspace_bytes(key_begin, num_filters, bits_per_key);
    if (!b) return 0;
    return aux_bytes(num_filters) + 256 + b + 256;
  } catch (...) {
    return 0;
  }
}

int adl_bloom_filter_cache_build(adl_bloom_filter_cache *c, const uint8_t *h_keys, const uint64_t *h_offsets,
                                 uint32_t key_stride, const uint64_t *key_begin, uint32_t num_filters,
                                 int32_t bits_per_key, uint32_t flags, uint8_t *h_block, uint64_t block_bytes,
                                 adl_bloom_cache_ticket **ticket, void *stream) {
  if (flags & ~kKnownFlags) return ADL_ERR_INVALID_ARG;
  if (!c || !key_begin || !h_block || !ticket || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  *ticket = nullptr;
  try {
    const uint32_t nf = num_filters;
    BlockPlan P;
    if (int rc = plan_block(key_begin, nf, bits_per_key, P)) return rc;
    if (block_bytes < P.block_bytes) return ADL_ERR_INVALID_ARG;
    const uint64_t k0 = key_begin[0], k1 = key_begin[nf], n = k1 - k0;
    if (n && (!h_keys || (!h_offsets && key_stride == 0))) return ADL_ERR_INVALID_ARG;
    const uint64_t ws_bytes = adl_bloom_filter_cache_build_workspace_bytes(key_begin, nf, bits_per_key);
    if (!ws_bytes) return ADL_ERR_TOO_LARGE;
    auto *t = new adl_bloom_cache_ticket;
    const uint64_t size = adl_host::round_up(std::max(P.block_bytes, P.region() + 1), kAlign);
    if (int rc = reserve_range(c, size, std::vector<uint64_t>(P.off), (uint8_t)adl_host::num_probes(bits_per_key),
                               t->it)) {
      delete t;
      return rc;
    }
    hipStream_t st = adl_host::sync_stream(stream);
    // the keys of the block's filters: bytes [b0, b1) of h_keys.  Var-len
    // offsets stay absolute, so the upload starts 16-byte aligned below the
    // first key and the device key pointer is shifted back by b0.
    auto key_byte = [&](uint64_t k) -> uint64_t { return h_offsets ? h_offsets[k] : k * (uint64_t)key_stride; };
    const uint64_t b0 = n ? (h_offsets ? key_byte(k0) & ~15ull : key_byte(k0)) : 0, b1 = n ? key_byte(k1) : 0;
    const uint64_t kb = b1 - b0, kb_al = adl_host::round_up(kb + 16, 256);
    const uint64_t off_bytes = h_offsets && n ? (n + 1) * 8 : 0, off_al = adl_host::round_up(off_bytes, 256);
    const bool pin_in = !n || (adl_host::is_pinned(h_keys) && (!h_offsets || adl_host::is_pinned(h_offsets)));
    const bool pin_out = adl_host::is_pinned(h_block);
    // pinned host staging: [verify result][keys, offsets][bitmap region]; device: [keys][offsets][workspace]
    const uint64_t ho_in = 256, ho_out = ho_in + (pin_in ? 0 : kb_al + off_al);
    const uint64_t hbytes = ho_out + (pin_out ? 0 : adl_host::round_up(P.region(), 256));
    adl_host::Staging &sg = adl_host::t_stage;
    int rc = sg.reserve(hbytes, kb_al + off_al + ws_bytes);
    uint64_t *d_result = nullptr;
    if (rc == ADL_OK && nf) {
      uint8_t *d_in = sg.dev, *d_ws = sg.dev + kb_al + off_al;
      rc = [&]() -> int {
        const uint8_t *src_keys = h_keys + b0;
        const uint8_t *src_offs = reinterpret_cast<const uint8_t *>(h_offsets ? h_offsets + k0 : nullptr);
        if (!pin_in) {
          if (kb) memcpy(sg.host + ho_in, src_keys, kb);
          if (off_bytes) memcpy(sg.host + ho_in + kb_al, src_offs, off_bytes);
          src_keys = sg.host + ho_in;
          src_offs = sg.host + ho_in + kb_al;
        }
        if (kb) ADL_HIP_TRY(hipMemcpyAsync(d_in, src_keys, kb, hipMemcpyHostToDevice, st));
        if (off_bytes) ADL_HIP_TRY(hipMemcpyAsync(d_in + kb_al, src_offs, off_bytes, hipMemcpyHostToDevice, st));
        std::vector<uint64_t> local(nf + 1);
        for (uint32_t f = 0; f <= nf; ++f) local[f] = key_begin[f] - k0;
        const uint8_t *d_keys = h_offsets ? d_in - b0 : d_in;
        const uint64_t *d_offs = off_bytes ? reinterpret_cast<const uint64_t *>(d_in + kb_al) : nullptr;
        // (a block of empty var-len filters has no offsets to upload: any stride serves)
        BuildSource src;
        src.d_keys = d_keys;
        src.d_offsets = d_offs;
        src.key_stride = d_offs ? 0 : (key_stride ? key_stride : 16);
        if (int r = enqueue_build(c, t->it, P, src, local.data(), nf, bits_per_key, flags, d_ws, ws_bytes, &d_result,
                                  pin_out ? h_block : sg.host + ho_out, st))
          return r;
        if (flags & ADL_BLOOM_CACHE_VERIFY)
          ADL_HIP_TRY(hipMemcpyAsync(sg.host, d_result, 16, hipMemcpyDeviceToHost, st));
        return ADL_OK;
      }();
      // every exit waits for what was enqueued: nothing reads the caller's
      // keys, writes its block or the arena range once this call has returned
      if (hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
      if (rc != ADL_OK) (void)hipGetLastError();
    }
    if (rc == ADL_OK && nf && (flags & ADL_BLOOM_CACHE_VERIFY)) {
      uint64_t res[2];
      memcpy(res, sg.host, 16);
      if (res[0]) {
        report_missing(res[0], res[1]);
        rc = ADL_FILTER_BLOCK_ERROR;
      }
    }
    if (rc != ADL_OK) {
      release_range(c, t->it);
      delete t;
      return rc;
    }
    if (!pin_out && P.region()) memcpy(h_block, sg.host + ho_out, P.region());
    frame_trailer(h_block, P, nf, bits_per_key);
    *ticket = t;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_build_device(adl_bloom_filter_cache *c, const uint8_t *d_keys, const uint64_t *d_offsets,
                                        uint32_t key_stride, const uint64_t *key_begin, uint32_t num_filters,
                                        int32_t bits_per_key, uint32_t flags, void *d_workspace,
                                        uint64_t workspace_bytes, uint8_t *h_block, uint64_t block_bytes,
                                        adl_bloom_cache_ticket **ticket, void *stream) {
  if (flags & ~kKnownFlags) return ADL_ERR_INVALID_ARG;
  if (!c || !key_begin || !ticket || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  *ticket = nullptr;
  try {
    const uint32_t nf = num_filters;
    BlockPlan P;
    if (int rc = plan_block(key_begin, nf, bits_per_key, P)) return rc;
    if (h_block && block_bytes < P.block_bytes) return ADL_ERR_INVALID_ARG;
    if (key_begin[nf] > key_begin[0] && (!d_keys || (!d_offsets && key_stride == 0))) return ADL_ERR_INVALID_ARG;
    const uint64_t need = adl_bloom_filter_cache_build_workspace_bytes(key_begin, nf, bits_per_key);
    if (!need) return ADL_ERR_TOO_LARGE;
    if (!d_workspace || reinterpret_cast<uintptr_t>(d_workspace) % 256 || workspace_bytes < need)
      return ADL_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    auto *t = new adl_bloom_cache_ticket;
    const bool verify = nf && (flags & ADL_BLOOM_CACHE_VERIFY);
    int rc = hipEventCreateWithFlags(&t->done, hipEventDisableTiming) == hipSuccess ? ADL_OK : ADL_ERR_DEVICE;
    if (rc == ADL_OK && verify) {  // a pinned slot the result is copied into, read by publish
      std::lock_guard<std::mutex> g(c->mu);
      if (!c->verify_slots) {
        if (hipHostMalloc((void **)&c->verify_slots, kVerifySlots * 16, hipHostMallocDefault) == hipSuccess) {
          for (uint32_t s = kVerifySlots; s-- > 0;) c->verify_free.push_back(s);
        } else {
          c->verify_slots = nullptr;
          (void)hipGetLastError();
        }
      }
      if (c->verify_free.empty()) {
        rc = ADL_ERR_OUT_OF_MEMORY;
      } else {
        t->slot = (int32_t)c->verify_free.back();
        c->verify_free.pop_back();
      }
    }
    const uint64_t size = adl_host::round_up(std::max(P.block_bytes, P.region() + 1), kAlign);
    bool reserved = false;
    if (rc == ADL_OK) {
      rc = reserve_range(c, size, std::vector<uint64_t>(P.off), (uint8_t)adl_host::num_probes(bits_per_key), t->it);
      reserved = rc == ADL_OK;
    }
    if (rc == ADL_OK && nf) {
      rc = [&]() -> int {
        uint64_t *d_result = nullptr;
        BuildSource src;
        src.d_keys = d_keys;
        src.d_offsets = d_offsets;
        src.key_stride = key_stride;
        if (int r = enqueue_build(c, t->it, P, src, key_begin, nf, bits_per_key, flags,
                                  static_cast<uint8_t *>(d_workspace), workspace_bytes, &d_result, h_block, st))
          return r;
        if (verify)
          ADL_HIP_TRY(hipMemcpyAsync(c->verify_slots + 2 * (size_t)t->slot, d_result, 16, hipMemcpyDeviceToHost, st));
        return ADL_OK;
      }();
    }
    if (rc == ADL_OK && hipEventRecord(t->done, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    if (rc != ADL_OK) {
      // what was enqueued may still write the range: it ends before the range goes back
      if (reserved) (void)hipStreamSynchronize(st);
      (void)hipGetLastError();
      if (reserved) {
        release_range(c, t->it, t->slot);
      } else if (t->slot >= 0) {
        std::lock_guard<std::mutex> g(c->mu);
        c->verify_free.push_back((uint32_t)t->slot);
      }
      if (t->done) (void)hipEventDestroy(t->done);
      delete t;
      return rc;
    }
    if (h_block) frame_trailer(h_block, P, nf, bits_per_key);  // (behind the bytes the D2H writes)
    *ticket = t;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// The write-through build with a stream as its key source: as
// adl_bloom_filter_cache_build, with nothing to upload -- the filters are
// built from the stream's pairs into the reserved range, and with
// ADL_BLOOM_CACHE_VERIFY every pair is probed again.
int adl_bloom_filter_cache_build_stream(adl_bloom_filter_cache *c, adl_bloom_stream *s, int32_t bits_per_key,
                                        uint32_t flags, uint8_t *h_block, uint64_t block_capacity,
                                        uint64_t *block_bytes, adl_bloom_cache_ticket **ticket, void *stream) {
  if (flags & ~kKnownFlags) return ADL_ERR_INVALID_ARG;
  if (!c || !s || !h_block || !block_bytes || !ticket || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  *ticket = nullptr;
  *block_bytes = 0;
  try {
    uint32_t nf = 0;
    if (int rc = adl_bloom_stream_counts(s, &nf, nullptr, 0)) return rc;
    std::vector<uint64_t> kb((size_t)nf + 1, 0);
    if (int rc = adl_bloom_stream_counts(s, &nf, kb.data(), nf + 1)) return rc;
    BlockPlan P;
    if (int rc = plan_block(kb.data(), nf, bits_per_key, P)) return rc;
    *block_bytes = P.block_bytes;
    if (block_capacity < P.block_bytes) return ADL_ERR_INVALID_ARG;
    const uint64_t ws_bytes = adl_bloom_filter_cache_build_workspace_bytes(kb.data(), nf, bits_per_key);
    if (!ws_bytes) return ADL_ERR_TOO_LARGE;
    auto *t = new adl_bloom_cache_ticket;
    const uint64_t size = adl_host::round_up(std::max(P.block_bytes, P.region() + 1), kAlign);
    if (int rc = reserve_range(c, size, std::vector<uint64_t>(P.off), (uint8_t)adl_host::num_probes(bits_per_key),
                               t->it)) {
      delete t;
      return rc;
    }
    hipStream_t st = adl_host::sync_stream(stream);
    const bool pin_out = adl_host::is_pinned(h_block);
    // pinned host staging: [verify result][bitmap region]; device: the workspace
    const uint64_t ho_out = 256, hbytes = ho_out + (pin_out ? 0 : adl_host::round_up(P.region(), 256));
    adl_host::Staging &sg = adl_host::t_stage;
    int rc = sg.reserve(hbytes, ws_bytes);
    if (rc == ADL_OK && nf) {
      rc = [&]() -> int {
        BuildSource src;
        src.from_pairs = true;
        const void *pairs = nullptr;
        std::vector<uint64_t> kb2;
        if (int r = adl_host::stream_acquire(s, st, &pairs, kb2, &src.pair_dedup)) return r;
        src.d_pairs = static_cast<const uint2 *>(pairs);
        uint64_t *d_result = nullptr;
        if (int r = enqueue_build(c, t->it, P, src, kb.data(), nf, bits_per_key, flags, sg.dev, ws_bytes, &d_result,
                                  pin_out ? h_block : sg.host + ho_out, st))
          return r;
        if (flags & ADL_BLOOM_CACHE_VERIFY)
          ADL_HIP_TRY(hipMemcpyAsync(sg.host, d_result, 16, hipMemcpyDeviceToHost, st));
        return adl_host::stream_release(s, st);
      }();
      // every exit waits for what was enqueued (the block, the arena range, the stream's pairs)
      if (hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
      if (rc != ADL_OK) (void)hipGetLastError();
    }
    if (rc == ADL_OK && nf && (flags & ADL_BLOOM_CACHE_VERIFY)) {
      uint64_t res[2];
      memcpy(res, sg.host, 16);
      if (res[0]) {
        report_missing(res[0], res[1]);
        rc = ADL_FILTER_BLOCK_ERROR;
      }
    }
    if (rc != ADL_OK) {
      release_range(c, t->it);
      delete t;
      return rc;
    }
    if (!pin_out && P.region()) memcpy(h_block, sg.host + ho_out, P.region());
    frame_trailer(h_block, P, nf, bits_per_key);
    *ticket = t;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_publish(adl_bloom_filter_cache *c, adl_bloom_cache_ticket *t, const char *oid,
                                   uint64_t oid_len) {
  if (!c || !t || !oid) return ADL_ERR_INVALID_ARG;
  try {
    const std::string key(oid, oid_len);
    int rc = ADL_OK;
    // the build's kernels have written the range before it can be probed
    if (t->done) {
      if (hipEventSynchronize(t->done) != hipSuccess) {
        rc = ADL_ERR_DEVICE;
        (void)hipGetLastError();
      }
      (void)hipEventDestroy(t->done);
    }
    if (rc == ADL_OK && t->slot >= 0) {
      const uint64_t missing = c->verify_slots[2 * (size_t)t->slot], first = c->verify_slots[2 * (size_t)t->slot + 1];
      if (missing) {
        report_missing(missing, first);
        rc = ADL_FILTER_BLOCK_ERROR;
      }
    }
    if (rc != ADL_OK) {
      release_range(c, t->it, t->slot);
    } else {
      std::lock_guard<std::mutex> g(c->mu);
      if (t->slot >= 0) c->verify_free.push_back((uint32_t)t->slot);
      // The invariant the resident probe server rests on: every write of the
      // arena is followed by an epoch bump before any probe can resolve the
      // written range.  Here the writes are the build's kernels, not an H2D
      // copy: they completed above (the host variant synchronised its stream
      // before it made the ticket, the device variant's event has fired), the
      // bump (release order) happens in publish() under this lock, and only
      // then does the index name the range.  A probe that resolves it reads
      // the epoch (acquire) afterwards, and the server invalidates its caches
      // before it reads bits of a range written since it last did.
      c->publish(t->it, key);
    }
    delete t;
    return rc;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_filter_cache_abandon(adl_bloom_filter_cache *c, adl_bloom_cache_ticket *t) {
  if (!c || !t) return ADL_ERR_INVALID_ARG;
  if (t->done) {  // the range is not reused while the build still writes it
    if (hipEventSynchronize(t->done) != hipSuccess) (void)hipGetLastError();
    (void)hipEventDestroy(t->done);
  }
  release_range(c, t->it, t->slot);
  delete t;
  return ADL_OK;
}

int adl_bloom_verify_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n, uint32_t key_stride,
                            const uint64_t *d_key_begin, uint32_t num_filters, const uint8_t *d_bitmaps,
                            const uint64_t *d_begin, const uint64_t *d_end, int32_t bits_per_key,
                            uint64_t *d_result, void *stream) {
  if (!d_result || bits_per_key < 0 || reinterpret_cast<uintptr_t>(d_result) % 8) return ADL_ERR_INVALID_ARG;
  if (n && num_filters && (!d_keys || !d_key_begin || !d_bitmaps || !d_begin)) return ADL_ERR_INVALID_ARG;
  if (n && num_filters && !d_offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  return verify_launch(d_keys, d_offsets, n, key_stride, d_key_begin, num_filters, d_bitmaps, d_begin, d_end,
                       bits_per_key, d_result, (hipStream_t)stream);
}

int adl_bloom_verify(const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n, uint32_t key_stride,
                     const uint64_t *key_begin, uint32_t num_filters, const uint8_t *h_bitmaps,
                     const uint64_t *h_bitmap_off, int32_t bits_per_key, uint64_t *missing, uint64_t *first_missing,
                     void *stream) {
  if (!missing || !first_missing || bits_per_key < 0) return ADL_ERR_INVALID_ARG;
  *missing = 0;
  *first_missing = ~0ull;
  if (n == 0 || num_filters == 0) return ADL_OK;
  if (!h_keys || !key_begin || !h_bitmap_off || (!h_offsets && key_stride == 0)) return ADL_ERR_INVALID_ARG;
  for (uint32_t f = 0; f < num_filters; ++f)
    if (key_begin[f + 1] < key_begin[f] || h_bitmap_off[f + 1] < h_bitmap_off[f]) return ADL_ERR_INVALID_ARG;
  const uint64_t bm_bytes = h_bitmap_off[num_filters];
  if (bm_bytes && !h_bitmaps) return ADL_ERR_INVALID_ARG;
  try {
    hipStream_t st = adl_host::sync_stream(stream);
    const uint64_t tab = ((uint64_t)num_filters + 1) * 8;
    adl_host::StagePlan plan;
    const adl_host::KeyBlock kb(plan, h_offsets, n, key_stride);
    const uint64_t o_kb = plan.take(tab);
    const uint64_t o_bo = plan.take(tab);
    const uint64_t o_bm = plan.take(bm_bytes + 16);
    const uint64_t o_res = plan.take(16);  // the end of the upload
    adl_host::Staging &sg = adl_host::t_stage;
    if (int rc = sg.reserve(plan.end, plan.end)) return rc;
    kb.fill(sg.host, h_keys, h_offsets);
    memcpy(sg.host + o_kb, key_begin, tab);
    memcpy(sg.host + o_bo, h_bitmap_off, tab);
    if (bm_bytes) memcpy(sg.host + o_bm, h_bitmaps, bm_bytes);
    if (hipMemcpyAsync(sg.dev, sg.host, o_res, hipMemcpyHostToDevice, st) != hipSuccess) return ADL_ERR_DEVICE;
    uint64_t *d_res = reinterpret_cast<uint64_t *>(sg.dev + o_res);
    int rc = verify_launch(sg.dev, kb.offsets(sg.dev), n, key_stride, reinterpret_cast<uint64_t *>(sg.dev + o_kb),
                           num_filters, sg.dev + o_bm, reinterpret_cast<uint64_t *>(sg.dev + o_bo), nullptr,
                           bits_per_key, d_res, st);
    if (rc == ADL_OK && hipMemcpyAsync(sg.host + o_res, d_res, 16, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = ADL_ERR_DEVICE;
    if (hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
    if (rc) return rc;
    memcpy(missing, sg.host + o_res, 8);
    memcpy(first_missing, sg.host + o_res + 8, 8);
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

}  // extern "C"

// adlsm-tree_amd/csrc/stream_build.hip -- streamed filter build: keys are
// hashed as they arrive, the build starts from the stored hash pairs.
//
// The caller the build layer exists for, SSTableWriter::Add ->
// FilterBlockWriter::Update (reference src/sstable.cpp:28,
// src/filter_block.cpp:72-75), produces keys one at a time over the life of a
// table, and the filter's size (n*bpk+7 bytes) is known only at Final
// (src/filter_block.cpp:104-109, src/sstable.cpp:58).  Positions need m, the
// two murmur hashes of a key do not: an adl_bloom_stream takes keys in
// batches while the table fills, keeps 8 bytes per key on the device -- pair i
// of the i-th appended key, in one contiguous array -- and its finish runs
// the segmented build's two passes over those pairs (bloom_build.hip:
// SrcP / KeysPair).  A finish uploads and hashes nothing.
//
// An append hashes its batch with hash_pairs_device (hash_pairs.hip), pairs
// written at store + count + i in key order.  A 16-byte-aligned key buffer is
// read in whole blocks (up to 15 bytes past the batch's last key), any other
// one byte-exactly (include/adl_bloom.h).
//
// Ordering: every append records the object's append event on its stream and
// waits for the previous one (the store's growth and the upload buffer are
// reused in that order); a finish waits for the last append's event and for
// the previous finish's, and records its own, which the first append after a
// reset waits for (it overwrites pairs a finish on another stream may still
// read; the chain makes the one event stand for every finish so far).
//
// Buffers the object has outgrown are not freed where they are replaced (the
// growth copy and earlier appends may still read them, and hipFree waits for
// every stream of the device, so also for a resident probe server's kernel;
// see UploadRing, bloom_common.hpp): reset frees them once the object's last
// append and finish have completed, destroy frees the rest.  The store at
// least doubles, so what it has retired adds up to less than the store in use.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bloom_common.hpp"

constexpr uint64_t kMinStoreKeys = 4096;

struct adl_bloom_stream {
  uint2 *store = nullptr;
  uint64_t cap = 0, count = 0, reserve = 0;
  std::vector<uint64_t> bounds{0};  // as FilterBlockWriter::bounds_: closed filters end here
  uint8_t *inbox = nullptr;         // a host batch's keys and offsets on the device
  uint64_t inbox_cap = 0;
  hipEvent_t ev_app = nullptr, ev_fin = nullptr;
  bool app_used = false, fin_used = false;
  bool fin_wait = false;  // reset since a finish: appends overwrite pairs it may still read
  bool all16 = true;  // every key so far came as a 16-byte key
  std::vector<void *> retired;
};

namespace {

// key_begin of every filter so far; an open tail is a last filter
std::vector<uint64_t> stream_bounds(const adl_bloom_stream *s) {
  std::vector<uint64_t> kb = s->bounds;
  if (s->count > kb.back()) kb.push_back(s->count);
  return kb;
}

// `st` waits for whatever used the store and the inbox last
int order_behind(adl_bloom_stream *s, hipStream_t st) {
  if (!s->ev_app) ADL_HIP_TRY(hipEventCreateWithFlags(&s->ev_app, hipEventDisableTiming));
  if (!s->ev_fin) ADL_HIP_TRY(hipEventCreateWithFlags(&s->ev_fin, hipEventDisableTiming));
  if (s->app_used) ADL_HIP_TRY(hipStreamWaitEvent(st, s->ev_app, 0));
  if (s->fin_wait) ADL_HIP_TRY(hipStreamWaitEvent(st, s->ev_fin, 0));
  return ADL_OK;
}

bool stream_hash_dedup(const adl_bloom_stream *s) {
  const uint32_t dd = adl_host::knobs().stream_hash_dedup;
  return dd == 2 ? s->all16 : dd != 0;
}

// room for n more pairs; the copy into a larger store runs on st (which has
// waited for the last append), and the old store is retired, not freed
int grow_store(adl_bloom_stream *s, uint64_t n, hipStream_t st) {
  const uint64_t need = s->count + n;
  if (need <= s->cap) return ADL_OK;
  const uint64_t want = std::max({need, 2 * s->cap, s->reserve, kMinStoreKeys});
  uint2 *nw = nullptr;
  ADL_HIP_TRY(hipMalloc((void **)&nw, want * sizeof(uint2)));
  if (s->count) {
    const hipError_t e = hipMemcpyAsync(nw, s->store, s->count * sizeof(uint2), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      (void)hipFree(nw);
      return ADL_ERR_DEVICE;
    }
  }
  if (s->store) s->retired.push_back(s->store);
  s->store = nw;
  s->cap = want;
  return ADL_OK;
}

int grow_inbox(adl_bloom_stream *s, uint64_t bytes) {
  if (bytes <= s->inbox_cap) return ADL_OK;
  const uint64_t want = adl_host::round_up(std::max(bytes, 2 * s->inbox_cap), 1 << 16);
  uint8_t *nw = nullptr;
  ADL_HIP_TRY(hipMalloc((void **)&nw, want));
  if (s->inbox) s->retired.push_back(s->inbox);
  s->inbox = nw;
  s->inbox_cap = want;
  return ADL_OK;
}

// Hashes a device-resident batch into the store; `whole`: the key buffer may
// be read in whole aligned 16-byte blocks.
int launch_append(adl_bloom_stream *s, const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                  uint32_t key_stride, bool whole, hipStream_t st) {
  if (int rc = adl_host::hash_pairs_device(d_keys, d_offsets, key_stride, n, whole, s->store + s->count, st)) return rc;
  ADL_HIP_TRY(hipEventRecord(s->ev_app, st));
  s->app_used = true;
  s->fin_wait = false;  // this append waited for the finishes; later ones are ordered behind it
  s->count += n;
  if (d_offsets || key_stride != 16) s->all16 = false;
  return ADL_OK;
}

int check_append(const adl_bloom_stream *s, const void *keys, const uint64_t *offsets, uint64_t n, uint32_t key_stride) {
  if (!s) return ADL_ERR_INVALID_ARG;
  if (n == 0) return ADL_OK;
  if (!keys) return ADL_ERR_INVALID_ARG;
  if (!offsets && key_stride == 0) return ADL_ERR_INVALID_ARG;
  if (n > 0x7fffffffull || s->count + n > 0xffffffffull) return ADL_ERR_TOO_LARGE;
  return ADL_OK;
}

int check_finish(const adl_bloom_stream *s, int32_t bpk, uint32_t flags, const void *bitmaps, const uint64_t *bitmap_off) {
  if (!s || !bitmaps || !bitmap_off || bpk < 0) return ADL_ERR_INVALID_ARG;
  if (flags & ~(uint32_t)ADL_BLOOM_SKIP_ADJACENT_DUPLICATES) return ADL_ERR_INVALID_ARG;
  if (s->bounds.size() == 1 && s->count == 0) return ADL_ERR_INVALID_ARG;  // no filter
  return ADL_OK;
}

int finish_device(adl_bloom_stream *s, const std::vector<uint64_t> &kb, int32_t bpk, uint32_t flags, uint8_t *d_bitmaps,
                  const uint64_t *bitmap_off, void *d_workspace, uint64_t workspace_bytes, hipStream_t st) {
  const uint32_t nf = (uint32_t)(kb.size() - 1);
  for (uint32_t f = 0; f < nf; ++f) {
    if (bitmap_off[f] % 16) return ADL_ERR_INVALID_ARG;
    if (!adl_host::bitmap_bytes(kb[f + 1] - kb[f], bpk)) return ADL_ERR_TOO_LARGE;
  }
  // (a short workspace is refused before anything is enqueued)
  std::vector<uint64_t> counts(nf);
  for (uint32_t f = 0; f < nf; ++f) counts[f] = kb[f + 1] - kb[f];
  const uint64_t need = adl_bloom_build_workspace_bytes(counts.data(), nf, bpk);
  if (!need) return ADL_ERR_TOO_LARGE;
  if (!d_workspace || workspace_bytes < need) return ADL_ERR_WORKSPACE;
  if (int rc = order_behind(s, st)) return rc;
  // (finishes chain: ev_fin then stands for every finish so far, so an append
  // after a reset that waits for it waits for them all)
  if (s->fin_used) ADL_HIP_TRY(hipStreamWaitEvent(st, s->ev_fin, 0));
  // the repeated-pair table pays for 16-byte keys only (bloom_build.hip; DESIGN.md §5, streamed build)
  if (int rc = adl_host::adl_build_pairs_device(s->store, kb.data(), nf, bpk, d_bitmaps, bitmap_off, flags,
                                                stream_hash_dedup(s), d_workspace, workspace_bytes, st))
    return rc;
  ADL_HIP_TRY(hipEventRecord(s->ev_fin, st));
  s->fin_used = true;
  return ADL_OK;
}

}  // namespace

int adl_host::stream_acquire(adl_bloom_stream *s, hipStream_t st, const void **d_pairs,
                             std::vector<uint64_t> &key_begin, bool *hash_dedup) {
  if (int rc = order_behind(s, st)) return rc;
  if (s->fin_used) ADL_HIP_TRY(hipStreamWaitEvent(st, s->ev_fin, 0));
  *d_pairs = s->store;
  key_begin = stream_bounds(s);
  *hash_dedup = stream_hash_dedup(s);
  return ADL_OK;
}

int adl_host::stream_release(adl_bloom_stream *s, hipStream_t st) {
  ADL_HIP_TRY(hipEventRecord(s->ev_fin, st));
  s->fin_used = true;
  return ADL_OK;
}

// ====================================================================== C-ABI
extern "C" {

int adl_bloom_stream_create(uint64_t reserve_keys, adl_bloom_stream **stream_out) {
  if (!stream_out) return ADL_ERR_INVALID_ARG;
  *stream_out = nullptr;
  if (reserve_keys > 0xffffffffull) return ADL_ERR_TOO_LARGE;
  try {
    adl_bloom_stream *s = new adl_bloom_stream();
    s->reserve = reserve_keys;
    *stream_out = s;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_stream_destroy(adl_bloom_stream *s) {
  if (!s) return ADL_ERR_INVALID_ARG;
  // (hipFree waits for the device, and so for the appends and finishes in flight)
  if (s->app_used) (void)hipEventSynchronize(s->ev_app);
  if (s->fin_used) (void)hipEventSynchronize(s->ev_fin);
  if (s->store) (void)hipFree(s->store);
  if (s->inbox) (void)hipFree(s->inbox);
  for (void *p : s->retired) (void)hipFree(p);
  if (s->ev_app) (void)hipEventDestroy(s->ev_app);
  if (s->ev_fin) (void)hipEventDestroy(s->ev_fin);
  delete s;
  return ADL_OK;
}

int adl_bloom_stream_reset(adl_bloom_stream *s) {
  if (!s) return ADL_ERR_INVALID_ARG;
  s->count = 0;
  s->bounds.assign(1, 0);
  s->all16 = true;
  s->fin_wait = s->fin_used;
  // Outgrown buffers go once nothing of the object is in flight (their last
  // readers, a growth copy or a finish, are behind these events); otherwise
  // they wait for a later reset or for destroy.  (Queries only: no wait here.)
  if (!s->retired.empty()) {
    if ((!s->app_used || hipEventQuery(s->ev_app) == hipSuccess) &&
        (!s->fin_used || hipEventQuery(s->ev_fin) == hipSuccess)) {
      for (void *p : s->retired) (void)hipFree(p);
      s->retired.clear();
    }
    (void)hipGetLastError();  // (hipErrorNotReady of a query is no error)
  }
  return ADL_OK;
}

int adl_bloom_stream_append(adl_bloom_stream *s, const uint8_t *h_keys, const uint64_t *h_offsets, uint64_t n,
                            uint32_t key_stride, void *stream) {
  try {
    if (int rc = check_append(s, h_keys, h_offsets, n, key_stride)) return rc;
    if (n == 0) return ADL_OK;
    // the batch in one pinned slot: the key bytes at their alignment mod 16
    // (+16: the run's whole-block loads of the last key stay inside), then the
    // offsets as they are (the device key pointer is shifted back instead)
    const uint64_t b0 = h_offsets ? h_offsets[0] : 0;
    const uint64_t b1 = h_offsets ? h_offsets[n] : n * (uint64_t)key_stride;
    if (b1 < b0) return ADL_ERR_INVALID_ARG;
    const uint64_t pad = b0 & 15u;
    const uint64_t o_offs = adl_host::round_up(pad + (b1 - b0) + 16, 256);
    const uint64_t total = o_offs + (h_offsets ? (n + 1) * 8 : 0);
    if (h_offsets)  // the kernel trusts them
      for (uint64_t i = 0; i < n; ++i)
        if (h_offsets[i + 1] < h_offsets[i]) return ADL_ERR_INVALID_ARG;
    hipStream_t st = adl_host::sync_stream(stream);  // NULL: the calling thread's own stream, as for every host-pointer call
    if (int rc = order_behind(s, st)) return rc;
    if (int rc = grow_store(s, n, st)) return rc;
    if (int rc = grow_inbox(s, total)) return rc;
    uint8_t *h = nullptr;
    if (int rc = adl_host::t_upload.begin(total, &h)) return rc;
    if (b1 > b0) memcpy(h + pad, h_keys + b0, b1 - b0);
    if (h_offsets) memcpy(h + o_offs, h_offsets, (n + 1) * 8);
    if (int rc = adl_host::t_upload.commit(s->inbox, total, st)) return rc;
    const uint8_t *d_keys = s->inbox + pad - b0;
    const uint64_t *d_offs = h_offsets ? reinterpret_cast<const uint64_t *>(s->inbox + o_offs) : nullptr;
    return launch_append(s, d_keys, d_offs, n, key_stride, true, st);
  } catch (...) {
    return ADL_ERR_DEVICE;
  }
}

int adl_bloom_stream_append_device(adl_bloom_stream *s, const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t n,
                                   uint32_t key_stride, void *stream) {
  try {
    if (int rc = check_append(s, d_keys, d_offsets, n, key_stride)) return rc;
    if (n == 0) return ADL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_behind(s, st)) return rc;
    if (int rc = grow_store(s, n, st)) return rc;
    return launch_append(s, d_keys, d_offsets, n, key_stride, reinterpret_cast<uintptr_t>(d_keys) % 16 == 0, st);
  } catch (...) {
    return ADL_ERR_DEVICE;
  }
}

int adl_bloom_stream_cut(adl_bloom_stream *s) {
  if (!s) return ADL_ERR_INVALID_ARG;
  try {
    s->bounds.push_back(s->count);
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

int adl_bloom_stream_counts(const adl_bloom_stream *s, uint32_t *num_filters, uint64_t *key_begin, uint32_t capacity) {
  if (!s || !num_filters) return ADL_ERR_INVALID_ARG;
  try {
    const std::vector<uint64_t> kb = stream_bounds(s);
    *num_filters = (uint32_t)(kb.size() - 1);
    if (!key_begin) return ADL_OK;
    if (capacity < kb.size()) return ADL_ERR_INVALID_ARG;
    std::copy(kb.begin(), kb.end(), key_begin);
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

uint64_t adl_bloom_stream_finish_workspace_bytes(const adl_bloom_stream *s, int32_t bits_per_key) {
  if (!s || bits_per_key < 0) return 0;
  try {
    const std::vector<uint64_t> kb = stream_bounds(s);
    std::vector<uint64_t> counts(kb.size() - 1);
    for (size_t f = 0; f + 1 < kb.size(); ++f) counts[f] = kb[f + 1] - kb[f];
    return adl_bloom_build_workspace_bytes(counts.data(), (uint32_t)counts.size(), bits_per_key);
  } catch (...) {
    return 0;
  }
}

int adl_bloom_stream_finish_device(adl_bloom_stream *s, int32_t bits_per_key, uint32_t flags, uint8_t *d_bitmaps,
                                   const uint64_t *bitmap_off, void *d_workspace, uint64_t workspace_bytes,
                                   void *stream) {
  try {
    if (int rc = check_finish(s, bits_per_key, flags, d_bitmaps, bitmap_off)) return rc;
    if (reinterpret_cast<uintptr_t>(d_bitmaps) % 16) return ADL_ERR_INVALID_ARG;
    return finish_device(s, stream_bounds(s), bits_per_key, flags, d_bitmaps, bitmap_off, d_workspace, workspace_bytes,
                         (hipStream_t)stream);
  } catch (...) {
    return ADL_ERR_DEVICE;
  }
}

int adl_bloom_stream_finish(adl_bloom_stream *s, int32_t bits_per_key, uint32_t flags, uint8_t *h_bitmaps,
                            const uint64_t *h_bitmap_off, void *stream) {
  try {
    if (int rc = check_finish(s, bits_per_key, flags, h_bitmaps, h_bitmap_off)) return rc;
    const std::vector<uint64_t> kb = stream_bounds(s);
    const uint32_t nf = (uint32_t)(kb.size() - 1);
    std::vector<uint64_t> dev_off(nf), counts(nf);
    uint64_t out_bytes = 0;
    for (uint32_t f = 0; f < nf; ++f) {
      counts[f] = kb[f + 1] - kb[f];
      const uint64_t b = adl_host::bitmap_bytes(counts[f], bits_per_key);
      if (!b) return ADL_ERR_TOO_LARGE;
      dev_off[f] = out_bytes;
      out_bytes += adl_host::round_up(b, 16);
    }
    const uint64_t ws_bytes = adl_bloom_build_workspace_bytes(counts.data(), nf, bits_per_key);
    if (!ws_bytes) return ADL_ERR_TOO_LARGE;
    // the calling thread's staging: the device bitmaps, then the workspace
    adl_host::StagePlan sp;
    sp.take(out_bytes);
    const uint64_t o_ws = sp.take(ws_bytes);
    adl_host::Staging &sg = adl_host::t_stage;
    if (int rc = sg.reserve(out_bytes, sp.end)) return rc;
    hipStream_t st = adl_host::sync_stream(stream);
    int rc = finish_device(s, kb, bits_per_key, flags, sg.dev, dev_off.data(), sg.dev + o_ws, ws_bytes, st);
    if (rc == ADL_OK) {
      const hipError_t e = hipMemcpyAsync(sg.host, sg.dev, out_bytes, hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) rc = ADL_ERR_DEVICE;
    }
    // (every exit waits for what it enqueued on the staging buffers)
    if (hipStreamSynchronize(st) != hipSuccess && rc == ADL_OK) rc = ADL_ERR_DEVICE;
    if (rc) return rc;
    for (uint32_t f = 0; f < nf; ++f)
      memcpy(h_bitmaps + h_bitmap_off[f], sg.host + dev_off[f], adl_host::bitmap_bytes(counts[f], bits_per_key));
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_DEVICE;
  }
}

}  // extern "C"

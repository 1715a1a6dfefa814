// adlsm-tree_amd/csrc/level_index.hip -- the resident level index: which
// tables of a level a multi-get has to ask, selected on the device.
//
// Level::Get (src/revision.cpp:265-310) walks the level's files newest first
// and skips a table whose [min_inner_key, max_inner_key] range does not cover
// the lookup key (:279-287).  The candidate list of a key depends on where the
// key falls among the tables' boundary user keys (level_index_core.hpp), so
// the level is described once -- adl_bloom_level_create, where a revision
// installs it -- and asked about many times.  The device copy holds the
// boundary prefixes, their bytes, the region lists and the tables' max
// (seq, op); a batch then sends only its keys, and three launches turn them
// into the (pair_begin, pair_table) arrays the fan-out probe consumes:
//
//   level_locate_kernel  one lane per key: binary search of the boundaries
//                        (16-byte big-endian prefix, the whole bytes on a tie),
//                        its region and its candidate count at `seq`; one total
//                        per workgroup
//   level_scan_kernel    ONE workgroup: exclusive scan of the workgroup totals
//   level_expand_kernel  pair_begin, and the lists copied out with the lanes
//                        striding over a workgroup's pairs, so a key with
//                        hundreds of candidates is spread over the workgroup
//
// No workgroup ever waits on another: the hand-offs are launch boundaries.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <string_view>

#include "bloom_common.hpp"
#include "level_index_device.hpp"
#include "level_index_impl.hpp"

namespace {

using adl_level::kTableMask;
using namespace adl_level_dev;  // LevelDev, KeySet, the prefix, the comparison and the search

// One lane per key: region[i], count[i] (its candidates at seq), and
// block_total[blockIdx.x].  The grid covers the keys exactly (no grid stride:
// workgroup b owns keys [256 b, 256 b + 256), as in the expand kernel).
__global__ __launch_bounds__(kBlockL) void level_locate_kernel(KeySet ks, uint64_t nkeys, LevelDev lv, int64_t seq,
                                                               uint32_t *__restrict__ region,
                                                               uint32_t *__restrict__ count,
                                                               uint64_t *__restrict__ block_total) {
  __shared__ uint64_t spref[2 * kLdsBoundaries];
  __shared__ uint32_t scratch[kBlockL / adl_dev::kWave + 1];
  const bool lds_pref = lv.nb <= kLdsBoundaries;
  if (lds_pref) {
    for (uint32_t j = threadIdx.x; j < 2 * lv.nb; j += kBlockL) spref[j] = lv.pref[j];
    __syncthreads();
  }
  const uint64_t i = blockIdx.x * (uint64_t)kBlockL + threadIdx.x;
  uint32_t cnt = 0;
  if (i < nkeys) {
    uint32_t klen;
    const uint8_t *key = ks.at(i, klen);
    uint64_t khi, klo;
    prefix_of(key, klen, khi, klo);
    const uint32_t r = locate_region(lv, spref, lds_pref, key, klen, khi, klo);
    cnt = region_count(lv, r, seq);
    region[i] = r;
    count[i] = cnt;
  }
  uint32_t total;
  (void)adl_dev::block_excl_scan<kBlockL>(cnt, scratch, &total);
  if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// ONE workgroup: block_off = exclusive scan of block_total (u64), *num_pairs =
// the sum.  Each thread owns a contiguous run of the entries.
__global__ __launch_bounds__(kBlockL) void level_scan_kernel(const uint64_t *__restrict__ block_total,
                                                             uint64_t nblk, uint64_t *__restrict__ block_off,
                                                             uint64_t *__restrict__ num_pairs) {
  __shared__ uint64_t ssum[kBlockL];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (nblk + kBlockL - 1) / kBlockL;
  const uint64_t b0 = t * per < nblk ? t * per : nblk;
  const uint64_t b1 = b0 + per < nblk ? b0 + per : nblk;
  uint64_t s = 0;
  for (uint64_t b = b0; b < b1; ++b) s += block_total[b];
  ssum[t] = s;
  __syncthreads();
  // inclusive scan of the 256 run sums
  for (uint32_t d = 1; d < kBlockL; d <<= 1) {
    const uint64_t add = t >= d ? ssum[t - d] : 0;
    __syncthreads();
    ssum[t] += add;
    __syncthreads();
  }
  uint64_t run = ssum[t] - s;
  for (uint64_t b = b0; b < b1; ++b) {
    const uint64_t v = block_total[b];
    block_off[b] = run;
    run += v;
  }
  if (t == kBlockL - 1) *num_pairs = ssum[t];
}

// Workgroup b writes pair_begin of its 256 keys and copies their lists out:
// pair p of the workgroup is found by an upper-bound search of the keys'
// starts in LDS (as the fan-out probe finds a pair's key), so every lane
// copies one entry per round however the candidates are spread over the keys.
// A key some of whose entries are dropped at `seq` (it equals a boundary at
// which a table ends) is copied by its own lane instead, which skips them.
// Pairs at pair_capacity and beyond are not written.
__global__ __launch_bounds__(kBlockL) void level_expand_kernel(uint64_t nkeys, LevelDev lv, int64_t seq,
                                                               const uint32_t *__restrict__ region,
                                                               const uint32_t *__restrict__ count,
                                                               const uint64_t *__restrict__ block_off,
                                                               uint32_t *__restrict__ pair_begin,
                                                               uint32_t *__restrict__ pair_table,
                                                               uint64_t pair_capacity) {
  __shared__ uint32_t sstart[kBlockL + 1], slist[kBlockL];
  __shared__ uint8_t sown[kBlockL];
  __shared__ uint32_t scratch[kBlockL / adl_dev::kWave + 1];
  const uint32_t t = threadIdx.x;
  const uint64_t kb = blockIdx.x * (uint64_t)kBlockL;
  const uint64_t i = kb + t;
  const uint32_t nk = (uint32_t)(nkeys - kb < (uint64_t)kBlockL ? nkeys - kb : (uint64_t)kBlockL);
  const uint32_t cnt = i < nkeys ? count[i] : 0u;
  uint32_t btotal;
  const uint32_t excl = adl_dev::block_excl_scan<kBlockL>(cnt, scratch, &btotal);
  const uint64_t base = block_off[blockIdx.x];
  sstart[t] = excl;
  if (t == 0) sstart[kBlockL] = btotal;
  sown[t] = 0;
  if (i < nkeys) {
    pair_begin[i] = (uint32_t)(base + excl);
    if (i == nkeys - 1) pair_begin[nkeys] = (uint32_t)(base + excl + cnt);
    const uint32_t r = region[i];
    const uint32_t l0 = lv.rbeg[r], l1 = lv.rbeg[r + 1];
    slist[t] = l0;
    if (cnt != l1 - l0) {
      sown[t] = 1;
      uint64_t w = base + excl;
      for (uint32_t p = l0; p < l1; ++p) {
        const uint32_t e = lv.rlist[p];
        if (entry_gone(lv, e, seq)) continue;
        if (w < pair_capacity) pair_table[w] = e & kTableMask;
        ++w;
      }
    }
  }
  __syncthreads();
  for (uint32_t p = t; p < btotal; p += kBlockL) {
    // the first j in [1, nk] with sstart[j] > p (sstart[nk..] = btotal > p): key j - 1 owns p
    uint32_t lo = 1, hi = nk;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sstart[mid] > p) hi = mid; else lo = mid + 1;
    }
    const uint32_t o = lo - 1;
    if (sown[o]) continue;
    const uint64_t w = base + p;
    if (w < pair_capacity) pair_table[w] = lv.rlist[slist[o] + (p - sstart[o])] & kTableMask;
  }
}

// selection's workspace: [region][count] per key, [block_total][block_off] per workgroup
uint64_t ws_layout(uint64_t num_keys, uint64_t &o_count, uint64_t &o_btot, uint64_t &o_boff) {
  const uint64_t nblk = (num_keys + kBlockL - 1) / kBlockL;
  adl_host::StagePlan p;
  p.take(num_keys * 4);
  o_count = p.take(num_keys * 4);
  o_btot = p.take(nblk * 8);
  o_boff = p.take(nblk * 8);
  return p.end + 256;
}

// the device copy, made once (under lv->mu)
int upload_locked(adl_bloom_level *lv) {
  const adl_level::Index &ix = lv->ix;
  adl_host::StagePlan plan;
  auto place = [&](uint64_t bytes) { return plan.take(bytes + 16); };  // (never empty, and byte reads stay inside)
  const uint64_t o_pref = place(16ull * ix.num_boundaries), o_bb = place(ix.bbytes.size()),
                 o_boff = place(4ull * ix.boff.size()), o_rbeg = place(4ull * ix.rbeg.size()),
                 o_rlist = place(4ull * ix.rlist.size()), o_seq = place(8ull * ix.mx_seq.size()),
                 o_op = place(ix.mx_op.size()), o = plan.end;
  // the arrays laid out in one pinned buffer and sent as one DMA (no copy from
  // pageable memory anywhere, see Staging); the buffer is the index's size and
  // used once, so it is not a thread's staging buffer
  uint8_t *h_blob = nullptr;
  if (hipHostMalloc((void **)&h_blob, o, hipHostMallocDefault) != hipSuccess) return ADL_ERR_OUT_OF_MEMORY;
  memset(h_blob, 0, o);
  auto put = [&](uint64_t at, const void *src, uint64_t bytes) {
    if (bytes) memcpy(h_blob + at, src, bytes);
  };
  static_assert(sizeof(adl_level::Pref) == 16, "prefixes upload as (hi, lo) u64 pairs");
  put(o_pref, ix.pref.data(), 16ull * ix.num_boundaries);
  put(o_bb, ix.bbytes.data(), ix.bbytes.size());
  put(o_boff, ix.boff.data(), 4ull * ix.boff.size());
  put(o_rbeg, ix.rbeg.data(), 4ull * ix.rbeg.size());
  put(o_rlist, ix.rlist.data(), 4ull * ix.rlist.size());
  put(o_seq, ix.mx_seq.data(), 8ull * ix.mx_seq.size());
  put(o_op, ix.mx_op.data(), ix.mx_op.size());
  int rc = ADL_OK;
  if (hipMalloc((void **)&lv->d_blob, o) != hipSuccess) {
    lv->d_blob = nullptr;
    rc = ADL_ERR_OUT_OF_MEMORY;
  } else {
    hipStream_t st = adl_host::sync_stream(nullptr);
    if (hipMemcpyAsync(lv->d_blob, h_blob, o, hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ADL_ERR_DEVICE;
  }
  (void)hipHostFree(h_blob);
  if (rc) return rc;
  lv->d_pref = reinterpret_cast<const uint64_t *>(lv->d_blob + o_pref);
  lv->d_bbytes = lv->d_blob + o_bb;
  lv->d_boff = reinterpret_cast<const uint32_t *>(lv->d_blob + o_boff);
  lv->d_rbeg = reinterpret_cast<const uint32_t *>(lv->d_blob + o_rbeg);
  lv->d_rlist = reinterpret_cast<const uint32_t *>(lv->d_blob + o_rlist);
  lv->d_mx_seq = reinterpret_cast<const int64_t *>(lv->d_blob + o_seq);
  lv->d_mx_op = lv->d_blob + o_op;
  return ADL_OK;
}

}  // namespace

int adl_host::level_ensure_uploaded(adl_bloom_level *lv) { return ensure_uploaded(lv, upload_locked); }

int adl_host::level_scan_launch(const uint64_t *d_block_total, uint64_t nblk, uint64_t *d_block_off, uint64_t *d_total,
                                hipStream_t st) {
  hipLaunchKernelGGL(level_scan_kernel, dim3(1), dim3(kBlockL), 0, st, d_block_total, nblk, d_block_off, d_total);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

int adl_host::level_select_device(adl_bloom_level *lv, const uint8_t *d_keys, const uint64_t *d_offsets,
                                  uint64_t num_keys, uint32_t key_stride, int64_t seq, uint32_t *d_pair_begin,
                                  uint32_t *d_pair_table, uint64_t pair_capacity, uint64_t *d_num_pairs,
                                  void *d_workspace, uint64_t workspace_bytes, hipStream_t st) {
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;  // pair_begin is u32, one entry per key and one more
  uint64_t o_count, o_btot, o_boff;
  if (workspace_bytes < ws_layout(num_keys, o_count, o_btot, o_boff)) return ADL_ERR_WORKSPACE;
  if (num_keys == 0) {
    ADL_HIP_TRY(hipMemsetAsync(d_pair_begin, 0, 4, st));
    ADL_HIP_TRY(hipMemsetAsync(d_num_pairs, 0, 8, st));
    return ADL_OK;
  }
  if (int rc = level_ensure_uploaded(lv)) return rc;
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  uint32_t *region = reinterpret_cast<uint32_t *>(ws), *count = reinterpret_cast<uint32_t *>(ws + o_count);
  uint64_t *btot = reinterpret_cast<uint64_t *>(ws + o_btot), *boff = reinterpret_cast<uint64_t *>(ws + o_boff);
  const LevelDev dv = lv->dev();
  const KeySet ks{d_keys, d_offsets, key_stride};
  const uint64_t nblk = (num_keys + kBlockL - 1) / kBlockL;
  hipLaunchKernelGGL(level_locate_kernel, dim3((uint32_t)nblk), dim3(kBlockL), 0, st, ks, num_keys, dv, seq, region,
                     count, btot);
  ADL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(level_scan_kernel, dim3(1), dim3(kBlockL), 0, st, btot, nblk, boff, d_num_pairs);
  ADL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(level_expand_kernel, dim3((uint32_t)nblk), dim3(kBlockL), 0, st, num_keys, dv, seq, region,
                     count, boff, d_pair_begin, d_pair_table, pair_capacity);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

extern "C" {

int adl_bloom_level_create(const char *const *oids, const uint64_t *oid_lens, const char *const *min_inner_keys,
                           const uint64_t *min_lens, const char *const *max_inner_keys, const uint64_t *max_lens,
                           uint32_t num_tables, uint64_t max_index_bytes, adl_bloom_level **level) {
  if (!level) return ADL_ERR_INVALID_ARG;
  *level = nullptr;
  if (num_tables && (!min_inner_keys || !min_lens || !max_inner_keys || !max_lens)) return ADL_ERR_INVALID_ARG;
  if (oids && num_tables && !oid_lens) return ADL_ERR_INVALID_ARG;
  try {
    std::vector<std::string_view> mins(num_tables), maxs(num_tables);
    for (uint32_t t = 0; t < num_tables; ++t) {
      if ((min_lens[t] && !min_inner_keys[t]) || (max_lens[t] && !max_inner_keys[t])) return ADL_ERR_INVALID_ARG;
      mins[t] = std::string_view(min_inner_keys[t] ? min_inner_keys[t] : "", min_lens[t]);
      maxs[t] = std::string_view(max_inner_keys[t] ? max_inner_keys[t] : "", max_lens[t]);
    }
    auto *lv = new adl_bloom_level;
    if (!adl_level::Build(mins.data(), maxs.data(), num_tables,
                          max_index_bytes ? max_index_bytes : adl_level::kDefaultIndexBytes, lv->ix)) {
      delete lv;
      return ADL_ERR_TOO_LARGE;
    }
    if (oids) {
      lv->oids.reserve(num_tables);
      for (uint32_t t = 0; t < num_tables; ++t) lv->oids.emplace_back(oids[t] ? oids[t] : "", oid_lens[t]);
    }
    *level = lv;
    return ADL_OK;
  } catch (...) {
    return ADL_ERR_OUT_OF_MEMORY;
  }
}

// No call on the level may be running or start once this is called.
int adl_bloom_level_destroy(adl_bloom_level *level) {
  if (!level) return ADL_OK;
  int rc = ADL_OK;
  if (level->d_blob && hipFree(level->d_blob) != hipSuccess) rc = ADL_ERR_DEVICE;
  delete level;
  return rc;
}

int adl_bloom_level_stats(const adl_bloom_level *level, uint32_t *regions, uint64_t *list_entries,
                          uint64_t *device_bytes, uint32_t *longest_list) {
  if (!level) return ADL_ERR_INVALID_ARG;
  if (regions) *regions = 2 * level->ix.num_boundaries + 1;
  if (list_entries) *list_entries = level->ix.rlist.size();
  if (device_bytes) *device_bytes = level->ix.bytes();
  if (longest_list) *longest_list = level->ix.longest;
  return ADL_OK;
}

uint64_t adl_bloom_level_candidates_workspace_bytes(uint64_t num_keys) {
  uint64_t a, b, c;
  return ws_layout(num_keys, a, b, c);
}

int adl_bloom_level_candidates_device(adl_bloom_level *level, const uint8_t *d_keys, const uint64_t *d_offsets,
                                      uint64_t num_keys, uint32_t key_stride, int64_t seq, uint32_t *d_pair_begin,
                                      uint32_t *d_pair_table, uint64_t pair_capacity, uint64_t *d_num_pairs,
                                      void *d_workspace, uint64_t workspace_bytes, void *stream) {
  if (!adl_host::candidates_args_ok(level, d_keys, d_offsets, num_keys, key_stride, d_pair_begin, d_pair_table,
                                    pair_capacity, d_num_pairs, d_workspace))
    return ADL_ERR_INVALID_ARG;
  return adl_host::level_select_device(level, d_keys, d_offsets, num_keys, key_stride, seq, d_pair_begin,
                                       d_pair_table, pair_capacity, d_num_pairs, d_workspace, workspace_bytes,
                                       (hipStream_t)stream);
}

}  // extern "C"

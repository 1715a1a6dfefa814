// adlsm-tree_amd/csrc/revision_index.hip -- the whole revision asked once:
// which tables of ALL its levels a multi-get has to ask, selected on the
// device.
//
// Revision::Get (src/revision.cpp:391-403) walks levels 0..4 in order and calls
// Level::Get (:265-310) on each that is not Empty().  A revision here borrows
// the resident level indices (level_index.hip) of its levels; its device copy
// holds the non-empty levels' descriptors and the global id of each level's
// table 0, so the launches take one pointer and their number does not depend
// on the number of levels:
//
//   revision_locate_kernel  one lane per key: the 16-byte prefix once, then the
//                           binary search of level_locate_kernel in every
//                           level; region[l][i], the per-level and the summed
//                           candidate counts at `seq`, one total per workgroup
//   level_scan_kernel       (level_index.hip) the workgroup totals scanned
//   revision_expand_kernel  pair_begin, and the lists of the levels copied out
//                           back to back as global ids, the lanes striding over
//                           a workgroup's pairs: the (key, level) segments'
//                           starts sit in LDS (at most 256 x 8 of them)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "bloom_common.hpp"
#include "level_index_device.hpp"
#include "level_index_impl.hpp"

namespace {

using namespace adl_level_dev;

constexpr uint32_t kMaxL = ADL_BLOOM_MAX_LEVELS;

// The device copy of a revision: its non-empty levels, in visiting order.
struct RevDev {
  uint32_t nl;
  uint32_t base[kMaxL];  // the global id of the level's table 0
  LevelDev lv[kMaxL];
};

// One lane per key; workgroup b owns keys [256 b, 256 b + 256).  The levels are
// searched one after the other (a level's prefixes staged in LDS where they
// fit, as level_locate_kernel stages them), the key's bytes and prefix read
// once.  region and cntl are level-major: [l * nkeys + i].
__global__ __launch_bounds__(kBlockL) void revision_locate_kernel(KeySet ks, uint64_t nkeys,
                                                                  const RevDev *__restrict__ rev, int64_t seq,
                                                                  uint32_t *__restrict__ region,
                                                                  uint32_t *__restrict__ cntl,
                                                                  uint32_t *__restrict__ count,
                                                                  uint64_t *__restrict__ block_total) {
  __shared__ uint64_t spref[2 * kLdsBoundaries];
  __shared__ uint32_t scratch[kBlockL / adl_dev::kWave + 1];
  const uint64_t i = blockIdx.x * (uint64_t)kBlockL + threadIdx.x;
  const uint32_t nl = rev->nl;
  uint32_t klen = 0;
  const uint8_t *key = nullptr;
  uint64_t khi = 0, klo = 0;
  if (i < nkeys) {
    key = ks.at(i, klen);
    prefix_of(key, klen, khi, klo);
  }
  uint32_t cnt = 0;
  for (uint32_t l = 0; l < nl; ++l) {
    const LevelDev lv = rev->lv[l];
    const bool lds_pref = lv.nb <= kLdsBoundaries;
    if (lds_pref) {
      __syncthreads();  // the searches of the level before are done with spref
      for (uint32_t j = threadIdx.x; j < 2 * lv.nb; j += kBlockL) spref[j] = lv.pref[j];
      __syncthreads();
    }
    if (i < nkeys) {
      const uint32_t r = locate_region(lv, spref, lds_pref, key, klen, khi, klo);
      const uint32_t c = region_count(lv, r, seq);
      region[l * nkeys + i] = r;
      cntl[l * nkeys + i] = c;
      cnt += c;
    }
  }
  if (i < nkeys) count[i] = cnt;
  uint32_t total;
  (void)adl_dev::block_excl_scan<kBlockL>(cnt, scratch, &total);
  if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// Workgroup b writes pair_begin of its 256 keys and copies their lists out.
// Segment s = 256-key slot * nl + level holds one key's candidates in one
// level; the segments' starts within the workgroup's pairs sit in LDS, pair p
// finds its segment by an upper-bound search of them (as level_expand_kernel
// finds a pair's key), so every lane copies one entry per round however the
// candidates are spread over keys and levels.  A segment some of whose entries
// are dropped at `seq` is copied by its key's own lane, which skips them.
// Pairs at pair_capacity and beyond are not written.
__global__ __launch_bounds__(kBlockL) void revision_expand_kernel(uint64_t nkeys, const RevDev *__restrict__ rev,
                                                                  int64_t seq, const uint32_t *__restrict__ region,
                                                                  const uint32_t *__restrict__ cntl,
                                                                  const uint32_t *__restrict__ count,
                                                                  const uint64_t *__restrict__ block_off,
                                                                  uint32_t *__restrict__ pair_begin,
                                                                  uint32_t *__restrict__ pair_table,
                                                                  uint64_t pair_capacity) {
  __shared__ uint32_t sstart[kBlockL * kMaxL + 1], slist[kBlockL * kMaxL];
  __shared__ uint8_t sown[kBlockL * kMaxL];
  __shared__ const uint32_t *srlist[kMaxL];
  __shared__ uint32_t sbase[kMaxL];
  __shared__ uint32_t scratch[kBlockL / adl_dev::kWave + 1];
  const uint32_t t = threadIdx.x;
  const uint32_t nl = rev->nl;
  const uint64_t i = blockIdx.x * (uint64_t)kBlockL + t;
  if (t < nl) {
    srlist[t] = rev->lv[t].rlist;
    sbase[t] = rev->base[t];
  }
  const uint32_t cnt = i < nkeys ? count[i] : 0u;
  uint32_t btotal;
  const uint32_t excl = adl_dev::block_excl_scan<kBlockL>(cnt, scratch, &btotal);
  const uint64_t base = block_off[blockIdx.x];
  if (i < nkeys) {
    pair_begin[i] = (uint32_t)(base + excl);
    if (i == nkeys - 1) pair_begin[nkeys] = (uint32_t)(base + excl + cnt);
  }
  uint32_t run = excl;  // (a slot past the last key: btotal, an empty segment at the end)
  for (uint32_t l = 0; l < nl; ++l) {
    const uint32_t s = t * nl + l;
    uint32_t c = 0, l0 = 0;
    bool own = false;
    if (i < nkeys) {
      const LevelDev lv = rev->lv[l];
      const uint32_t r = region[l * nkeys + i];
      c = cntl[l * nkeys + i];
      l0 = lv.rbeg[r];
      const uint32_t l1 = lv.rbeg[r + 1];
      own = c != l1 - l0;
      if (own) {
        const uint32_t tb = rev->base[l];
        uint64_t w = base + run;
        for (uint32_t p = l0; p < l1; ++p) {
          const uint32_t e = lv.rlist[p];
          if (entry_gone(lv, e, seq)) continue;
          if (w < pair_capacity) pair_table[w] = (e & kTableMask) + tb;
          ++w;
        }
      }
    }
    sstart[s] = run;
    slist[s] = l0;
    sown[s] = own;
    run += c;
  }
  const uint32_t nseg = kBlockL * nl;
  if (t == 0) sstart[nseg] = btotal;
  __syncthreads();
  for (uint32_t p = t; p < btotal; p += kBlockL) {
    // the first j in [1, nseg] with sstart[j] > p (sstart[nseg] = btotal > p): segment j - 1 owns p
    uint32_t lo = 1, hi = nseg;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sstart[mid] > p) hi = mid; else lo = mid + 1;
    }
    const uint32_t s = lo - 1;
    if (sown[s]) continue;
    const uint32_t l = s % nl;
    const uint64_t w = base + p;
    if (w < pair_capacity) pair_table[w] = (srlist[l][slist[s] + (p - sstart[s])] & kTableMask) + sbase[l];
  }
}

uint64_t ws_layout(uint32_t live, uint64_t num_keys, uint64_t &o_cntl, uint64_t &o_count, uint64_t &o_btot,
                   uint64_t &o_boff) {
  const uint64_t nblk = (num_keys + kBlockL - 1) / kBlockL;
  adl_host::StagePlan p;
  p.take((uint64_t)live * num_keys * 4);
  o_cntl = p.take((uint64_t)live * num_keys * 4);
  o_count = p.take(num_keys * 4);
  o_btot = p.take(nblk * 8);
  o_boff = p.take(nblk * 8);
  return p.end + 256;
}

// the device copy, made once (under rev->mu); every level's own copy first
int upload_locked(adl_bloom_revision *rev) {
  RevDev *h = nullptr;
  if (hipHostMalloc((void **)&h, sizeof(RevDev), hipHostMallocDefault) != hipSuccess) return ADL_ERR_OUT_OF_MEMORY;
  memset(h, 0, sizeof(RevDev));
  int rc = ADL_OK;
  uint32_t nl = 0;
  for (size_t l = 0; l < rev->levels.size() && !rc; ++l) {
    adl_bloom_level *lv = rev->levels[l];
    if (!lv || lv->ix.num_tables == 0) continue;
    rc = adl_host::level_ensure_uploaded(lv);
    h->base[nl] = rev->table_base[l];
    h->lv[nl] = lv->dev();
    ++nl;
  }
  h->nl = nl;
  if (!rc && hipMalloc((void **)&rev->d_blob, sizeof(RevDev)) != hipSuccess) {
    rev->d_blob = nullptr;
    rc = ADL_ERR_OUT_OF_MEMORY;
  }
  if (!rc) {
    hipStream_t st = adl_host::sync_stream(nullptr);
    if (hipMemcpyAsync(rev->d_blob, h, sizeof(RevDev), hipMemcpyHostToDevice, st) != hipSuccess) rc = ADL_ERR_DEVICE;
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ADL_ERR_DEVICE;
  }
  (void)hipHostFree(h);
  return rc;
}

}  // namespace

int adl_host::revision_select_device(adl_bloom_revision *rev, const uint8_t *d_keys, const uint64_t *d_offsets,
                                     uint64_t num_keys, uint32_t key_stride, int64_t seq, uint32_t *d_pair_begin,
                                     uint32_t *d_pair_table, uint64_t pair_capacity, uint64_t *d_num_pairs,
                                     void *d_workspace, uint64_t workspace_bytes, hipStream_t st) {
  if (num_keys >= 0xffffffffull) return ADL_ERR_TOO_LARGE;  // pair_begin is u32, one entry per key and one more
  uint64_t o_cntl, o_count, o_btot, o_boff;
  if (workspace_bytes < ws_layout(rev->live, num_keys, o_cntl, o_count, o_btot, o_boff)) return ADL_ERR_WORKSPACE;
  if (num_keys == 0 || rev->live == 0) {  // (every level empty: no key has a candidate)
    ADL_HIP_TRY(hipMemsetAsync(d_pair_begin, 0, (num_keys + 1) * 4, st));
    ADL_HIP_TRY(hipMemsetAsync(d_num_pairs, 0, 8, st));
    return ADL_OK;
  }
  if (int rc = ensure_uploaded(rev, upload_locked)) return rc;
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  uint32_t *region = reinterpret_cast<uint32_t *>(ws), *cntl = reinterpret_cast<uint32_t *>(ws + o_cntl),
           *count = reinterpret_cast<uint32_t *>(ws + o_count);
  uint64_t *btot = reinterpret_cast<uint64_t *>(ws + o_btot), *boff = reinterpret_cast<uint64_t *>(ws + o_boff);
  const RevDev *dv = reinterpret_cast<const RevDev *>(rev->d_blob);
  const KeySet ks{d_keys, d_offsets, key_stride};
  const uint64_t nblk = (num_keys + kBlockL - 1) / kBlockL;
  hipLaunchKernelGGL(revision_locate_kernel, dim3((uint32_t)nblk), dim3(kBlockL), 0, st, ks, num_keys, dv, seq,
                     region, cntl, count, btot);
  ADL_HIP_TRY(hipGetLastError());
  if (int rc = adl_host::level_scan_launch(btot, nblk, boff, d_num_pairs, st)) return rc;
  hipLaunchKernelGGL(revision_expand_kernel, dim3((uint32_t)nblk), dim3(kBlockL), 0, st, num_keys, dv, seq, region,
                     cntl, count, boff, d_pair_begin, d_pair_table, pair_capacity);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

extern "C" {

int adl_bloom_revision_create(adl_bloom_level *const *levels, uint32_t num_levels, adl_bloom_revision **rev) {
  if (!rev) return ADL_ERR_INVALID_ARG;
  *rev = nullptr;
  if (num_levels > ADL_BLOOM_MAX_LEVELS || (num_levels && !levels)) return ADL_ERR_INVALID_ARG;
  uint64_t tables = 0, longest = 0;
  uint32_t live = 0;
  for (uint32_t l = 0; l < num_levels; ++l) {
    if (!levels[l] || levels[l]->ix.num_tables == 0) continue;
    tables += levels[l]->ix.num_tables;
    longest += levels[l]->ix.longest;
    ++live;
  }
  if (tables >= adl_level::kTableMask) return ADL_ERR_TOO_LARGE;
  if (longest >= (1u << 24)) return ADL_ERR_TOO_LARGE;  // 256 lists of a workgroup's keys add up in a u32
  auto *r = new (std::nothrow) adl_bloom_revision;
  if (!r) return ADL_ERR_OUT_OF_MEMORY;
  try {
    r->levels.assign(levels, levels + num_levels);
    r->table_base.assign(num_levels + 1, 0);
  } catch (...) {
    delete r;
    return ADL_ERR_OUT_OF_MEMORY;
  }
  for (uint32_t l = 0; l < num_levels; ++l)
    r->table_base[l + 1] = r->table_base[l] + (levels[l] ? levels[l]->ix.num_tables : 0u);
  r->longest = (uint32_t)longest;
  r->live = live;
  *rev = r;
  return ADL_OK;
}

// No call on the revision may be running or start once this is called.  The
// levels are the caller's.
int adl_bloom_revision_destroy(adl_bloom_revision *rev) {
  if (!rev) return ADL_OK;
  int rc = ADL_OK;
  if (rev->d_blob && hipFree(rev->d_blob) != hipSuccess) rc = ADL_ERR_DEVICE;
  delete rev;
  return rc;
}

int adl_bloom_revision_stats(const adl_bloom_revision *rev, uint32_t *num_levels, uint32_t *table_base,
                             uint32_t *longest_list) {
  if (!rev) return ADL_ERR_INVALID_ARG;
  if (num_levels) *num_levels = (uint32_t)rev->levels.size();
  if (table_base) memcpy(table_base, rev->table_base.data(), rev->table_base.size() * 4);
  if (longest_list) *longest_list = rev->longest;
  return ADL_OK;
}

// One key looked up in every non-empty level's host index, level 0 first: no
// device copy is made or used, nothing is allocated.
int adl_bloom_revision_candidates_host(const adl_bloom_revision *rev, const uint8_t *h_key, uint64_t key_len,
                                       int64_t seq, uint32_t *h_table, uint32_t capacity, uint32_t *num) {
  if (!rev || !num || (key_len && !h_key) || (capacity && !h_table)) return ADL_ERR_INVALID_ARG;
  const std::string_view u(key_len ? reinterpret_cast<const char *>(h_key) : "", key_len);
  uint32_t n = 0;
  for (size_t l = 0; l < rev->levels.size(); ++l) {
    const adl_bloom_level *lv = rev->levels[l];
    if (!lv || lv->ix.num_tables == 0) continue;
    const uint32_t base = rev->table_base[l];
    adl_level::LookupOne(lv->ix, u, seq, [&](uint32_t t) {
      if (n < capacity) h_table[n] = base + t;
      ++n;
    });
  }
  *num = n;
  return ADL_OK;
}

uint64_t adl_bloom_revision_candidates_workspace_bytes(const adl_bloom_revision *rev, uint64_t num_keys) {
  if (!rev) return 0;
  uint64_t a, b, c, d;
  return ws_layout(rev->live, num_keys, a, b, c, d);
}

int adl_bloom_revision_candidates_device(adl_bloom_revision *rev, const uint8_t *d_keys, const uint64_t *d_offsets,
                                         uint64_t num_keys, uint32_t key_stride, int64_t seq, uint32_t *d_pair_begin,
                                         uint32_t *d_pair_table, uint64_t pair_capacity, uint64_t *d_num_pairs,
                                         void *d_workspace, uint64_t workspace_bytes, void *stream) {
  if (!adl_host::candidates_args_ok(rev, d_keys, d_offsets, num_keys, key_stride, d_pair_begin, d_pair_table,
                                    pair_capacity, d_num_pairs, d_workspace))
    return ADL_ERR_INVALID_ARG;
  return adl_host::revision_select_device(rev, d_keys, d_offsets, num_keys, key_stride, seq, d_pair_begin,
                                          d_pair_table, pair_capacity, d_num_pairs, d_workspace, workspace_bytes,
                                          (hipStream_t)stream);
}

}  // extern "C"

// adlsm-tree_amd/csrc/level_index_impl.hpp -- adl_bloom_level and
// adl_bloom_revision as level_index.hip and revision_index.hip (index, kernels,
// selection), bloom_probe.hip (the hit kernels' scan) and filter_cache.hip (the
// multi-gets through a cache) share them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "level_index_core.hpp"
#include "level_index_device.hpp"

// The host copy is immutable after creation; the device copy (one allocation,
// `d_blob`) is made by the first device call, under `mu`, and immutable from
// then on.
struct adl_bloom_level {
  adl_level::Index ix;
  std::vector<std::string> oids;  // empty: created without oids (selection only)
  std::mutex mu;
  bool uploaded = false;
  int upload_status = 0;
  uint8_t *d_blob = nullptr;
  // views into d_blob
  const uint64_t *d_pref = nullptr;   // NB x (hi, lo)
  const uint8_t *d_bbytes = nullptr;  // boundary bytes
  const uint32_t *d_boff = nullptr;   // NB + 1
  const uint32_t *d_rbeg = nullptr;   // 2 NB + 2
  const uint32_t *d_rlist = nullptr;
  const int64_t *d_mx_seq = nullptr;  // per table
  const uint8_t *d_mx_op = nullptr;
  // what the kernels take (valid once uploaded)
  adl_level_dev::LevelDev dev() const {
    return {d_pref, d_bbytes, d_boff, d_rbeg, d_rlist, d_mx_seq, d_mx_op, ix.num_boundaries};
  }
};

namespace adl_host {

// The argument checks of adl_bloom_level_candidates_device and
// adl_bloom_revision_candidates_device, `handle` the level or the revision.
inline bool candidates_args_ok(const void *handle, const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys,
                               uint32_t key_stride, const uint32_t *d_pair_begin, const uint32_t *d_pair_table,
                               uint64_t pair_capacity, const uint64_t *d_num_pairs, const void *d_workspace) {
  if (!handle || !d_pair_begin || !d_num_pairs || !d_workspace) return false;
  if (num_keys && (!d_keys || (!d_offsets && key_stride == 0))) return false;
  if (pair_capacity && !d_pair_table) return false;
  return reinterpret_cast<uintptr_t>(d_workspace) % 256 == 0;
}

// The device copy of a level or a revision: made by upload(h), under h->mu, on
// the handle's first device call; every call gets that upload's status.
template <class Handle, class Upload>
int ensure_uploaded(Handle *h, Upload &&upload) {
  std::lock_guard<std::mutex> g(h->mu);
  if (!h->uploaded) {
    h->upload_status = upload(h);
    h->uploaded = true;
  }
  return h->upload_status;
}

// Uploads the index if this is the level's first device call (synchronous,
// on a stream of the calling thread's), then enqueues selection on `st`:
// adl_bloom_level_candidates_device after its argument checks.
__attribute__((visibility("hidden"))) int level_select_device(adl_bloom_level *lv, const uint8_t *d_keys,
                                                              const uint64_t *d_offsets, uint64_t num_keys,
                                                              uint32_t key_stride, int64_t seq,
                                                              uint32_t *d_pair_begin, uint32_t *d_pair_table,
                                                              uint64_t pair_capacity, uint64_t *d_num_pairs,
                                                              void *d_workspace, uint64_t workspace_bytes,
                                                              hipStream_t st);

// The level's device copy, made if this is its first device call (revision_index.hip).
__attribute__((visibility("hidden"))) int level_ensure_uploaded(adl_bloom_level *lv);

// level_scan_kernel on `st`: d_block_off = the exclusive scan of nblk u64
// block totals, *d_total their sum (revision_index.hip, bloom_probe.hip).
__attribute__((visibility("hidden"))) int level_scan_launch(const uint64_t *d_block_total, uint64_t nblk,
                                                            uint64_t *d_block_off, uint64_t *d_total,
                                                            hipStream_t st);

}  // namespace adl_host

// A revision: its levels in Revision::Get's visiting order, borrowed.  The
// host part is immutable after creation; the device copy (`d_blob`: the
// non-empty levels' descriptors and table bases, revision_index.hip) is made by
// the first device call, under `mu`.
struct adl_bloom_revision {
  std::vector<adl_bloom_level *> levels;  // as given; NULL or 0 tables: an empty level
  std::vector<uint32_t> table_base;       // levels.size() + 1
  uint32_t longest = 0;                   // the sum of the levels' longest lists
  std::mutex mu;
  bool uploaded = false;
  int upload_status = 0;
  uint8_t *d_blob = nullptr;
  uint32_t live = 0;  // non-empty levels (what the device copy describes)
};

namespace adl_host {

// adl_bloom_revision_candidates_device after its argument checks.
__attribute__((visibility("hidden"))) int revision_select_device(adl_bloom_revision *rev, const uint8_t *d_keys,
                                                                 const uint64_t *d_offsets, uint64_t num_keys,
                                                                 uint32_t key_stride, int64_t seq,
                                                                 uint32_t *d_pair_begin, uint32_t *d_pair_table,
                                                                 uint64_t pair_capacity, uint64_t *d_num_pairs,
                                                                 void *d_workspace, uint64_t workspace_bytes,
                                                                 hipStream_t st);

// adl_bloom_probe_fanout_hits_device with a probe count per filter (d_k[f];
// NULL: the k of bits_per_key), bloom_probe.hip.
__attribute__((visibility("hidden"))) int probe_fanout_hits_device(
    const uint8_t *d_keys, const uint64_t *d_offsets, uint64_t num_keys, uint32_t key_stride,
    const uint32_t *d_pair_begin, const uint32_t *d_pair_filter, uint64_t num_pairs, uint32_t num_filters,
    const uint8_t *d_bitmaps, const uint64_t *d_begin, const uint64_t *d_end, int32_t bits_per_key,
    const uint8_t *d_k, uint32_t *d_hit_begin, uint32_t *d_hit_filter, uint64_t hit_capacity, uint64_t *d_num_hits,
    void *d_workspace, uint64_t workspace_bytes, hipStream_t st);

// adl_bloom_hits_by_table_device on `st`, read_plan.hip.
__attribute__((visibility("hidden"))) int hits_by_table_device(
    const uint32_t *d_hit_begin, const uint32_t *d_hit_table, uint64_t num_keys, uint32_t num_tables,
    uint32_t *d_group_table, uint32_t *d_group_begin, uint64_t group_capacity, uint32_t *d_entry_key,
    uint64_t entry_capacity, uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes, hipStream_t st);

}  // namespace adl_host

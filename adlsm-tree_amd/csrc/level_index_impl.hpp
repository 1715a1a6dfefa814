// adlsm-tree_amd/csrc/level_index_impl.hpp -- adl_bloom_level as
// level_index.hip (index, kernels, selection) and filter_cache.hip (the
// multi-get through a cache) share it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "level_index_core.hpp"

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
};

namespace adl_host {

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

}  // namespace adl_host

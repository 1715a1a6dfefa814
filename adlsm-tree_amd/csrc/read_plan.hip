// adlsm-tree_amd/csrc/read_plan.hip -- the hits of a multi-get grouped by table
// on the device: the transposition a batched reader needs.
//
// Level::Get (reference src/revision.cpp:279-308) reads EVERY candidate table
// of a level and keeps the smallest inner key, so each surviving (key, table)
// pair of a level is a certain read, and each read opens the table's reader
// (DB::GetSSTableReader, src/db.cpp:340-364) before it walks the index block.
// A reader that opens each table once wants the hits table-major: which
// tables, ascending by global id (levels ascending, src/revision.cpp:391-403),
// and per table the batch's keys in batch order.
//
// The key-major hit lists (adl_bloom_probe_fanout_hits_device's output) are
// sorted by table id with a stable LSD radix sort, 8 bits per pass:
//   expand   hit e -> the key that owns it (a workgroup per 256 keys, the same
//            LDS upper-bound search as the fan-out probe);
//   per pass hits_hist_kernel      a tile's digit counts, digit-major
//            hits_row_scan_kernel  a workgroup per digit scans its row of tiles
//            hits_scatter_kernel   stable scatter: the rank of an entry inside
//                                  its wave from peer masks (eight ballots),
//                                  per-wave digit counts in LDS scanned in
//                                  wave order, the digit's base from the rows;
//   groups   a flag-and-scan compaction of the sorted ids' run heads; after a
//            sort of one pass (up to 256 tables) the scanned histogram rows
//            are the groups already, and the scatter's first tile writes them.
// No atomic decides a position (the histogram's LDS atomics only count), so
// the output is a function of the input.  Every kernel reads H =
// d_hit_begin[num_keys] itself and stops there: four launches up to 256
// tables, 4 + 3 * passes beyond, whatever the batch holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom_common.hpp"
#include "level_index_impl.hpp"
#include "probe_device.hpp"

using namespace adl_dev;
using adl_host::grid_for;

namespace {

constexpr int kBlk = 256;                   // threads of every kernel here
constexpr int kWaves = kBlk / kWave;        // 4
constexpr int kRounds = 8;                  // entries per lane and tile
constexpr uint32_t kTile = kBlk * kRounds;  // 2048 entries per workgroup (adlbloom.HITS_TILE)
constexpr uint32_t kWaveSpan = kWave * kRounds;  // a wave's contiguous share of a tile

// What every kernel learns first: H, and the tiles that hold entries.  H above
// the capacity: nothing is grouped (the counts say so).
struct Extent {
  uint32_t H, tiles;
  bool run;
};
__device__ __forceinline__ Extent extent_of(const uint32_t *__restrict__ hit_begin, uint64_t nkeys, uint64_t cap) {
  const uint32_t H = hit_begin[nkeys];
  return {H, (uint32_t)(((uint64_t)H + kTile - 1) / kTile), (uint64_t)H <= cap};
}

// owner[e] = the key whose list holds hit e.  Workgroup b takes keys [256 b,
// 256 b + 256): their begin entries into LDS, the lanes stride over the block's
// hits, an upper-bound search (8 steps) finds the owner -- as
// bloom_probe_fanout_kernel finds the key of a pair.
__global__ __launch_bounds__(kBlk) void hits_expand_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                           uint64_t cap, uint32_t *__restrict__ owner) {
  __shared__ uint32_t spb[kBlk + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  if (!x.run) return;
  const uint32_t t = threadIdx.x;
  const uint64_t nblk = (nkeys + kBlk - 1) / kBlk;
  for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t kb = blk * kBlk;
    const uint32_t nk = (uint32_t)(nkeys - kb < (uint64_t)kBlk ? nkeys - kb : (uint64_t)kBlk);
    if (t < nk) {
      spb[t] = hit_begin[kb + t];
      if (t == nk - 1) spb[nk] = hit_begin[kb + nk];
    }
    __syncthreads();
    const uint32_t p1 = spb[nk] < x.H ? spb[nk] : x.H;
    for (uint64_t p = (uint64_t)spb[0] + t; p < p1; p += kBlk) {
      // the first j in [1, nk] with spb[j] > p: key j - 1 owns p
      uint32_t lo = 1, hi = nk;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (spb[mid] > (uint32_t)p) hi = mid; else lo = mid + 1;
      }
      owner[p] = (uint32_t)(kb + lo - 1);
    }
    __syncthreads();  // the next block of keys reuses spb
  }
}

// hist[d * tiles + tile] = the entries of `tile` whose digit is d.
__global__ __launch_bounds__(kBlk) void hits_hist_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                         uint64_t cap, const uint32_t *__restrict__ id, uint32_t shift,
                                                         uint32_t *__restrict__ hist) {
  __shared__ uint32_t lh[256];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  if (!x.run || blockIdx.x >= x.tiles) return;  // (uniform)
  const uint32_t t = threadIdx.x;
  lh[t] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)blockIdx.x * kTile;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t e = e0 + (uint32_t)r * kBlk + t;
    if (e < x.H) atomicAdd(&lh[(id[e] >> shift) & 255u], 1u);  // (LDS: a count, no order hangs on it)
  }
  __syncthreads();
  hist[(uint64_t)t * x.tiles + blockIdx.x] = lh[t];
}

// Workgroup d: the exclusive scan of digit d's row of tile counts, in place,
// and the row's total.
__global__ __launch_bounds__(kBlk) void hits_row_scan_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                             uint64_t cap, uint32_t *__restrict__ hist,
                                                             uint32_t *__restrict__ row_total) {
  __shared__ uint32_t scratch[kWaves + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  if (!x.run) return;
  const uint32_t t = threadIdx.x;
  uint32_t *row = hist + (uint64_t)blockIdx.x * x.tiles;
  uint32_t run = 0;
  for (uint32_t b = 0; b < x.tiles; b += kBlk) {
    const bool in = b + t < x.tiles;
    const uint32_t v = in ? row[b + t] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan<kBlk>(v, scratch, &total);
    if (in) row[b + t] = run + ex;
    run += total;
  }
  if (t == 0) row_total[blockIdx.x] = run;
}

// The stable scatter of one tile.  Wave w owns entries [512 w, 512 w + 512) of
// the tile, eight rounds of 64: an entry's rank among the wave's entries of
// its digit is the wave's count so far (LDS) plus its peers on lower lanes
// (peers: the lanes of this round with the same digit, eight ballots ANDed).
// After the rounds the per-wave counts are scanned in wave order on top of the
// digit's base: the scanned row totals plus the row's entry for this tile.
//
// kGroups (a sort of one pass, so ids below 256): the scanned row totals ARE
// the groups -- digit d is table d, its row total the group's size -- and tile
// 0 writes them and the counts, which saves the three launches that find the
// run heads of the sorted ids.
template <bool kGroups>
__global__ __launch_bounds__(kBlk) void hits_scatter_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                            uint64_t cap, const uint32_t *__restrict__ id,
                                                            const uint32_t *__restrict__ val, uint32_t shift,
                                                            const uint32_t *__restrict__ hist,
                                                            const uint32_t *__restrict__ row_total,
                                                            uint32_t *__restrict__ id_out,
                                                            uint32_t *__restrict__ val_out,
                                                            uint32_t *__restrict__ group_table,
                                                            uint32_t *__restrict__ group_begin,
                                                            uint64_t group_capacity, uint64_t *__restrict__ counts) {
  __shared__ uint32_t wcnt[kWaves][256];
  __shared__ uint32_t scratch[kWaves + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  if (kGroups && blockIdx.x == 0 && t == 0 && (!x.run || x.tiles == 0)) {  // nothing to group: the counts all the same
    counts[0] = x.H;
    counts[1] = 0;
    if (x.run) group_begin[0] = 0;
  }
  if (!x.run || blockIdx.x >= x.tiles) return;  // (uniform)
  uint32_t total;
  const uint32_t row = row_total[t], row_at = block_excl_scan<kBlk>(row, scratch, &total);
  const uint32_t digit_base = row_at + hist[(uint64_t)t * x.tiles + blockIdx.x];
  if (kGroups && blockIdx.x == 0) {  // (uniform)
    uint32_t groups;
    const uint32_t g = block_excl_scan<kBlk>(row ? 1u : 0u, scratch, &groups);
    if (row && g <= group_capacity) {  // (group_begin has one entry more than group_table)
      if (g < group_capacity) group_table[g] = t;
      group_begin[g] = row_at;
    }
    if (t == 0) {
      counts[0] = x.H;
      counts[1] = groups;
      if (groups <= group_capacity) group_begin[groups] = x.H;
    }
  }
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wcnt[w][t] = 0;
  __syncthreads();
  const uint64_t e0 = (uint64_t)blockIdx.x * kTile + wave * kWaveSpan + lane;
  const uint64_t below = (1ull << lane) - 1;
  uint32_t ids[kRounds], rank[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t e = e0 + (uint32_t)r * kWave;
    const bool valid = e < x.H;
    ids[r] = valid ? id[e] : 0u;
    const uint32_t d = (ids[r] >> shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t before = wcnt[wave][d];
    __builtin_amdgcn_wave_barrier();  // every lane has read the count before the digit's first lane updates it
    const uint32_t lower = (uint32_t)__popcll(peers & below);
    if (valid && lower == 0) wcnt[wave][d] = before + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    rank[r] = before + lower;
  }
  __syncthreads();
  {
    uint32_t at = digit_base;  // thread t: digit t over the waves
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t c = wcnt[w][t];
      wcnt[w][t] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t e = e0 + (uint32_t)r * kWave;
    if (e < x.H) {
      const uint64_t pos = (uint64_t)wcnt[wave][(ids[r] >> shift) & 255u] + rank[r];
      if (pos < cap) {  // (pos < H <= cap on any input whose counts the scans saw)
        id_out[pos] = ids[r];
        val_out[pos] = val[e];
      }
    }
  }
}

// Entry e of the sorted ids starts a group when it differs from its predecessor.
__device__ __forceinline__ bool group_head(const uint32_t *__restrict__ sorted, uint64_t e, uint32_t H) {
  return e < H && (e == 0 || sorted[e] != sorted[e - 1]);
}

__global__ __launch_bounds__(kBlk) void hits_heads_count_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                                uint64_t cap, const uint32_t *__restrict__ sorted,
                                                                uint32_t *__restrict__ tile_heads) {
  __shared__ uint32_t scratch[kWaves + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  if (!x.run || blockIdx.x >= x.tiles) return;  // (uniform)
  const uint64_t e0 = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t mine = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) mine += group_head(sorted, e0 + (uint32_t)r * kBlk, x.H);
  uint32_t total;
  (void)block_excl_scan<kBlk>(mine, scratch, &total);
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = total;
}

// One workgroup: the tiles' head counts scanned in place, the counts, and the
// end of the last group.
__global__ __launch_bounds__(kBlk) void hits_heads_scan_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                               uint64_t cap, uint32_t *__restrict__ tile_heads,
                                                               uint32_t *__restrict__ group_begin,
                                                               uint64_t group_capacity, uint64_t *__restrict__ counts) {
  __shared__ uint32_t scratch[kWaves + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  const uint32_t t = threadIdx.x;
  if (!x.run) {
    if (t == 0) {
      counts[0] = x.H;
      counts[1] = 0;
    }
    return;
  }
  uint32_t run = 0;
  for (uint32_t b = 0; b < x.tiles; b += kBlk) {
    const bool in = b + t < x.tiles;
    const uint32_t v = in ? tile_heads[b + t] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan<kBlk>(v, scratch, &total);
    if (in) tile_heads[b + t] = run + ex;
    run += total;
  }
  if (t == 0) {
    counts[0] = x.H;
    counts[1] = run;
    if (run <= group_capacity) group_begin[run] = x.H;
  }
}

// The stable compaction of a tile's group heads, in rounds of 256 (a lane per
// entry, the flags scanned over the workgroup), as fanout_compact_kernel
// compacts the hits.
__global__ __launch_bounds__(kBlk) void hits_heads_write_kernel(const uint32_t *__restrict__ hit_begin, uint64_t nkeys,
                                                                uint64_t cap, const uint32_t *__restrict__ sorted,
                                                                const uint32_t *__restrict__ tile_heads,
                                                                uint32_t *__restrict__ group_table,
                                                                uint32_t *__restrict__ group_begin,
                                                                uint64_t group_capacity) {
  __shared__ uint32_t scratch[kWaves + 1];
  const Extent x = extent_of(hit_begin, nkeys, cap);
  if (!x.run || blockIdx.x >= x.tiles) return;  // (uniform)
  const uint64_t e0 = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t w = tile_heads[blockIdx.x];
  for (int r = 0; r < kRounds; ++r) {
    const uint64_t e = e0 + (uint32_t)r * kBlk;
    const bool head = group_head(sorted, e, x.H);
    uint32_t total;
    const uint32_t at = block_excl_scan<kBlk>(head ? 1u : 0u, scratch, &total);
    if (head && w + at <= group_capacity) {  // (group_begin has one entry more than group_table)
      if (w + at < group_capacity) group_table[w + at] = sorted[e];
      group_begin[w + at] = (uint32_t)e;
    }
    w += total;
  }
}

uint32_t sort_passes(uint32_t num_tables) {
  uint32_t bits = 0;
  for (uint32_t v = num_tables ? num_tables - 1 : 0; v; v >>= 1) ++bits;
  return bits <= 8 ? 1 : (bits + 7) / 8;
}

// keyA | idB | (two passes or more: idA | keyB) | hist | row totals | tile heads
struct PlanLayout {
  uint64_t o_key[2], o_id[2], o_hist, o_rows, o_heads, end;
  PlanLayout(uint64_t cap, uint32_t passes) {
    adl_host::StagePlan p;
    const uint64_t tiles = (cap + kTile - 1) / kTile;
    o_key[0] = p.take(cap * 4);
    o_id[1] = p.take(cap * 4);
    o_id[0] = passes > 1 ? p.take(cap * 4) : 0;
    o_key[1] = passes > 1 ? p.take(cap * 4) : 0;
    o_hist = p.take(tiles * 256 * 4);
    o_rows = p.take(256 * 4);
    o_heads = p.take(tiles * 4);
    end = p.end;
  }
};

}  // namespace

int adl_host::hits_by_table_device(const uint32_t *d_hit_begin, const uint32_t *d_hit_table, uint64_t num_keys,
                                   uint32_t num_tables, uint32_t *d_group_table, uint32_t *d_group_begin,
                                   uint64_t group_capacity, uint32_t *d_entry_key, uint64_t entry_capacity,
                                   uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes, hipStream_t st) {
  if (!d_group_begin || !d_counts) return ADL_ERR_INVALID_ARG;
  if (num_keys >= 0xffffffffull || entry_capacity > 0xffffffffull) return ADL_ERR_TOO_LARGE;  // positions are u32
  if (num_keys == 0) {
    ADL_HIP_TRY(hipMemsetAsync(d_group_begin, 0, 4, st));
    ADL_HIP_TRY(hipMemsetAsync(d_counts, 0, 16, st));
    return ADL_OK;
  }
  if (!d_hit_begin || !d_workspace) return ADL_ERR_INVALID_ARG;
  if (entry_capacity && (!d_hit_table || !d_entry_key)) return ADL_ERR_INVALID_ARG;
  if (group_capacity && !d_group_table) return ADL_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(d_workspace) % 256) return ADL_ERR_INVALID_ARG;
  const uint32_t passes = sort_passes(num_tables);
  const PlanLayout lay(entry_capacity, passes);
  if (workspace_bytes < lay.end) return ADL_ERR_WORKSPACE;
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  auto u32 = [&](uint64_t at) { return reinterpret_cast<uint32_t *>(ws + at); };
  uint32_t *key[2] = {u32(lay.o_key[0]), u32(lay.o_key[1])}, *id[2] = {u32(lay.o_id[0]), u32(lay.o_id[1])};
  uint32_t *hist = u32(lay.o_hist), *rows = u32(lay.o_rows), *heads = u32(lay.o_heads);
  const uint32_t tiles = (uint32_t)((entry_capacity + kTile - 1) / kTile);
  const uint32_t *sorted = d_hit_table;
  if (tiles) {
    hipLaunchKernelGGL(hits_expand_kernel, dim3(grid_for(num_keys, kBlk, 8)), dim3(kBlk), 0, st, d_hit_begin, num_keys,
                       entry_capacity, key[0]);
    ADL_HIP_TRY(hipGetLastError());
    // pass p reads (id, key)[p & 1] -- the first the caller's ids -- and writes the other pair; the last
    // writes its keys to d_entry_key
    for (uint32_t p = 0; p < passes; ++p) {
      const uint32_t *src_id = p ? id[p & 1] : d_hit_table, *src_key = key[p & 1];
      uint32_t *dst_id = id[(p + 1) & 1], *dst_key = p + 1 == passes ? d_entry_key : key[(p + 1) & 1];
      hipLaunchKernelGGL(hits_hist_kernel, dim3(tiles), dim3(kBlk), 0, st, d_hit_begin, num_keys, entry_capacity,
                         src_id, 8 * p, hist);
      ADL_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(hits_row_scan_kernel, dim3(256), dim3(kBlk), 0, st, d_hit_begin, num_keys, entry_capacity,
                         hist, rows);
      ADL_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(passes == 1 ? hits_scatter_kernel<true> : hits_scatter_kernel<false>, dim3(tiles), dim3(kBlk),
                         0, st, d_hit_begin, num_keys, entry_capacity, src_id, src_key, 8 * p, hist, rows, dst_id,
                         dst_key, d_group_table, d_group_begin, group_capacity, d_counts);
      ADL_HIP_TRY(hipGetLastError());
      sorted = dst_id;
    }
    if (passes == 1) return ADL_OK;  // (the scatter wrote the groups and the counts)
    hipLaunchKernelGGL(hits_heads_count_kernel, dim3(tiles), dim3(kBlk), 0, st, d_hit_begin, num_keys, entry_capacity,
                       sorted, heads);
    ADL_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(hits_heads_scan_kernel, dim3(1), dim3(kBlk), 0, st, d_hit_begin, num_keys, entry_capacity, heads,
                     d_group_begin, group_capacity, d_counts);
  ADL_HIP_TRY(hipGetLastError());
  if (tiles) {
    hipLaunchKernelGGL(hits_heads_write_kernel, dim3(tiles), dim3(kBlk), 0, st, d_hit_begin, num_keys, entry_capacity,
                       sorted, heads, d_group_table, d_group_begin, group_capacity);
    ADL_HIP_TRY(hipGetLastError());
  }
  return ADL_OK;
}

extern "C" uint64_t adl_bloom_hits_by_table_workspace_bytes(uint64_t /*num_keys*/, uint64_t entry_capacity,
                                                            uint32_t num_tables) {
  if (entry_capacity > 0xffffffffull) return 0;
  return PlanLayout(entry_capacity, sort_passes(num_tables)).end;
}

extern "C" int adl_bloom_hits_by_table_device(const uint32_t *d_hit_begin, const uint32_t *d_hit_table,
                                              uint64_t num_keys, uint32_t num_tables, uint32_t *d_group_table,
                                              uint32_t *d_group_begin, uint64_t group_capacity,
                                              uint32_t *d_entry_key, uint64_t entry_capacity, uint64_t *d_counts,
                                              void *d_workspace, uint64_t workspace_bytes, void *stream) {
  return adl_host::hits_by_table_device(d_hit_begin, d_hit_table, num_keys, num_tables, d_group_table, d_group_begin,
                                        group_capacity, d_entry_key, entry_capacity, d_counts, d_workspace,
                                        workspace_bytes, (hipStream_t)stream);
}

// adlsm-tree_amd/csrc/hash_pairs.hip -- both murmur hashes of n keys of any
// shape, pair i at out[i] in key order: the one key-to-pairs launcher, of a
// streamed build's appends (stream_build.hip) and of the binned probe's queries
// (probe_binned.hip).  Aligned 16-byte keys take a lane per key; every other
// shape one workgroup per run of kRunKeys keys through hash_run (hash_run.hpp)
// with the output at the key's own index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloom_common.hpp"
#include "hash_run.hpp"

using namespace adl_dev;

namespace {

constexpr int kRunBlk = 256;
constexpr uint32_t kRunKeys = ADL_BLOOM_STREAM_RUN_KEYS;  // keys per run (the build's measured shape)

__global__ __launch_bounds__(256) void hash16_pairs_kernel(const uint4 *__restrict__ keys, uint64_t n,
                                                           uint2 *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t h1, h2;
  hash16(load_nt(keys + i), h1, h2);
  out[i] = make_uint2(h1, h2);
}

template <uint32_t S, class Keys, bool EXACT>
__global__ __launch_bounds__(kRunBlk) void hash_run_pairs_kernel(Keys keys, uint64_t n, uint2 *__restrict__ out) {
  const uint64_t q0 = (uint64_t)blockIdx.x * S;
  const uint32_t cnt = (uint32_t)min((uint64_t)S, n - q0);
  if constexpr (EXACT) hash_run<S, kRunBlk>(keys, q0, cnt, ReadExactBytes{n}, PairsByIndex{out + q0});
  else hash_run<S, kRunBlk>(keys, q0, cnt, ReadWholeBlocks{}, PairsByIndex{out + q0});
}

template <class Keys>
void launch_runs(const Keys &k, uint64_t n, bool whole, uint2 *out, hipStream_t st) {
  constexpr size_t kLds = run_lds_bytes<kRunKeys>(true);
  static_assert(kLds == 30736, "the run's LDS at the measured shape, with the index array");
  const dim3 runs((uint32_t)((n + kRunKeys - 1) / kRunKeys));
  if (whole) hipLaunchKernelGGL((hash_run_pairs_kernel<kRunKeys, Keys, false>), runs, dim3(kRunBlk), kLds, st, k, n, out);
  else hipLaunchKernelGGL((hash_run_pairs_kernel<kRunKeys, Keys, true>), runs, dim3(kRunBlk), kLds, st, k, n, out);
}

}  // namespace

int adl_host::hash_pairs_device(const uint8_t *d_keys, const uint64_t *d_offsets, uint32_t key_stride, uint64_t n,
                                bool whole, uint2 *out, hipStream_t st) {
  if (n == 0) return ADL_OK;
  if (d_offsets) launch_runs(KeysVar{d_keys, d_offsets}, n, whole, out, st);
  else if (key_stride == 16 && whole)
    hipLaunchKernelGGL(hash16_pairs_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const uint4 *>(d_keys), n, out);
  else launch_runs(KeysStride{d_keys, key_stride}, n, whole, out, st);
  ADL_HIP_TRY(hipGetLastError());
  return ADL_OK;
}

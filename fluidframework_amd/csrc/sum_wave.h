// sum_wave.h — the wave-level helpers the bulk summary kernels share (summary.hip, summary_v1.hip):
// one wave per document, match classes of prop sets in LDS; and the ones of the readers that deal one
// wave per work item (text.hip, runs.hip, pos.hip): the item clamp, the lane scan, the item loop, the grid.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/fmt.h"

namespace fmt_kernels {

constexpr int kSumWaves = 4;
constexpr int kSumMaxProps = 4096;  // prop sets per document (the huge tier's table)

__device__ __forceinline__ void sumSync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t sumUni(uint32_t x) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x))); }

__device__ __forceinline__ uint32_t sumLane(uint32_t v, int lane) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lane));
}

// Entry k of the prop set whose first record is p (fmt.h: wide sets take consecutive records).
__device__ __forceinline__ uint32_t sumKv(const fmt_mt_propset* T, uint32_t p, uint32_t k) {
  return T[p + k / FMT_MT_PROPS_MAX].kv[k % FMT_MT_PROPS_MAX];
}

// Sets p and q (first records, np records in all) hold the same (key, value) pairs, any order.
__device__ __forceinline__ bool sumSameSet(const fmt_mt_propset* T, uint32_t p, uint32_t q, uint32_t np) {
  const uint32_t n = T[p].n;
  if (n != T[q].n || n == FMT_MT_PROPS_CONT || n > FMT_MT_PROPS_KEYS_MAX) return false;
  if (p + (n ? (n - 1) / FMT_MT_PROPS_MAX : 0) >= np || q + (n ? (n - 1) / FMT_MT_PROPS_MAX : 0) >= np) return false;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t x = sumKv(T, p, i);
    bool found = false;
    for (uint32_t j = 0; j < n; j++) found = found || sumKv(T, q, j) == x;
    if (!found) return false;
  }
  return true;
}

// ---- one wave per work item, kSumWaves waves per workgroup, items dealt grid-stride

// The leaves of the tile [firstLeaf, firstLeaf + nLeaves) that the document of header h has: 0 when it failed.
__device__ __forceinline__ uint32_t waveItemLeaves(const fmt_mt_doc_result& h, uint32_t firstLeaf, uint32_t nLeaves) {
  const int32_t status = h.status;
  const uint32_t n = h.n_leaves;
  if (status != FMT_OK || firstLeaf >= n) return 0;
  return nLeaves < n - firstLeaf ? nLeaves : n - firstLeaf;
}

// Inclusive prefix of x over the wave's 64 lanes.
__device__ __forceinline__ uint32_t waveScan(uint32_t x, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = static_cast<uint32_t>(__shfl_up(static_cast<int>(x), o));
    if (lane >= o) x += t;
  }
  return x;
}

// A wave's items: for (uint64_t k = waveItemFirst(); k < n; k += waveItemStride()).
__device__ __forceinline__ uint64_t waveItemFirst() { return static_cast<uint64_t>(blockIdx.x) * kSumWaves + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t waveItemStride() { return static_cast<uint64_t>(gridDim.x) * kSumWaves; }

// Workgroups for n items (host): one wave each up to 8 workgroups per CU, the rest by stride; at least 1.
inline uint32_t waveGrid(uint64_t n, int numCUs) {
  const uint64_t wanted = (n + kSumWaves - 1) / kSumWaves;
  const uint64_t cap = static_cast<uint64_t>(numCUs) * 8u;
  return static_cast<uint32_t>(wanted < cap ? (wanted > 0 ? wanted : 1) : cap);
}

}  // namespace fmt_kernels

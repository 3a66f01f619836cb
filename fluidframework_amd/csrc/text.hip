// text.hip — bulk SharedString.getText: every document's visible text (include/fmt_text.h), packed in
// document order on the device.
//
// A work item is a (document, tile) pair, a tile being at most kTextTileLeaves consecutive leaves
// (text_plan.h): a small document is one item, a huge one thousands spread over the device. One wave
// per item, 4 per workgroup, items dealt grid-stride; no wave talks to another. A leaf contributes its
// `len` units when it is not removed (rm_seq == FMT_NOT_REMOVED) and not a Marker; a Marker that is
// not removed contributes the placeholder once when there is one, nothing otherwise.
//
//   pass 1  textTileUnitsKernel: the units each item contributes (64-bit), leaves read 64 at a time.
//   host    exclusive prefix of those (text_plan.h textOffsets): the callers' offsets, each tile's base.
//   pass 2  textGatherKernel: per chunk of 64 leaves the exclusive prefix of contributions by wave
//           scan, then one lane per output unit, which finds its source leaf by a shuffle binary search
//           over that prefix (as summaryRunsKernel does) and stores one unit: leaf records stream in,
//           units stream out.
//
// Every leaf index read is below the document's n_leaves (items are clamped against the header again
// here); every char read lies inside [char_off, char_off + len) of such a leaf.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "kernels.h"
#include "sum_wave.h"

namespace fmt_kernels {

namespace {

__device__ __forceinline__ uint32_t textUnitsOf(const fmt_mt_leaf& L, uint32_t placeholder) {
  if (L.rm_seq != FMT_NOT_REMOVED) return 0;
  if ((L.pad & FMT_MT_LEAF_MARKER) != 0) return placeholder != 0 ? 1u : 0u;
  return L.len;
}

}  // namespace

__global__ __launch_bounds__(64 * kSumWaves) void textTileUnitsKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                                const SumView* __restrict__ views,
                                                                const fmt_plan::TextItem* __restrict__ items,
                                                                uint32_t nItems, uint32_t placeholder,
                                                                unsigned long long* __restrict__ tileUnits) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const fmt_plan::TextItem it = items[k];
    const uint32_t n = waveItemLeaves(hdrs[it.doc], it.firstLeaf, it.nLeaves);
    const fmt_mt_leaf* leaves = views[it.doc].leaves + it.firstLeaf;
    unsigned long long acc = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + lane;
      if (i < n) acc += textUnitsOf(leaves[i], placeholder);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) tileUnits[k] = acc;
  }
}

__global__ __launch_bounds__(64 * kSumWaves) void textGatherKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                             const SumView* __restrict__ views,
                                                             const fmt_plan::TextItem* __restrict__ items,
                                                             uint32_t nItems, uint32_t placeholder,
                                                             const unsigned long long* __restrict__ tileBase,
                                                             uint16_t* __restrict__ packed) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const fmt_plan::TextItem it = items[k];
    const uint32_t n = waveItemLeaves(hdrs[it.doc], it.firstLeaf, it.nLeaves);
    const SumView V = views[it.doc];
    const fmt_mt_leaf* leaves = V.leaves + it.firstLeaf;
    uint16_t* dst = packed + tileBase[k];
    uint64_t running = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + static_cast<uint32_t>(lane);
      uint32_t len = 0, off = 0, marker = 0;
      if (i < n) {
        const fmt_mt_leaf L = leaves[i];
        len = textUnitsOf(L, placeholder);
        off = L.char_off;
        marker = (L.pad & FMT_MT_LEAF_MARKER) != 0 ? 1u : 0u;
      }
      uint32_t ex = waveScan(len, lane);  // inclusive, then exclusive prefix of len over the lanes
      const uint32_t chunkUnits = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(ex), 63)));
      ex -= len;
      for (uint32_t u0 = 0; u0 < chunkUnits; u0 += 64) {
        const uint32_t t = u0 + static_cast<uint32_t>(lane);
        // source leaf of unit t: the last lane whose start <= t (it has len > 0 whenever t < chunkUnits)
        int pos = 0;
        for (int step = 32; step >= 1; step >>= 1) {
          const uint32_t s = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos + step));
          if (s <= t) pos += step;
        }
        const uint32_t st = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos));
        const uint32_t so = static_cast<uint32_t>(__shfl(static_cast<int>(off), pos));
        const uint32_t mk = static_cast<uint32_t>(__shfl(static_cast<int>(marker), pos));
        if (t < chunkUnits) dst[running + t] = mk != 0 ? static_cast<uint16_t>(placeholder) : V.chars[so + (t - st)];
      }
      running += chunkUnits;
    }
  }
}

hipError_t launchTextTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                               uint32_t nItems, uint16_t placeholder, unsigned long long* tileUnits, int numCUs,
                               hipStream_t stream) {
  hipLaunchKernelGGL(textTileUnitsKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views,
                     items, nItems, static_cast<uint32_t>(placeholder), tileUnits);
  return hipGetLastError();
}

hipError_t launchTextGather(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                            uint32_t nItems, uint16_t placeholder, const unsigned long long* tileBase, uint16_t* packed,
                            int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(textGatherKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views,
                     items, nItems, static_cast<uint32_t>(placeholder), tileBase, packed);
  return hipGetLastError();
}

}  // namespace fmt_kernels

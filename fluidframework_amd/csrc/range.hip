// range.hip — bulk range reads (include/fmt_range.h): the text of many (document, start, end, view) ranges,
// packed in query order on the device.
//
// Same shape as text.hip and pos.hip: one wave per work item, 4 per workgroup, items dealt grid-stride; no wave
// talks to another and no atomic decides anything: every output word has one writer whose index the host
// fixed, so two calls return equal bytes. A work item (range_plan.h RangeItem) is one range clipped to one
// tile: [lo, hi) in units of the item's view, counted from the tile's first leaf. The view rule is pos.hip's
// (pos_view.h); the tile's units per view come from pos.hip's posTileUnitsKernel, which this read launches
// as its sizing pass A.
//
//   pass B  rangeTileUnitsKernel (no placeholder only): the text units of each item. The tile is walked in
//           chunks of 64 leaves with a wave scan of the view's units; the lane whose leaf covers [s, s + u)
//           contributes the length of its overlap with [lo, hi) when the leaf is text, 0 when it is a Marker.
//           The walk stops at the first chunk that reaches hi.
//   host    range_plan.h rangeOffsets: the exclusive prefix of those in query order.
//   pass C  rangeGatherKernel: the same walk; the clipped contributions (a Marker inside [lo, hi): one
//           placeholder unit when there is one) are scanned a second time, then one lane per output unit
//           finds its source lane by textGatherKernel's shuffle binary search and stores one unit.
//
// Every leaf index read is below the document's n_leaves (items are clamped against the header again here);
// every char read lies inside [char_off, char_off + len) of such a leaf and below n_chars; every store goes
// to an index below `cap`.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "../../include/fmt_range.h"
#include "kernels.h"
#include "pos_view.h"
#include "sum_wave.h"

namespace fmt_kernels {

namespace {

using fmt_plan::RangeItem;

// The units of [s, s + u) inside [lo, hi).
__device__ __forceinline__ uint32_t rangeClip(uint32_t s, uint32_t u, uint32_t lo, uint32_t hi) {
  const uint32_t a = s > lo ? s : lo, b = s + u < hi ? s + u : hi;
  return b > a ? b - a : 0u;
}

}  // namespace

__global__ __launch_bounds__(64 * kSumWaves) void rangeTileUnitsKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                                 const SumView* __restrict__ views,
                                                                 const RangeItem* __restrict__ items, uint32_t nItems,
                                                                 unsigned long long* __restrict__ itemUnits) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const RangeItem it = items[k];
    const uint32_t n = waveItemLeaves(hdrs[it.doc], it.firstLeaf, it.nLeaves);
    const fmt_mt_leaf* leaves = views[it.doc].leaves + it.firstLeaf;
    unsigned long long acc = 0;
    uint32_t before = 0;  // the view's units of the chunks walked so far (sums of one tile: below 2^32)
    for (uint32_t b = 0; b < n && before < it.hi; b += 64) {
      const uint32_t i = b + static_cast<uint32_t>(lane);
      uint32_t u = 0;
      bool marker = false;
      if (i < n) {
        const fmt_mt_leaf L = leaves[i];
        u = posVisible(L, it.refSeq, it.client) ? posUnitsOf(L) : 0u;
        marker = (L.pad & FMT_MT_LEAF_MARKER) != 0;
      }
      const uint32_t incl = waveScan(u, lane);
      if (!marker) acc += rangeClip(before + incl - u, u, it.lo, it.hi);
      before += sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63)));
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) itemUnits[k] = acc;
  }
}

__global__ __launch_bounds__(64 * kSumWaves) void rangeGatherKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                              const SumView* __restrict__ views,
                                                              const RangeItem* __restrict__ items, uint32_t nItems,
                                                              uint32_t placeholder,
                                                              const unsigned long long* __restrict__ itemBase,
                                                              uint16_t* __restrict__ out, uint64_t cap) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const RangeItem it = items[k];
    const fmt_mt_doc_result h = hdrs[it.doc];
    const uint32_t n = waveItemLeaves(h, it.firstLeaf, it.nLeaves);
    const SumView V = views[it.doc];
    const fmt_mt_leaf* leaves = V.leaves + it.firstLeaf;
    uint64_t at = itemBase[k];  // where the next chunk's units go
    uint32_t before = 0;
    for (uint32_t b = 0; b < n && before < it.hi; b += 64) {
      const uint32_t i = b + static_cast<uint32_t>(lane);
      uint32_t u = 0, len = 0, off = 0, marker = 0;
      if (i < n) {
        const fmt_mt_leaf L = leaves[i];
        u = posVisible(L, it.refSeq, it.client) ? posUnitsOf(L) : 0u;
        marker = (L.pad & FMT_MT_LEAF_MARKER) != 0 ? 1u : 0u;
        len = L.len;
        off = L.char_off;
      }
      const uint32_t incl = waveScan(u, lane);
      const uint32_t s = before + incl - u;
      uint32_t c = rangeClip(s, u, it.lo, it.hi);  // this lane's output units
      if (marker != 0) {
        c = placeholder != 0 ? c : 0u;
      } else {
        const uint32_t skip = it.lo > s ? it.lo - s : 0u;  // units of the leaf before the range
        c = skip < len ? (c < len - skip ? c : len - skip) : 0u;  // (inside [char_off, char_off + len))
        off += skip;
      }
      uint32_t ex = waveScan(c, lane);
      const uint32_t chunkUnits = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(ex), 63)));
      ex -= c;
      for (uint32_t u0 = 0; u0 < chunkUnits; u0 += 64) {
        const uint32_t t = u0 + static_cast<uint32_t>(lane);
        // source leaf of unit t: the last lane whose start <= t (it has c > 0 whenever t < chunkUnits)
        int pos = 0;
        for (int step = 32; step >= 1; step >>= 1) {
          const uint32_t st = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos + step));
          if (st <= t) pos += step;
        }
        const uint32_t st = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos));
        const uint32_t so = static_cast<uint32_t>(__shfl(static_cast<int>(off), pos));
        const uint32_t mk = static_cast<uint32_t>(__shfl(static_cast<int>(marker), pos));
        if (t < chunkUnits && at + t < cap) {
          const uint64_t src = static_cast<uint64_t>(so) + (t - st);
          out[at + t] = mk != 0 ? static_cast<uint16_t>(placeholder) : (src < h.n_chars ? V.chars[src] : static_cast<uint16_t>(0));
        }
      }
      at += chunkUnits;
      before += sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63)));
    }
  }
}

hipError_t launchRangeTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::RangeItem* items,
                                uint32_t nItems, unsigned long long* itemUnits, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(rangeTileUnitsKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, items,
                     nItems, itemUnits);
  return hipGetLastError();
}

hipError_t launchRangeGather(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::RangeItem* items,
                             uint32_t nItems, uint16_t placeholder, const unsigned long long* itemBase, uint16_t* out,
                             uint64_t cap, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(rangeGatherKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, items,
                     nItems, static_cast<uint32_t>(placeholder), itemBase, out, cap);
  return hipGetLastError();
}

}  // namespace fmt_kernels

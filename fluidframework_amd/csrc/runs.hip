// runs.hip — bulk property runs: every document's "where each formatting starts and ends"
// (include/fmt_runs.h), packed in document order on the device.
//
// Work items are the text read's (text_plan.h): (document, tile of at most kTextTileLeaves leaves), one
// wave per item, 4 per workgroup, items dealt grid-stride. No wave talks to another and no atomic decides
// an order: every output word has one writer whose index the host fixed, so two calls return equal bytes.
//
//   classes  runClassKernel: one wave per document that has prop sets and no classes of the engine's own
//            (SumView::cls, huge documents), lanes over sets as summaryRunsKernel derives them, written
//            to clsBuf + clsOff[doc] so that the tiles read a class instead of deriving it.
//   pass 1   runTileReportKernel: per tile its units, its heads and what its two ends look like (RunTile).
//            Leaves are read 64 at a time; a visible lane takes class and marker flag of the previous
//            visible lane (the highest set bit below it in the ballot) by shuffle, or the wave-uniform
//            carry of the chunks before. A visible leaf is a head iff it is a Marker, its predecessor is
//            a Marker, the classes differ, or it has no predecessor in the tile.
//   host     runs_plan.h stitchRuns: which tiles continue the run open where they begin, every tile's
//            run and position base, the callers' offsets.
//   pass 2   runEmitKernel: heads again, minus the tile's first when the stitch says it continues. A
//            head's rank is the popcount of the heads below it plus the running count; that lane writes
//            start, first_leaf, props and flags of its run and, as it is where the run before ends, that
//            run's len = its start - the start of the head before (by shuffle, or the carry: at the
//            tile's start the start of the run it continues). The tile's last run is closed by lane 0
//            when the stitch says it ends with the tile.
//
// Every leaf index read is below the document's n_leaves (items are clamped against the header again
// here); a props id indexes a class table only when it is below the document's n_props. Every run index
// written is below the total the stitch counted from these same heads.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "../../include/fmt_runs.h"
#include "kernels.h"
#include "sum_wave.h"

namespace fmt_kernels {

namespace {

using fmt_plan::RunTile;
using fmt_plan::RunTileBase;
using fmt_plan::TextItem;

constexpr uint32_t kKeyMarker = fmt_plan::kRunEndMarker;

// A chunk of 64 leaves as both passes see it: per lane whether its leaf counts, its units, its class with
// the marker flag (key), and whether it is a head given the carry of the chunks before.
struct RunChunk {
  bool vis, head;
  uint32_t units, key;
  uint64_t mask;  // the visible lanes
};

__device__ __forceinline__ RunChunk runChunk(const fmt_mt_leaf* leaves, uint32_t i, uint32_t n, int lane, const SumView& V,
                                             const uint16_t* cls, uint32_t np, bool carryHas, uint32_t carryKey) {
  RunChunk c{false, false, 0u, 0xFFFFu, 0ull};
  if (i < n) {
    const fmt_mt_leaf L = leaves[i];
    const bool marker = (L.pad & FMT_MT_LEAF_MARKER) != 0;
    c.vis = L.rm_seq == FMT_NOT_REMOVED && L.len != 0;
    c.units = c.vis ? (marker ? 1u : L.len) : 0u;
    const uint32_t p = L.props;
    uint32_t k = 0xFFFFu;
    if (c.vis && p != 0xFFFFu && p < np) k = V.cls != nullptr ? (V.cls[p] & 0xFFFFu) : static_cast<uint32_t>(cls[p]);
    c.key = k | (marker ? kKeyMarker : 0u);
  }
  c.mask = __ballot(c.vis);
  const uint64_t below = c.mask & ((1ull << lane) - 1ull);
  const int prev = below != 0 ? 63 - __clzll(static_cast<long long>(below)) : 0;
  const uint32_t fromLane = static_cast<uint32_t>(__shfl(static_cast<int>(c.key), prev));  // (every lane takes part)
  const bool hasPrev = below != 0 || carryHas;
  const uint32_t prevKey = below != 0 ? fromLane : carryKey;
  c.head = c.vis && (!hasPrev || ((c.key | prevKey) & kKeyMarker) != 0 || (c.key & 0xFFFFu) != (prevKey & 0xFFFFu));
  return c;
}

}  // namespace

__global__ __launch_bounds__(64 * kSumWaves) void runClassKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                           const SumView* __restrict__ views, uint32_t nDocs,
                                                           const unsigned long long* __restrict__ clsOff,
                                                           uint16_t* __restrict__ clsBuf) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t d = waveItemFirst(); d < nDocs; d += waveItemStride()) {
    const SumView V = views[d];
    // document d's span, sized by the host from its header: n_props entries, none for a failed or a huge document
    const uint32_t np = static_cast<uint32_t>(clsOff[d + 1] - clsOff[d]);
    if (hdrs[d].status != FMT_OK || V.cls != nullptr) continue;
    uint16_t* cls = clsBuf + clsOff[d];
    for (uint32_t p = lane; p < np; p += 64) {
      const uint32_t an = V.props[p].n;
      uint16_t c = an == 0 ? 0xFFFFu : static_cast<uint16_t>(p);
      if (an != 0 && an != FMT_MT_PROPS_CONT)  // (continuation records: no leaf names them)
        for (uint32_t q = 0; q < p; q++)
          if (sumSameSet(V.props, q, p, np)) {
            c = static_cast<uint16_t>(q);
            break;
          }
      cls[p] = c;
    }
  }
}

__global__ __launch_bounds__(64 * kSumWaves) void runTileReportKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                                const SumView* __restrict__ views,
                                                                const TextItem* __restrict__ items, uint32_t nItems,
                                                                const unsigned long long* __restrict__ clsOff,
                                                                const uint16_t* __restrict__ clsBuf,
                                                                RunTile* __restrict__ tiles) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const TextItem it = items[k];
    const fmt_mt_doc_result h = hdrs[it.doc];
    const uint32_t n = waveItemLeaves(h, it.firstLeaf, it.nLeaves);
    const SumView V = views[it.doc];
    const fmt_mt_leaf* leaves = V.leaves + it.firstLeaf;
    const uint16_t* cls = clsBuf + clsOff[it.doc];
    const uint32_t np = V.cls != nullptr ? h.n_props : static_cast<uint32_t>(clsOff[it.doc + 1] - clsOff[it.doc]);
    RunTile r{0u, 0u, 0u, 0u, 0u};
    bool carryHas = false;
    uint32_t carryKey = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      const RunChunk c = runChunk(leaves, b + static_cast<uint32_t>(lane), n, lane, V, cls, np, carryHas, carryKey);
      const uint32_t incl = waveScan(c.units, lane);
      const uint32_t chunkUnits = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63)));
      const uint64_t heads = __ballot(c.head);
      const int lastHead = heads != 0 ? 63 - __clzll(static_cast<long long>(heads)) : 0;
      const uint32_t before = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl - c.units), lastHead)));
      r.tail = heads != 0 ? chunkUnits - before : r.tail + chunkUnits;
      r.units += chunkUnits;
      r.heads += static_cast<uint32_t>(__popcll(heads));
      if (c.mask != 0) {
        const int firstVis = __ffsll(static_cast<long long>(c.mask)) - 1, lastVis = 63 - __clzll(static_cast<long long>(c.mask));
        const uint32_t fk = sumLane(c.key, firstVis), lk = sumLane(c.key, lastVis);
        if (!carryHas) r.first = fk | fmt_plan::kRunEndHas;
        carryHas = true;
        carryKey = lk;
      }
    }
    if (carryHas) r.last = carryKey | fmt_plan::kRunEndHas;
    if (lane == 0) tiles[k] = r;
  }
}

__global__ __launch_bounds__(64 * kSumWaves) void runEmitKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                          const SumView* __restrict__ views,
                                                          const TextItem* __restrict__ items, uint32_t nItems,
                                                          const unsigned long long* __restrict__ clsOff,
                                                          const uint16_t* __restrict__ clsBuf,
                                                          const RunTileBase* __restrict__ bases, uint64_t nRuns,
                                                          fmt_mt_prop_run* __restrict__ runs) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const TextItem it = items[k];
    const fmt_mt_doc_result h = hdrs[it.doc];
    const uint32_t n = waveItemLeaves(h, it.firstLeaf, it.nLeaves);
    const SumView V = views[it.doc];
    const fmt_mt_leaf* leaves = V.leaves + it.firstLeaf;
    const uint16_t* cls = clsBuf + clsOff[it.doc];
    const uint32_t np = V.cls != nullptr ? h.n_props : static_cast<uint32_t>(clsOff[it.doc + 1] - clsOff[it.doc]);
    const RunTileBase B = bases[k];
    const bool continues = (B.flags & fmt_plan::kRunContinues) != 0;
    bool carryHas = false;
    uint32_t carryKey = 0;
    uint64_t rank = 0;                 // new runs of this tile so far
    uint32_t pos = B.posBase;          // position of the chunk's first leaf
    uint32_t openStart = B.openStart;  // start of the run open at the chunk's first leaf (when there is one)
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + static_cast<uint32_t>(lane);
      const RunChunk c = runChunk(leaves, i, n, lane, V, cls, np, carryHas, carryKey);
      const uint32_t incl = waveScan(c.units, lane);
      const uint32_t chunkUnits = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63)));
      const uint32_t start = pos + incl - c.units;
      // the tile's first visible leaf is no head when it continues the run open at the tile's start
      const bool head = c.head && !(continues && !carryHas && (c.mask & ((1ull << lane) - 1ull)) == 0);
      const uint64_t heads = __ballot(head);
      const uint64_t headsBelow = heads & ((1ull << lane) - 1ull);
      const int prevHead = headsBelow != 0 ? 63 - __clzll(static_cast<long long>(headsBelow)) : 0;
      const uint32_t prevStartLane = static_cast<uint32_t>(__shfl(static_cast<int>(start), prevHead));
      if (head) {
        const uint64_t r = B.runBase + rank + static_cast<uint64_t>(__popcll(headsBelow));
        if (r < nRuns) {
          runs[r].start = start;
          runs[r].first_leaf = it.firstLeaf + i;
          runs[r].props = static_cast<uint16_t>(c.key & 0xFFFFu);
          runs[r].flags = (c.key & kKeyMarker) != 0 ? static_cast<uint16_t>(FMT_MT_RUN_MARKER) : static_cast<uint16_t>(0);
        }
        // the run before ends here; the tile's first new run has one before it only when it continues
        const bool hasBefore = headsBelow != 0 || rank != 0 || continues;
        if (hasBefore && r >= 1 && r - 1 < nRuns) runs[r - 1].len = start - (headsBelow != 0 ? prevStartLane : openStart);
      }
      if (heads != 0) {
        const int lastHead = 63 - __clzll(static_cast<long long>(heads));
        openStart = sumLane(start, lastHead);
        rank += static_cast<uint64_t>(__popcll(heads));
      }
      if (c.mask != 0) {
        carryKey = sumLane(c.key, 63 - __clzll(static_cast<long long>(c.mask)));
        carryHas = true;
      }
      pos += chunkUnits;
    }
    if ((B.flags & fmt_plan::kRunCloses) != 0 && lane == 0 && (rank != 0 || continues)) {
      const uint64_t r = B.runBase + rank - 1;
      if (r < nRuns) runs[r].len = pos - openStart;
    }
  }
}

hipError_t launchRunClasses(const fmt_mt_doc_result* hdrs, const SumView* views, uint32_t nDocs,
                            const unsigned long long* clsOff, uint16_t* clsBuf, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(runClassKernel, dim3(waveGrid(nDocs, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, nDocs,
                     clsOff, clsBuf);
  return hipGetLastError();
}

hipError_t launchRunTileReport(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                               uint32_t nItems, const unsigned long long* clsOff, const uint16_t* clsBuf,
                               fmt_plan::RunTile* tiles, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(runTileReportKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views,
                     items, nItems, clsOff, clsBuf, tiles);
  return hipGetLastError();
}

hipError_t launchRunEmit(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                         uint32_t nItems, const unsigned long long* clsOff, const uint16_t* clsBuf,
                         const fmt_plan::RunTileBase* bases, uint64_t nRuns, fmt_mt_prop_run* runs, int numCUs,
                         hipStream_t stream) {
  hipLaunchKernelGGL(runEmitKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, items,
                     nItems, clsOff, clsBuf, bases, nRuns, runs);
  return hipGetLastError();
}

}  // namespace fmt_kernels

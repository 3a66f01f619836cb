// pos.hip — bulk position queries (include/fmt_pos.h): which leaf holds position p of document d in a
// view (ref_seq, client), where that unit lies in the local view, its properties and its UTF-16 unit.
//
// Same shape as text.hip: one wave per work item, 4 per workgroup, items dealt grid-stride; no wave talks to
// another and no atomic decides anything: every output word has one writer whose index the host fixed, so
// two calls return equal bytes. A leaf's units in a view are fmt_pos.h's: visible in the local view iff
// rm_seq == FMT_NOT_REMOVED; in a remote view iff (ins_seq <= ref_seq || ins_client == client) and not
// (rm_seq <= ref_seq || bit `client` of rm_clients); a visible text leaf counts len, a visible Marker 1.
//
//   pass 1  posTileUnitsKernel: per (view, tile) item (pos_plan.h PosItem) the tile's units in that view
//           and in the local view, 64-bit, leaves read 64 at a time.
//   host    pos_plan.h resolvePosQueries: the exclusive prefix of each view's tiles, each query's tile by
//           binary search, positions at or past the view's end answered there.
//   pass 2  posResolveKernel: per query (PosDevQuery) its one tile walked in chunks of 64 leaves, a wave
//           scan of the view's and the local view's contributions; the one lane whose [start, start + len)
//           holds the position writes the 32-byte hit. A wave that finds no such lane writes nothing: the
//           host pre-filled the record with FMT_E_DATA.
//
// Every leaf index read is below the document's n_leaves (items are clamped against the header again
// here); the char read lies inside [char_off, char_off + len) of such a leaf and below n_chars; a record is
// written only at an index below the number of queries. Clients are 0..63 (the host refuses the others), so
// the shift is defined.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "../../include/fmt_pos.h"
#include "kernels.h"
#include "pos_view.h"
#include "sum_wave.h"

namespace fmt_kernels {

namespace {

using fmt_plan::PosDevQuery;
using fmt_plan::PosItem;
using fmt_plan::PosTileUnits;

}  // namespace

__global__ __launch_bounds__(64 * kSumWaves) void posTileUnitsKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                               const SumView* __restrict__ views,
                                                               const PosItem* __restrict__ items, uint32_t nItems,
                                                               PosTileUnits* __restrict__ tileUnits) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t k = waveItemFirst(); k < nItems; k += waveItemStride()) {
    const PosItem it = items[k];
    const uint32_t n = waveItemLeaves(hdrs[it.doc], it.firstLeaf, it.nLeaves);
    const fmt_mt_leaf* leaves = views[it.doc].leaves + it.firstLeaf;
    unsigned long long inView = 0, inLocal = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + lane;
      if (i < n) {
        const fmt_mt_leaf L = leaves[i];
        const uint32_t u = posUnitsOf(L);
        if (posVisible(L, it.refSeq, it.client)) inView += u;
        if (posVisibleLocal(L)) inLocal += u;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      inView += __shfl_xor(inView, off);
      inLocal += __shfl_xor(inLocal, off);
    }
    if (lane == 0) tileUnits[k] = PosTileUnits{inView, inLocal};
  }
}

__global__ __launch_bounds__(64 * kSumWaves) void posResolveKernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                             const SumView* __restrict__ views,
                                                             const PosDevQuery* __restrict__ queries, uint64_t nDev,
                                                             uint64_t nQueries, fmt_mt_pos_hit* __restrict__ out) {
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t k = waveItemFirst(); k < nDev; k += waveItemStride()) {
    const PosDevQuery Q = queries[k];
    const fmt_mt_doc_result h = hdrs[Q.doc];
    const uint32_t n = waveItemLeaves(h, Q.firstLeaf, Q.nLeaves);
    const SumView V = views[Q.doc];
    const fmt_mt_leaf* leaves = V.leaves + Q.firstLeaf;
    uint32_t before = 0, beforeLocal = 0;  // units of the chunks walked so far
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + static_cast<uint32_t>(lane);
      fmt_mt_leaf L{};
      uint32_t u = 0, ul = 0;
      if (i < n) {
        L = leaves[i];
        const uint32_t units = posUnitsOf(L);
        u = posVisible(L, Q.refSeq, Q.client) ? units : 0u;
        ul = posVisibleLocal(L) ? units : 0u;
      }
      const uint32_t incl = waveScan(u, lane), inclLocal = waveScan(ul, lane);
      const uint32_t start = before + incl - u;  // (sums of one tile of one document: below 2^32)
      const bool hit = u != 0 && start <= Q.pos && Q.pos - start < u;
      if (hit && Q.out < nQueries) {
        const bool marker = (L.pad & FMT_MT_LEAF_MARKER) != 0;
        const uint32_t offset = Q.pos - start;
        const uint32_t at = L.char_off + (marker ? 0u : offset);
        fmt_mt_pos_hit r;
        r.leaf = Q.firstLeaf + i;
        r.offset = offset;
        r.leaf_start = Q.viewBase + start;
        r.leaf_len = u;
        r.local_pos = Q.localBase + beforeLocal + inclLocal - ul + (ul != 0 ? offset : 0u);
        r.props = L.props;
        r.unit = L.len != 0 && at < h.n_chars ? V.chars[at] : static_cast<uint16_t>(0);
        r.status = FMT_OK;
        r.flags = (marker ? FMT_MT_POS_F_MARKER : 0u) | (ul == 0 ? FMT_MT_POS_F_HIDDEN_LOCALLY : 0u);
        out[Q.out] = r;
      }
      if (__ballot(hit) != 0) break;  // (wave-uniform)
      before += sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63)));
      beforeLocal += sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(inclLocal), 63)));
    }
  }
}

hipError_t launchPosTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::PosItem* items,
                              uint32_t nItems, fmt_plan::PosTileUnits* tileUnits, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(posTileUnitsKernel, dim3(waveGrid(nItems, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, items,
                     nItems, tileUnits);
  return hipGetLastError();
}

hipError_t launchPosResolve(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::PosDevQuery* queries,
                            uint64_t nDev, uint64_t nQueries, fmt_mt_pos_hit* out, int numCUs, hipStream_t stream) {
  hipLaunchKernelGGL(posResolveKernel, dim3(waveGrid(nDev, numCUs)), dim3(64 * kSumWaves), 0, stream, hdrs, views, queries,
                     nDev, nQueries, out);
  return hipGetLastError();
}

}  // namespace fmt_kernels

// summary_v1.hip — bulk SnapshotV1 SharedString summaries: SnapshotV1.extractSync's segmentation
// (merge-tree/src/snapshotV1.ts:170-276) for every document of a replay, on the device.
//
// The layout of summary.hip: one wave per document (4 per workgroup, grid-stride), leaves read 64 at
// a time. With the header's minSeq a leaf is skipped (removed at/below minSeq: the merge chain
// continues across it), mergeable (inserted at/below minSeq, not removed: appended onto the open run
// under the legacy rule, canAppend && matchProperties) or solo (any other: it closes the open run and
// is written alone with its merge info). Properties are the leaf's own (snapshotV1.ts:211), not the
// getAtSeq view. The text of every emitted leaf, removed solo ones included, is copied lane-parallel
// into one compact text per document. A removed solo leaf's first remove stamp is the first op of the
// document, in record order, whose seq is the leaf's rm_seq and whose type removes (REMOVE or an
// obliterate): found in the resident op records by a lane-parallel lower bound on seq. The later
// stamps (the remove-order slab) are joined on the host.
#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "kernels.h"
#include "sum_wave.h"

namespace fmt_kernels {

namespace {

// The first op of ops[lo, n), nondecreasing in seq, with seq == target and a remove type: its client
// and stamp kind. Wave-uniform arguments and result; false when there is none.
__device__ bool v1FirstRemover(const fmt_mt_op* __restrict__ ops, uint32_t lo, uint32_t n, int32_t target, int lane,
                               int32_t* client, uint32_t* kind) {
  uint32_t hi = n;
  // lower bound on seq, 64 probes a step: the answer stays in [lo, hi)
  while (hi - lo > 64u) {
    const uint32_t step = (hi - lo + 63u) / 64u;
    const uint32_t nProbe = (hi - lo + step - 1u) / step;  // <= 64
    const uint32_t at = lo + static_cast<uint32_t>(lane) * step;
    const bool ge = static_cast<uint32_t>(lane) < nProbe && ops[at].seq >= target;
    const uint64_t m = __ballot(ge);
    const uint32_t f = m ? static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1) : nProbe;
    const uint32_t lo2 = f == 0 ? lo : lo + (f - 1u) * step + 1u;
    if (f < nProbe) hi = lo + f * step + 1u;
    lo = lo2;
  }
  {
    const uint32_t at = lo + static_cast<uint32_t>(lane);
    const uint64_t m = __ballot(at < hi && ops[at].seq >= target);
    if (m == 0) return false;  // (every seq below the target)
    lo += static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
  }
  // forward over the records of that seq (group members and bunches share one)
  for (uint32_t b = lo; b < n; b += 64u) {
    const uint32_t at = b + static_cast<uint32_t>(lane);
    bool rm = false, past = true;
    uint32_t cl = 0, ty = 0;
    if (at < n) {
      const fmt_mt_op op = ops[at];
      past = op.seq != target;
      ty = op.type;
      cl = op.client;
      rm = !past && (ty == FMT_MT_REMOVE || ty == FMT_MT_OBLITERATE || ty == FMT_MT_OBLITERATE_SIDED);
    }
    const uint64_t mRm = __ballot(rm), mPast = __ballot(past);
    const int fRm = mRm ? __ffsll(static_cast<long long>(mRm)) - 1 : 64;
    const int fPast = mPast ? __ffsll(static_cast<long long>(mPast)) - 1 : 64;
    if (fRm < fPast) {
      *client = static_cast<int32_t>(sumLane(cl, fRm));
      *kind = sumLane(ty, fRm) == FMT_MT_REMOVE ? FMT_MT_RM_SET : FMT_MT_RM_SLICE;
      return true;
    }
    if (fPast < 64) return false;
  }
  return false;
}

}  // namespace

__global__ __launch_bounds__(64 * kSumWaves) void summaryV1Kernel(const fmt_mt_doc_result* __restrict__ hdrs,
                                                            const SumView* __restrict__ views,
                                                            const fmt_mt_op* __restrict__ opsAll,
                                                            const uint64_t* __restrict__ opOffs, uint32_t nDocs,
                                                            SumV1Seg* __restrict__ segs, uint16_t* __restrict__ text,
                                                            unsigned long long* __restrict__ cursors,
                                                            SumDocOut* __restrict__ docOut) {
  __shared__ uint16_t clsAll[kSumWaves][kSumMaxProps];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  uint16_t* cls = clsAll[wave];
  for (uint32_t d = blockIdx.x * kSumWaves + wave; d < nDocs; d += gridDim.x * kSumWaves) {
    const fmt_mt_doc_result h = hdrs[d];
    SumDocOut od{};
    od.status = static_cast<uint32_t>(h.status);
    const SumView V = views[d];
    if (h.status != FMT_OK || (V.cls == nullptr && h.n_props > static_cast<uint32_t>(kSumMaxProps))) {
      if (h.status == FMT_OK) od.status = static_cast<uint32_t>(FMT_E_CAPACITY);
      if (lane == 0) docOut[d] = od;
      continue;
    }
    const uint32_t n = h.n_leaves, np = h.n_props;
    const int32_t minSeq = h.min_seq;
    // match classes: the first prop set with the same content (empty sets: undefined's class)
    for (uint32_t p = lane; p < np && V.cls == nullptr; p += 64) {  // (huge documents: the engine's classes)
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
    // emitted leaves (every leaf not skipped) and their units: the spans reserved for this document
    uint32_t nEmit = 0, nUnits = 0;
    bool anyRemoved = false;  // a removed leaf above minSeq: the op records are searched
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + lane;
      bool emit = false;
      uint32_t len = 0;
      if (i < n) {
        const fmt_mt_leaf L = V.leaves[i];
        emit = !(L.rm_seq != FMT_NOT_REMOVED && L.rm_seq <= minSeq);
        len = emit ? L.len : 0u;
        anyRemoved = anyRemoved || (emit && L.rm_seq != FMT_NOT_REMOVED);
      }
      nEmit += static_cast<uint32_t>(__popcll(__ballot(emit)));
      for (int off = 32; off > 0; off >>= 1) len += static_cast<uint32_t>(__shfl_xor(static_cast<int>(len), off));
      nUnits += len;
    }
    unsigned long long segBase = 0, textBase = 0;
    if (lane == 0) {
      segBase = atomicAdd(&cursors[0], static_cast<unsigned long long>(nEmit));
      textBase = atomicAdd(&cursors[1], static_cast<unsigned long long>(nUnits));
    }
    segBase = __shfl(segBase, 0);
    textBase = __shfl(textBase, 0);
    // the document's op records past the loader's segments (FMT_MT_F_LOADSEG: a prefix, seqs unordered)
    const fmt_mt_op* ops = opsAll + opOffs[d];
    const uint32_t nOps = static_cast<uint32_t>(opOffs[d + 1] - opOffs[d]);
    uint32_t opLo = 0;
    if (__ballot(anyRemoved) != 0) {
      opLo = nOps;
      for (uint32_t b = 0; b < nOps; b += 64) {
        const uint32_t at = b + lane;
        const uint64_t m = __ballot(at < nOps && (ops[at].flags & FMT_MT_F_LOADSEG) == 0);
        if (m) {
          opLo = b + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
          break;
        }
      }
    }
    sumSync();
    // serial decisions over the emitted leaves, text copied chunk by chunk
    uint32_t nSegs = 0, runLen = 0, runProps = 0xFFFFu, runCls = 0xFFFFu, runLast = 0;
    bool have = false, runMarker = false, unknown = false;
    uint64_t tpos = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t i = b + lane;
      uint32_t kind = 0;  // 0 skipped, 1 mergeable, 2 solo
      uint32_t len = 0, props = 0xFFFFu, last = 0, off = 0, marker = 0;
      int32_t insSeq = 0, insClient = 0, rmSeq = FMT_NOT_REMOVED;
      if (i < n) {
        const fmt_mt_leaf L = V.leaves[i];
        const bool removed = L.rm_seq != FMT_NOT_REMOVED;
        if (!(removed && L.rm_seq <= minSeq)) {
          kind = (L.ins_seq <= minSeq && !removed) ? 1u : 2u;
          len = L.len;
          props = L.props;
          off = L.char_off;
          marker = (L.pad & FMT_MT_LEAF_MARKER) != 0 ? 1u : 0u;
          last = len > 0 ? V.chars[off + len - 1] : 0u;
          insSeq = L.ins_seq;
          insClient = L.ins_client;
          rmSeq = L.rm_seq;
        }
      }
      // text: emitted leaves' units to text[textBase + tpos + prefix]
      uint32_t ex = waveScan(len, lane);  // inclusive, then exclusive prefix of len over the lanes
      const uint32_t chunkUnits = sumUni(static_cast<uint32_t>(__shfl(static_cast<int>(ex), 63)));
      ex -= len;
      for (uint32_t u0 = 0; u0 < chunkUnits; u0 += 64) {
        const uint32_t t = u0 + lane;
        // source leaf of unit t: the last lane whose start <= t (binary search by shuffles)
        int pos = 0;
        for (int step = 32; step >= 1; step >>= 1) {
          const uint32_t s = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos + step));
          if (s <= t) pos += step;
        }
        const uint32_t st = static_cast<uint32_t>(__shfl(static_cast<int>(ex), pos));
        const uint32_t so = static_cast<uint32_t>(__shfl(static_cast<int>(off), pos));
        if (t < chunkUnits) text[textBase + tpos + t] = V.chars[so + (t - st)];
      }
      tpos += chunkUnits;
      uint64_t m = __ballot(kind != 0);
      while (m) {
        const int k = __ffsll(static_cast<long long>(m)) - 1;
        m &= m - 1;
        const uint32_t l = sumLane(len, k), p = sumLane(props, k), lc = sumLane(last, k);
        const bool mk = sumLane(marker, k) != 0;
        if (sumLane(kind, k) == 2u) {  // closes the run; the next mergeable leaf starts a fresh one
          if (have && lane == 0)
            segs[segBase + nSegs] = SumV1Seg{runLen, static_cast<uint16_t>(runProps), static_cast<uint16_t>(runMarker ? kV1Marker : 0), 0u, 0, 0, 0, 0, 0u};
          nSegs += have ? 1u : 0u;
          have = false;
          SumV1Seg s{l, static_cast<uint16_t>(p), static_cast<uint16_t>(kV1Solo | (mk ? kV1Marker : 0)), b + static_cast<uint32_t>(k),
                     static_cast<int32_t>(sumLane(static_cast<uint32_t>(insSeq), k)),
                     static_cast<int32_t>(sumLane(static_cast<uint32_t>(insClient), k)), 0, 0, 0u};
          const int32_t rs = static_cast<int32_t>(sumLane(static_cast<uint32_t>(rmSeq), k));
          if (rs != FMT_NOT_REMOVED) {
            int32_t rc = 0;
            uint32_t rk = 0;
            if (v1FirstRemover(ops, opLo, nOps, rs, lane, &rc, &rk)) {
              s.flags |= kV1Removed;
              s.rm_client = rc;
              s.rm_seq = rs;
              s.rm_kind = rk;
            } else {
              unknown = true;  // (a loaded stamp above minSeq: no op of this batch made it)
            }
          }
          if (lane == 0) segs[segBase + nSegs] = s;
          nSegs++;
          continue;
        }
        const uint32_t c = (p == 0xFFFFu || p >= np) ? 0xFFFFu : V.cls != nullptr ? (V.cls[p] & 0xFFFFu) : static_cast<uint32_t>(cls[p]);
        const bool append = have && !runMarker && !mk && runLast != 10u &&
                            (runLen <= 256u || l <= 256u) && runCls == c;
        if (append) {
          runLen += l;
          runLast = lc;
        } else {
          if (have && lane == 0)
            segs[segBase + nSegs] = SumV1Seg{runLen, static_cast<uint16_t>(runProps), static_cast<uint16_t>(runMarker ? kV1Marker : 0), 0u, 0, 0, 0, 0, 0u};
          nSegs += have ? 1u : 0u;
          have = true;
          runLen = l;
          runProps = p;
          runCls = c;
          runLast = lc;
          runMarker = mk;
        }
      }
    }
    if (have) {
      if (lane == 0)
        segs[segBase + nSegs] = SumV1Seg{runLen, static_cast<uint16_t>(runProps), static_cast<uint16_t>(runMarker ? kV1Marker : 0), 0u, 0, 0, 0, 0, 0u};
      nSegs++;
    }
    if (unknown) od.status = static_cast<uint32_t>(FMT_E_UNSUPPORTED);
    od.run_off = segBase;
    od.text_off = textBase;
    od.n_runs = nSegs;
    od.n_units = nUnits;
    if (lane == 0) docOut[d] = od;
    sumSync();
  }
}

hipError_t launchSummaryV1(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_mt_op* ops,
                           const uint64_t* opOffs, uint32_t nDocs, SumV1Seg* segs, uint16_t* text,
                           unsigned long long* cursors, SumDocOut* docOut, int numCUs, hipStream_t stream) {
  const uint32_t wanted = (nDocs + kSumWaves - 1) / kSumWaves;
  const uint32_t cap = static_cast<uint32_t>(numCUs) * 4u;
  const uint32_t grid = wanted < cap ? (wanted > 0 ? wanted : 1) : cap;
  hipLaunchKernelGGL(summaryV1Kernel, dim3(grid), dim3(64 * kSumWaves), 0, stream, hdrs, views, ops, opOffs, nDocs, segs,
                     text, cursors, docOut);
  return hipGetLastError();
}

}  // namespace fmt_kernels

// mergetree.hip — merge-tree replay, small tier (8 register rows: 512 leaves, 2 waves/SIMD), the
// overflow-list kernel and the tier cascade (kernel template: mergetree_kernel.h).
//
// A plain batch replays every document in the micro tier first (mergetree_micro.hip: 2 rows); the
// documents it overflows go on in the compact tier (mergetree_compact.hip: 4 rows) from a device-side
// list, and those that one overflows in this tier from a second list; those this tier overflows go to
// the large tier (mergetree_large.hip) after the host reads the list length. With checkpoints the
// compact and small tiers run kDescendRounds times: in every round but the last a small-tier document
// that shrank to half of the compact tier stops (fmt_mt::kCkptDescend) and goes on a "down" list, which
// the compact tier replays in the next round, so it pays for the rows it has, not for the rows it once
// had. Every list length stays on the device; a round whose lists are empty costs launches that exit
// at once. Batches with obliterates start in the compact tier; batches with remove-order recording or
// adjusts start in this tier; neither steps down.
#define FMT_MT_COLLECT_DEFINE 1
#include "mergetree_kernel.h"

namespace fmt_kernels {

constexpr int kMtWaves = 4;  // small tier: 4 documents per workgroup, 2 waves/SIMD

int mergeTreeProfileCompact(uint64_t* out, int n, bool reset);
int mergeTreeProfileMicro(uint64_t* out, int n, bool reset);
int mergeTreeProfileLarge(uint64_t* out, int n, bool reset);

int mergeTreeProfile(uint64_t* out, int n, bool reset) {
  for (int c = 0; c < n; c++) out[c] = 0;
  if (addTuProfile(out, n, reset) < 0 || mergeTreeProfileCompact(out, n, reset) < 0 ||
      mergeTreeProfileMicro(out, n, reset) < 0 || mergeTreeProfileLarge(out, n, reset) < 0)
    return -1;
  return fmt_mt::kPfCount;
}

MtCaps mergeTreeCaps(bool large) {
  if (large)
    return MtCaps{static_cast<uint32_t>(Slab<fmt_mt::LargeTier>::kLeaves), static_cast<uint32_t>(Slab<fmt_mt::LargeTier>::kChars),
                  static_cast<uint32_t>(Slab<fmt_mt::LargeTier>::kProps)};
  return MtCaps{static_cast<uint32_t>(Slab<fmt_mt::SmallTier>::kLeaves), static_cast<uint32_t>(Slab<fmt_mt::SmallTier>::kChars),
                static_cast<uint32_t>(Slab<fmt_mt::SmallTier>::kProps)};
}

size_t mergeTreeCheckpointBytes() { return sizeof(uint32_t) * fmt_mt::Doc<false, fmt_mt::CompactTier>::kCkptWords; }

hipError_t launchMergeTreeCompact(const MtDeviceBatch& batch, const MtDeviceOut& out, const uint32_t* docList,
                                  uint32_t count, uint32_t* esc, int numCUs, hipStream_t stream, uint32_t* next,
                                  bool obliterate, const uint32_t* countDev);
hipError_t launchMergeTreeMicro(const MtDeviceBatch& batch, const MtDeviceOut& out, const uint32_t* docList,
                                uint32_t count, uint32_t* esc, int numCUs, hipStream_t stream, uint32_t* next);

// Rounds of the plain cascade (see the header comment). DESIGN.md §4.1 has the hop counts behind it.
#ifndef FMT_DESCEND_ROUNDS
#define FMT_DESCEND_ROUNDS 2
#endif
constexpr int kDescendRounds = FMT_DESCEND_ROUNDS;  // (1: a document only ever moves up)
constexpr size_t kDescendHead = 64;  // dealing counters of the rounds after the first, 2 a round

size_t mergeTreeDescendWords(uint32_t count) {
  return kDescendHead + static_cast<size_t>(2 * (kDescendRounds - 1)) * (static_cast<size_t>(count) + 1);
}

// A tier's overflow list in[0] = n, in[1..n] reordered into out by remaining ops,
// longest first (64 buckets between 0 and the largest remainder): with documents dealt to waves
// in list order, the next tier's pass then ends on short documents (longest-processing-time first).
// A checkpointed document has ops [ckpt next, end) left, any other one its whole stream.
constexpr int kOrderBuckets = 64;
__global__ __launch_bounds__(1024) void orderByRemainingKernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                               const fmt_mt_doc_result* __restrict__ headers,
                                                               const uint64_t* __restrict__ offs,
                                                               const uint32_t* __restrict__ ckpt, uint32_t ckptWords) {
  __shared__ uint32_t cnt[kOrderBuckets], base[kOrderBuckets], maxRem;
  const uint32_t n = in[0];
  if (threadIdx.x < kOrderBuckets) cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) maxRem = 0;
  __syncthreads();
  auto remaining = [&](uint32_t d) -> uint32_t {
    uint64_t first = offs[d];
    if (headers[d].status == fmt_mt::kCkptEscalate || headers[d].status == fmt_mt::kCkptDescend) {
      const uint32_t* h = ckpt + static_cast<size_t>(d) * ckptWords;
      first = h[0] | (static_cast<uint64_t>(h[1]) << 32);
    }
    const uint64_t r = offs[d + 1] - first;
    return r > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(r);
  };
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicMax(&maxRem, remaining(in[1 + i]));
  __syncthreads();
  const uint64_t span = static_cast<uint64_t>(maxRem) + 1;
  auto bucket = [&](uint32_t r) -> uint32_t {  // 0 = the longest remainders
    return kOrderBuckets - 1 - static_cast<uint32_t>(static_cast<uint64_t>(r) * kOrderBuckets / span);
  };
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&cnt[bucket(remaining(in[1 + i]))], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int b = 0; b < kOrderBuckets; b++) {
      base[b] = s;
      s += cnt[b];
    }
    out[0] = n;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const uint32_t d = in[1 + i];
    out[1 + atomicAdd(&base[bucket(remaining(d))], 1u)] = d;
  }
}

// Variants: obliterates (Ob) and/or the remove-order recording of SnapshotV1 batches (Rm).
hipError_t launchMergeTree(const MtDeviceBatch& batch, const MtDeviceOut& out, const uint32_t* docList,
                           uint32_t count, uint32_t* esc, uint32_t* esc2, uint32_t* esc3, uint32_t* esc4, int numCUs,
                           hipStream_t stream, bool obliterate, bool removeOrder, uint32_t* sched, bool adjust,
                           uint32_t* desc) {
  using S = fmt_mt::SmallTier;
  uint32_t* n1 = sched ? sched + 1 : nullptr;
  if (adjust) {  // annotate-adjust batches: the Adj variants, small tier over every document (no checkpoints)
    // (1 wave/SIMD: 512 registers a wave; at 2 the property-manager code spilled 3710 VGPRs to scratch,
    // at 1 the overflow lives in AGPRs)
    if (removeOrder)
      return launchTier<true, S, true, kMtWaves, 1, true>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
    return launchTier<true, S, false, kMtWaves, 1, true>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
  }
  if (obliterate && removeOrder)
    return launchTier<true, S, true, kMtWaves, 2>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
  if (obliterate && (esc == nullptr || esc2 == nullptr))
    return launchTier<true, S, false, kMtWaves, 2>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
  if (removeOrder)
    return launchTier<false, S, true, kMtWaves, 2>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
  if (esc == nullptr || esc2 == nullptr)
    return launchTier<false, S, false, kMtWaves, 2>(batch, out, docList, count, esc, numCUs, stream, nullptr, n1);
  constexpr uint32_t kCkptWords = static_cast<uint32_t>(fmt_mt::Doc<false, fmt_mt::CompactTier>::kCkptWords);
  const bool order = esc3 != nullptr && out.ckpt != nullptr;  // longest remaining streams first
  hipError_t e;
  if (!obliterate && esc4 != nullptr) {
    // Round 0: micro tier over everything → overflow list esc2 → compact tier over that list → overflow
    // list esc4 → this tier over that list → overflow list esc. Every list is reordered into esc3 first
    // (order). Without checkpoints (out.ckpt == nullptr) each tier restarts its documents from their
    // first op, and nothing steps down.
    // Round r > 0 (desc: two lists a round): compact tier over this tier's down list of round r - 1 →
    // this tier over the compact tier's overflow → esc, appended. The last round lets nothing step
    // down, so every document finishes (or is in esc).
    const int rounds = order && desc != nullptr ? kDescendRounds : 1;
    const size_t stride = static_cast<size_t>(count) + 1;
    const auto roundList = [&](int r, int k) { return desc + kDescendHead + (static_cast<size_t>(2 * (r - 1) + k)) * stride; };
    const auto ordered = [&](uint32_t* list) {
      if (!order) return list;
      hipLaunchKernelGGL(orderByRemainingKernel, dim3(1), dim3(1024), 0, stream, list, esc3, out.headers,
                         batch.docOpOffsets, out.ckpt, kCkptWords);
      return esc3;
    };
    e = launchMergeTreeMicro(batch, out, docList, count, esc2, numCUs, stream, sched ? sched + 3 : nullptr);
    if (e != hipSuccess) return e;
    for (int r = 0; r < rounds; r++) {
      MtDeviceOut o = out;
      o.descend = r + 1 < rounds;
      uint32_t* toCompact = r == 0 ? esc2 : roundList(r, 0);
      uint32_t* toSmall = r == 0 ? esc4 : roundList(r, 1);
      uint32_t* down = o.descend ? roundList(r + 1, 0) : nullptr;  // → the next round's compact tier
      uint32_t* deal = sched && r > 0 ? desc + 2 * (r - 1) : nullptr;
      const uint32_t* list = ordered(toCompact);
      e = launchMergeTreeCompact(batch, o, list + 1, count, toSmall, numCUs, stream, r == 0 ? sched : deal, false, list);
      if (e != hipSuccess) return e;
      list = ordered(toSmall);
      e = launchTier<false, S, false, kMtWaves, 2>(batch, o, list + 1, count, esc, numCUs, stream, list,
                                                   r == 0 ? n1 : (deal ? deal + 1 : nullptr), down);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  // obliterate batches: compact tier over everything → overflow list esc2 → this tier over that list →
  // overflow list esc
  e = launchMergeTreeCompact(batch, out, docList, count, esc2, numCUs, stream, sched, obliterate, nullptr);
  if (e != hipSuccess) return e;
  if (order) {
    hipLaunchKernelGGL(orderByRemainingKernel, dim3(1), dim3(1024), 0, stream, esc2, esc3, out.headers,
                       batch.docOpOffsets, out.ckpt, kCkptWords);
    esc2 = esc3;
  }
  if (obliterate)
    return launchTier<true, S, false, kMtWaves, 2>(batch, out, esc2 + 1, count, esc, numCUs, stream, esc2, n1);
  return launchTier<false, S, false, kMtWaves, 2>(batch, out, esc2 + 1, count, esc, numCUs, stream, esc2, n1);
}

}  // namespace fmt_kernels

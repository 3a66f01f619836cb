// mergetree.hip — merge-tree replay, small tier (8 register rows: 512 leaves, 2 waves/SIMD), the
// overflow-list kernel and the tier cascade (kernel template: mergetree_kernel.h).
//
// The cascade itself is planned on the host (mt_route.h planRoute): a plain batch replays every document
// in the micro tier first (mergetree_micro.hip: 2 rows); the documents it overflows go on in the compact
// tier (mergetree_compact.hip: 4 rows) from a device-side list, and those that one overflows in this
// tier from a second list; those this tier overflows go to the large tier (mergetree_large.hip) after
// the host reads the list length. With checkpoints the compact and small tiers run kDescendRounds
// times, so that a document that shrank pays for the rows it has, not for the rows it once had.
// Batches with obliterates start in the compact tier; batches with remove-order recording or adjusts
// start in this tier; neither steps down. launchMergeTree below walks the route's steps.
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

// one variant switch per translation unit
hipError_t launchMicroTier(fmt_plan::MtVariant v, const TierLaunch& a);
hipError_t launchCompactTier(fmt_plan::MtVariant v, const TierLaunch& a);
hipError_t launchLocalTier(fmt_plan::MtTier tier, fmt_plan::MtVariant v, const TierLaunch& a);

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

// Variants: obliterates (Ob) and/or the remove-order recording of SnapshotV1 batches (Rm); annotate-adjust
// batches run the Adj variants.
static hipError_t launchSmallTier(fmt_plan::MtVariant v, const TierLaunch& a) {
  using S = fmt_mt::SmallTier;
  using fmt_plan::mtKey;
  switch (v.key()) {
    // (Adj, 1 wave/SIMD: 512 registers a wave; at 2 the property-manager code spilled 3710 VGPRs to scratch,
    // at 1 the overflow lives in AGPRs)
    case mtKey(true, true, true): return launchTier<true, S, true, kMtWaves, 1, true>(a);
    case mtKey(true, false, true): return launchTier<true, S, false, kMtWaves, 1, true>(a);
    case mtKey(true, true): return launchTier<true, S, true, kMtWaves, 2>(a);
    case mtKey(true, false): return launchTier<true, S, false, kMtWaves, 2>(a);
    case mtKey(false, true): return launchTier<false, S, true, kMtWaves, 2>(a);
    case mtKey(false, false): return launchTier<false, S, false, kMtWaves, 2>(a);
  }
  return hipErrorInvalidValue;
}

hipError_t launchMergeTree(const MtDeviceBatch& batch, const MtDeviceOut& out, const fmt_plan::MtRoute& route,
                           const MtLists& lists, const MtLaunchEnv& env) {
  using fmt_plan::MtListKind;
  using fmt_plan::MtTier;
  constexpr uint32_t kCkptWords = static_cast<uint32_t>(fmt_mt::Doc<false, fmt_mt::CompactTier>::kCkptWords);
  if (route.nSteps == 0) return hipSuccess;
  const bool caller = route.steps[0].in.kind == MtListKind::kCaller;
  if ((caller && lists.docs == nullptr) || (route.rounds > 1 && lists.desc == nullptr)) return hipErrorInvalidValue;
  // every launch's bound on its list, and the stride of the step-down slab's lists
  const uint32_t count = caller ? lists.count : batch.nDocs;
  const auto list = [&](fmt_plan::MtList l) -> uint32_t* {
    switch (l.kind) {
      case MtListKind::kMicroUp: return lists.microUp;
      case MtListKind::kCompactUp: return lists.compactUp;
      case MtListKind::kToLarge: return lists.toLarge;
      case MtListKind::kOrdered: return lists.ordered;
      case MtListKind::kRound:
        return lists.desc + fmt_plan::kDescendHead + static_cast<size_t>(2 * (l.r - 1) + l.k) * (static_cast<size_t>(count) + 1);
      default: return nullptr;
    }
  };
  for (int i = 0; i < route.nSteps; i++) {
    const fmt_plan::MtStep& s = route.steps[i];
    MtDeviceOut o = out;
    o.descend = s.descend;
    const uint32_t* in = s.in.onDevice() ? list(s.in) : nullptr;
    if (in != nullptr && s.orderInto.kind != MtListKind::kNone) {  // longest remaining streams first
      uint32_t* ordered = list(s.orderInto);
      hipLaunchKernelGGL(orderByRemainingKernel, dim3(1), dim3(1024), 0, env.stream, in, ordered, out.headers,
                         batch.docOpOffsets, out.ckpt, kCkptWords);
      in = ordered;
    }
    uint32_t* next = s.deal.kind == fmt_plan::MtDealKind::kRound ? lists.desc + 2 * (s.deal.r - 1) + s.deal.k
                                                                 : lists.sched + static_cast<int>(s.deal.kind);
    const TierLaunch a{batch, o, in ? in + 1 : caller ? lists.docs : nullptr, count, list(s.up), env.numCUs, env.stream, in,
                       next, list(s.down)};
    const hipError_t e = s.variant.loc               ? launchLocalTier(s.tier, s.variant, a)
                         : s.tier == MtTier::kMicro   ? launchMicroTier(s.variant, a)
                         : s.tier == MtTier::kCompact ? launchCompactTier(s.variant, a)
                         : s.tier == MtTier::kSmall   ? launchSmallTier(s.variant, a)
                                                      : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fmt_kernels

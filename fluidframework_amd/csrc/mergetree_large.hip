// mergetree_large.hip — merge-tree replay, large tier (32 rows in private memory: 2048 leaves,
// 131071 UTF-16 units in HBM; one document per workgroup) for the documents the small tier overflows.
#include "mergetree_kernel.h"

namespace fmt_kernels {

constexpr int kMtWavesLarge = 1;  // large tier: one document per workgroup, 1 wave/SIMD (VGPRs)

int mergeTreeProfileLarge(uint64_t* out, int n, bool reset) { return addTuProfile(out, n, reset); }

hipError_t launchMergeTreeLarge(const MtDeviceBatch& batch, const MtDeviceOut& out, const fmt_plan::MtRoute& route,
                                const MtLists& lists, uint32_t count, const MtLaunchEnv& env) {
  using G = fmt_mt::LargeTier;
  using fmt_plan::mtKey;
  // (nothing is collected: what this tier cannot hold the host reads from the headers)
  const TierLaunch a{batch, out, lists.toLarge + 1, count, nullptr, env.numCUs, env.stream, nullptr,
                     lists.sched + static_cast<int>(fmt_plan::MtDealKind::kLarge), nullptr};
  switch (route.large.key()) {
    case mtKey(false, false, true, true): return launchTier<false, G, false, kMtWavesLarge, 1, true, true>(a);  // f4 with annotate-adjust
    // f4: the local client's submissions, acks, rollbacks and reconnects (plain ops otherwise)
    case mtKey(false, false, false, true): return launchTier<false, G, false, kMtWavesLarge, 1, false, true>(a);
    case mtKey(true, true, true): return launchTier<true, G, true, kMtWavesLarge, 1, true>(a);
    case mtKey(true, false, true): return launchTier<true, G, false, kMtWavesLarge, 1, true>(a);
    case mtKey(true, true): return launchTier<true, G, true, kMtWavesLarge, 1>(a);
    case mtKey(true, false): return launchTier<true, G, false, kMtWavesLarge, 1>(a);
    case mtKey(false, true): return launchTier<false, G, true, kMtWavesLarge, 1>(a);
    case mtKey(false, false): return launchTier<false, G, false, kMtWavesLarge, 1>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace fmt_kernels

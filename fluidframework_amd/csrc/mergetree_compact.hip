// mergetree_compact.hip — merge-tree replay, compact tier (4 register rows: 256 leaves). Obliterate
// batches start here; plain batches replay the micro tier's overflow list in it (mergetree_micro.hip);
// see mergetree.hip for the cascade. Plain batches run it at 4 waves/SIMD (128 VGPRs, 29 spilled with
// the checkpoint restore compiled in; 16 waves × 9312 B of LDS per CU): A/B at full T1 449 -> 395 ms
// against 3 waves/SIMD at 152 VGPRs (profiles/r3/cw4/). Obliterate batches keep 3 (168 VGPRs, the
// full Scratch).
#include "mergetree_kernel.h"

namespace fmt_kernels {

constexpr int kMtWavesCompact = 4;  // 4 documents per workgroup

int mergeTreeProfileCompact(uint64_t* out, int n, bool reset) { return addTuProfile(out, n, reset); }

// a.countDev: the documents are the micro tier's overflow list (its length on the device); those it left
// at a checkpoint resume from it.
hipError_t launchCompactTier(fmt_plan::MtVariant v, const TierLaunch& a) {
  switch (v.key()) {
    // Doc<true>: the same 4 rows plus the live-obliterate table (163 VGPRs)
    case fmt_plan::mtKey(true, false): return launchTier<true, fmt_mt::CompactTier, false, kMtWavesCompact, 3>(a);
    case fmt_plan::mtKey(false, false): return launchTier<false, fmt_mt::CompactTier, false, kMtWavesCompact, 4>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace fmt_kernels

// mergetree_micro.hip — merge-tree replay, micro tier (2 register rows: 128 leaves, 1024 text units).
// Plain batches (no obliterates, remove order, adjusts or local records) start here; see mergetree.hip
// for the cascade. A document about to outgrow the rows or the text stops at a checkpoint that the
// compact tier resumes.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): at __launch_bounds__(256, 4) the
// kernel takes 106 VGPRs with no scratch, 7264 B of LDS per wave (Scratch<MicroTier> without the
// obliterate table), 4 waves/SIMD (16 waves × 7264 B = 114 KiB of the CU's 160). At (256, 5) it is
// squeezed into 96 VGPRs with 3 of them spilled (16 B/lane of scratch); the rule here is the highest
// occupancy without scratch, so 4.
#include "mergetree_kernel.h"

namespace fmt_kernels {

constexpr int kMtWavesMicro = 4;  // 4 documents per workgroup

int mergeTreeProfileMicro(uint64_t* out, int n, bool reset) { return addTuProfile(out, n, reset); }

hipError_t launchMicroTier(fmt_plan::MtVariant v, const TierLaunch& a) {
  switch (v.key()) {
    case fmt_plan::mtKey(false, false): return launchTier<false, fmt_mt::MicroTier, false, kMtWavesMicro, 4>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace fmt_kernels

// mergetree_local.hip — f4 local-client batches (FMT_MT_F_LOCAL / ACK / ROLLBACK / REGEN records),
// the tiers below the large one (round 6). Round 5 ran every local document in the large tier (one
// wave per workgroup, leaf rows in private memory). Now a local batch takes a register tier first, as
// plain batches do, but without checkpoints: the small tier's local variant
// (Doc<false, SmallTier, false, false, true>: 8 register rows, 512 leaves, 6144 UTF-16 units in LDS,
// the pending-group count as a sixth leaf word) replays every document, and the ones it cannot hold
// (FMT_E_CAPACITY) replay again, from their first op, in the large tier's local variant
// (mergetree_large.hip). The compact tier's local variant (4 rows) can go first instead
// (FMT_LOCAL_PATH). The local state itself — pending segment groups, group records,
// PropertiesManager records, regenerated ops, normalization scratch — lives in per-document HBM slabs
// (mt_engine.h LocalTables) in every tier, so a restart simply rewrites them.
#include "mergetree_kernel.h"

namespace fmt_kernels {

constexpr int kMtWavesLocal = 4;  // 4 documents per workgroup
// Which of them a batch takes: mt_route.h FMT_LOCAL_PATH. 0: compact → large; 1: small → large (kept: the
// reference farms' writer views overflow the compact tier in 17 of 28 streams; A/B at 20k documents 383 ms
// against 410 for 2 and 1379 for 0, profiles/r6/local2/ab_local.json); 2: compact → small → large

hipError_t launchLocalTier(fmt_plan::MtTier tier, fmt_plan::MtVariant v, const TierLaunch& a) {
  using K = fmt_mt::CompactTier;
  using S = fmt_mt::SmallTier;
  using fmt_plan::MtTier;
  switch (v.key() | static_cast<uint32_t>(tier) << 4) {
    // annotate-adjust batches (round 6): the PropertiesManager's remote and local change lists with
    // adjust folding (Doc<..., Adj, Loc>), small tier first whatever FMT_LOCAL_PATH says
    case fmt_plan::mtKey(false, false, true, true) | static_cast<uint32_t>(MtTier::kSmall) << 4:
      return launchTier<false, S, false, kMtWavesLocal, 2, true, true>(a);
    case fmt_plan::mtKey(false, false, false, true) | static_cast<uint32_t>(MtTier::kSmall) << 4:
      return launchTier<false, S, false, kMtWavesLocal, 2, false, true>(a);
    case fmt_plan::mtKey(false, false, false, true) | static_cast<uint32_t>(MtTier::kCompact) << 4:
      return launchTier<false, K, false, kMtWavesLocal, 3, false, true>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace fmt_kernels

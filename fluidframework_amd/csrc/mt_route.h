// mt_route.h — the host-planned route of a merge-tree batch through the tier cascade: which register
// tiers run, in which Doc variant, over which document lists, where each appends the documents it hands
// up or down, from which counter it deals them to waves, and what the result views of the register
// tiers and of the large pass may point at. planRoute is a pure function of the load plan's flags
// (mt_plan.h) and of two facts of the load, whether the checkpoint slab and the step-down slab were
// allocated. launchMergeTree (mergetree.hip) walks the steps, fmt_mt_run (runtime.cpp) builds its two
// MtDeviceOuts from the booleans, and the host emulations (tests/emu) execute the same steps, so the
// CPU suites run the cascade that ships (but for a step's orderInto: the emulations replay a list as it
// is, no result depends on its order, so orderByRemainingKernel is checked on the device only). Host only:
// no HIP include, no fmt_ctx, no heap (the export of a route as words for the test hooks: mt_route_words.h).
#pragma once

#include <cstddef>
#include <cstdint>

#include "mt_plan.h"

// Rounds of the plain cascade: in every round but the last a small-tier document that shrank to half
// of the compact tier stops (fmt_mt::kCkptDescend) and goes on a "down" list that the compact tier
// replays in the next round. DESIGN.md §4.1 has the hop counts behind it. (1: a document only ever
// moves up)
#ifndef FMT_DESCEND_ROUNDS
#define FMT_DESCEND_ROUNDS 2
#endif
// Local-client batches. 0: compact → large; 1: small → large (kept: the reference farms' writer views
// overflow the compact tier in 17 of 28 streams; A/B at 20k documents 383 ms against 410 for 2 and 1379
// for 0, profiles/r6/local2/ab_local.json); 2: compact → small → large
#ifndef FMT_LOCAL_PATH
#define FMT_LOCAL_PATH 1
#endif

namespace fmt_plan {

constexpr int kDescendRounds = FMT_DESCEND_ROUNDS;
constexpr int kMaxDescendRounds = 8;
constexpr size_t kDescendHead = 64;  // dealing counters of the rounds after the first, 2 a round
static_assert(kDescendRounds >= 1 && kDescendRounds <= kMaxDescendRounds && 2 * (kMaxDescendRounds - 1) <= kDescendHead,
              "the step-down slab's head holds two dealing counters per round after the first");

// Words of the step-down slab for `count` documents: the head, then two lists (count + 1 words each) per
// round after the first.
inline size_t mergeTreeDescendWords(uint32_t count, int rounds = kDescendRounds) {
  return kDescendHead + static_cast<size_t>(2 * (rounds - 1)) * (static_cast<size_t>(count) + 1);
}

enum class MtTier : uint8_t { kMicro, kCompact, kSmall, kLarge };

// A fmt_mt::Doc<Ob, Tier, Rm, Adj, Loc> variant: obliterates, remove-order recording, annotate-adjust,
// local-client records.
struct MtVariant {
  bool ob, rm, adj, loc;
  constexpr uint32_t key() const { return (ob ? 1u : 0u) | (rm ? 2u : 0u) | (adj ? 4u : 0u) | (loc ? 8u : 0u); }
};
constexpr uint32_t mtKey(bool ob, bool rm, bool adj = false, bool loc = false) { return MtVariant{ob, rm, adj, loc}.key(); }

// The (tier, variant) pairs that exist as mergeTreeKernel instantiations, each in the translation unit of
// its tier (the local variants of the register tiers: mergetree_local.hip). launchTier
// (mergetree_kernel.h) refuses to compile any other pair.
struct MtKernelId {
  MtTier tier;
  MtVariant variant;
};
constexpr MtKernelId kMtKernels[] = {
    {MtTier::kMicro, {false, false, false, false}},
    {MtTier::kCompact, {false, false, false, false}}, {MtTier::kCompact, {true, false, false, false}},
    {MtTier::kCompact, {false, false, false, true}},
    {MtTier::kSmall, {false, false, false, false}},   {MtTier::kSmall, {true, false, false, false}},
    {MtTier::kSmall, {false, true, false, false}},    {MtTier::kSmall, {true, true, false, false}},
    {MtTier::kSmall, {true, false, true, false}},     {MtTier::kSmall, {true, true, true, false}},
    {MtTier::kSmall, {false, false, false, true}},    {MtTier::kSmall, {false, false, true, true}},
    {MtTier::kLarge, {false, false, false, false}},   {MtTier::kLarge, {true, false, false, false}},
    {MtTier::kLarge, {false, true, false, false}},    {MtTier::kLarge, {true, true, false, false}},
    {MtTier::kLarge, {true, false, true, false}},     {MtTier::kLarge, {true, true, true, false}},
    {MtTier::kLarge, {false, false, false, true}},    {MtTier::kLarge, {false, false, true, true}},
};
constexpr bool hasMtKernel(MtTier tier, MtVariant v) {
  for (const MtKernelId& k : kMtKernels)
    if (k.tier == tier && k.variant.key() == v.key()) return true;
  return false;
}

// A document list of a step. kEvery: documents 0 .. nDocs. kCaller: the list the caller brings (the
// documents that are neither huge nor refused). The others live on the device, [0] = n, then ids:
// kMicroUp / kCompactUp, what the micro / compact tier hands up in the first round; kToLarge, what
// the last register tier hands to the large pass; kOrdered, a list reordered by remaining ops; kRound,
// list k (0: the small tier's down list, which the compact tier replays; 1: what that compact pass
// hands up) of round r >= 1 in the step-down slab.
enum class MtListKind : uint8_t { kNone, kEvery, kCaller, kMicroUp, kCompactUp, kToLarge, kOrdered, kRound };
struct MtList {
  MtListKind kind = MtListKind::kNone;
  uint8_t r = 0, k = 0;
  constexpr bool onDevice() const { return kind >= MtListKind::kMicroUp; }
};
constexpr MtList roundList(int r, int k) { return MtList{MtListKind::kRound, static_cast<uint8_t>(r), static_cast<uint8_t>(k)}; }

// The counter a step deals documents to waves from: one of the four per-tier counters (the large one is
// the large pass's), or counter k (0 compact, 1 small) of round r >= 1 in the step-down slab's head.
enum class MtDealKind : uint8_t { kCompact, kSmall, kLarge, kMicro, kRound };
struct MtDeal {
  MtDealKind kind = MtDealKind::kSmall;
  uint8_t r = 0, k = 0;
};

struct MtStep {
  MtTier tier;
  MtVariant variant;
  MtList in;         // the documents it replays
  MtList up;         // appended to: the documents it could not hold, or stopped at a checkpoint
  MtList down;       // appended to: the documents that stopped for the tier below (kNone: none may)
  MtList orderInto;  // `in` is first reordered, longest remaining streams first, into this list (kNone: as it is)
  MtDeal deal;
  bool descend;      // the launch's step-down switch (MtDeviceOut::descend)
};

struct MtRoute {
  // what the result views may point at (fmt_mt_run's MtDeviceOuts)
  bool tiersCkpt = false;         // the register tiers get the checkpoint slab
  bool largeCkpt = false;         // the large pass gets it (the live-obliterate table of the slots)
  bool largeResumesSmall = false; // the large pass resumes from the small tier's result slabs
  bool largeHugeCkpt = false;     // the large pass may leave large → huge checkpoints
  bool largeLocal = false;        // the large pass is the local variant (documents restart, none grows on)
  MtVariant large{};              // the large pass's variant
  bool startsSmall = false;       // remove-order batches: one register tier (nominalLaunches)
  int rounds = 1;
  int nSteps = 0;
  MtStep steps[1 + 2 * kMaxDescendRounds];

  // fmt_stats::launches: the register tiers as one or two nominal passes, the large pass, the pass over
  // the documents that grew into the huge tier.
  constexpr uint32_t nominalLaunches(bool largeRan, bool grew) const {
    return (startsSmall ? 1u : 2u) + (largeRan ? 1u : 0u) + (grew ? 1u : 0u);
  }
};

// rounds / localPath: the build's, or a test's.
inline MtRoute planRoute(const MtPlan& P, bool ckptSlab, bool descSlab, int rounds = kDescendRounds,
                         int localPath = FMT_LOCAL_PATH) {
  using L = MtListKind;
  const bool ob = P.obliterates, rm = P.hasRmOrder(), adj = P.anyAdjust, loc = P.local;
  const bool ckptOk = ckptSlab && !rm;  // (no slab is asked for with remove-order recording)
  MtRoute R;
  R.tiersCkpt = ckptOk && !adj;
  R.largeCkpt = ckptOk && ob && !adj;
  R.largeResumesSmall = !rm;
  R.largeHugeCkpt = !loc;
  R.largeLocal = loc;
  // (annotate-adjust batches run the Ob variants, unless local)
  R.large = loc ? MtVariant{false, false, adj, true} : MtVariant{ob || adj, rm, adj, false};
  R.startsSmall = rm;
  const MtList batch{!P.hugeDocs.empty() || !P.refused.empty() ? L::kCaller : L::kEvery};
  const MtList none{}, toLarge{L::kToLarge}, microUp{L::kMicroUp}, compactUp{L::kCompactUp};
  const MtList order{R.tiersCkpt ? L::kOrdered : L::kNone};
  const MtDeal dCompact{MtDealKind::kCompact}, dSmall{MtDealKind::kSmall};
  auto add = [&](MtTier t, MtVariant v, MtList in, MtList up, MtList down, MtList orderInto, MtDeal deal, bool descend) {
    R.steps[R.nSteps++] = MtStep{t, v, in, up, down, orderInto, deal, descend};
  };
  if (loc) {  // no checkpoints: a document a tier cannot hold restarts in the next
    const MtVariant v{false, false, adj, true};
    // (annotate-adjust: small tier first whatever localPath says)
    if (!adj && localPath != 1) add(MtTier::kCompact, v, batch, localPath == 2 ? compactUp : toLarge, none, none, dCompact, false);
    if (adj || localPath == 1) add(MtTier::kSmall, v, batch, toLarge, none, none, dSmall, false);
    else if (localPath == 2) add(MtTier::kSmall, v, compactUp, toLarge, none, none, dSmall, false);
    return R;
  }
  if (adj || rm) {  // the small tier over every document
    add(MtTier::kSmall, R.large, batch, toLarge, none, none, dSmall, false);
    return R;
  }
  const MtVariant v{ob, false, false, false};
  if (ob) {  // obliterate batches start compact; nothing steps down
    add(MtTier::kCompact, v, batch, compactUp, none, none, dCompact, false);
    add(MtTier::kSmall, v, compactUp, toLarge, none, order, dSmall, false);
    return R;
  }
  // Plain batches. Round 0: micro over everything → compact over microUp → small over compactUp →
  // toLarge. Round r > 0: compact over the small tier's down list of round r - 1 → small over what
  // that hands up → toLarge, appended. The last round lets nothing step down, so every document
  // finishes or is in toLarge. Without the checkpoint slab each tier restarts its documents from their
  // first op, nothing is reordered and nothing steps down.
  R.rounds = R.tiersCkpt && descSlab ? rounds : 1;
  add(MtTier::kMicro, v, batch, microUp, none, none, MtDeal{MtDealKind::kMicro}, false);
  for (int r = 0; r < R.rounds; r++) {
    const bool descend = r + 1 < R.rounds;
    const MtList toCompact = r == 0 ? microUp : roundList(r, 0), toSmall = r == 0 ? compactUp : roundList(r, 1);
    const auto deal = [&](int k) {
      return r == 0 ? (k == 0 ? dCompact : dSmall) : MtDeal{MtDealKind::kRound, static_cast<uint8_t>(r), static_cast<uint8_t>(k)};
    };
    add(MtTier::kCompact, v, toCompact, toSmall, none, order, deal(0), descend);
    add(MtTier::kSmall, v, toSmall, toLarge, descend ? roundList(r + 1, 0) : none, order, deal(1), descend);
  }
  return R;
}

// Whether fmt_mt_load asks for the step-down slab: exactly for the batches whose route has more than one
// round with it.
inline bool routeUsesDescSlab(const MtPlan& P, bool ckptSlab) { return planRoute(P, ckptSlab, true).rounds > 1; }

}  // namespace fmt_plan

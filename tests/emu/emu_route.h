// emu_route.h — TEST INFRASTRUCTURE ONLY: the route of csrc/mt_route.h executed on the host. replayTier is
// one launch of mergeTreeKernel plus collectOverflowKernel (csrc/mergetree_kernel.h) with the kernel's own
// binding (csrc/mt_bind.h); replayStep picks the Doc variant by the key of the per-TU switches
// (csrc/mergetree*.hip) out of kMtKernels; runRoute is launchMergeTree (csrc/mergetree.hip).
#pragma once
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "emu_batch.h"
#include "../../fluidframework_amd/csrc/mt_route.h"

namespace emu {

using fmt_kernels::HandOff;
using fmt_kernels::MtDeviceOut;
using fmt_kernels::Slab;
using fmt_plan::MtTier;
using fmt_plan::MtVariant;

// One launch. The register tiers write results at the small tier's strides, like the runtime's slabs, the
// large tier at its own (slot = document: one slab per document); ownStrides: a tier alone, at its own
// capacities. list: [0] = n, then ids, or null: every document. overList: a list that a launch before this
// one built (not the caller's own). failed (or null): the first failure among the launch's documents.
struct Launch {
  const EmuBatch& eb;
  const MtDeviceOut& out;
  const uint32_t* list;
  bool overList;
  uint32_t *up, *down;
  bool ownStrides;
  int* failed;
};

template <class C, bool Ob, bool Rm, bool Adj, bool Loc>
int replayTier(const Launch& a) {
  using Doc = fmt_mt::Doc<Ob, C, Rm, Adj, Loc>;
  auto scratch = std::make_unique<fmt_mt::Scratch<C>>();
  auto doc = std::make_unique<Doc>();
  const size_t leafStride = a.ownStrides ? Doc::kCapLeaves : Slab<C>::kLeaves, charStride = a.ownStrides ? Doc::kCapChars : Slab<C>::kChars;
  const uint32_t count = a.list ? a.list[0] : a.eb.view.nDocs;
  if (a.failed) *a.failed = FMT_OK;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t d = a.list ? a.list[1 + i] : i;
    std::memset(scratch.get(), 0xCD, sizeof(fmt_mt::Scratch<C>));  // poison: state must be initialized
    const fmt_kernels::DocBinding bd = fmt_kernels::bindDoc<Doc>(a.eb.view, a.out, d, d, leafStride, charStride, Slab<C>::kProps, a.overList);
    new (doc.get()) Doc();
    doc->s = scratch.get();
    doc->run(bd.in, bd.o);
    const HandOff to = fmt_kernels::collectHeader(a.out.headers[d]);
    uint32_t* dst = to == HandOff::kUp ? a.up : to == HandOff::kDown ? a.down : nullptr;
    if (dst != nullptr) dst[1 + dst[0]++] = d;
    const int st = a.out.headers[d].status;  // (a document stopped at a checkpoint goes on in another tier)
    if (a.failed && *a.failed == FMT_OK && st != fmt_mt::kCkptEscalate && st != fmt_mt::kCkptDescend && st != fmt_ckpt::kStatusHuge) *a.failed = st;
  }
  return static_cast<int>(count);
}

// Returns the documents replayed, -1 for a (tier, variant) that is no kernel.
inline int replayStep(MtTier tier, MtVariant v, const Launch& a) {
  using namespace fmt_mt;
#define EMU_STEP(T, C, ob, rm, adj, loc)                                                       \
  case static_cast<uint32_t>(T) << 4 | fmt_plan::mtKey(ob, rm, adj, loc):                      \
    static_assert(fmt_plan::hasMtKernel(T, MtVariant{ob, rm, adj, loc}), "not in kMtKernels"); \
    return replayTier<C, ob, rm, adj, loc>(a)
#define EMU_STEPS8(T, C)                  \
  EMU_STEP(T, C, false, false, false, false); \
  EMU_STEP(T, C, true, false, false, false);  \
  EMU_STEP(T, C, false, true, false, false);  \
  EMU_STEP(T, C, true, true, false, false);   \
  EMU_STEP(T, C, true, false, true, false);   \
  EMU_STEP(T, C, true, true, true, false);    \
  EMU_STEP(T, C, false, false, false, true);  \
  EMU_STEP(T, C, false, false, true, true)
  switch (static_cast<uint32_t>(tier) << 4 | v.key()) {
    EMU_STEP(MtTier::kMicro, MicroTier, false, false, false, false);
    EMU_STEP(MtTier::kCompact, CompactTier, false, false, false, false);
    EMU_STEP(MtTier::kCompact, CompactTier, true, false, false, false);
    EMU_STEP(MtTier::kCompact, CompactTier, false, false, false, true);
    EMU_STEPS8(MtTier::kSmall, SmallTier);
    EMU_STEPS8(MtTier::kLarge, LargeTier);
  }
#undef EMU_STEPS8
#undef EMU_STEP
  return -1;
}

// launchMergeTree on the host: the register-tier steps of `route` in order, each list where the route names
// it; the caller's list is every document (no huge tier here). orderInto only permutes a list, which no
// result depends on: the list is replayed as it is. toLarge ([0] = n, then ids): what is left for the large
// pass. failed: Launch::failed of the last step. Returns the steps run, -1 for a step it cannot run.
inline int runRoute(const fmt_plan::MtRoute& route, const EmuBatch& eb, const MtDeviceOut& out, uint32_t* toLarge, int* failed) {
  using fmt_plan::MtListKind;
  const size_t stride = eb.view.nDocs + 1ull;
  // (every device list of the route, zeroed as the runtime zeroes them: microUp, compactUp, the rounds')
  std::vector<uint32_t> lists(static_cast<size_t>(2 + 2 * route.rounds) * stride, 0u);
  toLarge[0] = 0;
  const auto list = [&](fmt_plan::MtList l) -> uint32_t* {
    switch (l.kind) {
      case MtListKind::kMicroUp: return lists.data();
      case MtListKind::kCompactUp: return lists.data() + stride;
      case MtListKind::kToLarge: return toLarge;
      case MtListKind::kRound: return lists.data() + static_cast<size_t>(2 * l.r + l.k) * stride;
      default: return nullptr;
    }
  };
  for (int i = 0; i < route.nSteps; i++) {
    const fmt_plan::MtStep& s = route.steps[i];
    MtDeviceOut o = out;
    o.descend = s.descend;
    if (replayStep(s.tier, s.variant, Launch{eb, o, list(s.in), s.in.onDevice(), list(s.up), list(s.down), false, failed}) < 0) return -1;
  }
  return route.nSteps;
}

// planRoute over the plan of `b`, as fmt_mt_load calls it (the large tier's capacities for
// the plan). rounds <= 0 / localPath < 0: the build's. force: the ob / loc variants whatever the ops hold.
// Returns the plan's status.
inline int planRouteOf(const fmt_mt_batch* b, bool ckptSlab, bool descSlab, int rounds, int localPath, fmt_plan::MtRoute& route,
                       MtVariant force = MtVariant{}) {
  struct {
    uint32_t leaves = Slab<fmt_mt::LargeTier>::kLeaves, chars = Slab<fmt_mt::LargeTier>::kChars;
  } large;
  fmt_plan::MtPlan P;
  const char* why = nullptr;
  const int rc = rounds > fmt_plan::kMaxDescendRounds ? FMT_E_USAGE : fmt_plan::planMergeTreeLoad(b, large, P, &why);
  if (rc != FMT_OK) return rc;
  P.obliterates = P.obliterates || force.ob;
  P.local = P.local || force.loc;
  route = fmt_plan::planRoute(P, ckptSlab, descSlab, rounds > 0 ? rounds : fmt_plan::kDescendRounds,
                              localPath >= 0 ? localPath : FMT_LOCAL_PATH);
  return FMT_OK;
}

}  // namespace emu

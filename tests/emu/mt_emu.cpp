// mt_emu.cpp — TEST INFRASTRUCTURE ONLY: the merge-tree engine source (mt_engine.h) and the launch
// binding around it (mt_bind.h) compiled for the host with the 64-lane emulation of wave.h, so the CPU
// parity suite can check the exact kernel logic against the oracle without a GPU. Never loaded by the
// product (libfmt.so has no CPU path).
#include <cstring>
#include <vector>

#define EMU_ROUTE_ALL_VARIANTS 1
#include "emu_route.h"

// Annotate-adjust state of the last emulated replay (the runtime's number slabs, fixed capacity
// here): the batch's host numbers sorted for number → id lookups, per-document number tables.
constexpr uint32_t kEmuNumCap = 4096;
static std::vector<double> g_numSorted, g_nums;
static std::vector<uint32_t> g_numSortedId, g_numCount;
static std::vector<uint64_t> g_numOffs;
static fmt_mt::AdjustTables g_adj;
// property-manager records (Doc::pm*) and the per-leaf legacy prop sets of the last replay
constexpr uint32_t kEmuPmCap = 1 << 14;
static std::vector<uint32_t> g_pm;
static std::vector<uint64_t> g_pmOffs;
static std::vector<uint16_t> g_legacy;
static size_t g_legacyStride = 0;

static std::vector<uint32_t> g_numSortedOffs;

static void prepareNumbers(const fmt_mt_batch* b) {
  g_numSorted.clear();
  g_numSortedId.clear();
  g_numSortedOffs.clear();
  g_nums.clear();
  g_numCount.assign(b->n_docs, 0u);
  if (b->adjusts == nullptr || b->value_num == nullptr) return;
  // the host numbers ascending with their first value id, as fmt_mt_load prepares them
  fmt_plan::prepareSortedNumbers(b->value_num, b->n_values, b->doc_value_base, b->n_docs, g_numSorted, g_numSortedId,
                                 g_numSortedOffs);
  g_nums.assign(static_cast<size_t>(b->n_docs) * kEmuNumCap, 0.0);
  g_numOffs.resize(b->n_docs + 1ull);
  for (uint32_t d = 0; d <= b->n_docs; d++) g_numOffs[d] = static_cast<uint64_t>(d) * kEmuNumCap;
  g_pm.assign(static_cast<size_t>(b->n_docs) * kEmuPmCap * 4, 0u);
  g_pmOffs.resize(b->n_docs + 1ull);
  for (uint32_t d = 0; d <= b->n_docs; d++) g_pmOffs[d] = static_cast<uint64_t>(d) * kEmuPmCap;
  g_adj = fmt_mt::AdjustTables{};
  g_adj.adjusts = b->adjusts;
  g_adj.nAdjusts = b->n_adjusts;
  g_adj.nValues = b->value_num ? b->n_values : 0u;
  g_adj.valueNum = b->value_num;
  g_adj.numSorted = g_numSorted.data();
  g_adj.numSortedId = g_numSortedId.data();
  g_adj.nNumSorted = static_cast<uint32_t>(g_numSorted.size());
  g_adj.valueBase = b->doc_value_base;
  g_adj.numSortedOffs = b->doc_value_base != nullptr ? g_numSortedOffs.data() : nullptr;
  g_adj.nums = g_nums.data();
  g_adj.numOffsets = g_numOffs.data();
  g_adj.numCount = g_numCount.data();
  g_adj.pm = g_pm.data();
  g_adj.pmOffsets = g_pmOffs.data();
}

// ckpt (plain batches): per-document tier checkpoints; the compact tier saves, the small tier resumes
// the documents whose header says kCkptEscalate and, with onlyEscalated, replays only those and the
// documents that overflowed (the runtime's cascade over the overflow list).
// f4 (the local client): per-document slabs of the last emu_mt_replay_local (fixed capacities)
constexpr uint32_t kEmuGroupCap = 4096, kEmuRecCap = 16384, kEmuRegenCap = 4096, kEmuRegenTextCap = 1 << 16,
                   kEmuScratchCap = 1 << 16;
static std::vector<uint32_t> g_lgroups, g_lrecs, g_lpm, g_lscratch, g_lregenCount;
static std::vector<uint64_t> g_lgroupOffs, g_lrecOffs, g_lpmOffs, g_lscratchOffs, g_lregenOffs, g_lregenTextOffs;
static std::vector<fmt_mt_op> g_lregen;
static std::vector<uint16_t> g_lregenText;
static fmt_mt::LocalTables g_loc;

static void prepareLocal(uint32_t nDocs) {
  auto offs = [&](std::vector<uint64_t>& v, uint64_t cap) {
    v.resize(nDocs + 1ull);
    for (uint32_t d = 0; d <= nDocs; d++) v[d] = static_cast<uint64_t>(d) * cap;
  };
  g_lgroups.assign(static_cast<size_t>(nDocs) * kEmuGroupCap * 8, 0u);
  g_lrecs.assign(static_cast<size_t>(nDocs) * kEmuRecCap * 2, 0u);
  g_lpm.assign(static_cast<size_t>(nDocs) * kEmuPmCap * 4, 0u);
  g_lscratch.assign(static_cast<size_t>(nDocs) * kEmuScratchCap, 0u);
  g_lregen.assign(static_cast<size_t>(nDocs) * kEmuRegenCap, fmt_mt_op{});
  g_lregenText.assign(static_cast<size_t>(nDocs) * kEmuRegenTextCap, 0u);
  g_lregenCount.assign(2ull * nDocs, 0u);
  offs(g_lgroupOffs, kEmuGroupCap);
  offs(g_lrecOffs, kEmuRecCap);
  offs(g_lpmOffs, kEmuPmCap);
  offs(g_lscratchOffs, kEmuScratchCap);
  offs(g_lregenOffs, kEmuRegenCap);
  offs(g_lregenTextOffs, kEmuRegenTextCap);
  g_loc = fmt_mt::LocalTables{g_lgroups.data(), g_lgroupOffs.data(), g_lrecs.data(), g_lrecOffs.data(),
                              g_lpm.data(), g_lpmOffs.data(), g_lregen.data(), g_lregenOffs.data(),
                              g_lregenText.data(), g_lregenTextOffs.data(), g_lregenCount.data(),
                              g_lscratch.data(), g_lscratchOffs.data()};
}

namespace {

using fmt_kernels::MtDeviceOut;
using fmt_kernels::Slab;
using fmt_plan::MtRoute;
using fmt_plan::MtTier;
using fmt_plan::MtVariant;
using S = fmt_mt::SmallTier;
using G = fmt_mt::LargeTier;

// The caller's arrays of one replay call: results (at the strides the entry point documents) and record slabs.
struct Call {
  const fmt_mt_batch* b;
  fmt_mt_doc_result* headers;
  fmt_mt_leaf* leaves;
  uint16_t* chars;
  fmt_mt_propset* props;
  fmt_mt_catchup_range* catchup = nullptr;
  uint32_t capCatchup = 0;
  fmt_mt_remove_order* rmOrder = nullptr;
  uint32_t capRm = 0;
  uint32_t* hugeCk = nullptr;
  EmuBatch batch(bool loc) const {
    return EmuBatch(b, catchup != nullptr, capCatchup, rmOrder != nullptr, capRm, g_nums.empty() ? nullptr : &g_adj, loc ? &g_loc : nullptr);
  }
};

// Annotate-adjust batches: the legacy getAtSeq views of the call (emu_mt_legacy_props) at `stride`.
uint16_t* legacyViews(const Call& c, bool adj, size_t stride) {
  if (!adj) return nullptr;
  g_legacyStride = stride;
  g_legacy.assign(c.b->n_docs * stride, 0xFFFFu);
  return g_legacy.data();
}

// One tier alone over every document from its first op, at its own strides, without checkpoints (the large
// tier of an annotate-adjust batch: with the legacy views).
int oneTier(const Call& c, MtTier tier, MtVariant v) {
  const EmuBatch eb = c.batch(v.loc);
  const MtDeviceOut out{c.headers, c.leaves, c.chars, c.props, c.catchup, c.rmOrder, nullptr, nullptr, nullptr,
                        legacyViews(c, v.adj && tier == MtTier::kLarge, Slab<G>::kLeaves), c.hugeCk};
  int failed = FMT_OK;
  return emu::replayStep(tier, v, emu::Launch{eb, out, nullptr, false, nullptr, nullptr, true, &failed}) < 0 ? FMT_E_UNSUPPORTED : failed;
}

// The route as fmt_mt_run runs it: its register tiers with the checkpoint slab (small-tier strides) and,
// withLarge, the large pass with the views the route's booleans name (large strides, every document).
int cascade(const Call& c, const MtRoute& R, bool withLarge) {
  const size_t n = c.b->n_docs, SL = Slab<S>::kLeaves, SC = Slab<S>::kChars, SP = Slab<S>::kProps;
  const bool adj = R.large.adj;
  const EmuBatch eb = c.batch(R.large.loc);
  std::vector<uint32_t> ck(n * fmt_mt::Doc<false, fmt_mt::CompactTier>::kCkptWords), toLarge(n + 1);
  std::vector<fmt_mt_leaf> sl(withLarge ? n * SL : 0);
  std::vector<uint16_t> sc(withLarge ? n * SC : 0), smallLegacy(withLarge && adj ? n * SL : 0, 0xFFFFu);
  std::vector<fmt_mt_propset> sp(withLarge ? n * SP : 0);
  fmt_mt_leaf* tl = withLarge ? sl.data() : c.leaves;
  uint16_t* tc = withLarge ? sc.data() : c.chars;
  fmt_mt_propset* tp = withLarge ? sp.data() : c.props;
  uint16_t* legacy = legacyViews(c, adj, withLarge ? Slab<G>::kLeaves : SL);
  const MtDeviceOut tiers{c.headers, tl, tc, tp, c.catchup, c.rmOrder, R.tiersCkpt ? ck.data() : nullptr, nullptr, nullptr,
                          withLarge && adj ? smallLegacy.data() : legacy};
  int failed = FMT_OK;
  if (emu::runRoute(R, eb, tiers, toLarge.data(), &failed) < 0) return FMT_E_UNSUPPORTED;
  if (!withLarge) return failed;
  std::vector<uint8_t> up(n, 0);
  for (uint32_t i = 0; i < toLarge[0]; i++) up[toLarge[1 + i]] = 1;
  for (size_t d = 0; d < n; d++) {  // documents done below the large tier: results to the large strides
    const fmt_mt_doc_result& h = c.headers[d];
    if (up[d]) continue;
    std::memcpy(c.leaves + d * Slab<G>::kLeaves, tl + d * SL, h.n_leaves * sizeof(fmt_mt_leaf));
    std::memcpy(c.chars + d * Slab<G>::kChars, tc + d * SC, h.n_chars * sizeof(uint16_t));
    std::memcpy(c.props + d * Slab<G>::kProps, tp + d * SP, h.n_props * sizeof(fmt_mt_propset));
    if (adj) std::memcpy(legacy + d * Slab<G>::kLeaves, smallLegacy.data() + d * SL, h.n_leaves * sizeof(uint16_t));
  }
  const MtDeviceOut large{c.headers, c.leaves, c.chars, c.props, c.catchup, c.rmOrder, R.largeCkpt ? ck.data() : nullptr,
                          R.largeResumesSmall ? tl : nullptr, R.largeResumesSmall ? tc : nullptr, legacy};
  const emu::Launch pass{eb, large, toLarge.data(), true, nullptr, nullptr, false, &failed};
  return emu::replayStep(MtTier::kLarge, R.large, pass) < 0 ? FMT_E_UNSUPPORTED : failed;
}

}  // namespace

extern "C" {

// large = 0: the small tier (registers + LDS text); 1: the large tier (HBM text) that the runtime
// replays overflowing documents in; 2: the compact tier (4 register rows); 3: the register tiers of the
// batch's route with checkpoints (small-tier strides); 4: the whole route, register tiers and the large
// pass (large-tier strides).
int emu_mt_capacity(int large, uint32_t* leaves, uint32_t* chars, uint32_t* props) {
  if (large == 3) large = 0;
  if (large == 4) large = 1;
  if (large == 2) {
    *leaves = fmt_mt::Doc<false, fmt_mt::CompactTier>::kCapLeaves;
    *chars = fmt_mt::CompactTier::kCapChars;
    *props = fmt_mt::CompactTier::kPropCap;
  } else if (large) {
    *leaves = fmt_mt::Doc<false, fmt_mt::LargeTier>::kCapLeaves;
    *chars = fmt_mt::LargeTier::kCapChars;
    *props = fmt_mt::LargeTier::kPropCap;
  } else {
    *leaves = fmt_mt::Doc<false, fmt_mt::SmallTier>::kCapLeaves;
    *chars = fmt_mt::SmallTier::kCapChars;
    *props = fmt_mt::SmallTier::kPropCap;
  }
  return 0;
}

// Same strides as the GPU result buffers of the tier. The flags are the plan's (mt_plan.h; forceOb: the
// obliterate variants whatever the ops hold), the variants the route's (mt_route.h). 3 and 4 execute the route;
// 0, 1 and 2 are one tier of it alone over every document from its first op. An annotate-adjust batch's route
// is the small tier, then the large pass: 0 and 3 are its register tier, anything else the whole of it.
int emu_mt_replay(const fmt_mt_batch* b, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
                  fmt_mt_propset* props, fmt_mt_catchup_range* catchup, uint32_t capCatchup, int forceOb, int large,
                  fmt_mt_remove_order* rmOrder, uint32_t capRm) {
  prepareNumbers(b);
  g_legacyStride = 0;
  MtRoute R;
  if (const int rc = emu::planRouteOf(b, true, true, 0, -1, R, MtVariant{forceOb != 0, false, false, false})) return rc;
  const Call c{b, headers, leaves, chars, props, catchup, capCatchup, rmOrder, capRm};
  const MtVariant v = R.large;  // (the small tier's variant where it is a batch's first tier is the large pass's)
  if (v.adj ? large != 0 && large != 3 : large == 4) return cascade(c, R, true);
  if (v.adj || large == 3) return cascade(c, R, false);
  if (large == 1) return oneTier(c, MtTier::kLarge, v);
  if (large == 2 && !v.rm) return oneTier(c, MtTier::kCompact, MtVariant{v.ob, false, false, false});
  return oneTier(c, MtTier::kSmall, v);
}

// The large tier over every document from its first op, each document it is about to outgrow
// stopping with its large → huge checkpoint (hugeCk: fmt_ckpt::kWords words per document; header
// status fmt_ckpt::kStatusHuge) for emu_huge_resume (results at large strides), in the route's large
// variant. With FMT_MT_F_RMORDER ops rmOrder[n_docs x capRm] receives the entries, which keep their leaf
// ids in a stopped document; catchup[n_docs x capCatchup] or nullptr. Annotate-adjust batches: the legacy
// views via emu_mt_legacy_props, the PropertiesManager records and computed numbers via emu_mt_adj_slab.
int emu_mt_replay_large_ckpt(const fmt_mt_batch* b, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
                             fmt_mt_propset* props, fmt_mt_catchup_range* catchup, uint32_t capCatchup,
                             fmt_mt_remove_order* rmOrder, uint32_t capRm, uint32_t* hugeCk) {
  g_nums.clear();
  g_legacyStride = 0;
  MtRoute R;
  if (const int rc = emu::planRouteOf(b, true, true, 0, -1, R)) return rc;
  if (R.large.rm && rmOrder == nullptr) return FMT_E_DATA;
  if (R.large.adj) prepareNumbers(b);
  const Call c{b, headers, leaves, chars, props, catchup, capCatchup, R.large.rm ? rmOrder : nullptr, capRm, hugeCk};
  return oneTier(c, MtTier::kLarge, R.large);
}

uint32_t emu_huge_ckpt_words() { return fmt_ckpt::kWords; }

// f4 batches (local submissions, acks, rollbacks, reconnects): the local route and its large pass (results
// at large strides). largeOnly 0: FMT_LOCAL_PATH 1 (small, then large from the first op); 3: FMT_LOCAL_PATH 2,
// the compact tier first; 2: that route's first step alone (its statuses); 1: every document in the large tier.
// Annotate-adjust batches: the Adj local variants, with emu_mt_numbers and emu_mt_legacy_props.
int emu_mt_replay_local(const fmt_mt_batch* b, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
                        fmt_mt_propset* props, int largeOnly) {
  g_nums.clear();
  g_legacyStride = 0;
  prepareLocal(b->n_docs);
  if (b->adjusts != nullptr) prepareNumbers(b);
  MtRoute R;
  if (const int rc = emu::planRouteOf(b, true, true, 0, largeOnly >= 2 ? 2 : 1, R, MtVariant{false, false, false, true})) return rc;
  const Call c{b, headers, leaves, chars, props};
  if (largeOnly == 1) return oneTier(c, MtTier::kLarge, R.large);
  if (largeOnly == 2) R.nSteps = 1;
  return cascade(c, R, largeOnly != 2);
}

// Document d's regenerated ops (and their text) after the last emu_mt_replay_local: copies <= the
// caps, returns the op count; *nText = the text units.
int emu_mt_regen(uint32_t d, fmt_mt_op* ops, uint32_t capOps, uint16_t* text, uint32_t capText, uint32_t* nText) {
  if (2ull * d + 1 >= g_lregenCount.size()) return -1;
  const uint32_t n = g_lregenCount[2 * d], t = g_lregenCount[2 * d + 1];
  for (uint32_t k = 0; k < n && k < capOps; k++) ops[k] = g_lregen[static_cast<size_t>(d) * kEmuRegenCap + k];
  for (uint32_t k = 0; k < t && k < capText; k++) text[k] = g_lregenText[static_cast<size_t>(d) * kEmuRegenTextCap + k];
  *nText = t;
  return static_cast<int>(n);
}

// Document d's legacy prop sets (getAtSeq at minSeq, per leaf) after the last emu_mt_replay of a batch
// with adjusts: copies <= cap, returns the count (0 without adjusts).
int emu_mt_legacy_props(uint32_t d, uint16_t* out, uint32_t cap) {
  if (g_legacyStride == 0 || (d + 1) * g_legacyStride > g_legacy.size()) return 0;
  for (uint32_t k = 0; k < cap && k < g_legacyStride; k++) out[k] = g_legacy[d * g_legacyStride + k];
  return static_cast<int>(g_legacyStride);
}

// Document d's annotate-adjust slabs after the last emu_mt_replay_large_ckpt: its PropertiesManager
// records (capRecs x 4 words from the slab's start) and computed numbers (<= capNums, *nNums = count).
int emu_mt_adj_slab(uint32_t d, uint32_t* pm, uint32_t capRecs, double* nums, uint32_t capNums, uint32_t* nNums) {
  if (g_nums.empty() || d >= g_numCount.size()) return -1;
  for (size_t k = 0; k < 4ull * capRecs && k < 4ull * kEmuPmCap; k++) pm[k] = g_pm[static_cast<size_t>(d) * kEmuPmCap * 4 + k];
  const uint32_t n = g_numCount[d];
  for (uint32_t k = 0; k < n && k < capNums; k++) nums[k] = g_nums[static_cast<size_t>(d) * kEmuNumCap + k];
  *nNums = n;
  return 0;
}

// Document d's computed numbers after the last emu_mt_replay: returns their count, copies <= cap.
int emu_mt_numbers(uint32_t d, double* out, uint32_t cap) {
  if (d >= g_numCount.size()) return 0;
  const uint32_t n = g_numCount[d];
  for (uint32_t k = 0; k < n && k < cap; k++) out[k] = g_nums[static_cast<size_t>(d) * kEmuNumCap + k];
  return static_cast<int>(n);
}

}  // extern "C"

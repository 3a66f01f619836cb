// mt_emu_tiers.cpp — TEST INFRASTRUCTURE ONLY: the plain-batch tier cascade micro → compact → small →
// large under host emulation (csrc/mt_engine.h and the launch binding csrc/mt_bind.h compiled for the
// CPU, wave.h's host half). One call is one launch of mergeTreeKernel plus collectOverflowKernel
// (mergetree_kernel.h) over a document list or over every document, with the step-down switch of the
// launch and both lists it appends to exposed, so a test can walk the steps of the route (csrc/mt_route.h,
// exported by emu_mt_route) itself and look at — and scribble over — the checkpoint slots between two
// launches, as launchMergeTree (mergetree.hip) walks them.
// Plain batches only (no obliterates, remove-order recording, adjusts or local records); the two
// queries at the end answer for the Ob variants too.
#include "emu_route.h"
#include "../../fluidframework_amd/csrc/mt_route_words.h"

namespace {

using fmt_kernels::HandOff;
using fmt_kernels::MtDeviceOut;

// bindDoc's resume decision for a document whose header says `status`, with nothing behind the views
// but that header and one-entry slabs (the binding only forms addresses).
template <class Doc>
int resumes(bool overList, int status, bool ckptSlab, bool smallSlabs) {
  const uint64_t offs[2] = {0, 0};
  fmt_mt_doc_result hdr{};
  hdr.status = status;
  fmt_mt_leaf leaf{};
  uint16_t unit = 0;
  fmt_mt_propset set{};
  uint32_t slot = 0;
  fmt_kernels::MtDeviceBatch batch{};
  batch.docOpOffsets = offs;
  batch.nDocs = 1;
  const MtDeviceOut out{&hdr, &leaf, &unit, &set, nullptr, nullptr, ckptSlab ? &slot : nullptr,
                        smallSlabs ? &leaf : nullptr, smallSlabs ? &unit : nullptr, nullptr};
  return fmt_kernels::bindDoc<Doc>(batch, out, 0, 0, 1, 1, 1, overList).o.ckptResume ? 1 : 0;
}

template <bool Ob>
int resumesTier(int tier, bool overList, int status, bool ckptSlab, bool smallSlabs) {
  switch (tier) {
    case 0: return resumes<fmt_mt::Doc<Ob, fmt_mt::MicroTier>>(overList, status, ckptSlab, smallSlabs);
    case 1: return resumes<fmt_mt::Doc<Ob, fmt_mt::CompactTier>>(overList, status, ckptSlab, smallSlabs);
    case 2: return resumes<fmt_mt::Doc<Ob, fmt_mt::SmallTier>>(overList, status, ckptSlab, smallSlabs);
    case 3: return resumes<fmt_mt::Doc<Ob, fmt_mt::LargeTier>>(overList, status, ckptSlab, smallSlabs);
  }
  return -1;
}

}  // namespace

extern "C" {

uint32_t emu_micro_ckpt_words() { return fmt_mt::Doc<false, fmt_mt::CompactTier>::kCkptWords; }

// Checkpoint slot layout, for tests that poison what a saver did not write: head words, rows of the
// leaf area (5 fields × rows × 64 words, field-major), words of the text area, and where the
// live-obliterate table starts (to the end of the slot; plain batches never write it).
void emu_micro_ckpt_layout(uint32_t* head, uint32_t* rows, uint32_t* charWords, uint32_t* obOff) {
  using D = fmt_mt::Doc<false, fmt_mt::CompactTier>;
  *head = D::kCkptHead;
  *rows = D::kCkptRows;
  *charWords = D::kCkptCharWords;
  *obOff = D::kCkptObOff;
}

// (leaves, chars) a tier holds: 0 micro, 1 compact, 2 small, 3 large
int emu_micro_caps(int tier, uint32_t* leaves, uint32_t* chars) {
  switch (tier) {
    case 0: *leaves = 64 * fmt_mt::MicroTier::kRows; *chars = fmt_mt::MicroTier::kCapChars; return 0;
    case 1: *leaves = 64 * fmt_mt::CompactTier::kRows; *chars = fmt_mt::CompactTier::kCapChars; return 0;
    case 2: *leaves = 64 * fmt_mt::SmallTier::kRows; *chars = fmt_mt::SmallTier::kCapChars; return 0;
    case 3: *leaves = 64 * fmt_mt::LargeTier::kRows; *chars = fmt_mt::LargeTier::kCapChars; return 0;
  }
  return -1;
}

int emu_descend_rounds() { return fmt_plan::kDescendRounds; }

// { kCkptDescend, kDescendLeaves4, kDescendChars4, kDescendMinOps }
void emu_descend_consts(int32_t* out) {
  out[0] = fmt_mt::kCkptDescend;
  out[1] = fmt_mt::kDescendLeaves4;
  out[2] = fmt_mt::kDescendChars4;
  out[3] = fmt_mt::kDescendMinOps;
}

// One launch of tier 0..3 (micro, compact, small, large) over `list` (null: every document). descend:
// the launch's step-down switch. up / down: lists ([0] = n, then ids; capacity n_docs + 1) the launch
// appends the documents to that stopped for the tier above / below; either may be null. ckpt: one
// slot of Doc::kCkptWords words per document, or null (no checkpoints: a document that outgrows the
// tier reports FMT_E_CAPACITY). Returns the documents replayed, -1 for a bad tier.
int emu_tier_launch(const fmt_mt_batch* b, int tier, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
                    fmt_mt_propset* props, fmt_mt_catchup_range* catchup, uint32_t capCatchup, uint32_t* ckpt,
                    const uint32_t* list, int descend, uint32_t* up, uint32_t* down, const fmt_mt_leaf* smallLeaves,
                    const uint16_t* smallChars) {
  const EmuBatch eb(b, catchup != nullptr, capCatchup, false, 0);
  MtDeviceOut out{headers, leaves, chars, props, catchup, nullptr, ckpt, nullptr, nullptr, nullptr};
  out.descend = descend != 0;
  if (tier < 0 || tier > 3) return -1;
  if (tier == 3) {  // (the runtime's large launch of a plain batch: no register-tier slots, nothing steps down)
    out.ckpt = nullptr;
    out.smallLeaves = smallLeaves;
    out.smallChars = smallChars;
  }
  return emu::replayStep(static_cast<fmt_plan::MtTier>(tier), fmt_plan::MtVariant{},
                         emu::Launch{eb, out, list, list != nullptr, up, tier == 3 ? nullptr : down, false, nullptr});
}

// The route the runtime plans for `b` (csrc/mt_route.h planRoute over planMergeTreeLoad's plan) with or
// without the checkpoint and step-down slabs, as routeWords lays it out. rounds <= 0 / localPath < 0: the
// build's. Returns the words written (<= cap), -1 for a batch the plan refuses or a cap too small.
int emu_mt_route(const fmt_mt_batch* b, int ckptSlab, int descSlab, int rounds, int localPath, uint32_t* out, uint32_t cap) {
  fmt_plan::MtRoute route;
  if (emu::planRouteOf(b, ckptSlab != 0, descSlab != 0, rounds, localPath, route) != FMT_OK) return -1;
  const std::vector<uint32_t> w = fmt_plan::routeWords(route);
  if (w.size() > cap) return -1;
  std::memcpy(out, w.data(), w.size() * sizeof(uint32_t));
  return static_cast<int>(w.size());
}

// Whether bindDoc resumes a document whose header says `status` from the checkpoint the tier before
// left: tier 0..3, the Ob variant or not, a launch over a device list or over every document, with or
// without the checkpoint slab (out.ckpt) and the small tier's slabs (out.smallLeaves / smallChars).
int emu_bind_resumes(int tier, int ob, int overList, int status, int ckptSlab, int smallSlabs) {
  return ob ? resumesTier<true>(tier, overList != 0, status, ckptSlab != 0, smallSlabs != 0)
            : resumesTier<false>(tier, overList != 0, status, ckptSlab != 0, smallSlabs != 0);
}

// collectHeader on a header that says `status`: the hand-off (0 none, 1 up, 2 down), *reported = the
// status the header holds afterwards.
int emu_bind_collect(int status, int32_t* reported) {
  fmt_mt_doc_result hdr{};
  hdr.status = status;
  const HandOff to = fmt_kernels::collectHeader(hdr);
  *reported = hdr.status;
  return to == HandOff::kUp ? 1 : to == HandOff::kDown ? 2 : 0;
}

}  // extern "C"

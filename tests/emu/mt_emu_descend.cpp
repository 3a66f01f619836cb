// Host emulation of the plain-batch tier cascade with stepping down (csrc/mt_engine.h compiled for the
// CPU, wave.h's host half): one call replays one tier over a document list, as one launch of
// mergeTreeKernel plus collectOverflowKernel does (mergetree_kernel.h), with the step-down switch of
// the launch and both lists it appends to exposed, so a test can drive the rounds of launchMergeTree
// (mergetree.hip) itself and look at — and scribble over — the checkpoint slots between two launches.
#include <cstring>
#include <memory>
#include <new>

#include "../../fluidframework_amd/csrc/mt_engine.h"

namespace {

using S = fmt_mt::SmallTier;

// Tiers 0..2 (micro, compact, small) write results at the small tier's strides, like the runtime's
// slabs; tier 3 (large) at its own, reading the small tier's checkpoints from smallLeaves / smallChars.
// list: [0] = n, then document ids (an overflow or down list), or null: every document, none resumed.
template <class C>
int replayTier(const fmt_mt_batch* b, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
               fmt_mt_propset* props, fmt_mt_catchup_range* catchup, uint32_t capCatchup, uint32_t* ckpt,
               const uint32_t* list, bool descend, uint32_t* up, uint32_t* down, const fmt_mt_leaf* smallLeaves,
               const uint16_t* smallChars) {
  using Doc = fmt_mt::Doc<false, C>;
  constexpr size_t kLeafStride = C::kHbmChars ? Doc::kCapLeaves : 64 * S::kRows;
  constexpr size_t kCharStride = C::kHbmChars ? C::kCapChars : S::kCapChars;
  constexpr size_t kPropStride = C::kHbmChars ? C::kPropCap : S::kPropCap;
  auto scratch = std::make_unique<fmt_mt::Scratch<C>>();
  auto doc = std::make_unique<Doc>();
  const uint32_t count = list ? list[0] : b->n_docs;
  for (uint32_t i = 0; i < count; i++) {
    const uint32_t d = list ? list[1 + i] : i;
    const int before = headers[d].status;
    std::memset(scratch.get(), 0xCD, sizeof(fmt_mt::Scratch<C>));  // poison: state must be initialized
    fmt_mt::DocInputs in{};
    in.ops = b->ops;
    in.begin = b->doc_op_offsets[d];
    in.end = b->doc_op_offsets[d + 1];
    in.text = b->text;
    in.initOff = b->doc_init ? b->doc_init[2 * d] : 0u;
    in.initLen = b->doc_init ? b->doc_init[2 * d + 1] : 0u;
    in.propsOff = b->props_off;
    in.propsKv = b->props_kv;
    in.nPropsOps = b->n_props_ops;
    in.markerKey = b->marker_id_key;
    in.doc = d;
    fmt_mt::DocOutputs o{};
    o.header = headers + d;
    o.leaves = leaves + d * kLeafStride;
    o.chars = chars + d * kCharStride;
    o.props = props + d * kPropStride;
    o.catchup = catchup ? catchup + static_cast<size_t>(d) * capCatchup : nullptr;
    o.catchupCap = catchup ? capCatchup : 0u;
    o.ckpt = ckpt && (Doc::kSavesCkpt || Doc::kResumesCkpt) ? ckpt + static_cast<size_t>(d) * Doc::kCkptWords : nullptr;
    // as mergeTreeKernel: a tier that also saves resumes only documents of a list
    o.ckptResume = Doc::kResumesCkpt && (!Doc::kSavesCkpt || list != nullptr) && o.ckpt != nullptr &&
                   (before == fmt_mt::kCkptEscalate || before == fmt_mt::kCkptDescend);
    if constexpr (Doc::kDescends) o.descend = descend;
    if (Doc::kSavesBig && ckpt != nullptr) {
      o.bigCkpt = reinterpret_cast<uint32_t*>(o.leaves);
      o.bigCkptChars = o.chars;
    }
    if (Doc::kResumesBig && smallLeaves != nullptr) {
      o.bigCkpt = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(smallLeaves + static_cast<size_t>(d) * 64 * S::kRows));
      o.bigCkptChars = const_cast<uint16_t*>(smallChars + static_cast<size_t>(d) * S::kCapChars);
      o.ckptResume = before == fmt_mt::kCkptEscalate;
    }
    new (doc.get()) Doc();
    doc->s = scratch.get();
    doc->run(in, o);
    // as collectOverflowKernel
    const int st = headers[d].status;
    if (st == fmt_mt::kCapacityFinal) headers[d].status = FMT_E_CAPACITY;
    if (st == FMT_E_CAPACITY || st == fmt_mt::kCkptEscalate) {
      if (up != nullptr) up[1 + up[0]++] = d;
    } else if (down != nullptr && st == fmt_mt::kCkptDescend) {
      down[1 + down[0]++] = d;
    }
  }
  return static_cast<int>(count);
}

}  // namespace

extern "C" {

// { kCkptDescend, kDescendLeaves4, kDescendChars4, kDescendMinOps }
void emu_descend_consts(int32_t* out) {
  out[0] = fmt_mt::kCkptDescend;
  out[1] = fmt_mt::kDescendLeaves4;
  out[2] = fmt_mt::kDescendChars4;
  out[3] = fmt_mt::kDescendMinOps;
}

// One launch of tier 0..3 (micro, compact, small, large) over `list` (null: every document). descend:
// the launch's step-down switch. up / down: lists ([0] = n, then ids; capacity n_docs + 1) the launch
// appends the documents to that stopped for the tier above / below; down may be null. ckpt: one
// slot of Doc::kCkptWords words per document, or null. Returns the documents replayed, -1 for a bad tier.
int emu_descend_tier(const fmt_mt_batch* b, int tier, fmt_mt_doc_result* headers, fmt_mt_leaf* leaves, uint16_t* chars,
                     fmt_mt_propset* props, fmt_mt_catchup_range* catchup, uint32_t capCatchup, uint32_t* ckpt,
                     const uint32_t* list, int descend, uint32_t* up, uint32_t* down, const fmt_mt_leaf* smallLeaves,
                     const uint16_t* smallChars) {
  const bool desc = descend != 0;
  switch (tier) {
    case 0:
      return replayTier<fmt_mt::MicroTier>(b, headers, leaves, chars, props, catchup, capCatchup, ckpt, list, desc, up, down,
                                           nullptr, nullptr);
    case 1:
      return replayTier<fmt_mt::CompactTier>(b, headers, leaves, chars, props, catchup, capCatchup, ckpt, list, desc, up,
                                             down, nullptr, nullptr);
    case 2:
      return replayTier<S>(b, headers, leaves, chars, props, catchup, capCatchup, ckpt, list, desc, up, down, nullptr, nullptr);
    case 3:
      return replayTier<fmt_mt::LargeTier>(b, headers, leaves, chars, props, catchup, capCatchup, nullptr, list, false, up,
                                           nullptr, smallLeaves, smallChars);
  }
  return -1;
}

}  // extern "C"

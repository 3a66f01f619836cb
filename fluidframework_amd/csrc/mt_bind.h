// mt_bind.h — the launch binding of the merge-tree replay: what turns a batch plus a document id into
// the engine's fmt_mt::DocInputs / DocOutputs (which slab and stride the results go to, which
// checkpoint slot the document gets and whether it resumes from it, where the small tier's big
// checkpoint lives), and how a finished header is sorted into the up list or the down list. Compiled
// twice like the engine (wave.h): for gfx950 by mergeTreeKernel / collectOverflowKernel
// (mergetree_kernel.h), for the host by the emulations under tests/emu, so the CPU suites run the
// routing that ships. No HIP runtime in here.
#pragma once

#include "mt_engine.h"

// hipcc's host pass reads wave.h's host half, where FMT_DEV is a plain host function: a free function
// a kernel calls (collectHeader) must be a device function in that pass too (the engine's members are
// not checked).
#if defined(__HIP__) && !FMT_GPU
#define FMT_BIND __host__ __device__ inline
#else
#define FMT_BIND FMT_DEV
#endif

namespace fmt_kernels {

struct MtDeviceBatch {
  const fmt_mt_op* ops;
  const uint64_t* docOpOffsets;
  uint32_t nDocs;
  const uint16_t* text;
  const uint32_t* docInit;  // (offset, len) per doc or nullptr
  const uint32_t* propsOff;
  const uint32_t* propsKv;
  uint32_t nPropsOps;
  const uint64_t* catchupOffsets;  // per-doc catch-up slab offsets (nDocs + 1), or nullptr
  const fmt_mt_snapshot_doc* snapshots;  // per-doc summary loads, or nullptr
  const fmt_mt_snapshot_seg* snapshotSegs;
  const uint64_t* rmOrderOffsets;  // per-doc remove-order slab offsets (nDocs + 1), or nullptr
  const fmt_mt_snapshot_info* snapshotInfo;  // SnapshotV1 merge info per snapshot segment, or nullptr
  const fmt_mt_stamp* snapshotStamps;
  uint64_t nSnapshotInfo;
  const fmt_mt_relpos* relpos;     // relative positions (FMT_MT_F_REL1/REL2 ops), or nullptr
  uint32_t nRelpos;
  uint32_t markerKey;              // key id of "markerId", FMT_MT_NO_MARKER if none
  const fmt_mt::AdjustTables* adj;  // annotate-adjust tables (device memory), nullptr when none
  const fmt_mt::LocalTables* loc = nullptr;  // f4 local-client slabs (device memory), nullptr when none
};

struct MtDeviceOut {
  fmt_mt_doc_result* headers;  // nDocs
  fmt_mt_leaf* leaves;         // nDocs * capLeaves
  uint16_t* chars;             // nDocs * capChars
  fmt_mt_propset* props;       // nDocs * capProps
  fmt_mt_catchup_range* catchup;  // slabs at catchupOffsets, or nullptr
  fmt_mt_remove_order* rmOrder;   // slabs at rmOrderOffsets, or nullptr
  uint32_t* ckpt;                 // plain batches: per-document register-tier checkpoints (one slot each), or nullptr
  // large tier over a plain batch: the small tier's result slabs, where it left its checkpoints
  const fmt_mt_leaf* smallLeaves;
  const uint16_t* smallChars;
  // annotate-adjust batches: per leaf the prop set of getAtSeq(minSeq) (legacy summaries), at the
  // leaves slab's stride; nullptr otherwise
  uint16_t* legacyProps;
  // large tier over a plain batch: per large-tier slot, its large → huge checkpoint record
  // (huge_ckpt.h, fmt_ckpt::kWords words), or nullptr
  uint32_t* hugeCkpt = nullptr;
  // set by launchMergeTree for the rounds of a plain batch in which documents may step down a tier
  bool descend = false;
};

// Result slabs: the compact and small tiers share the small tier's per-document strides (a document
// the compact tier overflows replays again into the same slab); the large tier has its own.
template <class C>
struct Slab {
  static constexpr size_t kLeaves = C::kHbmChars ? 64 * C::kRows : 64 * fmt_mt::SmallTier::kRows;
  static constexpr size_t kChars = C::kHbmChars ? C::kCapChars : fmt_mt::SmallTier::kCapChars;
  static constexpr size_t kProps = C::kHbmChars ? C::kPropCap : fmt_mt::SmallTier::kPropCap;
};

template <class Doc>
struct DocVariant;
template <bool Ob_, class C_, bool Rm_, bool Adj_, bool Loc_>
struct DocVariant<fmt_mt::Doc<Ob_, C_, Rm_, Adj_, Loc_>> {
  static constexpr bool kOb = Ob_, kRm = Rm_, kLoc = Loc_;
};

// Document d's inputs (`in`) and outputs (`o`, both declared here) for one launch of the Doc variant.
// slot: the slab of out.leaves / chars / props / legacyProps / hugeCkpt it writes (headers,
// checkpoints, catch-up and remove-order slabs are per document), at the given strides (the kernel's:
// Slab<C>). overList: the launch runs over a list a previous launch built on the device.
// A macro, expanded in mergeTreeKernel's own scope and in bindDoc below: as a force-inlined function
// the same statements reach the optimizer in another form and four register-tier kernels spill up to
// 53 more SGPRs (profiles/bind/README.md); as kernel text they compile as before. For the same
// reason the wave-uniform status read is the builtin itself there, not wave.h's uni() around it.
#if FMT_GPU
#define FMT_MT_UNI(x) __builtin_amdgcn_readfirstlane(x)
#else
#define FMT_MT_UNI(x) (x)
#endif
#define FMT_MT_BIND_DOC(Doc, batch, out, d, slot, leafStride, charStride, propStride, overList, in, o)                              \
  fmt_mt::DocInputs in;                                                                                                             \
  fmt_mt::DocOutputs o;                                                                                                             \
  in.ops = batch.ops;                                                                                                               \
  in.begin = batch.docOpOffsets[d];                                                                                                 \
  in.end = batch.docOpOffsets[d + 1];                                                                                               \
  in.text = batch.text;                                                                                                             \
  in.initOff = batch.docInit ? batch.docInit[2 * d] : 0u;                                                                           \
  in.initLen = batch.docInit ? batch.docInit[2 * d + 1] : 0u;                                                                       \
  in.propsOff = batch.propsOff;                                                                                                     \
  in.propsKv = batch.propsKv;                                                                                                       \
  in.nPropsOps = batch.nPropsOps;                                                                                                   \
  in.relpos = batch.relpos;                                                                                                         \
  in.nRelpos = batch.relpos ? batch.nRelpos : 0u;                                                                                   \
  in.markerKey = batch.markerKey;                                                                                                   \
  in.adj = batch.adj;                                                                                                               \
  in.loc = DocVariant<Doc>::kLoc ? batch.loc : nullptr;                                                                             \
  in.doc = d;                                                                                                                       \
  in.infoAll = batch.snapshotInfo;                                                                                                  \
  in.stampsAll = batch.snapshotStamps;                                                                                              \
  in.nInfoAll = batch.snapshotInfo ? batch.nSnapshotInfo : 0u;                                                                      \
  if (batch.snapshots && batch.snapshots[d].loaded) {                                                                               \
    const fmt_mt_snapshot_doc sd = batch.snapshots[d];                                                                              \
    in.snapSegs = batch.snapshotSegs + sd.first_seg;                                                                                \
    in.snapInfo = batch.snapshotInfo ? batch.snapshotInfo + sd.first_seg : nullptr;                                                 \
    in.snapStamps = batch.snapshotStamps;                                                                                           \
    in.nHeader = sd.n_header;                                                                                                       \
    in.nBody = sd.n_body;                                                                                                           \
    in.snapMinSeq = sd.min_seq;                                                                                                     \
    in.snapSeq = sd.seq;                                                                                                            \
    in.loaded = 1;                                                                                                                  \
  } else {                                                                                                                          \
    in.snapSegs = nullptr;                                                                                                          \
    in.snapInfo = nullptr;                                                                                                          \
    in.snapStamps = nullptr;                                                                                                        \
    in.nHeader = in.nBody = 0;                                                                                                      \
    in.snapMinSeq = in.snapSeq = 0;                                                                                                 \
    in.loaded = 0;                                                                                                                  \
  }                                                                                                                                 \
  o.header = out.headers + d;                                                                                                       \
  o.leaves = out.leaves + slot * leafStride;                                                                                        \
  o.chars = out.chars + slot * charStride;                                                                                          \
  o.props = out.props + slot * propStride;                                                                                          \
  if (batch.catchupOffsets) {                                                                                                       \
    const uint64_t c0 = batch.catchupOffsets[d], c1 = batch.catchupOffsets[d + 1];                                                  \
    o.catchup = out.catchup + c0;                                                                                                   \
    o.catchupCap = static_cast<uint32_t>(c1 - c0);                                                                                  \
  } else {                                                                                                                          \
    o.catchup = nullptr;                                                                                                            \
    o.catchupCap = 0;                                                                                                               \
  }                                                                                                                                 \
  if (DocVariant<Doc>::kRm && batch.rmOrderOffsets) {                                                                               \
    const uint64_t r0 = batch.rmOrderOffsets[d], r1 = batch.rmOrderOffsets[d + 1];                                                  \
    o.rmOrder = out.rmOrder + r0;                                                                                                   \
    o.rmOrderCap = static_cast<uint32_t>(r1 - r0);                                                                                  \
  } else {                                                                                                                          \
    o.rmOrder = nullptr;                                                                                                            \
    o.rmOrderCap = 0;                                                                                                               \
  }                                                                                                                                 \
  if (Doc::kSavesCkpt || Doc::kResumesCkpt || (DocVariant<Doc>::kOb && Doc::kResumesBig)) {  /* (large tier: live obliterates) */   \
    o.ckpt = out.ckpt ? out.ckpt + static_cast<size_t>(d) * Doc::kCkptWords : nullptr;                                              \
/* (a tier that also saves — the compact one — resumes only over an overflow list: over every */                                    \
/* document it is the first tier, and the headers hold whatever an earlier run left) */                                             \
/* (kCkptDescend: the tier above left it, see launchMergeTree's rounds; the Ob variants never step down) */                         \
    const int st = FMT_MT_UNI(out.headers[d].status);                                                                                      \
    o.ckptResume = Doc::kResumesCkpt && (!Doc::kSavesCkpt || (overList)) && o.ckpt != nullptr &&                                    \
                   (st == fmt_mt::kCkptEscalate || (!DocVariant<Doc>::kOb && st == fmt_mt::kCkptDescend));                          \
    if constexpr (Doc::kDescends) o.descend = out.descend;                                                                          \
  } else {                                                                                                                          \
    o.ckpt = nullptr;                                                                                                               \
    o.ckptResume = false;                                                                                                           \
  }                                                                                                                                 \
  o.bigCkpt = nullptr;                                                                                                              \
  o.bigCkptChars = nullptr;                                                                                                         \
  o.legacyProps = out.legacyProps ? out.legacyProps + slot * leafStride : nullptr;                                                  \
  o.hugeCkpt = Doc::kSavesHuge && out.hugeCkpt != nullptr ? out.hugeCkpt + slot * static_cast<size_t>(fmt_ckpt::kWords) : nullptr;  \
  if constexpr (Doc::kSavesBig) {  /* batches without remove order (out.ckpt set): the small tier's own slabs */                    \
    if (out.ckpt != nullptr) {                                                                                                      \
      o.bigCkpt = reinterpret_cast<uint32_t*>(o.leaves);                                                                            \
      o.bigCkptChars = o.chars;                                                                                                     \
    }                                                                                                                               \
  }                                                                                                                                 \
  if constexpr (Doc::kResumesBig) {  /* the small tier's slabs are per document, at its strides */                                  \
    if (out.smallLeaves != nullptr) {                                                                                               \
      o.bigCkpt = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(out.smallLeaves + d * Slab<fmt_mt::SmallTier>::kLeaves)); \
      o.bigCkptChars = const_cast<uint16_t*>(out.smallChars + d * Slab<fmt_mt::SmallTier>::kChars);                                 \
      o.ckptResume = FMT_MT_UNI(out.headers[d].status) == fmt_mt::kCkptEscalate;                                                           \
    }                                                                                                                               \
  }

struct DocBinding {
  fmt_mt::DocInputs in;
  fmt_mt::DocOutputs o;
};

// The same binding as a function: what the host emulations under tests/emu call.
template <class Doc>
FMT_DEV DocBinding bindDoc(const MtDeviceBatch& batch, const MtDeviceOut& out, uint32_t d, size_t slot, size_t leafStride,
                           size_t charStride, size_t propStride, bool overList) {
  FMT_MT_BIND_DOC(Doc, batch, out, d, slot, leafStride, charStride, propStride, overList, in, o);
  return DocBinding{in, o};
}

// Where a launch hands a finished document on: the list for the tier above, the one for the tier below,
// or nowhere (done, or failed for good).
enum class HandOff { kNone, kUp, kDown };

// The collect rule. A tier could not hold the document (FMT_E_CAPACITY) or stopped it at a checkpoint
// (kCkptEscalate): up. It stopped for the tier below (kCkptDescend): down. A limit the large tier
// shares (kCapacityFinal) is reported as FMT_E_CAPACITY without a hand-off.
FMT_BIND HandOff collectHeader(fmt_mt_doc_result& h) {
  const int st = h.status;
  if (st == fmt_mt::kCapacityFinal) h.status = FMT_E_CAPACITY;
  if (st == FMT_E_CAPACITY || st == fmt_mt::kCkptEscalate) return HandOff::kUp;
  return st == fmt_mt::kCkptDescend ? HandOff::kDown : HandOff::kNone;
}

}  // namespace fmt_kernels

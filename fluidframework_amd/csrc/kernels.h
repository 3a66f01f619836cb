// kernels.h — host-side launchers of the gfx950 kernels (one .hip translation unit each).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "../../include/fmt_pos.h"
#include "../../include/fmt_runs.h"
#include "map_plan.h"
#include "mt_bind.h"
#include "mt_route.h"
#include "pos_plan.h"
#include "range_plan.h"
#include "runs_plan.h"
#include "text_plan.h"

namespace fmt_kernels {

// ---- SharedMap LWW (map_lww.hip)
size_t mapLwwLdsBytes(uint32_t keyBound);
// key pools beyond the LDS table take the HBM-table path, which needs 2 * key_bound u32 of scratch
// per document (nullptr otherwise)
bool mapLwwNeedsScratch(uint32_t keyBound);
size_t mapSparseLdsBytes();
hipError_t launchMapSparse(const fmt_map_op* ops, const uint64_t* offsets, uint32_t nDocs, uint32_t keyBound,
                           fmt_map_entry* out, uint32_t* counts, int* error, int numCUs, hipStream_t stream);
// The same kernel, its tracking instantiation: every document it refuses is also appended to
// overflow ([0] = count, zeroed by the caller; then the document ids, in no order).
hipError_t launchMapSparseTracked(const fmt_map_op* ops, const uint64_t* offsets, uint32_t nDocs, uint32_t keyBound,
                                  fmt_map_entry* out, uint32_t* counts, int* error, uint32_t* overflow, int numCUs,
                                  hipStream_t stream);
hipError_t launchMapSparsePack(const fmt_map_entry* in, const uint64_t* offsets, const uint32_t* counts,
                               const uint64_t* packedOff, uint32_t nDocs, fmt_map_entry* packed, hipStream_t stream);
// ---- SharedMap sparse path, HBM tier (map_sparse_large.hip; layout and sizes: map_plan.h)
struct MapLargeArgs {
  const fmt_map_op* ops;                 // the staged batch
  const fmt_plan::MapLargeDoc* docs;     // the overflowing documents
  const uint32_t* tileDoc;               // tile -> index into docs
  const uint32_t* tileFirst;             // tile -> first op within the document
  uint32_t* scratch;                     // MapLargePlan::words() words
  fmt_map_entry* out;                    // as launchMapSparse
  uint32_t* counts;
  int* error;
  uint64_t slots, tileCountAt, clearAt;  // MapLargePlan::slots / tileCountAt() / clearAt()
  uint32_t nDocs, nTiles, keyBound;
};
hipError_t launchMapLarge(const MapLargeArgs& a, int numCUs, hipStream_t stream, uint32_t* launches);
// ---- SharedMap local-client pending state (map_pending.hip)
size_t mapPendingScratchBytes(uint64_t nEvents);
hipError_t launchMapPending(const fmt_map_local_op* events, const uint64_t* evOffs, const fmt_map_entry* seqEntries,
                            const uint64_t* seqOffs, const uint32_t* seqCounts, uint32_t nDocs, void* scratch,
                            const uint64_t* outBase, fmt_map_entry* out, uint32_t* outCounts, int32_t* outStatus,
                            hipStream_t stream);
// ---- bulk SharedMap summaries of the sparse path (map_summary.hip; the host half: map_sum_plan.h)
struct MapSummaryArgs {
  const fmt_map_entry* entries;  // the replay's entries (birth order) at offsets[d], counts[d] each: only read
  const uint64_t* offsets;
  const uint32_t* counts;
  const uint32_t* keyRank;       // per key id: its array-index value, or 0xFFFFFFFF
  const uint32_t* valUnits;      // per value id: UTF-16 units of its JSON text
  fmt_map_entry* ordered;        // out, same layout: the entries in summary order
  uint32_t* tags;                // out, same layout: the blob each ordered entry lands in, 0xFFFFFFFF: the header
  uint32_t* nBlobs;              // out, per document
  uint32_t* list;                // nDocs + 1 words, [0] zeroed by the caller: the documents of more than 64 entries
  uint32_t nDocs, nKeys, nValues;
};
// Documents of more than 2048 live entries are copied unordered (tags 0xFFFFFFFF, nBlobs 0).
hipError_t launchMapSummary(const MapSummaryArgs& a, int numCUs, hipStream_t stream);
// packed (32-bit words; N = packedOff[nDocs]): [0, 3N) entries, [3N, 4N) tags, [4N, 4N + nDocs) blob counts
hipError_t launchMapSummaryPack(const fmt_map_entry* ordered, const uint32_t* tags, const uint32_t* nBlobs,
                                const uint64_t* offsets, const uint32_t* counts, const uint64_t* packedOff, uint32_t nDocs,
                                uint32_t* packed, hipStream_t stream);
hipError_t launchMapLww(const fmt_map_op* ops, const uint64_t* offsets, uint32_t nDocs, uint32_t keyBound,
                        fmt_map_slot* out, int* error, int numCUs, hipStream_t stream, uint32_t* scratch);

// ---- merge-tree replay (mergetree.hip)
// MtDeviceBatch / MtDeviceOut, the views a launch takes: mt_bind.h
// Bytes of one document's tier checkpoint (mt_engine.h Doc::kCkptWords).
size_t mergeTreeCheckpointBytes();

// Per-document capacities of the small (LDS-text) and large (HBM-text) engine tiers.
// Bulk legacy summaries (summary.hip): a document's result buffers, its runs and its output spans.
struct SumView {
  const fmt_mt_leaf* leaves;
  const uint16_t* chars;
  const fmt_mt_propset* props;
  const uint16_t* legacyProps;  // per leaf: the prop set the legacy summary reads, or nullptr (leaf.props)
  const uint32_t* cls;          // per prop set its match class as the engine interned it (huge documents,
                                // up to 65534 sets), or nullptr: the summary kernel derives it in LDS
  const uint64_t* rmHi;         // per leaf its remove clients 64..253 (3 words: 64..127, 128..191, 192..253;
                                // huge documents of batches with such clients), or nullptr: none
};
struct SumRun {
  uint32_t len;    // UTF-16 units of the merged segment
  uint16_t props;  // prop set id of its head leaf (0xffff: undefined)
  uint16_t flags;  // 1: a Marker (its one unit is the refType)
};
struct SumDocOut {
  unsigned long long run_off, text_off;
  uint32_t n_runs, n_units, status, pad;
};
hipError_t launchSummaryRuns(const fmt_mt_doc_result* hdrs, const SumView* views, uint32_t nDocs, SumRun* runs,
                             uint16_t* text, unsigned long long* cursors, SumDocOut* docOut, int numCUs,
                             hipStream_t stream);
// Bulk SnapshotV1 summaries (summary_v1.hip): one record per summary segment, a merged run of acked
// leaves or one leaf above minSeq with its merge info (snapshotV1.ts:170-276). 32 bytes.
constexpr uint16_t kV1Marker = 1;   // a Marker (its one unit is the refType)
constexpr uint16_t kV1Solo = 2;     // one leaf, written with merge info ({"json": ...})
constexpr uint16_t kV1Removed = 4;  // a solo leaf that is removed: rm_* hold its first remove stamp
struct SumV1Seg {
  uint32_t len;        // UTF-16 units
  uint16_t props;      // prop set id of its head leaf (0xffff: undefined)
  uint16_t flags;      // kV1*
  uint32_t leaf;       // solo: the leaf's index (its later stamps are the remove-order entries naming it)
  int32_t ins_seq;     // solo: the insert stamp
  int32_t ins_client;
  int32_t rm_client;   // kV1Removed: the first remove stamp, from the op whose seq is the leaf's rm_seq
  int32_t rm_seq;
  uint32_t rm_kind;    // FMT_MT_RM_SET / FMT_MT_RM_SLICE
};
// ops / opOffs: the batch's resident op records (the first remover of a leaf is looked up there).
// Segments, text and per-document spans as launchSummaryRuns writes them (SumDocOut.n_runs: segments).
hipError_t launchSummaryV1(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_mt_op* ops,
                           const uint64_t* opOffs, uint32_t nDocs, SumV1Seg* segs, uint16_t* text,
                           unsigned long long* cursors, SumDocOut* docOut, int numCUs, hipStream_t stream);
// Packing before a D2H copy (transfer.hip): span i's `words` dwords from src to dst + dstWord.
struct GatherSpan {
  const uint32_t* src;
  uint64_t dstWord;
  uint32_t words, pad;
};
hipError_t launchGatherSpans(const GatherSpan* spans, uint32_t n, uint32_t* dst, int numCUs, hipStream_t stream);
// Per-document content digest of the converged state (digest.hip).
hipError_t launchStateDigest(const fmt_mt_doc_result* hdrs, const SumView* views, uint32_t nDocs, uint64_t* out,
                             int numCUs, hipStream_t stream);

// Bulk getText (text.hip; work items and the host scan between the passes: text_plan.h). One wave per
// item. Pass 1 writes the units each item contributes; pass 2 copies them to packed + tileBase[item].
hipError_t launchTextTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                               uint32_t nItems, uint16_t placeholder, unsigned long long* tileUnits, int numCUs,
                               hipStream_t stream);
hipError_t launchTextGather(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                            uint32_t nItems, uint16_t placeholder, const unsigned long long* tileBase, uint16_t* packed,
                            int numCUs, hipStream_t stream);

// Bulk property runs (runs.hip; include/fmt_runs.h; the stitch between the passes: runs_plan.h). Work items
// as above. clsOff[nDocs + 1]: each document's span of clsBuf, n_props entries, none for a document that
// failed or carries SumView::cls. launchRunClasses fills clsBuf; launchRunTileReport writes one RunTile
// per item; launchRunEmit writes the runs, every index below nRuns.
hipError_t launchRunClasses(const fmt_mt_doc_result* hdrs, const SumView* views, uint32_t nDocs,
                            const unsigned long long* clsOff, uint16_t* clsBuf, int numCUs, hipStream_t stream);
hipError_t launchRunTileReport(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                               uint32_t nItems, const unsigned long long* clsOff, const uint16_t* clsBuf,
                               fmt_plan::RunTile* tiles, int numCUs, hipStream_t stream);
hipError_t launchRunEmit(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::TextItem* items,
                         uint32_t nItems, const unsigned long long* clsOff, const uint16_t* clsBuf,
                         const fmt_plan::RunTileBase* bases, uint64_t nRuns, fmt_mt_prop_run* runs, int numCUs,
                         hipStream_t stream);

// Bulk position queries (pos.hip; include/fmt_pos.h; views, tile lookup and the records decided on the host:
// pos_plan.h). One wave per item. launchPosTileUnits writes per (view, tile) item its units in the view and in
// the local view; launchPosResolve writes the hit of each of the nDev queries at its `out` index, every
// index below nQueries, and nothing for a query whose tile does not hold its position.
hipError_t launchPosTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::PosItem* items,
                              uint32_t nItems, fmt_plan::PosTileUnits* tileUnits, int numCUs, hipStream_t stream);
hipError_t launchPosResolve(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::PosDevQuery* queries,
                            uint64_t nDev, uint64_t nQueries, fmt_mt_pos_hit* out, int numCUs, hipStream_t stream);

// Bulk range reads (range.hip; include/fmt_range.h; views, items and offsets decided on the host: range_plan.h;
// the sizing pass over (view, tile) items is launchPosTileUnits). One wave per item. launchRangeTileUnits writes
// the text units of each item; launchRangeGather copies each item's units (a placeholder per Marker when
// there is one) to out + itemBase[item], every index below cap.
hipError_t launchRangeTileUnits(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::RangeItem* items,
                                uint32_t nItems, unsigned long long* itemUnits, int numCUs, hipStream_t stream);
hipError_t launchRangeGather(const fmt_mt_doc_result* hdrs, const SumView* views, const fmt_plan::RangeItem* items,
                             uint32_t nItems, uint16_t placeholder, const unsigned long long* itemBase, uint16_t* out,
                             uint64_t cap, int numCUs, hipStream_t stream);

struct MtCaps {
  uint32_t leaves, chars, props;
};
MtCaps mergeTreeCaps(bool large);

// The device lists and counters a route's steps name (mt_route.h MtList / MtDeal), built in one place
// (runtime.cpp). Every list holds count + 1 words, [0] = n, then ids. toLarge[0], microUp[0], compactUp[0], the
// four sched counters (compact, small, large, micro) and the whole of desc (mergeTreeDescendWords words) must
// be zero before launchMergeTree. docs / count: the caller's list (MtListKind::kCaller), or nullptr.
struct MtLists {
  uint32_t* toLarge = nullptr;
  uint32_t* microUp = nullptr;
  uint32_t* compactUp = nullptr;
  uint32_t* ordered = nullptr;
  uint32_t* sched = nullptr;
  uint32_t* desc = nullptr;  // nullptr: not allocated for this batch (the route then has one round)
  size_t descWords = 0;
  const uint32_t* docs = nullptr;
  uint32_t count = 0;
};
struct MtLaunchEnv {
  int numCUs;
  hipStream_t stream;
};

// The register tiers: walks route.steps (mt_route.h planRoute), one mergeTreeKernel launch plus one
// collectOverflowKernel launch a step, and one orderByRemainingKernel launch before a step whose list is
// reordered. Every list length stays on the device. The documents left for the large pass are in lists.toLarge.
hipError_t launchMergeTree(const MtDeviceBatch& batch, const MtDeviceOut& out, const fmt_plan::MtRoute& route,
                           const MtLists& lists, const MtLaunchEnv& env);

// The large pass (route.large) over the `count` documents of lists.toLarge, dealt from the large counter:
// out.leaves/chars/props are slabs indexed by list position.
hipError_t launchMergeTreeLarge(const MtDeviceBatch& batch, const MtDeviceOut& out, const fmt_plan::MtRoute& route,
                                const MtLists& lists, uint32_t count, const MtLaunchEnv& env);

// Diagnostic: per-phase cycle totals of a FMT_PROFILE=1 build (all zero otherwise).
int mergeTreeProfile(uint64_t* out, int n, bool reset);

}  // namespace fmt_kernels

// ---- huge documents (hugedoc.hip, huge_engine.h): one wave per document, state in HBM
namespace fmt_huge {
struct HugeState;
struct HugeInputs;
}  // namespace fmt_huge

namespace fmt_kernels {

struct HugeOut {
  fmt_mt_doc_result* header;
  fmt_mt_leaf* leaves;
  uint64_t capLeaves;
  uint16_t* chars;
  uint64_t capChars;
  fmt_mt_propset* props;
  uint16_t* legacy;          // annotate-adjust batches: per leaf the getAtSeq(minSeq) prop set, else nullptr
  const uint32_t* cls;       // the engine's match class per prop set (HugeState::pClass)
  unsigned long long* prof;  // [24] shader-clock totals per phase (huge_engine.h HugeDoc::prof)
  uint64_t* leavesHi;        // per leaf its remove clients 64..253 (3 words, bit (c - 64) % 64 of word (c - 64) / 64;
                             // fmt_mt_fetch_rm_clients_hi / _hi2), or nullptr
};
size_t hugeLdsBytes();
hipError_t launchHugeDocs(const fmt_huge::HugeState* states, const fmt_huge::HugeInputs* inputs, const HugeOut* outs,
                          uint32_t count, bool adjust, bool rmOrder, hipStream_t stream);

}  // namespace fmt_kernels

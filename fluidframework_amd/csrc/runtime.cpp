// runtime.cpp — the C ABI of include/fmt.h over HIP (host side of libfmt.so).
//
// Owns the device, the stream, device buffers and HIP events. Inputs cross host→HBM once per batch
// in fmt_*_load (the only PCIe traffic); fmt_*_run only launches kernels on resident data, so a
// caller can time run() alone ("inputs already resident in HBM"). No exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/fmt.h"
#include "../../include/fmt_map_summary.h"
#include "../../include/fmt_map_tiered.h"
#include "../../include/fmt_pos.h"
#include "../../include/fmt_range.h"
#include "../../include/fmt_runs.h"
#include "../../include/fmt_text.h"
#include "../../include/fmt_v1.h"
#include "huge_engine.h"
#include "jsnum.h"
#include "mt_engine.h"  // fmt_mt::AdjustTables
#include "mt_plan.h"
#include "mt_route_words.h"
#include "map_sum_plan.h"
#include "kernels.h"

namespace {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  hipError_t reserve(size_t n) {
    if (n <= cap && p != nullptr) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t bytes = (n > 0 ? n : 1) * sizeof(T);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Large host <-> device copies through pinned staging. The caller's arrays are pageable (numpy, JS
// ArrayBuffers), which the DMA engines reach only through the runtime's own small bounce buffer
// (measured: 4.3 GB/s H2D for T1's 7.3 GB, 0.18 GB/s for the catch-up fetch). Here kStageWorkers
// host threads each own two pinned chunks and a stream, and move every kStageWorkers-th chunk of
// the copy: one chunk's host memcpy overlaps the DMA of the chunk before it.
constexpr size_t kStageChunk = 8u << 20;
constexpr int kStageWorkers = 8;
constexpr size_t kStageMin = 16u << 20;  // smaller copies go straight through hipMemcpy

// Pinned host memory the ctx keeps across calls (hipHostMalloc'd, grown on demand): DMA lands in it
// directly, no staging copy.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    void* q = nullptr;
    const hipError_t e = hipHostMalloc(&q, (n ? n : 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q);
    cap = n;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  ~PinnedBuf() { release(); }
};

struct Stager {
  bool ready = false;
  void* buf[kStageWorkers][2] = {};
  hipStream_t st[kStageWorkers] = {};
  hipEvent_t ev[kStageWorkers][2] = {};
  void release() {
    for (int w = 0; w < kStageWorkers; w++) {
      for (int k = 0; k < 2; k++) {
        if (buf[w][k]) (void)hipHostFree(buf[w][k]);
        if (ev[w][k]) (void)hipEventDestroy(ev[w][k]);
        buf[w][k] = nullptr;
        ev[w][k] = nullptr;
      }
      if (st[w]) (void)hipStreamDestroy(st[w]);
      st[w] = nullptr;
    }
    ready = false;
  }
};

}  // namespace

struct fmt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool ownStream = false;
  int numCUs = 256;
  std::string arch;
  std::string err;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the run's (first) launch
  hipEvent_t ev2 = nullptr, ev3 = nullptr;  // around a second launch (large-tier replay), if any
  hipEvent_t evS0 = nullptr, evS1 = nullptr;  // around the bulk summary kernel (fmt_mt_summarize_legacy)
  bool timed = false, timed2 = false;
  fmt_stats stats{};

  // SharedMap
  DevBuf<fmt_map_op> mapOps;
  DevBuf<uint64_t> mapOffs;
  DevBuf<fmt_map_slot> mapOut;
  DevBuf<uint32_t> mapScratch;  // kill / first tables of the HBM-table path (large key pools)
  DevBuf<int> errWord;
  uint64_t mapNOps = 0;
  uint32_t mapDocs = 0, mapKeyBound = 0;
  bool mapLoaded = false;
  bool mapRan = false;     // fmt_map_run was issued for the loaded (dense) batch
  bool mapErrValid = false;  // errWord holds the word of a map run (staged, sparse or fmt_map_replay_device)
  // SharedMap, sparse path: entries at each document's op offset, live counts, packed copy
  DevBuf<fmt_map_entry> mapEntries, mapPacked;
  DevBuf<uint32_t> mapCounts;
  DevBuf<uint64_t> mapPackedOff;
  bool mapSparse = false;
  bool mapSparseRan = false;
  std::vector<uint64_t> mapOffsHost;  // the staged batch's doc_op_offsets
  // sparse path, HBM tier (fmt_map_run_sparse_tiered): the LDS tier's overflow list ([0] = count),
  // the plan of the last run that had one (map_plan.h) and its device copies, the tables
  DevBuf<uint32_t> mapOvf, mapLgTiles, mapLgScratch;
  DevBuf<fmt_plan::MapLargeDoc> mapLgDocs;
  fmt_plan::MapLargePlan mapLgPlan;
  // SharedMap local-client pending state (fmt_map_pending_run): events, per-event scratch, the
  // optimistic entries at mapPendBase[d] = op offset + event offset of the document
  DevBuf<fmt_map_local_op> mapEv;
  DevBuf<uint64_t> mapEvOffs, mapPendBase;
  DevBuf<uint8_t> mapPendScratch;
  DevBuf<fmt_map_entry> mapPendOut;
  DevBuf<uint32_t> mapPendCounts;
  DevBuf<int32_t> mapPendStatus;
  bool mapPendRan = false;
  // bulk summaries of the sparse path (fmt_map_summarize, map_summary.hip): the tiered run completed
  // (no document is left refused), the ordered entries and tags in the entries' layout, per-document
  // blob counts, the list of documents past one wave, the tables, the packed host copy, the blobs
  bool mapTieredDone = false;
  bool mapSumHostOnly = false;  // fmt_internal_map_summary_host_only: every document ordered on the host
  DevBuf<fmt_map_entry> mapSumEntries;
  DevBuf<uint32_t> mapSumTags, mapSumNBlobs, mapSumList, mapSumKeyRank, mapSumValUnits, mapSumPacked;
  PinnedBuf<uint32_t> mapSumHost;
  fmt_plan::MapSumBlobs mapSumBlobs;
  std::vector<int32_t> mapSumStatus;
  bool mapSumDone = false;
  uint64_t mapSumN = 0;  // live entries of the last summary

  // merge-tree
  DevBuf<fmt_mt_op> mtOps;
  DevBuf<uint64_t> mtOffs;
  DevBuf<uint16_t> mtText;
  DevBuf<uint32_t> mtInit, mtPropsOff, mtPropsKv;
  DevBuf<fmt_mt_doc_result> mtHdr;
  DevBuf<fmt_mt_leaf> mtLeaves;
  DevBuf<uint16_t> mtChars;
  DevBuf<fmt_mt_propset> mtProps;
  // the device lists and dealing counters a route's steps name (kernels.h MtLists), and what they point into:
  // mtListBuf (the four per-tier counters, then four lists of n_docs + 1 words) and mtDesc (the step-down rounds)
  fmt_kernels::MtLists mtLists;
  DevBuf<uint32_t> mtListBuf, mtDesc;
  DevBuf<uint32_t> mtCkpt;                   // per-document compact → small tier checkpoints
  DevBuf<uint32_t> mtHugeCk;                 // per large-tier slot: its large → huge checkpoint record (huge_ckpt.h)
  bool mtCkptOk = false;                     // allocated for this batch (else tiers replay overflow from op 0)
  fmt_plan::MtRoute mtRoute;                 // how this batch goes through the tiers (planned at load)
  DevBuf<fmt_mt_leaf> mtBigLeaves;           // large-tier result slabs, one per escalated doc
  DevBuf<uint16_t> mtBigChars;
  DevBuf<fmt_mt_propset> mtBigProps;
  std::vector<int32_t> mtBigSlot;            // doc -> large-tier slab, or -1
  DevBuf<fmt_mt_snapshot_doc> mtSnap;       // per-doc summary loads (f3)
  DevBuf<fmt_mt_snapshot_seg> mtSnapSegs;
  DevBuf<fmt_mt_relpos> mtRelpos;            // relative positions (FMT_MT_F_REL1/REL2 ops)
  DevBuf<fmt_mt_snapshot_info> mtSnapInfo;   // SnapshotV1 merge info of loaded segments
  DevBuf<fmt_mt_stamp> mtSnapStamps;
  bool mtHasSnapInfo = false;
  uint64_t mtNSnapSegs = 0;
  uint32_t mtNRelpos = 0, mtMarkerKey = FMT_MT_NO_MARKER;
  bool mtHasSnap = false;
  // what the loaded batch decided on the host (mt_plan.h): scan totals and flags, slab offsets, sorted
  // numbers, the per-document facts of the huge tier. Replaced only by a batch that passes validation.
  fmt_plan::MtPlan mtPlan;
  DevBuf<uint64_t> mtCuOffs;                 // per-doc catch-up slab offsets (n_docs + 1)
  DevBuf<fmt_mt_catchup_range> mtCatchup;    // catch-up range slabs
  DevBuf<uint64_t> mtRmOffs;                 // per-doc remove-order slab offsets (n_docs + 1)
  DevBuf<fmt_mt_remove_order> mtRmOrder;     // remove-order slabs (FMT_MT_F_RMORDER ops)
  // huge documents (T3, huge_engine.h): one wave each, state in per-document HBM buffers
  struct HugeDocBufs {
    std::vector<void*> allocs;
    fmt_huge::HugeState state{};
    fmt_huge::HugeInputs in{};
    fmt_kernels::HugeOut out{};
    std::vector<uint32_t> shape;             // host copy of in.shape (kept until the load completes)
  };
  std::vector<HugeDocBufs> huge;             // per huge document
  std::vector<int32_t> mtHugeSlot;           // doc -> index in huge, or -1
  // (documents that outgrow the large tier replay again in the huge tier, which holds every feature
  // but local-client records; mtPlan keeps their starts)
  uint32_t mtHugeLoaded = 0;                 // huge documents routed at load (the rest were escalated)
  // documents refused at load (a feature the huge tier lacks, or no device memory for its state):
  // their headers are written at load and no tier runs them; the rest of the batch is unaffected
  std::vector<uint32_t> mtRefused;
  std::vector<fmt_mt_doc_result> mtRefusedHdr;  // their headers, parallel (fmt_mt_fetch_headers before a run)
  bool mtUseList = false;                    // the small tiers run mtSmallList (huge or refused docs)
  uint32_t mtGrown = 0;                      // documents the last run escalated into the huge tier
  std::vector<uint64_t> mtOffsHost;          // host copies of doc_op_offsets and the snapshot docs
  std::vector<fmt_mt_snapshot_doc> mtSnapHost;
  DevBuf<fmt_mt_snapshot_seg> mtStartSegDev;
  DevBuf<fmt_huge::HugeState> hugeStates2;     // descriptors of the documents a run escalated (uploadHuge)
  DevBuf<fmt_huge::HugeInputs> hugeInputs2;
  DevBuf<fmt_kernels::HugeOut> hugeOuts2;
  // The read frame: what every bulk read of a run's results starts from. readFrame builds
  // it for the first read after a run, invalidateReads (fmt_mt_load, fmt_mt_run) makes it stale. The headers
  // and every document's views (docView) on the host, which the asynchronous copies read, the views in
  // sumViews, and, from the first reader that walks tiles on (frameTiles), the tile plan at kTextTileLeaves
  // with its items in tileItems.
  struct ReadFrame {
    bool current = false, tiled = false;
    std::vector<fmt_mt_doc_result> hdr;
    std::vector<fmt_kernels::SumView> views;
    fmt_plan::TextPlan tiles;
  } frame;
  DevBuf<fmt_kernels::SumView> sumViews;
  DevBuf<fmt_plan::TextItem> tileItems;
  // bulk legacy summaries (fmt_mt_summarize_legacy): device runs / text, host blobs
  DevBuf<fmt_kernels::SumRun> sumRuns;
  DevBuf<uint16_t> sumText;
  DevBuf<unsigned long long> sumCursors;
  DevBuf<fmt_kernels::SumDocOut> sumDocs;
  DevBuf<uint64_t> digests;                   // fmt_mt_state_digest output
  Stager stage;                               // pinned staging of large host <-> device copies
  DevBuf<fmt_kernels::GatherSpan> spans;      // packing before a D2H copy
  DevBuf<uint32_t> packed;
  std::vector<std::string> sumBlobs;          // per document: header, then body
  std::vector<uint32_t> sumSplit;             // per document: header length in sumBlobs[d]
  std::vector<int32_t> sumStatus;
  PinnedBuf<fmt_kernels::SumDocOut> sumHostDocs;  // host copies of the device runs / text / prop sets
  PinnedBuf<fmt_kernels::SumRun> sumHostRuns;
  PinnedBuf<uint16_t> sumHostText;
  PinnedBuf<fmt_mt_propset> sumHostProps;
  // annotate-adjust: rows, numbers of host value ids, host numbers sorted for number → id lookups,
  // per-document computed-number slabs and their counts
  DevBuf<fmt_mt_adjust> mtAdjusts;
  DevBuf<double> mtValueNum, mtNumSorted, mtNums;
  DevBuf<uint32_t> mtNumSortedId, mtNumCount;
  DevBuf<uint32_t> mtValueBase, mtNumSortedOffs;  // document-local value ids (doc_value_base)
  std::vector<uint32_t> mtValueBaseHost;         // empty: batch-global value ids
  DevBuf<uint64_t> mtNumOffs;
  DevBuf<fmt_mt::AdjustTables> mtAdjTab;      // the pointers above, for the kernels
  DevBuf<uint32_t> mtPm;                      // PropertiesManager records (4 words each) per document
  DevBuf<uint64_t> mtPmOffs;
  DevBuf<uint16_t> mtLegacy, mtBigLegacy;     // per leaf: the getAtSeq(minSeq) prop set (small / large slabs)
  DevBuf<uint32_t> mtSmallList;              // the other documents (small tier), when huge ones exist
  // f4 (local-client records): every document replays in the compact tier's Loc variant first, the ones
  // it cannot hold in the small tier's, then the large tier's (round 6; mergetree_local.hip); its pending
  // groups, group records, PropertiesManager records, regenerated ops / text and normalization
  // scratch live in per-document slabs (mt_engine.h LocalTables)
  DevBuf<uint32_t> mtLocGroups, mtLocRecs, mtLocPm, mtLocScratch, mtLocRegenCount;
  DevBuf<uint64_t> mtLocOffs;                // 6 offset arrays of n + 1: groups, recs, pm, regen, text, scratch
  DevBuf<fmt_mt_op> mtLocRegen;
  DevBuf<uint16_t> mtLocRegenText;
  DevBuf<fmt_mt::LocalTables> mtLocTab;
  uint32_t mtNSmall = 0;
  DevBuf<fmt_huge::HugeState> hugeStates;
  DevBuf<fmt_huge::HugeInputs> hugeInputs;
  DevBuf<fmt_kernels::HugeOut> hugeOuts;
  uint64_t mtNOps = 0, mtTextLen = 0;
  uint32_t mtDocs = 0, mtNProps = 0;
  bool mtHasInit = false, mtLoaded = false;
  bool mtRan = false;                         // fmt_mt_run completed for the loaded batch
  // bulk SnapshotV1 summaries (fmt_mt_summarize_v1): the kernel's segments, the remove-order entries,
  // host blobs (the text, spans and prop sets go through the legacy path's transient buffers)
  DevBuf<fmt_kernels::SumV1Seg> v1Segs;
  PinnedBuf<fmt_kernels::SumV1Seg> v1HostSegs;
  PinnedBuf<fmt_mt_remove_order> v1HostRm;
  std::vector<std::string> v1Blobs;           // per document: header, then body_0, body_1, ...
  std::vector<std::vector<uint64_t>> v1Ends;  // per document: where each of those blobs ends in v1Blobs[d]
  std::vector<int32_t> v1Status;
  // bulk getText (fmt_mt_fetch_text_all, text.hip): per work item of the frame's tiles its units and its
  // base in the packed text, the packed text. Its own buffers: no other read sees them.
  std::vector<uint64_t> textOffs;               // the offsets of the cached pass 1 (n_docs + 1)
  DevBuf<unsigned long long> textUnits, textBases;
  DevBuf<uint16_t> textPacked;
  PinnedBuf<uint64_t> textHostUnits, textHostBases;
  bool textSized = false;                       // pass 1 and the scan hold for textPlaceholder since the last run
  uint16_t textPlaceholder = 0;
  // bulk property runs (fmt_mt_fetch_prop_runs_all, runs.hip): each document's span of match classes, per work
  // item of the frame's tiles pass 1's report and the stitch's bases (runs_plan.h), the packed runs.
  std::vector<uint64_t> runsOffs;               // the offsets of the cached sizing pass (n_docs + 1)
  std::vector<uint64_t> runsClsOffs;            // n_docs + 1
  DevBuf<unsigned long long> runsClsOff;
  DevBuf<uint16_t> runsCls;
  DevBuf<fmt_plan::RunTile> runsTiles;
  DevBuf<fmt_plan::RunTileBase> runsBases;
  DevBuf<fmt_mt_prop_run> runsPacked;
  PinnedBuf<fmt_plan::RunTile> runsHostTiles;
  PinnedBuf<fmt_plan::RunTileBase> runsHostBases;
  bool runsSized = false;                       // classes, pass 1 and the stitch hold since the last run
  // bulk position queries (fmt_mt_query_positions, pos.hip): the plan of the call over the frame's tiles
  // (pos_plan.h), its items, the units per item, the queries that go to the device, the records. Its own
  // buffers and nothing cached between calls: no other read sees them.
  fmt_plan::PosPlan posPlan;
  DevBuf<fmt_plan::PosItem> posItems;
  DevBuf<fmt_plan::PosTileUnits> posUnits;
  DevBuf<fmt_plan::PosDevQuery> posQueries;
  DevBuf<fmt_mt_pos_hit> posHits;
  PinnedBuf<fmt_plan::PosTileUnits> posHostUnits;
  // bulk range reads (fmt_mt_fetch_text_ranges, range.hip): the plan of the call over the frame's tiles
  // (range_plan.h), the (view, tile) sizing items and their units, the range items with their text units and
  // bases, the packed text. Its own buffers and nothing cached between calls: no other read sees them.
  fmt_plan::RangePlan rngPlan;
  DevBuf<fmt_plan::PosItem> rngViewItems;
  DevBuf<fmt_plan::PosTileUnits> rngViewUnits;
  PinnedBuf<fmt_plan::PosTileUnits> rngHostViewUnits;
  DevBuf<fmt_plan::RangeItem> rngItems;
  DevBuf<unsigned long long> rngUnits, rngBases;
  PinnedBuf<uint64_t> rngHostUnits;
  DevBuf<uint16_t> rngPacked;
};

namespace {

int setErr(fmt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

// Call order (fmt.h): what a fetch, digest or summary reads is written by fmt_mt_run. After a load and
// before a run the result buffers hold an earlier batch, or nothing; the call is refused on the host.
int mtNeedsRun(fmt_ctx* c, const char* what) {
  return setErr(c, FMT_E_USAGE, std::string(what) + " before fmt_mt_run: no run has completed since the last fmt_mt_load");
}

int hipErr(fmt_ctx* c, hipError_t e, const char* what) {
  return setErr(c, FMT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define FMT_HIP(ctx, expr)                                 \
  do {                                                     \
    hipError_t e_ = (expr);                                \
    if (e_ != hipSuccess) return hipErr((ctx), e_, #expr); \
  } while (0)

hipError_t stageInit(fmt_ctx* c) {
  Stager& S = c->stage;
  if (S.ready) return hipSuccess;
  for (int w = 0; w < kStageWorkers; w++) {
    for (int k = 0; k < 2; k++) {
      hipError_t e = hipHostMalloc(&S.buf[w][k], kStageChunk, hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&S.ev[w][k], hipEventDisableTiming);
      if (e != hipSuccess) {
        S.release();
        return e;
      }
    }
    const hipError_t e = hipStreamCreateWithFlags(&S.st[w], hipStreamNonBlocking);
    if (e != hipSuccess) {
      S.release();
      return e;
    }
  }
  S.ready = true;
  return hipSuccess;
}

// Copies `bytes` between pageable host memory and the device, synchronously with respect to the
// ctx stream (it waits for the work already queued there first). toDevice: dst is device memory.
hipError_t stagedCopy(fmt_ctx* c, void* dst, const void* src, size_t bytes, bool toDevice) {
  if (bytes == 0) return hipSuccess;
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return e;
  if (bytes < kStageMin || stageInit(c) != hipSuccess)  // (no pinned memory: the runtime's own path)
    return hipMemcpy(dst, src, bytes, toDevice ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
  const size_t nChunks = (bytes + kStageChunk - 1) / kStageChunk;
  const int workers = static_cast<int>(std::min<size_t>(kStageWorkers, nChunks));
  std::vector<hipError_t> errs(workers, hipSuccess);
  std::vector<std::thread> pool;
  for (int w = 0; w < workers; w++)
    pool.emplace_back([&, w] {
      Stager& S = c->stage;
      hipError_t err = hipSetDevice(c->device);
      auto span = [&](size_t k) { return std::min(kStageChunk, bytes - k * kStageChunk); };
      if (toDevice) {
        int slot = 0;
        for (size_t k = w; k < nChunks && err == hipSuccess; k += workers, slot ^= 1) {
          err = hipEventSynchronize(S.ev[w][slot]);  // the DMA that last read this chunk is done
          if (err != hipSuccess) break;
          std::memcpy(S.buf[w][slot], static_cast<const char*>(src) + k * kStageChunk, span(k));
          err = hipMemcpyAsync(static_cast<char*>(dst) + k * kStageChunk, S.buf[w][slot], span(k), hipMemcpyHostToDevice,
                               S.st[w]);
          if (err == hipSuccess) err = hipEventRecord(S.ev[w][slot], S.st[w]);
        }
      } else {
        // two chunks in flight: issue both, then drain one and refill it while the other lands
        auto issue = [&](size_t k, int slot) {
          hipError_t r = hipMemcpyAsync(S.buf[w][slot], static_cast<const char*>(src) + k * kStageChunk, span(k),
                                        hipMemcpyDeviceToHost, S.st[w]);
          return r == hipSuccess ? hipEventRecord(S.ev[w][slot], S.st[w]) : r;
        };
        size_t k0 = w, k1 = w + workers;
        if (k0 < nChunks) err = issue(k0, 0);
        if (err == hipSuccess && k1 < nChunks) err = issue(k1, 1);
        int slot = 0;
        for (size_t k = k0; k < nChunks && err == hipSuccess; k += workers, slot ^= 1) {
          err = hipEventSynchronize(S.ev[w][slot]);
          if (err != hipSuccess) break;
          std::memcpy(static_cast<char*>(dst) + k * kStageChunk, S.buf[w][slot], span(k));
          if (k + 2 * workers < nChunks) err = issue(k + 2 * workers, slot);
        }
      }
      const hipError_t e2 = hipStreamSynchronize(S.st[w]);
      errs[w] = err != hipSuccess ? err : e2;
    });
  for (auto& t : pool) t.join();
  for (hipError_t x : errs)
    if (x != hipSuccess) return x;
  return hipSuccess;
}

// ---- reads of a merge-tree run's results

// The entry of every such read. `bad`, the function's own message: a null ctx, nothing loaded, or argsOk false
// (the caller's own arguments, which may look into c only behind `c &&`). Not run since the load: mtNeedsRun
// under the name `what`, or `bad` again when what is null. Then the device is made current.
int mtReadEntry(fmt_ctx* c, bool argsOk, const char* what, const std::string& bad) {
  if (c == nullptr || !c->mtLoaded || !argsOk) return setErr(c, FMT_E_USAGE, bad);
  if (!c->mtRan) return what != nullptr ? mtNeedsRun(c, what) : setErr(c, FMT_E_USAGE, bad);
  FMT_HIP(c, hipSetDevice(c->device));
  return FMT_OK;
}

// Where document d's converged state lives: the small tier's slabs, a large-tier slab, or a huge
// document's own buffers.
fmt_kernels::SumView docView(const fmt_ctx* c, uint32_t d) {
  const int32_t hs = d < c->mtHugeSlot.size() ? c->mtHugeSlot[d] : -1;
  if (hs >= 0) {
    const fmt_kernels::HugeOut& O = c->huge[static_cast<size_t>(hs)].out;
    return {O.leaves, O.chars, O.props, c->mtPlan.anyAdjust ? O.legacy : nullptr, O.cls, O.leavesHi};
  }
  const int32_t slot = d < c->mtBigSlot.size() ? c->mtBigSlot[d] : -1;
  const fmt_kernels::MtCaps caps = fmt_kernels::mergeTreeCaps(slot >= 0);
  const size_t at = slot >= 0 ? static_cast<size_t>(slot) : d;
  return {(slot >= 0 ? c->mtBigLeaves.p : c->mtLeaves.p) + at * caps.leaves,
          (slot >= 0 ? c->mtBigChars.p : c->mtChars.p) + at * caps.chars,
          (slot >= 0 ? c->mtBigProps.p : c->mtProps.p) + at * caps.props,
          c->mtPlan.anyAdjust ? (slot >= 0 ? c->mtBigLegacy.p : c->mtLegacy.p) + at * caps.leaves : nullptr};
}

// The two places that know which reads cache something between calls: fmt_mt_load and fmt_mt_run.
void invalidateReads(fmt_ctx* c) {
  c->frame.current = false;
  c->frame.tiled = false;
  c->textSized = false;
  c->runsSized = false;
}

// Makes the read frame current and returns it (nullptr: FMT_E_DEVICE, the message set): the headers come down
// once, every document's view goes up once. Nothing is in flight when it returns, so a later reserve moves
// nothing a copy still reads.
const fmt_ctx::ReadFrame* readFrame(fmt_ctx* c) {
  fmt_ctx::ReadFrame& F = c->frame;
  if (F.current) return &F;
  const uint32_t nd = c->mtDocs;
  F.hdr.resize(nd);
  F.views.resize(nd);
  for (uint32_t d = 0; d < nd; d++) F.views[d] = docView(c, d);
  hipError_t e = c->sumViews.reserve(nd);
  if (e == hipSuccess)
    e = hipMemcpyAsync(F.hdr.data(), c->mtHdr.p, nd * sizeof(fmt_mt_doc_result), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->sumViews.p, F.views.data(), nd * sizeof(fmt_kernels::SumView), hipMemcpyHostToDevice, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e != hipSuccess || e2 != hipSuccess) {
    hipErr(c, e != hipSuccess ? e : e2, "read frame");
    return nullptr;
  }
  F.current = true;
  return &F;
}

// The frame with its tile plan and the plan's items on the device, for the readers that walk tiles.
// `tooMany`: the caller's message for more than 2^32 - 1 items (FMT_E_CAPACITY).
int frameTiles(fmt_ctx* c, const char* tooMany, const fmt_ctx::ReadFrame** out) {
  const fmt_ctx::ReadFrame* F = readFrame(c);
  if (F == nullptr) return FMT_E_DEVICE;
  *out = F;
  if (F->tiled) return FMT_OK;
  fmt_plan::planTextTiles(F->hdr.data(), c->mtDocs, fmt_plan::kTextTileLeaves, c->frame.tiles);
  const size_t ni = F->tiles.items.size();
  if (ni > 0xFFFFFFFFull) return setErr(c, FMT_E_CAPACITY, tooMany);
  FMT_HIP(c, c->tileItems.reserve(ni));
  FMT_HIP(c, hipMemcpyAsync(c->tileItems.p, F->tiles.items.data(), ni * sizeof(fmt_plan::TextItem), hipMemcpyHostToDevice,
                            c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->frame.tiled = true;
  return FMT_OK;
}

// Packs the spans into c->packed on the device (transfer.hip; `words` dwords in all) and, with dst, brings the
// first `bytes` of the packing to the host in one staged copy, which returns when they are there. Without
// dst the packing is queued on the stream for the caller's own copies; `sp` lives until the caller's wait.
int gatherPacked(fmt_ctx* c, const std::vector<fmt_kernels::GatherSpan>& sp, uint64_t words, void* dst, size_t bytes) {
  if (sp.empty()) return FMT_OK;
  FMT_HIP(c, c->spans.reserve(sp.size()));
  FMT_HIP(c, c->packed.reserve(words));
  FMT_HIP(c, hipMemcpyAsync(c->spans.p, sp.data(), sp.size() * sizeof(fmt_kernels::GatherSpan), hipMemcpyHostToDevice,
                            c->stream));
  FMT_HIP(c, fmt_kernels::launchGatherSpans(c->spans.p, static_cast<uint32_t>(sp.size()), c->packed.p, c->numCUs, c->stream));
  if (dst != nullptr) FMT_HIP(c, stagedCopy(c, dst, c->packed.p, bytes, false));
  return FMT_OK;
}

}  // namespace

extern "C" {

int fmt_open(const fmt_config* cfg, fmt_ctx** out) {
  if (out == nullptr) return FMT_E_USAGE;
  *out = nullptr;
  auto* c = new (std::nothrow) fmt_ctx();
  if (c == nullptr) return FMT_E_DEVICE;
  *out = c;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return setErr(c, FMT_E_DEVICE, "no HIP device visible");
  c->device = cfg ? cfg->device : 0;
  if (c->device < 0 || c->device >= n) return setErr(c, FMT_E_USAGE, "device ordinal out of range");
  FMT_HIP(c, hipSetDevice(c->device));
  hipDeviceProp_t prop;
  FMT_HIP(c, hipGetDeviceProperties(&prop, c->device));
  c->arch = prop.gcnArchName;
  c->numCUs = prop.multiProcessorCount;
  if (c->arch.rfind("gfx950", 0) != 0)
    return setErr(c, FMT_E_DEVICE, "libfmt is built for gfx950 only; device is " + c->arch);
  if (cfg && cfg->stream) {
    c->stream = static_cast<hipStream_t>(cfg->stream);
  } else {
    FMT_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->ownStream = true;
  }
  FMT_HIP(c, hipEventCreate(&c->ev0));
  FMT_HIP(c, hipEventCreate(&c->ev1));
  FMT_HIP(c, hipEventCreate(&c->ev2));
  FMT_HIP(c, hipEventCreate(&c->ev3));
  FMT_HIP(c, hipEventCreate(&c->evS0));
  FMT_HIP(c, hipEventCreate(&c->evS1));
  FMT_HIP(c, c->errWord.reserve(1));
  return FMT_OK;
}

void fmt_close(fmt_ctx* c) {
  if (c == nullptr) return;
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->mapOps.release();
  c->mapOffs.release();
  c->mapOut.release();
  c->mapScratch.release();
  c->mapEntries.release();
  c->mapPacked.release();
  c->mapEv.release();
  c->mapEvOffs.release();
  c->mapPendBase.release();
  c->mapPendScratch.release();
  c->mapPendOut.release();
  c->mapPendCounts.release();
  c->mapPendStatus.release();
  c->mapCounts.release();
  c->mapOvf.release();
  c->mapLgTiles.release();
  c->mapLgScratch.release();
  c->mapLgDocs.release();
  c->mapPackedOff.release();
  c->mapSumEntries.release();
  for (auto* q : {&c->mapSumTags, &c->mapSumNBlobs, &c->mapSumList, &c->mapSumKeyRank, &c->mapSumValUnits, &c->mapSumPacked})
    q->release();
  c->errWord.release();
  c->mtOps.release();
  c->mtOffs.release();
  c->mtText.release();
  c->mtInit.release();
  c->mtPropsOff.release();
  c->mtPropsKv.release();
  c->mtHdr.release();
  c->mtLeaves.release();
  c->mtChars.release();
  c->mtProps.release();
  c->mtListBuf.release();
  c->mtCkpt.release();
  c->mtDesc.release();
  c->mtHugeCk.release();
  c->mtBigLeaves.release();
  c->mtBigChars.release();
  c->mtBigProps.release();
  c->mtSnap.release();
  c->mtSnapSegs.release();
  c->mtRelpos.release();
  c->mtSnapInfo.release();
  c->mtSnapStamps.release();
  c->mtCuOffs.release();
  c->mtCatchup.release();
  c->mtRmOffs.release();
  c->mtRmOrder.release();
  for (auto& h : c->huge)
    for (void* p : h.allocs) (void)hipFree(p);
  c->huge.clear();
  c->mtSmallList.release();
  c->hugeStates.release();
  c->hugeInputs.release();
  c->hugeOuts.release();
  c->stage.release();
  c->mtPm.release();
  c->mtPmOffs.release();
  c->mtLegacy.release();
  c->mtBigLegacy.release();
  for (auto* q : {&c->mtLocGroups, &c->mtLocRecs, &c->mtLocPm, &c->mtLocScratch, &c->mtLocRegenCount}) q->release();
  c->mtLocOffs.release();
  c->mtLocRegen.release();
  c->mtLocRegenText.release();
  c->mtLocTab.release();
  c->spans.release();
  c->packed.release();
  c->digests.release();
  c->v1Segs.release();
  c->tileItems.release();
  c->textUnits.release();
  c->textBases.release();
  c->textPacked.release();
  c->runsClsOff.release();
  c->runsCls.release();
  c->runsTiles.release();
  c->runsBases.release();
  c->runsPacked.release();
  c->posItems.release();
  c->posUnits.release();
  c->posQueries.release();
  c->posHits.release();
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ev3) (void)hipEventDestroy(c->ev3);
  if (c->evS0) (void)hipEventDestroy(c->evS0);
  if (c->evS1) (void)hipEventDestroy(c->evS1);
  if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* fmt_last_error(const fmt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int fmt_sync(fmt_ctx* c) {
  if (c == nullptr) return FMT_E_USAGE;
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  return FMT_OK;
}

int fmt_get_stats(const fmt_ctx* cc, fmt_stats* out) {
  auto* c = const_cast<fmt_ctx*>(cc);
  if (c == nullptr || out == nullptr) return FMT_E_USAGE;
  if (c->timed) {
    FMT_HIP(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    FMT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (c->timed2) {
      float ms2 = 0;
      FMT_HIP(c, hipEventSynchronize(c->ev3));
      FMT_HIP(c, hipEventElapsedTime(&ms2, c->ev2, c->ev3));
      ms += ms2;
    }
    c->stats.kernel_ms = ms;
    c->stats.total_ms = ms;
  }
  *out = c->stats;
  return FMT_OK;
}

int fmt_device_info(fmt_ctx* c, char* buf, size_t cap) {
  if (c == nullptr || buf == nullptr || cap == 0) return FMT_E_USAGE;
  std::snprintf(buf, cap, "%s device=%d CUs=%d", c->arch.c_str(), c->device, c->numCUs);
  return FMT_OK;
}

// ------------------------------------------------------------------------------ SharedMap
static int mapValidate(fmt_ctx* c, const fmt_map_op* ops, uint64_t nOps, const uint64_t* offs, uint32_t nDocs,
                       uint32_t keyBound) {
  if (c == nullptr || (nOps > 0 && ops == nullptr) || offs == nullptr || keyBound == 0)
    return setErr(c, FMT_E_USAGE, "fmt_map_load: bad arguments");
  if (offs[0] != 0 || offs[nDocs] != nOps) return setErr(c, FMT_E_USAGE, "doc_op_offsets do not cover ops");
  // (all of them before any op is read: with both ends checked, ascending offsets stay inside `ops`)
  for (uint32_t d = 0; d < nDocs; d++)
    if (offs[d + 1] < offs[d]) return setErr(c, FMT_E_USAGE, "doc_op_offsets not monotone");
  for (uint32_t d = 0; d < nDocs; d++) {
    // seq 0 is the dense kernels' "no kill yet / no set yet" (map_lww.hip): a set at seq 0 would be dropped
    if (offs[d + 1] > offs[d] && ops[offs[d]].seq == 0) {
      char m[96];
      std::snprintf(m, sizeof m, "doc %u: seq 0 (seqs are >= 1)", d);
      return setErr(c, FMT_E_DATA, m);
    }
    for (uint64_t i = offs[d] + 1; i < offs[d + 1]; i++) {
      if (ops[i].seq <= ops[i - 1].seq) {
        char m[128];
        std::snprintf(m, sizeof m, "doc %u: seq %u after %u (ops must be in increasing seq order)", d,
                      ops[i].seq, ops[i - 1].seq);
        return setErr(c, FMT_E_DATA, m);
      }
    }
  }
  return FMT_OK;
}

static int mapStage(fmt_ctx* c, const fmt_map_op* ops, uint64_t nOps, const uint64_t* offs, uint32_t nDocs,
                    uint32_t keyBound, bool sparse) {
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, c->mapOps.reserve(nOps));
  FMT_HIP(c, c->mapOffs.reserve(nDocs + 1ull));
  if (sparse) {
    FMT_HIP(c, c->mapEntries.reserve(nOps));
    FMT_HIP(c, c->mapCounts.reserve(nDocs));
  } else {
    FMT_HIP(c, c->mapOut.reserve(static_cast<size_t>(nDocs) * keyBound));
  }
  if (nOps) FMT_HIP(c, stagedCopy(c, c->mapOps.p, ops, nOps * sizeof(fmt_map_op), true));
  FMT_HIP(c, hipMemcpyAsync(c->mapOffs.p, offs, (nDocs + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->mapNOps = nOps;
  c->mapDocs = nDocs;
  c->mapKeyBound = keyBound;
  c->mapLoaded = true;
  c->mapSparse = sparse;
  c->mapRan = false;
  c->mapErrValid = false;
  c->mapSparseRan = false;
  c->mapPendRan = false;
  c->mapTieredDone = false;
  c->mapSumDone = false;  // (a summary's blobs are valid until the next map load)
  c->mapSumBlobs = fmt_plan::MapSumBlobs{};
  c->mapOffsHost.assign(offs, offs + nDocs + 1ull);
  return FMT_OK;
}

int fmt_map_load(fmt_ctx* c, const fmt_map_op* ops, uint64_t nOps, const uint64_t* offs, uint32_t nDocs,
                 uint32_t keyBound) {
  const int rc = mapValidate(c, ops, nOps, offs, nDocs, keyBound);
  return rc != FMT_OK ? rc : mapStage(c, ops, nOps, offs, nDocs, keyBound, false);
}

int fmt_map_load_sparse(fmt_ctx* c, const fmt_map_op* ops, uint64_t nOps, const uint64_t* offs, uint32_t nDocs,
                        uint32_t keyBound) {
  const int rc = mapValidate(c, ops, nOps, offs, nDocs, keyBound);
  return rc != FMT_OK ? rc : mapStage(c, ops, nOps, offs, nDocs, keyBound, true);
}

int fmt_map_run_sparse(fmt_ctx* c) {
  if (c == nullptr || !c->mapLoaded || !c->mapSparse) return setErr(c, FMT_E_USAGE, "fmt_map_run_sparse before fmt_map_load_sparse");
  c->mapSparseRan = false;  // (until this run is issued: a device error leaves no run to fetch)
  c->mapErrValid = false;
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, hipMemsetAsync(c->errWord.p, 0, sizeof(int), c->stream));
  FMT_HIP(c, hipEventRecord(c->ev0, c->stream));
  FMT_HIP(c, fmt_kernels::launchMapSparse(c->mapOps.p, c->mapOffs.p, c->mapDocs, c->mapKeyBound, c->mapEntries.p,
                                          c->mapCounts.p, c->errWord.p, c->numCUs, c->stream));
  FMT_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  c->timed2 = false;
  c->stats = fmt_stats{};
  c->stats.ops = c->mapNOps;
  c->stats.docs = c->mapDocs;
  c->stats.bytes_read = c->mapNOps * sizeof(fmt_map_op) + (c->mapDocs + 1ull) * sizeof(uint64_t);
  c->stats.bytes_written = static_cast<uint64_t>(c->mapDocs) * sizeof(uint32_t);  // + entries, at fetch
  c->stats.launches = 1;
  c->mapSparseRan = true;
  c->mapErrValid = true;
  c->mapPendRan = false;
  c->mapTieredDone = false;
  return FMT_OK;
}

// The LDS tier with its refusals listed, then the HBM tier (map_sparse_large.hip) over the list.
int fmt_map_run_sparse_tiered(fmt_ctx* c) {
  if (c == nullptr || !c->mapLoaded || !c->mapSparse)
    return setErr(c, FMT_E_USAGE, "fmt_map_run_sparse_tiered before fmt_map_load_sparse");
  c->mapSparseRan = false;
  c->mapErrValid = false;
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, c->mapOvf.reserve(c->mapDocs + 1ull));
  FMT_HIP(c, hipMemsetAsync(c->errWord.p, 0, sizeof(int), c->stream));
  FMT_HIP(c, hipMemsetAsync(c->mapOvf.p, 0, sizeof(uint32_t), c->stream));
  FMT_HIP(c, hipEventRecord(c->ev0, c->stream));
  FMT_HIP(c, fmt_kernels::launchMapSparseTracked(c->mapOps.p, c->mapOffs.p, c->mapDocs, c->mapKeyBound, c->mapEntries.p,
                                                 c->mapCounts.p, c->errWord.p, c->mapOvf.p, c->numCUs, c->stream));
  FMT_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  c->timed2 = false;
  c->stats = fmt_stats{};
  c->stats.ops = c->mapNOps;
  c->stats.docs = c->mapDocs;
  c->stats.bytes_read = c->mapNOps * sizeof(fmt_map_op) + (c->mapDocs + 1ull) * sizeof(uint64_t);
  c->stats.bytes_written = static_cast<uint64_t>(c->mapDocs) * sizeof(uint32_t);  // + entries, at fetch
  c->stats.launches = 1;
  c->mapSparseRan = true;  // (the LDS tier's documents are valid whatever becomes of the rest)
  c->mapErrValid = true;
  c->mapPendRan = false;
  c->mapTieredDone = false;
  uint32_t nOvf = 0;
  FMT_HIP(c, hipMemcpyAsync(&nOvf, c->mapOvf.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->mapTieredDone = nOvf == 0;
  if (nOvf == 0) return FMT_OK;
  std::vector<uint32_t> ovf(nOvf);
  FMT_HIP(c, hipMemcpy(ovf.data(), c->mapOvf.p + 1, nOvf * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::sort(ovf.begin(), ovf.end());
  fmt_plan::MapLargePlan& P = c->mapLgPlan;
  if (const char* why = fmt_plan::planMapLarge(c->mapOffsHost.data(), c->mapDocs, ovf.data(), nOvf, P))
    return setErr(c, FMT_E_CAPACITY, why);
  const size_t nTiles = P.tileDoc.size();
  if (c->mapLgScratch.reserve(P.words()) != hipSuccess || c->mapLgDocs.reserve(nOvf) != hipSuccess ||
      c->mapLgTiles.reserve(2 * nTiles) != hipSuccess) {
    (void)hipGetLastError();
    char m[160];
    std::snprintf(m, sizeof m, "no device memory for the HBM tier of %u document(s): %llu bytes of tables; they stay refused",
                  nOvf, static_cast<unsigned long long>(P.scratchBytes()));
    return setErr(c, FMT_E_DEVICE, m);
  }
  FMT_HIP(c, hipMemcpyAsync(c->mapLgDocs.p, P.docs.data(), nOvf * sizeof(fmt_plan::MapLargeDoc), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipMemcpyAsync(c->mapLgTiles.p, P.tileDoc.data(), nTiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipMemcpyAsync(c->mapLgTiles.p + nTiles, P.tileFirst.data(), nTiles * sizeof(uint32_t), hipMemcpyHostToDevice,
                            c->stream));
  fmt_kernels::MapLargeArgs a{};
  a.ops = c->mapOps.p;
  a.docs = c->mapLgDocs.p;
  a.tileDoc = c->mapLgTiles.p;
  a.tileFirst = c->mapLgTiles.p + nTiles;
  a.scratch = c->mapLgScratch.p;
  a.out = c->mapEntries.p;
  a.counts = c->mapCounts.p;
  a.error = c->errWord.p;
  a.slots = P.slots;
  a.tileCountAt = P.tileCountAt();
  a.clearAt = P.clearAt();
  a.nDocs = nOvf;
  a.nTiles = static_cast<uint32_t>(nTiles);
  a.keyBound = c->mapKeyBound;
  uint32_t launches = 0;
  FMT_HIP(c, hipEventRecord(c->ev2, c->stream));
  FMT_HIP(c, fmt_kernels::launchMapLarge(a, c->numCUs, c->stream, &launches));
  FMT_HIP(c, hipEventRecord(c->ev3, c->stream));
  c->timed2 = true;
  FMT_HIP(c, hipStreamSynchronize(c->stream));  // (the plan's host arrays are read by the copies above)
  // the passes' streamed traffic (map_sparse_large.hip); the table atomics and probes are not counted
  c->stats.bytes_read += P.ops * (2 * sizeof(fmt_map_op) + 3 * 4) + nTiles * (2 * 8 + 2 * 4);
  c->stats.bytes_written += P.slots * 20 + P.ops * 4 + nTiles * 8 + nOvf * 4ull;
  c->stats.launches += launches;
  c->mapTieredDone = true;
  return FMT_OK;
}

int fmt_map_fetch_sparse(fmt_ctx* c, uint32_t* counts, fmt_map_entry* entries, uint64_t capEntries, uint64_t* nEntries) {
  if (c == nullptr || counts == nullptr || !c->mapLoaded || !c->mapSparse)
    return setErr(c, FMT_E_USAGE, "fmt_map_fetch_sparse: nothing loaded");
  if (!c->mapSparseRan) {
    // Before a run (fmt.h "Call order"): the batch with no op applied, from the host. mapCounts still
    // holds an earlier batch's counts, or nothing.
    std::memset(counts, 0, c->mapDocs * sizeof(uint32_t));
    if (nEntries) *nEntries = 0;
    return FMT_OK;
  }
  FMT_HIP(c, hipSetDevice(c->device));
  int errWord = 0;
  FMT_HIP(c, hipMemcpyAsync(&errWord, c->errWord.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipMemcpyAsync(counts, c->mapCounts.p, c->mapDocs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<uint64_t> packedOff(c->mapDocs + 1ull, 0);
  for (uint32_t d = 0; d < c->mapDocs; d++) packedOff[d + 1] = packedOff[d] + counts[d];
  const uint64_t n = packedOff[c->mapDocs];
  if (nEntries) *nEntries = n;
  c->stats.bytes_written = static_cast<uint64_t>(c->mapDocs) * sizeof(uint32_t) + n * sizeof(fmt_map_entry);
  if (entries != nullptr) {
    if (capEntries < n) return setErr(c, FMT_E_USAGE, "fmt_map_fetch_sparse: cap_entries below the live entries");
    FMT_HIP(c, c->mapPackedOff.reserve(c->mapDocs + 1ull));
    FMT_HIP(c, c->mapPacked.reserve(n));
    FMT_HIP(c, hipMemcpyAsync(c->mapPackedOff.p, packedOff.data(), (c->mapDocs + 1ull) * sizeof(uint64_t),
                              hipMemcpyHostToDevice, c->stream));
    FMT_HIP(c, fmt_kernels::launchMapSparsePack(c->mapEntries.p, c->mapOffs.p, c->mapCounts.p, c->mapPackedOff.p,
                                                c->mapDocs, c->mapPacked.p, c->stream));
    FMT_HIP(c, hipMemcpyAsync(entries, c->mapPacked.p, n * sizeof(fmt_map_entry), hipMemcpyDeviceToHost, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (errWord & 1) return setErr(c, FMT_E_DATA, "an op referenced a key id >= key_bound");
  if (errWord & 2) return setErr(c, FMT_E_CAPACITY, "a document exceeded the sparse path's keys or ops per document");
  return FMT_OK;
}

int fmt_map_pending_run(fmt_ctx* c, const fmt_map_local_op* events, uint64_t nEvents, const uint64_t* evOffs) {
  if (c == nullptr || !c->mapLoaded || !c->mapSparse || !c->mapSparseRan)
    return setErr(c, FMT_E_USAGE, "fmt_map_pending_run needs a sparse map run (fmt_map_run_sparse) first");
  if ((nEvents > 0 && events == nullptr) || evOffs == nullptr)
    return setErr(c, FMT_E_USAGE, "fmt_map_pending_run: null events or offsets");
  if (nEvents >= 0xFFFFFFFFull) return setErr(c, FMT_E_USAGE, "fmt_map_pending_run: too many events");
  const uint32_t n = c->mapDocs;
  if (evOffs[0] != 0 || evOffs[n] != nEvents) return setErr(c, FMT_E_USAGE, "doc_event_offsets must span [0, n_events)");
  std::vector<uint64_t> base(n);
  for (uint32_t d = 0; d < n; d++) {
    if (evOffs[d + 1] < evOffs[d]) return setErr(c, FMT_E_USAGE, "doc_event_offsets is not ascending");
    for (uint64_t i = evOffs[d]; i < evOffs[d + 1]; i++) {
      const fmt_map_local_op& e = events[i];
      const uint32_t kind = e.kind_value >> FMT_MAP_KIND_SHIFT;
      if (e.doc != d || e.event > FMT_MAP_EV_ROLLBACK || kind > FMT_MAP_CLEAR ||
          (kind != FMT_MAP_CLEAR && e.key >= c->mapKeyBound))
        return setErr(c, FMT_E_DATA, "a local event with a bad document, event, kind or key id");
    }
    base[d] = c->mapOffsHost[d] + evOffs[d];  // room for the sequenced entries plus one per event
  }
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, c->mapEv.reserve(nEvents));
  FMT_HIP(c, c->mapEvOffs.reserve(n + 1ull));
  FMT_HIP(c, c->mapPendBase.reserve(n));
  FMT_HIP(c, c->mapPendScratch.reserve(fmt_kernels::mapPendingScratchBytes(nEvents)));
  FMT_HIP(c, c->mapPendOut.reserve(c->mapNOps + nEvents));
  FMT_HIP(c, c->mapPendCounts.reserve(n));
  FMT_HIP(c, c->mapPendStatus.reserve(n));
  if (nEvents) FMT_HIP(c, stagedCopy(c, c->mapEv.p, events, nEvents * sizeof(fmt_map_local_op), true));
  FMT_HIP(c, hipMemcpyAsync(c->mapEvOffs.p, evOffs, (n + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipMemcpyAsync(c->mapPendBase.p, base.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipEventRecord(c->ev0, c->stream));
  FMT_HIP(c, fmt_kernels::launchMapPending(c->mapEv.p, c->mapEvOffs.p, c->mapEntries.p, c->mapOffs.p, c->mapCounts.p, n,
                                           c->mapPendScratch.p, c->mapPendBase.p, c->mapPendOut.p, c->mapPendCounts.p,
                                           c->mapPendStatus.p, c->stream));
  FMT_HIP(c, hipEventRecord(c->ev1, c->stream));
  // (the host arrays above are read by the copies before the call returns: synchronize)
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->timed = true;
  c->timed2 = false;
  c->stats = fmt_stats{};
  c->stats.ops = nEvents;
  c->stats.docs = n;
  c->stats.bytes_read = nEvents * sizeof(fmt_map_local_op) + c->mapNOps * sizeof(fmt_map_entry);
  c->stats.launches = 1;
  c->mapPendRan = true;
  return FMT_OK;
}

int fmt_map_pending_fetch(fmt_ctx* c, uint32_t* counts, int32_t* status, fmt_map_entry* entries, uint64_t capEntries,
                          uint64_t* nEntries) {
  if (c == nullptr || counts == nullptr || !c->mapPendRan)
    return setErr(c, FMT_E_USAGE, "fmt_map_pending_fetch before fmt_map_pending_run");
  const uint32_t n = c->mapDocs;
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, hipMemcpyAsync(counts, c->mapPendCounts.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (status) FMT_HIP(c, hipMemcpyAsync(status, c->mapPendStatus.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<uint64_t> packedOff(n + 1ull, 0);
  for (uint32_t d = 0; d < n; d++) packedOff[d + 1] = packedOff[d] + counts[d];
  const uint64_t total = packedOff[n];
  if (nEntries) *nEntries = total;
  if (entries != nullptr) {
    if (capEntries < total) return setErr(c, FMT_E_USAGE, "fmt_map_pending_fetch: cap_entries below the entries");
    FMT_HIP(c, c->mapPackedOff.reserve(n + 1ull));
    FMT_HIP(c, c->mapPacked.reserve(total));
    FMT_HIP(c, hipMemcpyAsync(c->mapPackedOff.p, packedOff.data(), (n + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice,
                              c->stream));
    FMT_HIP(c, fmt_kernels::launchMapSparsePack(c->mapPendOut.p, c->mapPendBase.p, c->mapPendCounts.p, c->mapPackedOff.p,
                                                n, c->mapPacked.p, c->stream));
    FMT_HIP(c, hipMemcpyAsync(entries, c->mapPacked.p, total * sizeof(fmt_map_entry), hipMemcpyDeviceToHost, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return FMT_OK;
}

// Bulk SharedMap summaries of the last sparse run (include/fmt_map_summary.h): the tables on the host
// threads, ordering and blob assignment on the device (map_summary.hip; documents past its tier and
// the host-only switch: map_sum_plan.h), one packed copy back, the JSON on the host threads.
int fmt_map_summarize(fmt_ctx* c, const char* const* keys, uint32_t nKeys, const char* const* values, uint32_t nValues,
                      uint32_t threads, fmt_map_summary_timing* timing) {
  if (c == nullptr || (nKeys && keys == nullptr) || (nValues && values == nullptr))
    return setErr(c, FMT_E_USAGE, "fmt_map_summarize: null arguments");
  if (!c->mapLoaded || !c->mapSparse || !c->mapSparseRan)
    return setErr(c, FMT_E_USAGE, "fmt_map_summarize needs a sparse map run (fmt_map_run_sparse or fmt_map_run_sparse_tiered) first");
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  FMT_HIP(c, hipSetDevice(c->device));
  const uint32_t nd = c->mapDocs;
  int errWord = 0;
  std::vector<uint32_t> counts(nd);
  FMT_HIP(c, hipMemcpyAsync(&errWord, c->errWord.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (nd) FMT_HIP(c, hipMemcpyAsync(counts.data(), c->mapCounts.p, nd * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  if (errWord & 1) return setErr(c, FMT_E_DATA, "an op referenced a key id >= key_bound");
  if ((errWord & 2) && !c->mapTieredDone)
    return setErr(c, FMT_E_CAPACITY,
                  "a document exceeded the sparse path's keys or ops per document and has no entries: run "
                  "fmt_map_run_sparse_tiered before fmt_map_summarize");
  c->mapSumDone = false;
  const uint32_t nt = threads ? threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  // host tables
  const auto tA = clk::now();
  fmt_plan::MapSumTables T;
  fmt_plan::mapSumBuildTables(keys, nKeys, values, nValues, nt, T);
  std::vector<uint64_t> at(nd + 1ull, 0);  // packed position of each document's first entry
  for (uint32_t d = 0; d < nd; d++) at[d + 1] = at[d] + counts[d];
  const uint64_t n = at[nd];
  const auto tB = clk::now();
  const bool device = !c->mapSumHostOnly;
  const uint64_t words = device ? 4 * n + nd : 3 * n;
  FMT_HIP(c, c->mapPackedOff.reserve(nd + 1ull));
  FMT_HIP(c, c->mapSumPacked.reserve(words));
  FMT_HIP(c, c->mapSumHost.reserve(4 * n + nd));
  FMT_HIP(c, hipMemcpyAsync(c->mapPackedOff.p, at.data(), (nd + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  float kms = 0.f;
  if (device) {
    FMT_HIP(c, c->mapSumEntries.reserve(c->mapNOps));
    FMT_HIP(c, c->mapSumTags.reserve(c->mapNOps));
    FMT_HIP(c, c->mapSumNBlobs.reserve(nd));
    FMT_HIP(c, c->mapSumList.reserve(nd + 1ull));
    FMT_HIP(c, c->mapSumKeyRank.reserve(nKeys));
    FMT_HIP(c, c->mapSumValUnits.reserve(nValues));
    if (nKeys) FMT_HIP(c, hipMemcpyAsync(c->mapSumKeyRank.p, T.keyRank.data(), nKeys * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (nValues)
      FMT_HIP(c, hipMemcpyAsync(c->mapSumValUnits.p, T.valUnits.data(), nValues * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    FMT_HIP(c, hipMemsetAsync(c->mapSumList.p, 0, sizeof(uint32_t), c->stream));
    fmt_kernels::MapSummaryArgs a{};
    a.entries = c->mapEntries.p;
    a.offsets = c->mapOffs.p;
    a.counts = c->mapCounts.p;
    a.keyRank = c->mapSumKeyRank.p;
    a.valUnits = c->mapSumValUnits.p;
    a.ordered = c->mapSumEntries.p;
    a.tags = c->mapSumTags.p;
    a.nBlobs = c->mapSumNBlobs.p;
    a.list = c->mapSumList.p;
    a.nDocs = nd;
    a.nKeys = nKeys;
    a.nValues = nValues;
    FMT_HIP(c, hipEventRecord(c->evS0, c->stream));  // (own events, as the merge-tree summaries)
    FMT_HIP(c, fmt_kernels::launchMapSummary(a, c->numCUs, c->stream));
    FMT_HIP(c, hipEventRecord(c->evS1, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
    FMT_HIP(c, hipEventElapsedTime(&kms, c->evS0, c->evS1));
  }
  // fetch: one pack, one copy
  const auto t0 = clk::now();
  if (device)
    FMT_HIP(c, fmt_kernels::launchMapSummaryPack(c->mapSumEntries.p, c->mapSumTags.p, c->mapSumNBlobs.p, c->mapOffs.p,
                                                 c->mapCounts.p, c->mapPackedOff.p, nd, c->mapSumPacked.p, c->stream));
  else  // the replay's entries as they are
    FMT_HIP(c, fmt_kernels::launchMapSparsePack(c->mapEntries.p, c->mapOffs.p, c->mapCounts.p, c->mapPackedOff.p, nd,
                                                reinterpret_cast<fmt_map_entry*>(c->mapSumPacked.p), c->stream));
  uint32_t* const host = c->mapSumHost.p;
  if (words) FMT_HIP(c, hipMemcpyAsync(host, c->mapSumPacked.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  const auto t1 = clk::now();
  fmt_map_entry* const ent = reinterpret_cast<fmt_map_entry*>(host);
  uint32_t* const tags = host + 3 * n;
  uint32_t* const nBlobs = host + 4 * n;
  // documents past the device tier (their entries came back in birth order) are ordered here, from a
  // copy the ordering reads while it writes the packed arrays in place
  uint32_t hostDocs = 0;
  {
    auto past = [&](uint32_t d) { return !device || counts[d] > fmt_plan::kMapSumDeviceMax; };
    std::vector<uint64_t> from(nd + 1ull, 0);
    for (uint32_t d = 0; d < nd; d++) from[d + 1] = from[d] + (past(d) ? counts[d] : 0u);
    std::vector<fmt_map_entry> birth(from[nd]);
    for (uint32_t d = 0; d < nd; d++)
      if (past(d) && counts[d]) std::memcpy(birth.data() + from[d], ent + at[d], counts[d] * sizeof(fmt_map_entry));
    hostDocs = fmt_plan::mapSumOrderDocs(birth.data(), from.data(), ent, tags, nBlobs, counts.data(), at.data(), nd, T, nt, past);
  }
  c->mapSumStatus.assign(nd, FMT_OK);
  fmt_plan::mapSumThreads(nt, [&](uint32_t t) {
    const uint32_t per = (nd + nt - 1) / nt, lo = std::min(nd, per * t), hi = std::min(nd, lo + per);
    for (uint32_t d = lo; d < hi; d++)
      if (!fmt_plan::mapSumInTables(ent + at[d], counts[d], nKeys, nValues)) c->mapSumStatus[d] = FMT_E_USAGE;
  });
  fmt_plan::mapSumFormat(ent, tags, nBlobs, counts.data(), at.data(), c->mapSumStatus.data(), nd, keys, values, T, nt,
                         c->mapSumBlobs);
  const auto t2 = clk::now();
  c->mapSumDone = true;
  c->mapSumN = n;
  c->timed = false;
  c->timed2 = false;
  c->stats = fmt_stats{};
  c->stats.kernel_ms = kms;
  c->stats.total_ms = kms;
  c->stats.ops = n;
  c->stats.docs = nd;
  // entries, their key ranks and value units, counts and offsets in; ordered entries, tags, blob counts out
  c->stats.bytes_read = device ? n * (sizeof(fmt_map_entry) + 8) + nd * 12ull : 0;
  c->stats.bytes_written = device ? n * (sizeof(fmt_map_entry) + 4) + nd * 4ull : 0;
  c->stats.launches = device ? 3 : 1;
  if (timing) {
    timing->kernel_ms = kms;
    timing->fetch_ms = ms(t0, t1);
    timing->format_ms = ms(tA, tB) + ms(t1, t2);
    timing->bytes = c->mapSumBlobs.bytes;
    timing->threads = nt;
    timing->host_ordered_docs = hostDocs;
  }
  return FMT_OK;
}

static int mapSummaryPiece(fmt_ctx* c, uint32_t doc, uint32_t piece, const char** out, size_t* len, uint32_t* nBlobs,
                           const char* what) {
  if (c == nullptr || !c->mapSumDone || doc >= c->mapSumStatus.size())
    return setErr(c, FMT_E_USAGE, std::string(what) + ": no summary for doc (fmt_map_summarize first)");
  if (c->mapSumStatus[doc] != FMT_OK)
    return setErr(c, c->mapSumStatus[doc], "a live entry's key or value id is outside the tables passed to fmt_map_summarize");
  const fmt_plan::MapSumBlobs& B = c->mapSumBlobs;
  const uint64_t first = B.pieceAt[doc], pieces = B.pieceAt[doc + 1] - first;
  if (piece >= pieces) return setErr(c, FMT_E_USAGE, std::string(what) + ": no such blob");
  const uint64_t b = piece ? B.ends[first + piece - 1] : 0, e = B.ends[first + piece];
  if (out) *out = B.buf[B.docThread[doc]].data() + B.docAt[doc] + b;
  if (len) *len = e - b;
  if (nBlobs) *nBlobs = static_cast<uint32_t>(pieces - 1);
  return FMT_OK;
}

int fmt_map_summary_blobs(fmt_ctx* c, uint32_t doc, const char** header, size_t* headerLen, uint32_t* nBlobs) {
  return mapSummaryPiece(c, doc, 0, header, headerLen, nBlobs, "fmt_map_summary_blobs");
}

int fmt_map_summary_blob(fmt_ctx* c, uint32_t doc, uint32_t k, const char** blob, size_t* blobLen) {
  if (k == 0xFFFFFFFFu) return setErr(c, FMT_E_USAGE, "fmt_map_summary_blob: no such blob");
  return mapSummaryPiece(c, doc, k + 1, blob, blobLen, nullptr, "fmt_map_summary_blob");
}

static int runMap(fmt_ctx* c, const fmt_map_op* ops, const uint64_t* offs, uint32_t nDocs, uint32_t keyBound,
                  uint64_t nOps, fmt_map_slot* out) {
  FMT_HIP(c, hipSetDevice(c->device));
  uint32_t* scratch = nullptr;
  if (fmt_kernels::mapLwwNeedsScratch(keyBound)) {  // key pool beyond the LDS table: HBM tables
    FMT_HIP(c, c->mapScratch.reserve(static_cast<size_t>(nDocs) * keyBound * 2));
    scratch = c->mapScratch.p;
  }
  FMT_HIP(c, hipMemsetAsync(c->errWord.p, 0, sizeof(int), c->stream));
  FMT_HIP(c, hipEventRecord(c->ev0, c->stream));
  FMT_HIP(c, fmt_kernels::launchMapLww(ops, offs, nDocs, keyBound, out, c->errWord.p, c->numCUs, c->stream, scratch));
  FMT_HIP(c, hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  c->timed2 = false;
  c->stats = fmt_stats{};
  c->stats.ops = nOps;
  c->stats.docs = nDocs;
  const uint64_t nSlots = static_cast<uint64_t>(nDocs) * keyBound;
  c->stats.bytes_read = nOps * sizeof(fmt_map_op) + (nDocs + 1ull) * sizeof(uint64_t);
  c->stats.bytes_written = nSlots * sizeof(fmt_map_slot);
  c->stats.launches = 1;
  c->mapErrValid = true;
  if (scratch != nullptr) {
    // HBM-table path: three table fills (8 B slot + 4 B kill + 4 B first per slot) and the finish
    // pass (reads slot + first, writes the slot) on top of the op stream and the kernel's atomics
    c->stats.bytes_written += nSlots * 16;
    c->stats.bytes_read += nSlots * 12;
    c->stats.launches = 5;
  }
  return FMT_OK;
}

int fmt_map_run(fmt_ctx* c) {
  if (c == nullptr || !c->mapLoaded || c->mapSparse) return setErr(c, FMT_E_USAGE, "fmt_map_run before fmt_map_load");
  c->mapRan = false;
  c->mapErrValid = false;
  const int rc = runMap(c, c->mapOps.p, c->mapOffs.p, c->mapDocs, c->mapKeyBound, c->mapNOps, c->mapOut.p);
  c->mapRan = rc == FMT_OK;
  return rc;
}

int fmt_map_fetch(fmt_ctx* c, fmt_map_slot* out) {
  if (c == nullptr || out == nullptr || !c->mapLoaded || c->mapSparse)
    return setErr(c, FMT_E_USAGE, "fmt_map_fetch: nothing loaded");
  if (!c->mapRan) {
    // Before a run (fmt.h "Call order"): the batch with no op applied, from the host. mapOut still
    // holds an earlier batch's slots, or nothing.
    const size_t nSlots = static_cast<size_t>(c->mapDocs) * c->mapKeyBound;
    for (size_t i = 0; i < nSlots; i++) out[i] = fmt_map_slot{FMT_MAP_ABSENT, 0u};
    return FMT_OK;
  }
  int errWord = 0;
  FMT_HIP(c, hipMemcpyAsync(&errWord, c->errWord.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipMemcpyAsync(out, c->mapOut.p, static_cast<size_t>(c->mapDocs) * c->mapKeyBound * sizeof(fmt_map_slot),
                            hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  if (errWord) return setErr(c, FMT_E_DATA, "an op referenced a key id >= key_bound");
  return FMT_OK;
}

int fmt_map_replay_device(fmt_ctx* c, const fmt_map_op* dOps, const uint64_t* dOffs, uint32_t nDocs,
                          uint32_t keyBound, fmt_map_slot* dOut) {
  if (c == nullptr || dOffs == nullptr || dOut == nullptr || keyBound == 0)
    return setErr(c, FMT_E_USAGE, "fmt_map_replay_device: bad arguments");
  // the HBM-table path runs 64-bit atomics on the output slots viewed as u64
  if (fmt_kernels::mapLwwNeedsScratch(keyBound) && (reinterpret_cast<uintptr_t>(dOut) & 7u) != 0)
    return setErr(c, FMT_E_USAGE, "fmt_map_replay_device: d_out must be 8-byte aligned for key_bound > 2560");
  return runMap(c, dOps, dOffs, nDocs, keyBound, 0, dOut);
}

int fmt_map_check(fmt_ctx* c) {
  if (c == nullptr) return FMT_E_USAGE;
  if (!c->mapErrValid)
    return setErr(c, FMT_E_USAGE, "fmt_map_check before a map run (fmt_map_run, fmt_map_run_sparse[_tiered] or fmt_map_replay_device) since the last map load");
  int errWord = 0;
  FMT_HIP(c, hipMemcpyAsync(&errWord, c->errWord.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  if (errWord) return setErr(c, FMT_E_DATA, "an op referenced a key id >= key_bound");
  return FMT_OK;
}

// ------------------------------------------------------------------------------ merge-tree
int fmt_mt_capacity(uint32_t* maxLeaves, uint32_t* maxChars, uint32_t* maxProps) {
  // A document is replayed in the large tier when it overflows the small one, so the limits are
  // the large tier's (the small tier's prop-set table is one larger: report the larger).
  const fmt_kernels::MtCaps big = fmt_kernels::mergeTreeCaps(true), small = fmt_kernels::mergeTreeCaps(false);
  if (maxLeaves) *maxLeaves = big.leaves;
  if (maxChars) *maxChars = big.chars;
  if (maxProps) *maxProps = big.props > small.props ? big.props : small.props;
  return FMT_OK;
}

// One huge-tier document (huge_engine.h): its HBM state sized from its op count and start, inputs
// (ops [o0, o1) of the staged batch, nSegs start segments at segsDev) and output buffers; header d.
// textPerOp bounds the merge area (zamboni appends build their text there).
static int setupHugeDoc(fmt_ctx* c, uint64_t textLen, uint32_t nPropsOps, uint32_t d, uint64_t o0,
                        uint64_t o1, const fmt_mt_snapshot_seg* segsDev, uint64_t nHeader, uint64_t nBody, int32_t minSeq,
                        int32_t seq, int32_t initClient, uint64_t textPerOp, uint64_t docChars) {
  const uint64_t nOps = o1 - o0, N = nHeader + nBody;
  c->mtHugeSlot[d] = static_cast<int32_t>(c->huge.size());
  c->huge.emplace_back();
  auto& H = c->huge.back();
  auto alloc = [&](size_t bytes, void** out) -> hipError_t {
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e == hipSuccess) H.allocs.push_back(*out);
    return e;
  };
  // a document whose state does not fit in device memory fails alone (FMT_E_CAPACITY): what it
  // allocated is released and it leaves the huge tier
  auto drop = [&](hipError_t e) -> int {
    for (void* q : H.allocs) (void)hipFree(q);
    c->huge.pop_back();
    c->mtHugeSlot[d] = -1;
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return FMT_E_CAPACITY;
    }
    return hipErr(c, e, "setupHugeDoc");
  };
  fmt_huge::HugeState& S = H.state;
  uint64_t shapeBlocks = 0;
  if (nBody > 0) {
    fmt_huge::loadShape(nHeader, nBody, H.shape);
    for (uint32_t l = 0; l < H.shape[0]; l++) shapeBlocks += H.shape[1 + l];
  }
  const uint64_t blockCap = shapeBlocks + 2 * (N / 7 + 1) + 2 * nOps + 1024;
  if (blockCap > 0xFFFFFFF0ull || N + 3 * nOps + 16 > 0xFFFFFFF0ull) return drop(hipErrorOutOfMemory);
  S.blockCap = static_cast<uint32_t>(blockCap);
  S.idCap = static_cast<uint32_t>(N + 3 * nOps + 16);
  S.winCap = S.idCap;  // every leaf can be in the window (a wide remove puts many there)
  // the merge area: two halves (huge_engine.h compactText), each able to hold the document's whole
  // text twice over (its live merged text plus one run as long as the document)
  const uint64_t merge = std::max<uint64_t>(textPerOp * nOps + 65536, 4 * docChars + 131072);
  const uint64_t textCap = std::min<uint64_t>(textLen + merge, 0xFFFFFFF0ull);
  if (textCap <= textLen) return drop(hipErrorOutOfMemory);  // (offsets are 32-bit)
  const size_t nl = static_cast<size_t>(S.blockCap) * 8, nb = S.blockCap;
  void* p;
  hipError_t e;
#define FMT_ALLOC(field, T, count)                                      \
  if ((e = alloc((count) * sizeof(T), &p)) != hipSuccess) return drop(e); \
  S.field = static_cast<T*>(p);
  FMT_ALLOC(lLen, uint32_t, nl) FMT_ALLOC(lIns, int32_t, nl) FMT_ALLOC(lRm, int32_t, nl)
  FMT_ALLOC(lMlo, uint32_t, nl) FMT_ALLOC(lMhi, uint32_t, nl) FMT_ALLOC(lId, uint32_t, nl)
  FMT_ALLOC(lText, uint32_t, nl) FMT_ALLOC(lMeta, uint32_t, nl)
  FMT_ALLOC(bCount, uint32_t, nb) FMT_ALLOC(bParent, uint32_t, nb) FMT_ALLOC(bLeaf, uint32_t, nb)
  FMT_ALLOC(bScour, int32_t, nb) FMT_ALLOC(bChild, uint32_t, nb * 8) FMT_ALLOC(bGroup, uint32_t, nb)
  FMT_ALLOC(bSlot, uint32_t, nb) FMT_ALLOC(freeBlk, uint32_t, nb)
  FMT_ALLOC(gSlotBlk, uint32_t, static_cast<size_t>(fmt_huge::kGroupCap) * fmt_huge::kSlotCap)
  FMT_ALLOC(gSlotStable, int32_t, static_cast<size_t>(fmt_huge::kGroupCap) * fmt_huge::kSlotCap)
  FMT_ALLOC(leafBlk, uint32_t, S.idCap) FMT_ALLOC(winIdx, uint32_t, S.idCap)
  FMT_ALLOC(wRec, uint32_t, static_cast<size_t>(S.winCap) * 4) FMT_ALLOC(wMask, uint32_t, static_cast<size_t>(S.winCap) * 2)
  FMT_ALLOC(wBlk, uint32_t, S.winCap)
  FMT_ALLOC(wLeaf, uint32_t, S.winCap)
  // the merge area only; the batch text is read in place (huge_engine.h HugeState::base)
  FMT_ALLOC(text, uint16_t, textCap - textLen)
  FMT_ALLOC(props, uint32_t, static_cast<size_t>(fmt_huge::kPropCap) * fmt_huge::kPropWords)
  FMT_ALLOC(pClass, uint32_t, fmt_huge::kPropCap)
  FMT_ALLOC(pHead, uint32_t, 2ull * fmt_huge::kPropHash)
  FMT_ALLOC(pNext, uint32_t, 2ull * fmt_huge::kPropCap)
  S.text -= textLen;
  S.base = c->mtText.p;
  S.textLen = textLen;
  S.textCap = textCap;
  fmt_huge::HugeInputs& I = H.in;
  I.ops = c->mtOps.p;
  I.begin = o0;
  I.end = o1;
  I.propsOff = c->mtPropsOff.p;
  I.propsKv = c->mtPropsKv.p;
  I.nPropsOps = nPropsOps;
  I.segs = segsDev;
  I.nSegs = static_cast<uint32_t>(N);
  I.segProps = c->mtPlan.segProps[d];
  // SnapshotV1 merge info of a summary-loaded document's segments (header chunk)
  I.info = nullptr;
  I.stamps = c->mtHasSnapInfo ? c->mtSnapStamps.p : nullptr;
  if (c->mtHasSnapInfo && c->mtSnapHost.size() > d && c->mtSnapHost[d].loaded) I.info = c->mtSnapInfo.p + c->mtSnapHost[d].first_seg;
  // V1 body-chunk segments with merge info (FMT_MT_F_LOADSEG ops) name rows of the batch's table
  I.infoAll = c->mtHasSnapInfo ? c->mtSnapInfo.p : nullptr;
  I.nInfoAll = c->mtHasSnapInfo ? c->mtNSnapSegs : 0;
  // catch-up ranges go to the document's slab, as in the other tiers
  I.catchup = nullptr;
  I.catchupCap = 0;
  S.cuIds = nullptr;
  if (c->mtPlan.hasCatchup() && c->mtPlan.cuOffs[d + 1] > c->mtPlan.cuOffs[d]) {
    I.catchup = c->mtCatchup.p + c->mtPlan.cuOffs[d];
    I.catchupCap = static_cast<uint32_t>(std::min<uint64_t>(c->mtPlan.cuOffs[d + 1] - c->mtPlan.cuOffs[d], 0xFFFFFFFFull));
    if ((e = alloc(static_cast<size_t>(S.idCap) * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    S.cuIds = static_cast<uint32_t*>(p);
  }
  // relative positions: the batch's table, and the document's marker list
  I.relpos = c->mtNRelpos ? c->mtRelpos.p : nullptr;
  I.nRelpos = c->mtNRelpos;
  I.markerKey = c->mtMarkerKey;
  // annotate-adjust: the batch's tables (computed numbers, PropertiesManager records), the leaf id ->
  // output index map of the getAtSeq output
  I.adj = c->mtPlan.anyAdjust ? c->mtAdjTab.p : nullptr;
  I.doc = d;
  S.outIdx = nullptr;
  if (c->mtPlan.anyAdjust) {
    if ((e = alloc(static_cast<size_t>(S.idCap) * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    S.outIdx = static_cast<uint32_t*>(p);
  }
  S.mkIds = nullptr;
  S.mkCap = 0;
  if (c->mtNRelpos) {
    if ((e = alloc(static_cast<size_t>(S.idCap) * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    S.mkIds = static_cast<uint32_t*>(p);
    S.mkCap = S.idCap;
  }
  // remove-order entries (SnapshotV1) go to the document's slab too
  I.rmOrder = nullptr;
  I.rmOrderCap = 0;
  S.rmIds = nullptr;
  if (c->mtPlan.hasRmOrder() && c->mtPlan.rmOffs[d + 1] > c->mtPlan.rmOffs[d]) {
    I.rmOrder = c->mtRmOrder.p + c->mtPlan.rmOffs[d];
    I.rmOrderCap = static_cast<uint32_t>(std::min<uint64_t>(c->mtPlan.rmOffs[d + 1] - c->mtPlan.rmOffs[d], 0xFFFFFFFFull));
    if ((e = alloc(static_cast<size_t>(S.idCap) * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    S.rmIds = static_cast<uint32_t*>(p);
  }
  I.shape = nullptr;
  if (!H.shape.empty()) {
    if ((e = alloc(H.shape.size() * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    FMT_HIP(c, hipMemcpyAsync(p, H.shape.data(), H.shape.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    I.shape = static_cast<const uint32_t*>(p);
  }
  I.snapMinSeq = minSeq;
  I.snapSeq = seq;
  I.initClient = initClient;
  fmt_kernels::HugeOut& O = H.out;
  O.header = c->mtHdr.p + d;
  O.capLeaves = N + 3 * nOps + 8;
  O.capChars = docChars + 8;  // (every unit the document can hold: its start plus its inserts)
  if ((e = alloc(O.capLeaves * sizeof(fmt_mt_leaf), &p)) != hipSuccess) return drop(e);
  O.leaves = static_cast<fmt_mt_leaf*>(p);
  if ((e = alloc(O.capChars * sizeof(uint16_t), &p)) != hipSuccess) return drop(e);
  O.chars = static_cast<uint16_t*>(p);
  if ((e = alloc(fmt_huge::kPropCap * sizeof(fmt_mt_propset), &p)) != hipSuccess) return drop(e);
  O.props = static_cast<fmt_mt_propset*>(p);
  O.cls = S.pClass;
  O.legacy = nullptr;  // annotate-adjust batches: per leaf the getAtSeq(minSeq) prop set
  if (c->mtPlan.anyAdjust) {
    if ((e = alloc(O.capLeaves * sizeof(uint16_t), &p)) != hipSuccess) return drop(e);
    O.legacy = static_cast<uint16_t*>(p);
  }
  if ((e = alloc(fmt_huge::HugeDoc::kProf * sizeof(unsigned long long), &p)) != hipSuccess) return drop(e);
  O.prof = static_cast<unsigned long long*>(p);
  // live obliterates: at most one per op of the document is alive at once (HBM; batches with obliterates)
  S.obRec = S.obUsed = S.obSeq = S.obStart = nullptr;
  S.obCap = 0;
  if (c->mtPlan.obliterates && nOps > 0) {
    if (nOps > 0x0FFFFFFFull) return drop(hipErrorOutOfMemory);
    S.obCap = static_cast<uint32_t>(std::max<uint64_t>(nOps, fmt_ckpt::kObSlots));  // (a checkpoint keeps its slot ids)
    if ((e = alloc(9ull * S.obCap * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    S.obRec = static_cast<uint32_t*>(p);
    S.obUsed = S.obRec + 6ull * S.obCap;
    S.obSeq = S.obUsed + S.obCap;
    S.obStart = S.obSeq + S.obCap;
  }
  // remove clients 64..253: the per-leaf-id side table (zeroed, kHiWords words per id) and its per-leaf
  // output (kHiOutWords 64-bit words per leaf: ids 64..127, 128..191, 192..253)
  S.hiMask = nullptr;
  O.leavesHi = nullptr;
  if (c->mtPlan.hiClients) {
    constexpr size_t kW = fmt_huge::kHiWords;
    if ((e = alloc(kW * S.idCap * sizeof(uint32_t), &p)) != hipSuccess) return drop(e);
    FMT_HIP(c, hipMemsetAsync(p, 0, kW * S.idCap * sizeof(uint32_t), c->stream));
    S.hiMask = static_cast<uint32_t*>(p);
    if ((e = alloc(O.capLeaves * fmt_huge::kHiOutWords * sizeof(uint64_t), &p)) != hipSuccess) return drop(e);
    O.leavesHi = static_cast<uint64_t*>(p);
  }
  return FMT_OK;
}

// The descriptors of huge documents c->huge[first ..) as the arrays launchHugeDocs takes.
static int uploadHuge(fmt_ctx* c, size_t first, DevBuf<fmt_huge::HugeState>& states, DevBuf<fmt_huge::HugeInputs>& inputs,
                      DevBuf<fmt_kernels::HugeOut>& outs) {
  const size_t nh = c->huge.size() - first;
  if (nh == 0) return FMT_OK;
  FMT_HIP(c, states.reserve(nh));
  FMT_HIP(c, inputs.reserve(nh));
  FMT_HIP(c, outs.reserve(nh));
  std::vector<fmt_huge::HugeState> hs(nh);
  std::vector<fmt_huge::HugeInputs> hi(nh);
  std::vector<fmt_kernels::HugeOut> ho(nh);
  for (size_t i = 0; i < nh; i++) {
    hs[i] = c->huge[first + i].state;
    hi[i] = c->huge[first + i].in;
    ho[i] = c->huge[first + i].out;
  }
  FMT_HIP(c, hipMemcpyAsync(states.p, hs.data(), nh * sizeof(fmt_huge::HugeState), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipMemcpyAsync(inputs.p, hi.data(), nh * sizeof(fmt_huge::HugeInputs), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipMemcpyAsync(outs.p, ho.data(), nh * sizeof(fmt_kernels::HugeOut), hipMemcpyHostToDevice, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));  // (hs / hi / ho are about to go out of scope)
  return FMT_OK;
}

// Plan (mt_plan.h: validation, slab sizing, routing; no device) then stage. A batch the plan refuses
// leaves the context as it was: the batch loaded before stays loaded and runnable.
int fmt_mt_load(fmt_ctx* c, const fmt_mt_batch* b) {
  if (c == nullptr) return FMT_E_USAGE;
  const fmt_kernels::MtCaps caps = fmt_kernels::mergeTreeCaps(false);
  const char* why = nullptr;
  // (the plan is built aside and moves into c->mtPlan only when the batch is valid)
  const int planned = fmt_plan::planMergeTreeLoad(b, fmt_kernels::mergeTreeCaps(true), c->mtPlan, &why);
  if (planned != FMT_OK) return setErr(c, planned, why);
  const fmt_plan::MtPlan& P = c->mtPlan;
  c->mtLoaded = false;  // (from here on the context holds this batch or, after a device error, none)
  c->mtRan = false;
  invalidateReads(c);
  const uint32_t n = b->n_docs;
  const uint32_t nKv = b->props_off ? b->props_off[b->n_props_ops] : 0;
  // host arrays the asynchronous copies below read; the stream is drained before they go, on every way out
  fmt_mt::AdjustTables adjTab{};
  fmt_mt::LocalTables locTab{};
  std::vector<fmt_mt_doc_result> refusedHdr;
  std::vector<uint32_t> small;
  struct Drain {
    hipStream_t stream;
    ~Drain() { (void)hipStreamSynchronize(stream); }
  } drain{c->stream};
  auto cp = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
  };
  FMT_HIP(c, hipSetDevice(c->device));
  FMT_HIP(c, c->mtOps.reserve(b->n_ops));
  FMT_HIP(c, c->mtOffs.reserve(n + 1ull));
  FMT_HIP(c, c->mtText.reserve(b->text_len));
  FMT_HIP(c, c->mtInit.reserve(2ull * n));
  FMT_HIP(c, c->mtPropsOff.reserve(b->n_props_ops + 1ull));
  FMT_HIP(c, c->mtPropsKv.reserve(nKv));
  FMT_HIP(c, c->mtHdr.reserve(n));
  FMT_HIP(c, c->mtLeaves.reserve(static_cast<size_t>(n) * caps.leaves));
  FMT_HIP(c, c->mtChars.reserve(static_cast<size_t>(n) * caps.chars));
  FMT_HIP(c, c->mtProps.reserve(static_cast<size_t>(n) * caps.props));
  FMT_HIP(c, c->mtListBuf.reserve(4 + 4 * (n + 1ull)));
  c->mtBigSlot.assign(n, -1);
  // catch-up and remove-order slabs (sizes: mt_plan.h catchupSlab / rmOrderSlab)
  if (P.hasCatchup()) {
    FMT_HIP(c, c->mtCuOffs.reserve(n + 1ull));
    FMT_HIP(c, c->mtCatchup.reserve(P.cuOffs[n]));
    FMT_HIP(c, cp(c->mtCuOffs.p, P.cuOffs.data(), (n + 1ull) * sizeof(uint64_t)));
  }
  if (P.hasRmOrder()) {
    FMT_HIP(c, c->mtRmOffs.reserve(n + 1ull));
    FMT_HIP(c, c->mtRmOrder.reserve(P.rmOffs[n]));
    FMT_HIP(c, cp(c->mtRmOffs.p, P.rmOffs.data(), (n + 1ull) * sizeof(uint64_t)));
  }
  // annotate-adjust: the rows, the host numbers (plain and sorted for number → id lookups), and the
  // per-document computed-number and PropertiesManager slabs (mt_plan.h numberSlab / pmSlab)
  if (b->doc_value_base != nullptr) c->mtValueBaseHost.assign(b->doc_value_base, b->doc_value_base + n + 1);
  else c->mtValueBaseHost.clear();
  if (P.anyAdjust) {
    const uint32_t nValues = b->value_num ? b->n_values : 0u;
    FMT_HIP(c, c->mtAdjusts.reserve(b->n_adjusts));
    FMT_HIP(c, c->mtValueNum.reserve(nValues));
    FMT_HIP(c, c->mtNumSorted.reserve(P.numSorted.size()));
    FMT_HIP(c, c->mtNumSortedId.reserve(P.numSortedId.size()));
    FMT_HIP(c, c->mtNumOffs.reserve(n + 1ull));
    FMT_HIP(c, c->mtNums.reserve(P.numOffs[n]));
    FMT_HIP(c, c->mtNumCount.reserve(n));
    FMT_HIP(c, c->mtPmOffs.reserve(n + 1ull));
    FMT_HIP(c, c->mtPm.reserve(4 * P.pmOffs[n]));
    FMT_HIP(c, c->mtLegacy.reserve(static_cast<size_t>(n) * caps.leaves));
    FMT_HIP(c, cp(c->mtPmOffs.p, P.pmOffs.data(), (n + 1ull) * sizeof(uint64_t)));
    FMT_HIP(c, cp(c->mtAdjusts.p, b->adjusts, b->n_adjusts * sizeof(fmt_mt_adjust)));
    FMT_HIP(c, cp(c->mtValueNum.p, b->value_num, nValues * sizeof(double)));
    FMT_HIP(c, cp(c->mtNumSorted.p, P.numSorted.data(), P.numSorted.size() * sizeof(double)));
    FMT_HIP(c, cp(c->mtNumSortedId.p, P.numSortedId.data(), P.numSortedId.size() * sizeof(uint32_t)));
    if (b->doc_value_base != nullptr) {
      FMT_HIP(c, c->mtValueBase.reserve(n + 1ull));
      FMT_HIP(c, c->mtNumSortedOffs.reserve(n + 1ull));
      FMT_HIP(c, cp(c->mtValueBase.p, b->doc_value_base, (n + 1ull) * sizeof(uint32_t)));
      FMT_HIP(c, cp(c->mtNumSortedOffs.p, P.numSortedOffs.data(), (n + 1ull) * sizeof(uint32_t)));
    }
    FMT_HIP(c, cp(c->mtNumOffs.p, P.numOffs.data(), (n + 1ull) * sizeof(uint64_t)));
    FMT_HIP(c, hipMemsetAsync(c->mtNumCount.p, 0, n * sizeof(uint32_t), c->stream));
    fmt_mt::AdjustTables& T = adjTab;
    T.adjusts = c->mtAdjusts.p;
    T.nAdjusts = b->n_adjusts;
    T.nValues = nValues;
    T.valueNum = c->mtValueNum.p;
    T.numSorted = c->mtNumSorted.p;
    T.numSortedId = c->mtNumSortedId.p;
    T.valueBase = b->doc_value_base != nullptr ? c->mtValueBase.p : nullptr;
    T.numSortedOffs = b->doc_value_base != nullptr ? c->mtNumSortedOffs.p : nullptr;
    T.nNumSorted = static_cast<uint32_t>(P.numSorted.size());
    T.nums = c->mtNums.p;
    T.numOffsets = c->mtNumOffs.p;
    T.numCount = c->mtNumCount.p;
    T.pm = c->mtPm.p;
    T.pmOffsets = c->mtPmOffs.p;
    FMT_HIP(c, c->mtAdjTab.reserve(1));
    FMT_HIP(c, cp(c->mtAdjTab.p, &T, sizeof T));
  }
  // f4: the per-document slabs of the local records (mt_plan.h localSlabs)
  if (P.local) {
    const uint64_t n1 = n + 1ull;
    FMT_HIP(c, c->mtLocOffs.reserve(P.locOffs.size()));
    FMT_HIP(c, c->mtLocGroups.reserve(8 * P.locSlabOffs(fmt_plan::kLocGroups)[n]));
    FMT_HIP(c, c->mtLocRecs.reserve(2 * P.locSlabOffs(fmt_plan::kLocRecs)[n]));
    FMT_HIP(c, c->mtLocPm.reserve(4 * P.locSlabOffs(fmt_plan::kLocPm)[n]));
    FMT_HIP(c, c->mtLocRegen.reserve(P.locSlabOffs(fmt_plan::kLocRegen)[n]));
    FMT_HIP(c, c->mtLocRegenText.reserve(P.locSlabOffs(fmt_plan::kLocRegenText)[n]));
    FMT_HIP(c, c->mtLocScratch.reserve(P.locSlabOffs(fmt_plan::kLocScratch)[n]));
    FMT_HIP(c, c->mtLocRegenCount.reserve(2ull * n));
    FMT_HIP(c, c->mtLocTab.reserve(1));
    FMT_HIP(c, cp(c->mtLocOffs.p, P.locOffs.data(), P.locOffs.size() * sizeof(uint64_t)));
    FMT_HIP(c, hipMemsetAsync(c->mtLocRegenCount.p, 0, 2ull * n * sizeof(uint32_t), c->stream));
    const uint64_t* O = c->mtLocOffs.p;
    locTab = fmt_mt::LocalTables{c->mtLocGroups.p, O + fmt_plan::kLocGroups * n1, c->mtLocRecs.p, O + fmt_plan::kLocRecs * n1,
                                 c->mtLocPm.p, O + fmt_plan::kLocPm * n1, c->mtLocRegen.p, O + fmt_plan::kLocRegen * n1,
                                 c->mtLocRegenText.p, O + fmt_plan::kLocRegenText * n1, c->mtLocRegenCount.p,
                                 c->mtLocScratch.p, O + fmt_plan::kLocScratch * n1};
    FMT_HIP(c, cp(c->mtLocTab.p, &locTab, sizeof locTab));
  }
  FMT_HIP(c, stagedCopy(c, c->mtOps.p, b->ops, b->n_ops * sizeof(fmt_mt_op), true));
  FMT_HIP(c, cp(c->mtOffs.p, b->doc_op_offsets, (n + 1ull) * sizeof(uint64_t)));
  FMT_HIP(c, stagedCopy(c, c->mtText.p, b->text, b->text_len * sizeof(uint16_t), true));
  if (b->doc_init) FMT_HIP(c, cp(c->mtInit.p, b->doc_init, 2ull * n * sizeof(uint32_t)));
  c->mtHasSnap = b->snapshots != nullptr;
  if (c->mtHasSnap) {
    FMT_HIP(c, c->mtSnap.reserve(n));
    FMT_HIP(c, c->mtSnapSegs.reserve(b->n_snapshot_segs));
    FMT_HIP(c, cp(c->mtSnap.p, b->snapshots, n * sizeof(fmt_mt_snapshot_doc)));
    FMT_HIP(c, stagedCopy(c, c->mtSnapSegs.p, b->snapshot_segs, b->n_snapshot_segs * sizeof(fmt_mt_snapshot_seg), true));
  }
  c->mtHasSnapInfo = c->mtHasSnap && b->snapshot_info != nullptr;
  c->mtNSnapSegs = b->n_snapshot_segs;
  if (c->mtHasSnapInfo) {
    FMT_HIP(c, c->mtSnapInfo.reserve(b->n_snapshot_segs));
    FMT_HIP(c, c->mtSnapStamps.reserve(b->n_snapshot_stamps));
    FMT_HIP(c, cp(c->mtSnapInfo.p, b->snapshot_info, b->n_snapshot_segs * sizeof(fmt_mt_snapshot_info)));
    FMT_HIP(c, cp(c->mtSnapStamps.p, b->snapshot_stamps, b->n_snapshot_stamps * sizeof(fmt_mt_stamp)));
  }
  c->mtNRelpos = b->relpos ? b->n_relpos : 0u;
  c->mtMarkerKey = b->marker_id_key;
  if (c->mtNRelpos) {
    FMT_HIP(c, c->mtRelpos.reserve(c->mtNRelpos));
    FMT_HIP(c, cp(c->mtRelpos.p, b->relpos, c->mtNRelpos * sizeof(fmt_mt_relpos)));
  }
  if (b->props_off) {
    FMT_HIP(c, cp(c->mtPropsOff.p, b->props_off, (b->n_props_ops + 1ull) * sizeof(uint32_t)));
    FMT_HIP(c, cp(c->mtPropsKv.p, b->props_kv, nKv * sizeof(uint32_t)));
  } else {
    FMT_HIP(c, hipMemsetAsync(c->mtPropsOff.p, 0, sizeof(uint32_t), c->stream));
  }
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->mtNOps = b->n_ops;
  c->mtDocs = n;
  c->mtTextLen = b->text_len;
  c->mtNProps = b->n_props_ops;
  c->mtOffsHost.assign(b->doc_op_offsets, b->doc_op_offsets + n + 1);
  if (b->snapshots) c->mtSnapHost.assign(b->snapshots, b->snapshots + n);
  else c->mtSnapHost.clear();
  c->mtHasInit = b->doc_init != nullptr;
  // A batch without remove-order recording starts in the micro tier (with obliterates: the compact
  // tier); a document about to outgrow a tier stops at a checkpoint (one slot of ≈17 KiB per document)
  // that the next tier resumes from.
  c->mtCkptOk = false;
  if (!P.hasRmOrder()) {
    // (a batch too large for the checkpoints still replays: overflowing documents then restart in
    // the next tier from their first op, as batches with obliterates do)
    c->mtCkptOk = c->mtCkpt.reserve(static_cast<size_t>(n) * (fmt_kernels::mergeTreeCheckpointBytes() / sizeof(uint32_t))) ==
                  hipSuccess;
    if (!c->mtCkptOk) (void)hipGetLastError();
  }
  // plain batches with checkpoints: the lists of the rounds in which documents step down a tier
  size_t descWords = 0;
  if (fmt_plan::routeUsesDescSlab(P, c->mtCkptOk)) {
    descWords = fmt_plan::mergeTreeDescendWords(n);
    if (c->mtDesc.reserve(descWords) != hipSuccess) {
      (void)hipGetLastError();
      descWords = 0;
    }
  }
  c->mtRoute = fmt_plan::planRoute(P, c->mtCkptOk, descWords > 0);
  // Huge documents: a summary-loaded document with more segments or text than the large tier holds
  // is replayed by the huge-document engine (huge_engine.h: one wave, state in HBM). One the plan
  // refused (local-client records), or whose state does not fit in device memory, fails alone at load
  // (its header says why) and the rest of the batch replays.
  for (auto& h : c->huge)
    for (void* p : h.allocs) (void)hipFree(p);
  c->huge.clear();
  c->mtHugeSlot.assign(n, -1);
  c->mtRefused = P.refused;
  c->mtRefusedHdr.clear();
  refusedHdr = P.refusedHdr;
  for (uint32_t d : P.hugeDocs) {
    const fmt_mt_snapshot_doc& sd = b->snapshots[d];
    const int rc = setupHugeDoc(c, b->text_len, b->n_props_ops, d, b->doc_op_offsets[d], b->doc_op_offsets[d + 1],
                                c->mtSnapSegs.p + sd.first_seg, sd.n_header, sd.n_body, sd.min_seq, sd.seq,
                                FMT_NON_COLLAB_CLIENT, 256, P.docChars[d]);
    if (rc == FMT_E_CAPACITY) {
      c->mtRefused.push_back(d);
      refusedHdr.push_back(fmt_plan::refusalHeader(sd, FMT_E_CAPACITY));
    } else if (rc != FMT_OK) {
      return rc;
    }
  }
  for (size_t i = 0; i < c->mtRefused.size(); i++)
    FMT_HIP(c, cp(c->mtHdr.p + c->mtRefused[i], &refusedHdr[i], sizeof(fmt_mt_doc_result)));
  c->mtRefusedHdr = refusedHdr;
  c->mtHugeLoaded = static_cast<uint32_t>(c->huge.size());
  // the small tiers run the other documents from a list
  c->mtUseList = !c->huge.empty() || !c->mtRefused.empty();
  if (c->mtUseList) {
    std::vector<uint8_t> skip(n, 0);
    for (uint32_t d : c->mtRefused) skip[d] = 1;
    for (uint32_t d = 0; d < n; d++)
      if (c->mtHugeSlot[d] < 0 && !skip[d]) small.push_back(d);
    c->mtNSmall = static_cast<uint32_t>(small.size());
    FMT_HIP(c, c->mtSmallList.reserve(small.size()));
    FMT_HIP(c, cp(c->mtSmallList.p, small.data(), small.size() * sizeof(uint32_t)));
  }
  {  // (mtListBuf: the counters, then toLarge, microUp, compactUp, ordered)
    uint32_t* w = c->mtListBuf.p;
    const size_t stride = n + 1ull;
    c->mtLists = fmt_kernels::MtLists{w + 4, w + 4 + stride, w + 4 + 2 * stride, w + 4 + 3 * stride, w,
                                      descWords > 0 ? c->mtDesc.p : nullptr, descWords,
                                      c->mtUseList ? c->mtSmallList.p : nullptr, c->mtUseList ? c->mtNSmall : 0u};
  }
  const int rc = uploadHuge(c, 0, c->hugeStates, c->hugeInputs, c->hugeOuts);
  if (rc != FMT_OK) return rc;
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->mtLoaded = true;
  return FMT_OK;
}

// ------------------------------------------------------------------ fmt_mt_run, in parts
static fmt_kernels::MtDeviceBatch mtBatchView(const fmt_ctx* c) {
  return fmt_kernels::MtDeviceBatch{c->mtOps.p, c->mtOffs.p, c->mtDocs, c->mtText.p,
                                    c->mtHasInit ? c->mtInit.p : nullptr, c->mtPropsOff.p, c->mtPropsKv.p, c->mtNProps,
                                    c->mtPlan.hasCatchup() ? c->mtCuOffs.p : nullptr,
                                    c->mtHasSnap ? c->mtSnap.p : nullptr, c->mtHasSnap ? c->mtSnapSegs.p : nullptr,
                                    c->mtPlan.hasRmOrder() ? c->mtRmOffs.p : nullptr,
                                    c->mtHasSnapInfo ? c->mtSnapInfo.p : nullptr, c->mtHasSnapInfo ? c->mtSnapStamps.p : nullptr,
                                    c->mtHasSnapInfo ? c->mtNSnapSegs : 0u, c->mtNRelpos ? c->mtRelpos.p : nullptr,
                                    c->mtNRelpos, c->mtMarkerKey, c->mtPlan.anyAdjust ? c->mtAdjTab.p : nullptr,
                                    c->mtPlan.local ? c->mtLocTab.p : nullptr};
}

// What a launch writes to, from the route's booleans: the register tiers' slabs, or the large pass's.
static fmt_kernels::MtDeviceOut mtOutView(const fmt_ctx* c, bool large, uint32_t* hugeCk = nullptr) {
  const fmt_plan::MtRoute& R = c->mtRoute;
  const bool ckpt = large ? R.largeCkpt : R.tiersCkpt, small = large && R.largeResumesSmall;
  return fmt_kernels::MtDeviceOut{c->mtHdr.p, large ? c->mtBigLeaves.p : c->mtLeaves.p, large ? c->mtBigChars.p : c->mtChars.p,
                                  large ? c->mtBigProps.p : c->mtProps.p, c->mtPlan.hasCatchup() ? c->mtCatchup.p : nullptr,
                                  c->mtPlan.hasRmOrder() ? c->mtRmOrder.p : nullptr, ckpt ? c->mtCkpt.p : nullptr,
                                  small ? c->mtLeaves.p : nullptr, small ? c->mtChars.p : nullptr,
                                  !c->mtPlan.anyAdjust ? nullptr : large ? c->mtBigLegacy.p : c->mtLegacy.p, hugeCk};
}

// The list heads, the per-tier dealing counters and the step-down slab, zeroed for a run.
static int zeroMtLists(fmt_ctx* c) {
  const fmt_kernels::MtLists& L = c->mtLists;
  for (uint32_t* head : {L.toLarge, L.microUp, L.compactUp}) FMT_HIP(c, hipMemsetAsync(head, 0, sizeof(uint32_t), c->stream));
  FMT_HIP(c, hipMemsetAsync(L.sched, 0, 4 * sizeof(uint32_t), c->stream));
  if (L.descWords > 0) FMT_HIP(c, hipMemsetAsync(L.desc, 0, L.descWords * sizeof(uint32_t), c->stream));
  return FMT_OK;
}

// Documents an earlier run escalated into the huge tier start over: only the load-time ones (mtHugeLoaded) stay.
static int releaseGrownHuge(fmt_ctx* c) {
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t h = c->mtHugeLoaded; h < c->huge.size(); h++)
    for (void* q : c->huge[h].allocs) (void)hipFree(q);
  for (uint32_t d = 0; d < c->mtDocs; d++)
    if (c->mtHugeSlot[d] >= static_cast<int32_t>(c->mtHugeLoaded)) c->mtHugeSlot[d] = -1;
  c->huge.resize(c->mtHugeLoaded);
  return FMT_OK;
}

// The route's register tiers (mt_route.h) and the load-time huge documents, between ev0 and ev1.
static int launchRegisterTiers(fmt_ctx* c, const fmt_kernels::MtDeviceBatch& db) {
  if (const int rc = zeroMtLists(c)) return rc;
  FMT_HIP(c, hipEventRecord(c->ev0, c->stream));
  if (!c->mtUseList || c->mtNSmall > 0)
    FMT_HIP(c, fmt_kernels::launchMergeTree(db, mtOutView(c, false), c->mtRoute, c->mtLists, {c->numCUs, c->stream}));
  if (c->mtHugeLoaded > 0)
    FMT_HIP(c, fmt_kernels::launchHugeDocs(c->hugeStates.p, c->hugeInputs.p, c->hugeOuts.p, c->mtHugeLoaded, c->mtPlan.anyAdjust, c->mtPlan.hasRmOrder(), c->stream));
  FMT_HIP(c, hipEventRecord(c->ev1, c->stream));  // device time excludes the host read-back below
  c->timed2 = false;
  return FMT_OK;
}

// The nEsc > 0 documents the register tiers left replay in the large tier, between ev2 and ev3 (list: their ids).
static int runLargePass(fmt_ctx* c, const fmt_kernels::MtDeviceBatch& db, uint32_t nEsc, std::vector<uint32_t>& list) {
  const fmt_kernels::MtCaps big = fmt_kernels::mergeTreeCaps(true);
  FMT_HIP(c, c->mtBigLeaves.reserve(static_cast<size_t>(nEsc) * big.leaves));
  FMT_HIP(c, c->mtBigChars.reserve(static_cast<size_t>(nEsc) * big.chars));
  FMT_HIP(c, c->mtBigProps.reserve(static_cast<size_t>(nEsc) * big.props));
  if (c->mtPlan.anyAdjust) FMT_HIP(c, c->mtBigLegacy.reserve(static_cast<size_t>(nEsc) * big.leaves));
  // every batch but a local one: a document the large tier is about to outgrow leaves a checkpoint
  // for the huge tier (huge_ckpt.h) instead of failing; without the slab it restarts there from its
  // first op
  const bool hugeCk = c->mtRoute.largeHugeCkpt &&
                      c->mtHugeCk.reserve(static_cast<size_t>(nEsc) * fmt_ckpt::kWords) == hipSuccess;
  if (!hugeCk) (void)hipGetLastError();
  FMT_HIP(c, hipEventRecord(c->ev2, c->stream));
  FMT_HIP(c, fmt_kernels::launchMergeTreeLarge(db, mtOutView(c, true, hugeCk ? c->mtHugeCk.p : nullptr), c->mtRoute,
                                               c->mtLists, nEsc, {c->numCUs, c->stream}));
  FMT_HIP(c, hipEventRecord(c->ev3, c->stream));
  c->timed2 = true;
  list.resize(nEsc);
  FMT_HIP(c, hipMemcpyAsync(list.data(), c->mtLists.toLarge + 1, nEsc * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < nEsc; i++) c->mtBigSlot[list[i]] = static_cast<int32_t>(i);
  return FMT_OK;
}

// Documents the large tier could not hold (FMT_E_CAPACITY: leaves, text, blocks, prop sets) replay
// again in the huge tier, which has no such limit but device memory — the reference grows a tree
// without bound (insertSegments, mergeTree.ts:1484-1517): from the checkpoint the large pass left
// them at, or from their start. Not a local batch's (the huge tier lacks its records).
static int growIntoHuge(fmt_ctx* c, const std::vector<uint32_t>& list) {
  const uint32_t nEsc = static_cast<uint32_t>(list.size());
  const fmt_kernels::MtCaps big = fmt_kernels::mergeTreeCaps(true);
  std::vector<fmt_mt_doc_result> hb(nEsc);
  std::vector<uint32_t> grow;
  std::vector<int32_t> growSlot;  // the large-tier slot of a checkpointed document (-1: restart from op 0)
  for (uint32_t i = 0; i < nEsc; i++) {
    FMT_HIP(c, hipMemcpyAsync(&hb[i], c->mtHdr.p + list[i], sizeof(fmt_mt_doc_result), hipMemcpyDeviceToHost, c->stream));
  }
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < nEsc; i++) {
    if ((hb[i].status == FMT_E_CAPACITY || hb[i].status == fmt_ckpt::kStatusHuge) && c->mtHugeSlot[list[i]] < 0 &&
        !c->mtRoute.largeLocal) {
      grow.push_back(list[i]);
      growSlot.push_back(hb[i].status == fmt_ckpt::kStatusHuge ? static_cast<int32_t>(i) : -1);
    }
  }
  if (grow.empty()) return FMT_OK;
  FMT_HIP(c, c->mtStartSegDev.reserve(grow.size()));
  std::vector<fmt_mt_snapshot_seg> starts(grow.size());
  for (size_t i = 0; i < grow.size(); i++) starts[i] = c->mtPlan.startSeg[grow[i]];
  FMT_HIP(c, hipMemcpyAsync(c->mtStartSegDev.p, starts.data(), grow.size() * sizeof(fmt_mt_snapshot_seg),
                            hipMemcpyHostToDevice, c->stream));
  // (a document whose huge-tier state does not fit in device memory keeps the large tier's
  // FMT_E_CAPACITY header)
  for (size_t i = 0; i < grow.size(); i++) {
    const uint32_t d = grow[i];
    const uint64_t o0 = c->mtOffsHost[d], o1 = c->mtOffsHost[d + 1];
    int rc;
    if (c->mtSnapHost.size() > d && c->mtSnapHost[d].loaded) {
      const fmt_mt_snapshot_doc& sd = c->mtSnapHost[d];
      rc = setupHugeDoc(c, c->mtTextLen, c->mtNProps, d, o0, o1, c->mtSnapSegs.p + sd.first_seg, sd.n_header,
                        sd.n_body, sd.min_seq, sd.seq, FMT_NON_COLLAB_CLIENT, 1024, c->mtPlan.docChars[d]);
    } else {
      rc = setupHugeDoc(c, c->mtTextLen, c->mtNProps, d, o0, o1, c->mtStartSegDev.p + i, starts[i].len > 0 ? 1 : 0,
                        0, 0, 0, FMT_LOCAL_CLIENT, 1024, c->mtPlan.docChars[d]);
    }
    if (rc != FMT_OK && rc != FMT_E_CAPACITY) return rc;
    if (growSlot[i] >= 0) {
      if (rc == FMT_OK) {  // resume from the large tier's checkpoint and result slabs
        const size_t k = static_cast<size_t>(growSlot[i]);
        fmt_huge::HugeInputs& I = c->huge.back().in;
        I.ck = c->mtHugeCk.p + k * fmt_ckpt::kWords;
        I.ckLeaves = c->mtBigLeaves.p + k * big.leaves;
        I.ckChars = c->mtBigChars.p + k * big.chars;
        I.ckProps = c->mtBigProps.p + k * big.props;
      } else {  // (no room in device memory: the document reports FMT_E_CAPACITY)
        const int32_t st = FMT_E_CAPACITY;
        FMT_HIP(c, hipMemcpyAsync(&c->mtHdr.p[d].status, &st, sizeof st, hipMemcpyHostToDevice, c->stream));
        FMT_HIP(c, hipStreamSynchronize(c->stream));
      }
    }
  }
  const size_t ng = c->huge.size() - c->mtHugeLoaded;
  if (ng > 0) {
    const int rc = uploadHuge(c, c->mtHugeLoaded, c->hugeStates2, c->hugeInputs2, c->hugeOuts2);
    if (rc != FMT_OK) return rc;
    FMT_HIP(c, fmt_kernels::launchHugeDocs(c->hugeStates2.p, c->hugeInputs2.p, c->hugeOuts2.p, static_cast<uint32_t>(ng),
                                           c->mtPlan.anyAdjust, c->mtPlan.hasRmOrder(), c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  c->mtGrown = static_cast<uint32_t>(ng);
  return FMT_OK;
}


int fmt_mt_run(fmt_ctx* c) {
  if (c == nullptr || !c->mtLoaded) return setErr(c, FMT_E_USAGE, "fmt_mt_run before fmt_mt_load");
  c->mtRan = false;  // (until this run completes: a device error half way leaves nothing to fetch)
  invalidateReads(c);
  FMT_HIP(c, hipSetDevice(c->device));
  if (const int rc = releaseGrownHuge(c)) return rc;
  const fmt_kernels::MtDeviceBatch db = mtBatchView(c);
  if (const int rc = launchRegisterTiers(c, db)) return rc;
  // Documents that overflowed the small tier replay again in the large tier: the host reads the list length.
  uint32_t nEsc = 0;
  c->mtGrown = 0;
  FMT_HIP(c, hipMemcpyAsync(&nEsc, c->mtLists.toLarge, sizeof nEsc, hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  c->mtBigSlot.assign(c->mtDocs, -1);
  if (nEsc > 0) {
    std::vector<uint32_t> list;
    if (const int rc = runLargePass(c, db, nEsc, list)) return rc;
    if (const int rc = growIntoHuge(c, list)) return rc;
  }
  c->timed = true;
  c->stats = fmt_stats{};
  c->stats.ops = c->mtNOps;
  c->stats.docs = c->mtDocs;
  // Algorithmic bytes: every op record and every inserted UTF-16 unit read once; results written
  // (headers + leaves + chars + prop sets) are added by fmt_mt_fetch_headers once sizes are known.
  c->stats.bytes_read = c->mtNOps * sizeof(fmt_mt_op) + (c->mtPlan.insertChars + c->mtPlan.initChars) * 2 +
                        (c->mtDocs + 1ull) * sizeof(uint64_t);
  c->stats.bytes_written = static_cast<uint64_t>(c->mtDocs) * sizeof(fmt_mt_doc_result);
  c->stats.launches = c->mtRoute.nominalLaunches(nEsc > 0, c->mtGrown > 0);
  c->mtRan = true;
  return FMT_OK;
}

int fmt_mt_fetch_headers(fmt_ctx* c, fmt_mt_doc_result* out) {
  if (c == nullptr || out == nullptr || !c->mtLoaded) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_headers: nothing loaded");
  if (!c->mtRan) {
    // Before a run (fmt.h "Call order"): what the load decided, from the host. mtHdr still holds an
    // earlier batch's headers, or nothing.
    std::memset(out, 0, c->mtDocs * sizeof(fmt_mt_doc_result));
    for (size_t i = 0; i < c->mtRefused.size(); i++) out[c->mtRefused[i]] = c->mtRefusedHdr[i];
  } else {
    FMT_HIP(c, hipMemcpyAsync(out, c->mtHdr.p, c->mtDocs * sizeof(fmt_mt_doc_result), hipMemcpyDeviceToHost, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  uint64_t w = static_cast<uint64_t>(c->mtDocs) * sizeof(fmt_mt_doc_result);
  int status = FMT_OK;
  for (uint32_t d = 0; d < c->mtDocs; d++) {
    w += out[d].n_leaves * sizeof(fmt_mt_leaf) + out[d].n_chars * 2ull + out[d].n_props * sizeof(fmt_mt_propset);
    if (out[d].status != FMT_OK && status == FMT_OK) {
      status = out[d].status;
      char m[160];
      std::snprintf(m, sizeof m, "doc %u failed with status %d at seq %d", d, out[d].status, out[d].fail_seq);
      c->err = m;
    }
  }
  c->stats.bytes_written = w;
  return status;
}

int fmt_mt_fetch_doc(fmt_ctx* c, uint32_t doc, fmt_mt_leaf* leaves, uint32_t capLeaves, uint16_t* chars,
                     uint32_t capChars, fmt_mt_propset* props, uint32_t capProps) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs, "fmt_mt_fetch_doc", "fmt_mt_fetch_doc: bad doc")) return rc;
  const fmt_kernels::SumView V = docView(c, doc);
  fmt_mt_doc_result h;
  FMT_HIP(c, hipMemcpy(&h, c->mtHdr.p + doc, sizeof h, hipMemcpyDeviceToHost));
  const uint32_t nl = h.n_leaves < capLeaves ? h.n_leaves : capLeaves;
  const uint32_t nc = h.n_chars < capChars ? h.n_chars : capChars;
  const uint32_t np = h.n_props < capProps ? h.n_props : capProps;
  if (leaves && nl) FMT_HIP(c, hipMemcpy(leaves, V.leaves, nl * sizeof(fmt_mt_leaf), hipMemcpyDeviceToHost));
  if (chars && nc) FMT_HIP(c, hipMemcpy(chars, V.chars, nc * 2ull, hipMemcpyDeviceToHost));
  if (props && np) FMT_HIP(c, hipMemcpy(props, V.props, np * sizeof(fmt_mt_propset), hipMemcpyDeviceToHost));
  return FMT_OK;
}

// ------------------------------------------------------------------ bulk legacy summaries
namespace {

// JSON.stringify of a UTF-16 string (well-formed: lone surrogates as \udXXX), as UTF-8.
void jsonQuote16(std::string& o, const uint16_t* s, size_t n) {
  static const char* hex = "0123456789abcdef";
  o.push_back('"');
  for (size_t i = 0; i < n; i++) {
    const uint32_t c = s[i];
    if (c == '"') o += "\\\"";
    else if (c == '\\') o += "\\\\";
    else if (c == '\b') o += "\\b";
    else if (c == '\f') o += "\\f";
    else if (c == '\n') o += "\\n";
    else if (c == '\r') o += "\\r";
    else if (c == '\t') o += "\\t";
    else if (c < 0x20) {
      o += "\\u00";
      o.push_back(hex[c >> 4]);
      o.push_back(hex[c & 15]);
    } else if (c < 0x80) {
      o.push_back(static_cast<char>(c));
    } else if (c < 0x800) {
      o.push_back(static_cast<char>(0xC0 | (c >> 6)));
      o.push_back(static_cast<char>(0x80 | (c & 0x3F)));
    } else if (c >= 0xD800 && c <= 0xDBFF && i + 1 < n && s[i + 1] >= 0xDC00 && s[i + 1] <= 0xDFFF) {
      const uint32_t cp = 0x10000 + ((c - 0xD800) << 10) + (s[i + 1] - 0xDC00);
      i++;
      o.push_back(static_cast<char>(0xF0 | (cp >> 18)));
      o.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F)));
      o.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
      o.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    } else if (c >= 0xD800 && c <= 0xDFFF) {
      o += "\\u";
      for (int k = 12; k >= 0; k -= 4) o.push_back(hex[(c >> k) & 15]);
    } else {
      o.push_back(static_cast<char>(0xE0 | (c >> 12)));
      o.push_back(static_cast<char>(0x80 | ((c >> 6) & 0x3F)));
      o.push_back(static_cast<char>(0x80 | (c & 0x3F)));
    }
  }
  o.push_back('"');
}

// A quoted key "digits" that is a canonical array index (< 2^32 - 1): its value, else -1.
int64_t arrayIndexOfQuoted(const std::string& q) {
  if (q.size() < 3 || q.size() > 12 || q.front() != '"' || q.back() != '"') return -1;
  const size_t n = q.size() - 2;
  if (n > 1 && q[1] == '0') return -1;
  int64_t v = 0;
  for (size_t i = 1; i + 1 < q.size(); i++) {
    if (q[i] < '0' || q[i] > '9') return -1;
    v = v * 10 + (q[i] - '0');
  }
  return v < 4294967295LL ? v : -1;
}

struct SumDict {
  std::vector<std::string> keys, values;  // keys JSON-quoted, values JSON texts (UTF-8)
  std::vector<int64_t> keyIndex;          // array-index value of each key, or -1
};

// A prop set as a JSON object in JS own-property order: array-index keys ascending, then the
// others in insertion order (properties' key order, snapshotChunks.ts via JSON.stringify).
// (ps: the set's first record; a set wider than FMT_MT_PROPS_MAX continues in the next records)
void propsObject(std::string& o, const fmt_mt_propset* ps, const SumDict& D, const std::vector<double>* nums,
                 uint32_t valueBase) {
  const uint32_t n = ps->n < FMT_MT_PROPS_KEYS_MAX ? ps->n : FMT_MT_PROPS_KEYS_MAX;
  uint32_t kvs[FMT_MT_PROPS_KEYS_MAX], order[FMT_MT_PROPS_KEYS_MAX];
  for (uint32_t i = 0; i < n; i++) kvs[i] = ps[i / FMT_MT_PROPS_MAX].kv[i % FMT_MT_PROPS_MAX];
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; i++)
    if (D.keyIndex[kvs[i] >> 16] >= 0) order[m++] = i;
  std::sort(order, order + m, [&](uint32_t a, uint32_t b) { return D.keyIndex[kvs[a] >> 16] < D.keyIndex[kvs[b] >> 16]; });
  for (uint32_t i = 0; i < n; i++)
    if (D.keyIndex[kvs[i] >> 16] < 0) order[m++] = i;
  o.push_back('{');
  for (uint32_t j = 0; j < m; j++) {
    if (j) o.push_back(',');
    const uint32_t kv = kvs[order[j]];
    o += D.keys[kv >> 16];
    o.push_back(':');
    const uint32_t v = kv & 0xFFFFu;
    if (nums != nullptr && v >= FMT_MT_VALUE_COMPUTED)  // an annotate-adjust result
      o += fmt_json::jsNumber((*nums)[v - FMT_MT_VALUE_COMPUTED]);
    else
      o += D.values[valueBase + v];
  }
  o.push_back('}');
}

// toJSONObject of a summary segment: a TextSegment's text or {text, props} (textSegment.ts:62-66), a
// Marker's {marker: {refType}, props?} (mergeTreeNodes.ts:514-518; its one unit is the refType).
// propsId: the segment's prop set in `props` (0xffff: undefined; an empty set writes no props either).
void segmentJson(std::string& out, const uint16_t* text, uint32_t len, uint32_t propsId, bool marker,
                 const fmt_mt_propset* props, const SumDict& D, const std::vector<double>* nums, uint32_t valueBase) {
  const bool hasProps = propsId != 0xFFFFu && props[propsId].n > 0;
  if (marker) {  // Marker.toJSONObject
    out += "{\"marker\":{\"refType\":" + std::to_string(text[0]) + "}";
    if (hasProps) {
      out += ",\"props\":";
      propsObject(out, props + propsId, D, nums, valueBase);
    }
    out.push_back('}');
  } else if (hasProps) {
    out += "{\"text\":";
    jsonQuote16(out, text, len);
    out += ",\"props\":";
    propsObject(out, props + propsId, D, nums, valueBase);
    out.push_back('}');
  } else {
    jsonQuote16(out, text, len);
  }
}

// Prop set p (0xffff: none) lies within the document's nProps records, and its key / value ids within
// the tables passed in (value id v names values[vBase + v] below vEnd, or a computed number).
bool propSetInTables(const fmt_mt_propset* props, uint32_t nProps, uint32_t p, uint32_t nKeys, uint32_t vBase,
                     uint64_t vEnd, const std::vector<double>* nums) {
  if (p == 0xFFFFu) return true;
  const uint32_t pn = p < nProps ? props[p].n : 0u;
  if (p >= nProps || pn > FMT_MT_PROPS_KEYS_MAX || (pn > 0 && p + (pn - 1) / FMT_MT_PROPS_MAX >= nProps)) return false;
  for (uint32_t k = 0; k < pn; k++) {
    const uint32_t kv = props[p + k / FMT_MT_PROPS_MAX].kv[k % FMT_MT_PROPS_MAX];
    const uint32_t v = kv & 0xFFFFu;
    const bool computed = nums != nullptr && v >= FMT_MT_VALUE_COMPUTED && v - FMT_MT_VALUE_COMPUTED < nums->size();
    if ((kv >> 16) >= nKeys || (vBase + static_cast<uint64_t>(v) >= vEnd && !computed)) return false;
  }
  return true;
}

// SnapshotLegacy.emit for one document (snapshotlegacy.ts:161-190 + snapshotChunks.ts:85-204):
// the header chunk (runs until >= chunk units) and, when runs remain, the body chunk.
void legacyBlobs(std::string& out, uint32_t* split, const fmt_kernels::SumRun* runs, uint32_t nRuns,
                 const uint16_t* text, const fmt_mt_propset* props, int32_t minSeq, uint32_t chunk,
                 const SumDict& D, const std::vector<double>* nums, uint32_t valueBase) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < nRuns; i++) total += runs[i].len;
  std::vector<uint64_t> start(nRuns + 1, 0);
  for (uint32_t i = 0; i < nRuns; i++) start[i + 1] = start[i] + runs[i].len;
  auto emit = [&](uint32_t s0, uint64_t approx, bool header, uint32_t* count) {
    uint32_t n = 0;
    uint64_t len = 0;
    while (len < approx && s0 + n < nRuns) len += runs[s0 + n++].len;
    out += "{\"chunkStartSegmentIndex\":" + std::to_string(s0) + ",\"chunkSegmentCount\":" + std::to_string(n) +
           ",\"chunkLengthChars\":" + std::to_string(len) + ",\"totalLengthChars\":" + std::to_string(total) +
           ",\"totalSegmentCount\":" + std::to_string(nRuns) + ",\"chunkSequenceNumber\":" + std::to_string(minSeq) +
           ",\"segmentTexts\":[";
    for (uint32_t i = s0; i < s0 + n; i++) {
      if (i > s0) out.push_back(',');
      const fmt_kernels::SumRun& r = runs[i];
      segmentJson(out, text + start[i], r.len, r.props, (r.flags & 1u) != 0, props, D, nums, valueBase);
    }
    out.push_back(']');
    if (header) {
      out += ",\"headerMetadata\":{\"orderedChunkMetadata\":[{\"id\":\"header\"}";
      if (len < total) out += ",{\"id\":\"body\"}";
      out += "],\"sequenceNumber\":" + std::to_string(minSeq) + ",\"totalLength\":" + std::to_string(total) +
             ",\"totalSegmentCount\":" + std::to_string(nRuns) + "}";
    }
    out.push_back('}');
    *count = n;
  };
  uint32_t n1 = 0, n2 = 0;
  emit(0, chunk, true, &n1);
  *split = static_cast<uint32_t>(out.size());
  if (n1 < nRuns) emit(n1, total, false, &n2);
}

// SnapshotV1.emit for one document (snapshotV1.ts:126-168) over the kernel's segments (extractSync,
// snapshotV1.ts:170-276): out holds the header blob, then body_0, body_1, ...; ends[k] is where blob k
// ends. A chunk takes segments until it holds >= chunk units (do ... while: the header always exists).
// rm: the document's remove-order entries, the later stamps of its removed leaves; names[k]: the
// JSON-quoted long id of short client k. FMT_E_USAGE when a stamp's client has no name.
int v1Blobs(std::string& out, std::vector<uint64_t>& ends, const fmt_kernels::SumV1Seg* segs, uint32_t nSegs,
            const uint16_t* text, const fmt_mt_propset* props, const fmt_mt_remove_order* rm, uint32_t nRm,
            const char* const* names, uint64_t nNames, int32_t minSeq, int32_t curSeq, uint32_t chunk, const SumDict& D,
            const std::vector<double>* nums, uint32_t valueBase) {
  // later stamps bucketed by leaf, each bucket in seq order (stamps.ts:144-158 keeps remote stamps so)
  std::vector<fmt_mt_remove_order> later;
  later.reserve(nRm);
  for (uint32_t i = 0; i < nRm; i++)
    if (rm[i].leaf != FMT_MT_LEAF_GONE) later.push_back(rm[i]);
  std::stable_sort(later.begin(), later.end(), [](const fmt_mt_remove_order& a, const fmt_mt_remove_order& b) {
    return a.leaf != b.leaf ? a.leaf < b.leaf : a.seq < b.seq;
  });
  struct Chunk {
    uint32_t start, count;
    uint64_t length;
  };
  std::vector<Chunk> chunks;
  uint64_t total = 0;
  for (uint32_t s0 = 0;;) {
    uint32_t n = 0;
    uint64_t len = 0;
    while (len < chunk && s0 + n < nSegs) len += segs[s0 + n++].len;
    chunks.push_back({s0, n, len});
    total += len;
    s0 += n;
    if (s0 >= nSegs) break;
  }
  bool noName = false;
  auto name = [&](int32_t client) {
    if (client < 0 || static_cast<uint64_t>(client) >= nNames) noName = true;
    else out += names[client];
  };
  std::vector<fmt_mt_remove_order> stamps;
  uint64_t tpos = 0;
  for (size_t k = 0; k < chunks.size(); k++) {
    const Chunk& ch = chunks[k];
    out += "{\"version\":\"1\",\"segmentCount\":" + std::to_string(ch.count) + ",\"length\":" + std::to_string(ch.length) +
           ",\"segments\":[";
    for (uint32_t i = ch.start; i < ch.start + ch.count; i++) {
      if (i > ch.start) out.push_back(',');
      const fmt_kernels::SumV1Seg& s = segs[i];
      const bool solo = (s.flags & fmt_kernels::kV1Solo) != 0;
      if (solo) out += "{\"json\":";
      segmentJson(out, text + tpos, s.len, s.props, (s.flags & fmt_kernels::kV1Marker) != 0, props, D, nums, valueBase);
      tpos += s.len;
      if (!solo) continue;
      if (s.ins_seq > minSeq) {  // snapshotV1.ts:226-233
        out += ",\"seq\":" + std::to_string(s.ins_seq) + ",\"client\":";
        name(s.ins_client);
      }
      if (s.flags & fmt_kernels::kV1Removed) {
        stamps.clear();
        stamps.push_back({s.leaf, s.rm_client, s.rm_seq, s.rm_kind});
        auto it = std::lower_bound(later.begin(), later.end(), s.leaf,
                                   [](const fmt_mt_remove_order& e, uint32_t leaf) { return e.leaf < leaf; });
        for (; it != later.end() && it->leaf == s.leaf; ++it) stamps.push_back(*it);
        // setRemove stamps (snapshotV1.ts:235-250), then sliceRemove stamps, "moves" in this format (:252-264)
        for (uint32_t kind : {static_cast<uint32_t>(FMT_MT_RM_SET), static_cast<uint32_t>(FMT_MT_RM_SLICE)}) {
          const fmt_mt_remove_order* first = nullptr;
          for (const auto& st : stamps)
            if (st.kind == kind) {
              first = &st;
              break;
            }
          if (first == nullptr) continue;
          if (kind == FMT_MT_RM_SET) {
            out += ",\"removedSeq\":" + std::to_string(first->seq) + ",\"removedClient\":";
            name(first->client);
            out += ",\"removedClientIds\":[";
          } else {
            out += ",\"movedSeq\":" + std::to_string(first->seq) + ",\"movedSeqs\":[";
            bool sep = false;
            for (const auto& st : stamps)
              if (st.kind == kind) {
                if (sep) out.push_back(',');
                sep = true;
                out += std::to_string(st.seq);
              }
            out += "],\"movedClientIds\":[";
          }
          bool sep = false;
          for (const auto& st : stamps)
            if (st.kind == kind) {
              if (sep) out.push_back(',');
              sep = true;
              name(st.client);
            }
          out.push_back(']');
        }
      }
      out.push_back('}');
    }
    out += "],\"startIndex\":" + std::to_string(ch.start);
    if (k == 0) {
      out += ",\"headerMetadata\":{\"minSequenceNumber\":" + std::to_string(minSeq) + ",\"sequenceNumber\":" +
             std::to_string(curSeq) + ",\"orderedChunkMetadata\":[{\"id\":\"header\"}";
      for (size_t b = 0; b + 1 < chunks.size(); b++) out += ",{\"id\":\"body_" + std::to_string(b) + "\"}";
      out += "],\"totalLength\":" + std::to_string(total) + ",\"totalSegmentCount\":" + std::to_string(nSegs) + "}";
    }
    out.push_back('}');
    ends.push_back(out.size());
  }
  return noName ? FMT_E_USAGE : FMT_OK;
}

void makeDict(SumDict& D, const char* const* keys, uint32_t nKeys, const char* const* values, uint32_t nValues) {
  D.keys.assign(keys, keys + nKeys);
  D.values.assign(values, values + nValues);
  D.keyIndex.resize(nKeys);
  for (uint32_t k = 0; k < nKeys; k++) D.keyIndex[k] = arrayIndexOfQuoted(D.keys[k]);
}

}  // namespace

int fmt_mt_state_digest(fmt_ctx* c, uint64_t* out) {
  if (const int rc = mtReadEntry(c, out != nullptr, "fmt_mt_state_digest", "fmt_mt_state_digest: nothing loaded")) return rc;
  if (readFrame(c) == nullptr) return FMT_E_DEVICE;
  const uint32_t nd = c->mtDocs;
  FMT_HIP(c, c->digests.reserve(nd));
  FMT_HIP(c, fmt_kernels::launchStateDigest(c->mtHdr.p, c->sumViews.p, nd, c->digests.p, c->numCUs, c->stream));
  FMT_HIP(c, hipMemcpyAsync(out, c->digests.p, nd * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  return FMT_OK;
}

int fmt_mt_summarize_legacy(fmt_ctx* c, const char* const* keys, uint32_t nKeys, const char* const* values,
                            uint32_t nValues, uint32_t chunk, uint32_t threads, fmt_summary_timing* timing) {
  if (const int rc = mtReadEntry(c, !(nKeys && keys == nullptr) && !(nValues && values == nullptr), "fmt_mt_summarize_legacy",
                                 "fmt_mt_summarize_legacy: bad arguments"))
    return rc;
  using clk = std::chrono::steady_clock;
  const uint32_t nd = c->mtDocs;
  const fmt_ctx::ReadFrame* F = readFrame(c);
  if (F == nullptr) return FMT_E_DEVICE;
  const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
  uint64_t capRuns = 0, capText = 0;
  for (uint32_t d = 0; d < nd; d++) {
    capRuns += hdr[d].n_leaves;
    capText += hdr[d].n_chars;
  }
  FMT_HIP(c, c->sumRuns.reserve(capRuns));
  FMT_HIP(c, c->sumText.reserve(capText));
  FMT_HIP(c, c->sumCursors.reserve(2));
  FMT_HIP(c, c->sumDocs.reserve(nd));
  FMT_HIP(c, hipMemsetAsync(c->sumCursors.p, 0, 2 * sizeof(unsigned long long), c->stream));
  FMT_HIP(c, hipEventRecord(c->evS0, c->stream));  // (own events: fmt_get_stats keeps reporting the replay)
  FMT_HIP(c, fmt_kernels::launchSummaryRuns(c->mtHdr.p, c->sumViews.p, nd, c->sumRuns.p, c->sumText.p, c->sumCursors.p,
                                            c->sumDocs.p, c->numCUs, c->stream));
  FMT_HIP(c, hipEventRecord(c->evS1, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  float kms = 0.f;
  FMT_HIP(c, hipEventElapsedTime(&kms, c->evS0, c->evS1));
  // fetch: per-document spans, runs, text and every document's prop sets (packed on the device:
  // only the sets a document has, not its tier's whole table), staged into host buffers the ctx keeps
  const auto t0 = clk::now();
  unsigned long long cur[2];
  FMT_HIP(c, hipMemcpy(cur, c->sumCursors.p, sizeof cur, hipMemcpyDeviceToHost));
  constexpr uint32_t kPW = sizeof(fmt_mt_propset) / 4;
  std::vector<uint64_t> propOff(nd + 1ull, 0);
  std::vector<fmt_kernels::GatherSpan> sp;
  for (uint32_t d = 0; d < nd; d++) {
    propOff[d + 1] = propOff[d] + hdr[d].n_props;
    if (hdr[d].n_props)
      sp.push_back({reinterpret_cast<const uint32_t*>(F->views[d].props), propOff[d] * kPW, hdr[d].n_props * kPW, 0u});
  }
  if (const int rc = gatherPacked(c, sp, propOff[nd] * kPW, nullptr, 0)) return rc;
  // (pinned destinations the ctx keeps: four DMAs back to back on the stream, one wait)
  FMT_HIP(c, c->sumHostDocs.reserve(nd));
  FMT_HIP(c, c->sumHostRuns.reserve(cur[0]));
  FMT_HIP(c, c->sumHostText.reserve(cur[1]));
  FMT_HIP(c, c->sumHostProps.reserve(propOff[nd] + 1));
  FMT_HIP(c, hipMemcpyAsync(c->sumHostDocs.p, c->sumDocs.p, nd * sizeof(fmt_kernels::SumDocOut), hipMemcpyDeviceToHost, c->stream));
  if (cur[0])
    FMT_HIP(c, hipMemcpyAsync(c->sumHostRuns.p, c->sumRuns.p, cur[0] * sizeof(fmt_kernels::SumRun), hipMemcpyDeviceToHost, c->stream));
  if (cur[1])
    FMT_HIP(c, hipMemcpyAsync(c->sumHostText.p, c->sumText.p, cur[1] * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  if (propOff[nd])
    FMT_HIP(c, hipMemcpyAsync(c->sumHostProps.p, c->packed.p, propOff[nd] * sizeof(fmt_mt_propset), hipMemcpyDeviceToHost,
                              c->stream));
  const fmt_kernels::SumDocOut* docs = c->sumHostDocs.p;
  const fmt_kernels::SumRun* runs = c->sumHostRuns.p;
  const uint16_t* text = c->sumHostText.p;
  std::vector<const fmt_mt_propset*> propsHost(nd);
  for (uint32_t d = 0; d < nd; d++) propsHost[d] = c->sumHostProps.p + propOff[d];
  // computed annotate-adjust numbers of the documents that have any
  std::vector<std::vector<double>> docNums(c->mtPlan.anyAdjust ? nd : 0);
  if (c->mtPlan.anyAdjust) {
    std::vector<uint32_t> cnt(nd);
    FMT_HIP(c, hipMemcpyAsync(cnt.data(), c->mtNumCount.p, nd * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t d = 0; d < nd; d++) {
      docNums[d].resize(cnt[d]);
      if (cnt[d])
        FMT_HIP(c, hipMemcpyAsync(docNums[d].data(), c->mtNums.p + c->mtPlan.numOffs[d], cnt[d] * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
    }
  }
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  const auto t1 = clk::now();
  // format on host threads
  SumDict D;
  makeDict(D, keys, nKeys, values, nValues);
  c->sumBlobs.assign(nd, std::string());
  c->sumSplit.assign(nd, 0);
  c->sumStatus.assign(nd, FMT_OK);
  const uint32_t nt = threads ? threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < nt; t++)
    pool.emplace_back([&, t] {
      for (uint32_t d = t; d < nd; d += nt) {
        const fmt_kernels::SumDocOut& o = docs[d];
        if (static_cast<int32_t>(o.status) != FMT_OK) {
          c->sumStatus[d] = static_cast<int32_t>(o.status);
          continue;
        }
        const std::vector<double>* nums = c->mtPlan.anyAdjust ? &docNums[d] : nullptr;
        // value id v names values[vBase + v] (document-local ids: v <= vCount)
        const uint32_t vBase = c->mtValueBaseHost.empty() ? 0u : c->mtValueBaseHost[d];
        const uint64_t vEnd = c->mtValueBaseHost.empty() ? nValues : std::min<uint64_t>(nValues, c->mtValueBaseHost[d + 1] + 1ull);
        // every prop set a run names, and every key / value id in it, within the tables passed in
        bool bad = false;
        for (uint32_t i = 0; i < o.n_runs && !bad; i++)
          bad = !propSetInTables(propsHost[d], hdr[d].n_props, runs[o.run_off + i].props, nKeys, vBase, vEnd, nums);
        if (bad) {
          c->sumStatus[d] = FMT_E_DATA;
          continue;
        }
        c->sumBlobs[d].reserve(o.n_units + 64ull * o.n_runs + 256);
        legacyBlobs(c->sumBlobs[d], &c->sumSplit[d], runs + o.run_off, o.n_runs, text + o.text_off,
                    propsHost[d], hdr[d].min_seq, chunk ? chunk : 10000u, D, nums, vBase);
      }
    });
  for (auto& th : pool) th.join();
  const auto t2 = clk::now();
  if (timing) {
    timing->kernel_ms = kms;
    timing->fetch_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    timing->format_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    uint64_t bytes = 0;
    for (const auto& b : c->sumBlobs) bytes += b.size();
    timing->bytes = bytes;
    timing->threads = nt;
  }
  return FMT_OK;
}

int fmt_mt_summary_blobs(fmt_ctx* c, uint32_t doc, const char** header, size_t* headerLen, const char** body,
                         size_t* bodyLen) {
  if (c == nullptr || doc >= c->sumBlobs.size()) return setErr(c, FMT_E_USAGE, "fmt_mt_summary_blobs: no summary for doc");
  if (c->sumStatus[doc] != FMT_OK) return setErr(c, c->sumStatus[doc], "document has no summary (replay status)");
  const std::string& b = c->sumBlobs[doc];
  const size_t split = c->sumSplit[doc];
  if (header) *header = b.data();
  if (headerLen) *headerLen = split;
  if (body) *body = b.data() + split;
  if (bodyLen) *bodyLen = b.size() - split;
  return FMT_OK;
}

int fmt_mt_summarize_v1(fmt_ctx* c, const char* const* keys, uint32_t nKeys, const char* const* values, uint32_t nValues,
                        const char* const* clientNames, const uint64_t* docClientOffs, uint32_t chunk, uint32_t threads,
                        fmt_summary_timing* timing) {
  const bool argsOk = c && c->mtLoaded && c->mtRan && !(nKeys && keys == nullptr) && !(nValues && values == nullptr) &&
                      docClientOffs != nullptr && !(docClientOffs[c->mtDocs] && clientNames == nullptr);
  if (const int rc = mtReadEntry(c, argsOk, nullptr, "fmt_mt_summarize_v1: bad arguments, or no fmt_mt_run since the load"))
    return rc;
  if (c->mtPlan.local)
    return setErr(c, FMT_E_UNSUPPORTED, "fmt_mt_summarize_v1: the batch holds local-client records (pending stamps have no SnapshotV1 form)");
  using clk = std::chrono::steady_clock;
  const uint32_t nd = c->mtDocs;
  const fmt_ctx::ReadFrame* F = readFrame(c);
  if (F == nullptr) return FMT_E_DEVICE;
  const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
  uint64_t capSegs = 0, capText = 0;
  for (uint32_t d = 0; d < nd; d++) {
    capSegs += hdr[d].n_leaves;
    capText += hdr[d].n_chars;
  }
  FMT_HIP(c, c->v1Segs.reserve(capSegs));
  FMT_HIP(c, c->sumText.reserve(capText));
  FMT_HIP(c, c->sumCursors.reserve(2));
  FMT_HIP(c, c->sumDocs.reserve(nd));
  FMT_HIP(c, hipMemsetAsync(c->sumCursors.p, 0, 2 * sizeof(unsigned long long), c->stream));
  FMT_HIP(c, hipEventRecord(c->evS0, c->stream));
  FMT_HIP(c, fmt_kernels::launchSummaryV1(c->mtHdr.p, c->sumViews.p, c->mtOps.p, c->mtOffs.p, nd, c->v1Segs.p, c->sumText.p,
                                          c->sumCursors.p, c->sumDocs.p, c->numCUs, c->stream));
  FMT_HIP(c, hipEventRecord(c->evS1, c->stream));
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  float kms = 0.f;
  FMT_HIP(c, hipEventElapsedTime(&kms, c->evS0, c->evS1));
  // fetch: spans, segments, text, and the prop sets and used remove-order prefixes of every document
  // that replayed, packed on the device (gatherSpansKernel) and brought over in one copy each
  const auto t0 = clk::now();
  unsigned long long cur[2];
  FMT_HIP(c, hipMemcpy(cur, c->sumCursors.p, sizeof cur, hipMemcpyDeviceToHost));
  constexpr uint32_t kPW = sizeof(fmt_mt_propset) / 4, kRW = sizeof(fmt_mt_remove_order) / 4;
  std::vector<uint64_t> propOff(nd + 1ull, 0), rmOff(nd + 1ull, 0);
  for (uint32_t d = 0; d < nd; d++) {
    const bool ok = hdr[d].status == FMT_OK;
    const uint64_t slab = c->mtPlan.hasRmOrder() ? c->mtPlan.rmOffs[d + 1] - c->mtPlan.rmOffs[d] : 0;
    propOff[d + 1] = propOff[d] + (ok ? hdr[d].n_props : 0u);
    rmOff[d + 1] = rmOff[d] + (ok ? std::min<uint64_t>(hdr[d].n_rm_order, slab) : 0u);
  }
  std::vector<fmt_kernels::GatherSpan> sp;
  for (uint32_t d = 0; d < nd; d++) {
    if (propOff[d + 1] > propOff[d])
      sp.push_back({reinterpret_cast<const uint32_t*>(F->views[d].props), propOff[d] * kPW,
                    static_cast<uint32_t>(propOff[d + 1] - propOff[d]) * kPW, 0u});
    if (rmOff[d + 1] > rmOff[d])
      sp.push_back({reinterpret_cast<const uint32_t*>(c->mtRmOrder.p + c->mtPlan.rmOffs[d]), propOff[nd] * kPW + rmOff[d] * kRW,
                    static_cast<uint32_t>(rmOff[d + 1] - rmOff[d]) * kRW, 0u});
  }
  if (const int rc = gatherPacked(c, sp, propOff[nd] * kPW + rmOff[nd] * kRW, nullptr, 0)) return rc;
  FMT_HIP(c, c->sumHostDocs.reserve(nd));
  FMT_HIP(c, c->v1HostSegs.reserve(cur[0]));
  FMT_HIP(c, c->sumHostText.reserve(cur[1]));
  FMT_HIP(c, c->sumHostProps.reserve(propOff[nd] + 1));
  FMT_HIP(c, c->v1HostRm.reserve(rmOff[nd] + 1));
  FMT_HIP(c, hipMemcpyAsync(c->sumHostDocs.p, c->sumDocs.p, nd * sizeof(fmt_kernels::SumDocOut), hipMemcpyDeviceToHost, c->stream));
  if (cur[0])
    FMT_HIP(c, hipMemcpyAsync(c->v1HostSegs.p, c->v1Segs.p, cur[0] * sizeof(fmt_kernels::SumV1Seg), hipMemcpyDeviceToHost, c->stream));
  if (cur[1])
    FMT_HIP(c, hipMemcpyAsync(c->sumHostText.p, c->sumText.p, cur[1] * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  if (propOff[nd])
    FMT_HIP(c, hipMemcpyAsync(c->sumHostProps.p, c->packed.p, propOff[nd] * sizeof(fmt_mt_propset), hipMemcpyDeviceToHost,
                              c->stream));
  if (rmOff[nd])
    FMT_HIP(c, hipMemcpyAsync(c->v1HostRm.p, c->packed.p + propOff[nd] * kPW, rmOff[nd] * sizeof(fmt_mt_remove_order),
                              hipMemcpyDeviceToHost, c->stream));
  std::vector<std::vector<double>> docNums(c->mtPlan.anyAdjust ? nd : 0);
  if (c->mtPlan.anyAdjust) {  // computed annotate-adjust numbers of the documents that have any
    std::vector<uint32_t> cnt(nd);
    FMT_HIP(c, hipMemcpyAsync(cnt.data(), c->mtNumCount.p, nd * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t d = 0; d < nd; d++) {
      docNums[d].resize(cnt[d]);
      if (cnt[d])
        FMT_HIP(c, hipMemcpyAsync(docNums[d].data(), c->mtNums.p + c->mtPlan.numOffs[d], cnt[d] * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
    }
  }
  FMT_HIP(c, hipStreamSynchronize(c->stream));
  const auto t1 = clk::now();
  // format on host threads
  const fmt_kernels::SumDocOut* docs = c->sumHostDocs.p;
  const fmt_kernels::SumV1Seg* segs = c->v1HostSegs.p;
  const uint16_t* text = c->sumHostText.p;
  SumDict D;
  makeDict(D, keys, nKeys, values, nValues);
  c->v1Blobs.assign(nd, std::string());
  c->v1Ends.assign(nd, std::vector<uint64_t>());
  c->v1Status.assign(nd, FMT_OK);
  const uint32_t nt = threads ? threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < nt; t++)
    pool.emplace_back([&, t] {
      for (uint32_t d = t; d < nd; d += nt) {
        const fmt_kernels::SumDocOut& o = docs[d];
        if (static_cast<int32_t>(o.status) != FMT_OK) {
          c->v1Status[d] = static_cast<int32_t>(o.status);
          continue;
        }
        const std::vector<double>* nums = c->mtPlan.anyAdjust ? &docNums[d] : nullptr;
        const uint32_t vBase = c->mtValueBaseHost.empty() ? 0u : c->mtValueBaseHost[d];
        const uint64_t vEnd = c->mtValueBaseHost.empty() ? nValues : std::min<uint64_t>(nValues, c->mtValueBaseHost[d + 1] + 1ull);
        const fmt_mt_propset* props = c->sumHostProps.p + propOff[d];
        bool bad = docClientOffs[d + 1] < docClientOffs[d];
        for (uint32_t i = 0; i < o.n_runs && !bad; i++)
          bad = !propSetInTables(props, hdr[d].n_props, segs[o.run_off + i].props, nKeys, vBase, vEnd, nums);
        if (bad) {
          c->v1Status[d] = FMT_E_DATA;
          continue;
        }
        std::string& out = c->v1Blobs[d];
        out.reserve(o.n_units + 64ull * o.n_runs + 256);
        c->v1Status[d] = v1Blobs(out, c->v1Ends[d], segs + o.run_off, o.n_runs, text + o.text_off, props,
                                 c->v1HostRm.p + rmOff[d], static_cast<uint32_t>(rmOff[d + 1] - rmOff[d]),
                                 clientNames + docClientOffs[d], docClientOffs[d + 1] - docClientOffs[d], hdr[d].min_seq,
                                 hdr[d].cur_seq, chunk ? chunk : 10000u, D, nums, vBase);
        if (c->v1Status[d] != FMT_OK) {
          out.clear();
          c->v1Ends[d].clear();
        }
      }
    });
  for (auto& th : pool) th.join();
  const auto t2 = clk::now();
  if (timing) {
    timing->kernel_ms = kms;
    timing->fetch_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    timing->format_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    uint64_t bytes = 0;
    for (const auto& b : c->v1Blobs) bytes += b.size();
    timing->bytes = bytes;
    timing->threads = nt;
  }
  return FMT_OK;
}

int fmt_mt_summary_v1_blobs(fmt_ctx* c, uint32_t doc, const char** header, size_t* headerLen, uint32_t* nBodies) {
  if (c == nullptr || doc >= c->v1Blobs.size()) return setErr(c, FMT_E_USAGE, "fmt_mt_summary_v1_blobs: no summary for doc");
  if (c->v1Status[doc] != FMT_OK) return setErr(c, c->v1Status[doc], "document has no SnapshotV1 summary (its V1 status)");
  if (header) *header = c->v1Blobs[doc].data();
  if (headerLen) *headerLen = c->v1Ends[doc][0];
  if (nBodies) *nBodies = static_cast<uint32_t>(c->v1Ends[doc].size() - 1);
  return FMT_OK;
}

int fmt_mt_summary_v1_body(fmt_ctx* c, uint32_t doc, uint32_t k, const char** body, size_t* bodyLen) {
  if (c == nullptr || doc >= c->v1Blobs.size()) return setErr(c, FMT_E_USAGE, "fmt_mt_summary_v1_body: no summary for doc");
  if (c->v1Status[doc] != FMT_OK) return setErr(c, c->v1Status[doc], "document has no SnapshotV1 summary (its V1 status)");
  const std::vector<uint64_t>& ends = c->v1Ends[doc];
  if (k + 1ull >= ends.size()) return setErr(c, FMT_E_USAGE, "fmt_mt_summary_v1_body: no such body chunk");
  if (body) *body = c->v1Blobs[doc].data() + ends[k];
  if (bodyLen) *bodyLen = ends[k + 1] - ends[k];
  return FMT_OK;
}

int fmt_mt_fetch_catchup(fmt_ctx* c, uint32_t doc, fmt_mt_catchup_range* out, uint32_t cap) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(out == nullptr && cap > 0), "fmt_mt_fetch_catchup",
                                 "fmt_mt_fetch_catchup: bad arguments"))
    return rc;
  if (!c->mtPlan.hasCatchup()) return FMT_OK;
  fmt_mt_doc_result h;
  FMT_HIP(c, hipMemcpy(&h, c->mtHdr.p + doc, sizeof h, hipMemcpyDeviceToHost));
  const uint32_t m = h.n_catchup < cap ? h.n_catchup : cap;
  if (m) FMT_HIP(c, hipMemcpy(out, c->mtCatchup.p + c->mtPlan.cuOffs[doc], m * sizeof(fmt_mt_catchup_range), hipMemcpyDeviceToHost));
  return FMT_OK;
}

int fmt_mt_fetch_catchup_all(fmt_ctx* c, uint64_t* offsets, fmt_mt_catchup_range* out, uint64_t cap) {
  if (const int rc = mtReadEntry(c, offsets != nullptr, "fmt_mt_fetch_catchup_all", "fmt_mt_fetch_catchup_all: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  offsets[0] = 0;
  if (!c->mtPlan.hasCatchup()) {
    for (uint32_t d = 0; d < nd; d++) offsets[d + 1] = 0;
    return FMT_OK;
  }
  const fmt_ctx::ReadFrame* F = readFrame(c);
  if (F == nullptr) return FMT_E_DEVICE;
  const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
  for (uint32_t d = 0; d < nd; d++) {
    const uint64_t slab = c->mtPlan.cuOffs[d + 1] - c->mtPlan.cuOffs[d];
    offsets[d + 1] = offsets[d] + std::min<uint64_t>(hdr[d].n_catchup, slab);
  }
  if (out == nullptr) return FMT_OK;
  if (cap < offsets[nd]) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_catchup_all: cap below the ranges recorded");
  // each document's recorded prefix packed on the device (gatherSpansKernel), then one staged copy of
  // exactly the recorded ranges
  constexpr uint32_t kW = sizeof(fmt_mt_catchup_range) / 4;
  std::vector<fmt_kernels::GatherSpan> sp;
  sp.reserve(nd);
  for (uint32_t d = 0; d < nd; d++)
    if (offsets[d + 1] > offsets[d])
      sp.push_back({reinterpret_cast<const uint32_t*>(c->mtCatchup.p + c->mtPlan.cuOffs[d]), offsets[d] * kW,
                    static_cast<uint32_t>(offsets[d + 1] - offsets[d]) * kW, 0u});
  return gatherPacked(c, sp, offsets[nd] * kW, out, offsets[nd] * sizeof(fmt_mt_catchup_range));
}

uint32_t fmt_mt_text_tile_leaves(void) { return fmt_plan::kTextTileLeaves; }

int fmt_mt_fetch_text_all(fmt_ctx* c, uint16_t placeholder, uint64_t* offsets, uint16_t* out, uint64_t cap) {
  if (const int rc = mtReadEntry(c, offsets != nullptr, "fmt_mt_fetch_text_all", "fmt_mt_fetch_text_all: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  const fmt_ctx::ReadFrame* F = nullptr;
  if (const int rc = frameTiles(c, "fmt_mt_fetch_text_all: more than 2^32 - 1 work items", &F)) return rc;
  const size_t ni = F->tiles.items.size();
  if (!c->textSized || c->textPlaceholder != placeholder) {
    // pass 1: the units each work item contributes under this placeholder, the scan on the host. (The tiles
    // are the frame's and know no placeholder; only these units do.)
    c->textSized = false;
    FMT_HIP(c, c->textUnits.reserve(ni));
    FMT_HIP(c, c->textBases.reserve(ni));
    FMT_HIP(c, c->textHostUnits.reserve(ni));
    FMT_HIP(c, c->textHostBases.reserve(ni));
    c->textOffs.assign(nd + 1ull, 0);
    if (ni) {
      FMT_HIP(c, fmt_kernels::launchTextTileUnits(c->mtHdr.p, c->sumViews.p, c->tileItems.p, static_cast<uint32_t>(ni),
                                                  placeholder, c->textUnits.p, c->numCUs, c->stream));
      FMT_HIP(c, hipMemcpyAsync(c->textHostUnits.p, c->textUnits.p, ni * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
      FMT_HIP(c, hipStreamSynchronize(c->stream));
      fmt_plan::textOffsets(F->tiles, c->textHostUnits.p, c->textOffs.data(), c->textHostBases.p);
      FMT_HIP(c, hipMemcpyAsync(c->textBases.p, c->textHostBases.p, ni * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      FMT_HIP(c, hipStreamSynchronize(c->stream));  // (nothing of this call is in flight past here)
    }
    c->textPlaceholder = placeholder;
    c->textSized = true;
  }
  std::memcpy(offsets, c->textOffs.data(), (nd + 1ull) * sizeof(uint64_t));
  const uint64_t total = c->textOffs[nd];
  if (out == nullptr) return FMT_OK;
  if (cap < total) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_text_all: cap below the units of the text");
  if (total == 0) return FMT_OK;
  // pass 2: every item's units to its base in the packed text, then one staged copy of exactly those
  // (stagedCopy waits for the stream first and returns when the units are in `out`)
  FMT_HIP(c, c->textPacked.reserve(total));
  FMT_HIP(c, fmt_kernels::launchTextGather(c->mtHdr.p, c->sumViews.p, c->tileItems.p, static_cast<uint32_t>(ni), placeholder,
                                           c->textBases.p, c->textPacked.p, c->numCUs, c->stream));
  FMT_HIP(c, stagedCopy(c, out, c->textPacked.p, total * sizeof(uint16_t), false));
  return FMT_OK;
}

int fmt_mt_fetch_prop_runs_all(fmt_ctx* c, uint64_t* offsets, fmt_mt_prop_run* out, uint64_t cap) {
  if (const int rc = mtReadEntry(c, offsets != nullptr, "fmt_mt_fetch_prop_runs_all", "fmt_mt_fetch_prop_runs_all: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  const fmt_ctx::ReadFrame* F = nullptr;
  if (const int rc = frameTiles(c, "fmt_mt_fetch_prop_runs_all: more than 2^32 - 1 work items", &F)) return rc;
  const size_t ni = F->tiles.items.size();
  if (!c->runsSized) {
    // the class spans from the headers (the views carry the huge documents' own classes, SumView::cls), the
    // classes, pass 1, the stitch on the host
    const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
    c->runsClsOffs.assign(nd + 1ull, 0);
    for (uint32_t d = 0; d < nd; d++)
      c->runsClsOffs[d + 1] = c->runsClsOffs[d] + (hdr[d].status == FMT_OK && F->views[d].cls == nullptr ? hdr[d].n_props : 0u);
    FMT_HIP(c, c->runsClsOff.reserve(nd + 1ull));
    FMT_HIP(c, c->runsCls.reserve(c->runsClsOffs[nd]));
    FMT_HIP(c, c->runsTiles.reserve(ni));
    FMT_HIP(c, c->runsBases.reserve(ni));
    FMT_HIP(c, c->runsHostTiles.reserve(ni));
    FMT_HIP(c, c->runsHostBases.reserve(ni));
    c->runsOffs.assign(nd + 1ull, 0);
    if (ni) {
      FMT_HIP(c, hipMemcpyAsync(c->runsClsOff.p, c->runsClsOffs.data(), (nd + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice,
                                c->stream));
      if (c->runsClsOffs[nd])
        FMT_HIP(c, fmt_kernels::launchRunClasses(c->mtHdr.p, c->sumViews.p, nd, c->runsClsOff.p, c->runsCls.p, c->numCUs, c->stream));
      FMT_HIP(c, fmt_kernels::launchRunTileReport(c->mtHdr.p, c->sumViews.p, c->tileItems.p, static_cast<uint32_t>(ni),
                                                  c->runsClsOff.p, c->runsCls.p, c->runsTiles.p, c->numCUs, c->stream));
      FMT_HIP(c, hipMemcpyAsync(c->runsHostTiles.p, c->runsTiles.p, ni * sizeof(fmt_plan::RunTile), hipMemcpyDeviceToHost, c->stream));
      FMT_HIP(c, hipStreamSynchronize(c->stream));
      fmt_plan::stitchRuns(F->tiles, c->runsHostTiles.p, c->runsOffs.data(), c->runsHostBases.p);
      FMT_HIP(c, hipMemcpyAsync(c->runsBases.p, c->runsHostBases.p, ni * sizeof(fmt_plan::RunTileBase), hipMemcpyHostToDevice, c->stream));
      FMT_HIP(c, hipStreamSynchronize(c->stream));  // (nothing of this call is in flight past here)
    }
    c->runsSized = true;
  }
  std::memcpy(offsets, c->runsOffs.data(), (nd + 1ull) * sizeof(uint64_t));
  const uint64_t total = c->runsOffs[nd];
  if (out == nullptr) return FMT_OK;
  if (cap < total) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_prop_runs_all: cap below the number of runs");
  if (total == 0) return FMT_OK;
  // pass 2: every item's runs to its base in the packed runs, then one staged copy of exactly those
  FMT_HIP(c, c->runsPacked.reserve(total));
  FMT_HIP(c, fmt_kernels::launchRunEmit(c->mtHdr.p, c->sumViews.p, c->tileItems.p, static_cast<uint32_t>(ni), c->runsClsOff.p,
                                        c->runsCls.p, c->runsBases.p, total, c->runsPacked.p, c->numCUs, c->stream));
  FMT_HIP(c, stagedCopy(c, out, c->runsPacked.p, total * sizeof(fmt_mt_prop_run), false));
  return FMT_OK;
}

int fmt_mt_fetch_props_all(fmt_ctx* c, uint64_t* offsets, fmt_mt_propset* out, uint64_t cap) {
  if (const int rc = mtReadEntry(c, offsets != nullptr, "fmt_mt_fetch_props_all", "fmt_mt_fetch_props_all: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  const fmt_ctx::ReadFrame* F = readFrame(c);
  if (F == nullptr) return FMT_E_DEVICE;
  const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
  offsets[0] = 0;
  for (uint32_t d = 0; d < nd; d++) offsets[d + 1] = offsets[d] + (hdr[d].status == FMT_OK ? hdr[d].n_props : 0u);
  if (out == nullptr) return FMT_OK;
  if (cap < offsets[nd]) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_props_all: cap below the number of prop-set records");
  // each document's records packed on the device (gatherSpansKernel), then one staged copy of exactly those
  constexpr uint32_t kPW = sizeof(fmt_mt_propset) / 4;
  std::vector<fmt_kernels::GatherSpan> sp;
  sp.reserve(nd);
  for (uint32_t d = 0; d < nd; d++)
    if (offsets[d + 1] > offsets[d])
      sp.push_back({reinterpret_cast<const uint32_t*>(F->views[d].props), offsets[d] * kPW,
                    static_cast<uint32_t>(offsets[d + 1] - offsets[d]) * kPW, 0u});
  return gatherPacked(c, sp, offsets[nd] * kPW, out, offsets[nd] * sizeof(fmt_mt_propset));
}

int fmt_mt_query_positions(fmt_ctx* c, const uint64_t* qOffsets, const fmt_mt_pos_query* q, uint64_t nQueries,
                           fmt_mt_pos_hit* out) {
  if (const int rc = mtReadEntry(c, qOffsets != nullptr && !(nQueries && (q == nullptr || out == nullptr)), "fmt_mt_query_positions",
                                 "fmt_mt_query_positions: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  if (!fmt_plan::posOffsetsValid(qOffsets, nd, nQueries))
    return setErr(c, FMT_E_USAGE, "fmt_mt_query_positions: q_offsets must ascend from 0 to n_queries");
  if (nQueries == 0) return FMT_OK;
  // the statuses the headers decide, the views and their (view, tile) items over the frame's tiles
  const fmt_ctx::ReadFrame* F = nullptr;
  if (const int frc = frameTiles(c, "fmt_mt_query_positions: more than 2^32 - 1 views or work items", &F)) return frc;
  const std::vector<fmt_mt_doc_result>& hdr = F->hdr;
  fmt_plan::PosPlan& P = c->posPlan;
  const int rc = fmt_plan::planPosViews(hdr.data(), nd, c->mtPlan.obliterates, F->tiles, qOffsets, q, nQueries, out, P);
  if (rc != FMT_OK) return setErr(c, rc, "fmt_mt_query_positions: more than 2^32 - 1 views or work items");
  // pass 1: every item's units in its view and in the local view; the prefixes and the tile lookup on the host
  const size_t ni = P.items.size();
  FMT_HIP(c, c->posHostUnits.reserve(ni));
  if (ni) {
    FMT_HIP(c, c->posItems.reserve(ni));
    FMT_HIP(c, c->posUnits.reserve(ni));
    FMT_HIP(c, hipMemcpyAsync(c->posItems.p, P.items.data(), ni * sizeof(fmt_plan::PosItem), hipMemcpyHostToDevice, c->stream));
    FMT_HIP(c, fmt_kernels::launchPosTileUnits(c->mtHdr.p, c->sumViews.p, c->posItems.p, static_cast<uint32_t>(ni), c->posUnits.p,
                                               c->numCUs, c->stream));
    FMT_HIP(c, hipMemcpyAsync(c->posHostUnits.p, c->posUnits.p, ni * sizeof(fmt_plan::PosTileUnits), hipMemcpyDeviceToHost,
                              c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  fmt_plan::resolvePosQueries(P, F->tiles, hdr.data(), c->posHostUnits.p, q, nQueries, out);
  const size_t nDev = P.dev.size();
  if (nDev == 0) return FMT_OK;
  // pass 2: the records as the host left them go up, every device query's lane writes its own, and one
  // staged copy brings them all back (stagedCopy waits for the stream first)
  FMT_HIP(c, c->posQueries.reserve(nDev));
  FMT_HIP(c, c->posHits.reserve(nQueries));
  FMT_HIP(c, stagedCopy(c, c->posHits.p, out, nQueries * sizeof(fmt_mt_pos_hit), true));
  FMT_HIP(c, stagedCopy(c, c->posQueries.p, P.dev.data(), nDev * sizeof(fmt_plan::PosDevQuery), true));
  FMT_HIP(c, fmt_kernels::launchPosResolve(c->mtHdr.p, c->sumViews.p, c->posQueries.p, nDev, nQueries, c->posHits.p, c->numCUs,
                                           c->stream));
  FMT_HIP(c, stagedCopy(c, out, c->posHits.p, nQueries * sizeof(fmt_mt_pos_hit), false));
  return FMT_OK;
}

int fmt_mt_fetch_text_ranges(fmt_ctx* c, uint16_t placeholder, const uint64_t* qOffsets, const fmt_mt_range_query* q,
                             uint64_t nQueries, fmt_mt_range_hit* hits, uint64_t* total, uint16_t* out, uint64_t cap) {
  if (const int rc = mtReadEntry(c, qOffsets != nullptr && total != nullptr && !(nQueries && (q == nullptr || hits == nullptr)),
                                 "fmt_mt_fetch_text_ranges", "fmt_mt_fetch_text_ranges: bad arguments"))
    return rc;
  const uint32_t nd = c->mtDocs;
  if (!fmt_plan::posOffsetsValid(qOffsets, nd, nQueries))
    return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_text_ranges: q_offsets must ascend from 0 to n_queries");
  *total = 0;
  if (nQueries == 0) return FMT_OK;
  // the statuses the headers decide, the views and their (view, tile) items over the frame's tiles
  const fmt_ctx::ReadFrame* F = nullptr;
  if (const int frc = frameTiles(c, "fmt_mt_fetch_text_ranges: more than 2^32 - 1 views or work items", &F)) return frc;
  fmt_plan::RangePlan& P = c->rngPlan;
  int rc = fmt_plan::planRangeViews(F->hdr.data(), nd, c->mtPlan.obliterates, F->tiles, qOffsets, q, nQueries, hits, P);
  if (rc != FMT_OK) return setErr(c, rc, "fmt_mt_fetch_text_ranges: more than 2^32 - 1 views or work items");
  // pass A (pos.hip): every (view, tile) item's units in its view; the prefixes and the cut into items on the host
  const size_t nv = P.views.items.size();
  FMT_HIP(c, c->rngHostViewUnits.reserve(nv));
  if (nv) {
    FMT_HIP(c, c->rngViewItems.reserve(nv));
    FMT_HIP(c, c->rngViewUnits.reserve(nv));
    FMT_HIP(c, hipMemcpyAsync(c->rngViewItems.p, P.views.items.data(), nv * sizeof(fmt_plan::PosItem), hipMemcpyHostToDevice, c->stream));
    FMT_HIP(c, fmt_kernels::launchPosTileUnits(c->mtHdr.p, c->sumViews.p, c->rngViewItems.p, static_cast<uint32_t>(nv),
                                               c->rngViewUnits.p, c->numCUs, c->stream));
    FMT_HIP(c, hipMemcpyAsync(c->rngHostViewUnits.p, c->rngViewUnits.p, nv * sizeof(fmt_plan::PosTileUnits), hipMemcpyDeviceToHost,
                              c->stream));
    FMT_HIP(c, hipStreamSynchronize(c->stream));
  }
  rc = fmt_plan::cutRanges(P, F->tiles, c->rngHostViewUnits.p, q, nQueries, hits);
  if (rc != FMT_OK) return setErr(c, rc, "fmt_mt_fetch_text_ranges: more than 2^32 - 1 work items");
  // pass B: the text units of every item (with a placeholder they are its positions); the offsets on the host
  const size_t ni = P.items.size();
  if (ni) {
    FMT_HIP(c, c->rngItems.reserve(ni));
    FMT_HIP(c, stagedCopy(c, c->rngItems.p, P.items.data(), ni * sizeof(fmt_plan::RangeItem), true));
  }
  if (ni && placeholder == 0) {
    FMT_HIP(c, c->rngUnits.reserve(ni));
    FMT_HIP(c, c->rngHostUnits.reserve(ni));
    FMT_HIP(c, fmt_kernels::launchRangeTileUnits(c->mtHdr.p, c->sumViews.p, c->rngItems.p, static_cast<uint32_t>(ni), c->rngUnits.p,
                                                 c->numCUs, c->stream));
    FMT_HIP(c, stagedCopy(c, c->rngHostUnits.p, c->rngUnits.p, ni * sizeof(uint64_t), false));
  }
  *total = fmt_plan::rangeOffsets(P, ni && placeholder == 0 ? c->rngHostUnits.p : nullptr, nQueries, hits);
  if (out == nullptr) return FMT_OK;
  if (cap < *total) return setErr(c, FMT_E_USAGE, "fmt_mt_fetch_text_ranges: cap below the units of the ranges");
  if (*total == 0) return FMT_OK;
  // pass C: every item's units to its base in the packed text, then one staged copy of exactly those
  FMT_HIP(c, c->rngBases.reserve(ni));
  FMT_HIP(c, c->rngPacked.reserve(*total));
  FMT_HIP(c, stagedCopy(c, c->rngBases.p, P.itemBase.data(), ni * sizeof(uint64_t), true));
  FMT_HIP(c, fmt_kernels::launchRangeGather(c->mtHdr.p, c->sumViews.p, c->rngItems.p, static_cast<uint32_t>(ni), placeholder,
                                            c->rngBases.p, c->rngPacked.p, *total, c->numCUs, c->stream));
  FMT_HIP(c, stagedCopy(c, out, c->rngPacked.p, *total * sizeof(uint16_t), false));
  return FMT_OK;
}

int fmt_mt_fetch_remove_order(fmt_ctx* c, uint32_t doc, fmt_mt_remove_order* out, uint32_t cap) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(out == nullptr && cap > 0), "fmt_mt_fetch_remove_order",
                                 "fmt_mt_fetch_remove_order: bad arguments"))
    return rc;
  if (!c->mtPlan.hasRmOrder()) return FMT_OK;
  fmt_mt_doc_result h;
  FMT_HIP(c, hipMemcpy(&h, c->mtHdr.p + doc, sizeof h, hipMemcpyDeviceToHost));
  const uint32_t m = h.n_rm_order < cap ? h.n_rm_order : cap;
  if (m) FMT_HIP(c, hipMemcpy(out, c->mtRmOrder.p + c->mtPlan.rmOffs[doc], m * sizeof(fmt_mt_remove_order), hipMemcpyDeviceToHost));
  return FMT_OK;
}

// word 0 of every leaf (ids 64..127), or words 1 and 2 (ids 128..191, 192..253) with `upper`
static int fetchRmClientsHi(fmt_ctx* c, uint32_t doc, uint64_t* out, uint32_t cap, bool upper, const char* what) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(out == nullptr && cap > 0), what, std::string(what) + ": bad arguments"))
    return rc;
  fmt_mt_doc_result h;
  FMT_HIP(c, hipMemcpy(&h, c->mtHdr.p + doc, sizeof h, hipMemcpyDeviceToHost));
  const uint32_t per = upper ? fmt_huge::kHiOutWords - 1 : 1;
  const uint32_t m = h.n_leaves < cap / per ? h.n_leaves : cap / per;
  const uint64_t* src = docView(c, doc).rmHi;
  if (src != nullptr && m) {
    std::vector<uint64_t> all(static_cast<size_t>(m) * fmt_huge::kHiOutWords);
    FMT_HIP(c, hipMemcpy(all.data(), src, all.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < m; i++)
      for (uint32_t k = 0; k < per; k++) out[static_cast<size_t>(i) * per + k] = all[static_cast<size_t>(i) * fmt_huge::kHiOutWords + (upper ? 1 + k : 0)];
  } else if (m) {
    std::memset(out, 0, static_cast<size_t>(m) * per * sizeof(uint64_t));  // (the other tiers hold ids 0..63 only)
  }
  return FMT_OK;
}

int fmt_mt_fetch_rm_clients_hi(fmt_ctx* c, uint32_t doc, uint64_t* out, uint32_t cap) {
  return fetchRmClientsHi(c, doc, out, cap, false, "fmt_mt_fetch_rm_clients_hi");
}

int fmt_mt_fetch_rm_clients_hi2(fmt_ctx* c, uint32_t doc, uint64_t* out, uint32_t cap) {
  return fetchRmClientsHi(c, doc, out, cap, true, "fmt_mt_fetch_rm_clients_hi2");
}

int fmt_mt_fetch_legacy_props(fmt_ctx* c, uint32_t doc, uint16_t* out, uint32_t cap) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(out == nullptr && cap > 0), "fmt_mt_fetch_legacy_props",
                                 "fmt_mt_fetch_legacy_props: bad arguments"))
    return rc;
  fmt_mt_doc_result h;
  FMT_HIP(c, hipMemcpy(&h, c->mtHdr.p + doc, sizeof h, hipMemcpyDeviceToHost));
  const uint32_t m = h.n_leaves < cap ? h.n_leaves : cap;
  if (m == 0) return FMT_OK;
  const fmt_kernels::SumView V = docView(c, doc);
  if (V.legacyProps != nullptr) {
    FMT_HIP(c, hipMemcpy(out, V.legacyProps, m * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (out[0] == fmt_mt::kLegacyUnavailable)  // (the engine marks every leaf)
      return setErr(c, FMT_E_CAPACITY, "fmt_mt_fetch_legacy_props: the document's getAtSeq view did not fit its prop-set table");
    return FMT_OK;
  }
  std::vector<fmt_mt_leaf> lv(m);  // (no annotate-adjust in the batch: getAtSeq is the current properties)
  FMT_HIP(c, hipMemcpy(lv.data(), V.leaves, m * sizeof(fmt_mt_leaf), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < m; i++) out[i] = lv[i].props;
  return FMT_OK;
}

int fmt_mt_fetch_numbers(fmt_ctx* c, uint32_t doc, double* out, uint32_t cap, uint32_t* nOut) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(out == nullptr && cap > 0), "fmt_mt_fetch_numbers",
                                 "fmt_mt_fetch_numbers: bad arguments"))
    return rc;
  uint32_t n = 0;
  if (c->mtPlan.anyAdjust) FMT_HIP(c, hipMemcpy(&n, c->mtNumCount.p + doc, sizeof n, hipMemcpyDeviceToHost));
  if (nOut) *nOut = n;
  const uint32_t m = n < cap ? n : cap;
  if (m) FMT_HIP(c, hipMemcpy(out, c->mtNums.p + c->mtPlan.numOffs[doc], m * sizeof(double), hipMemcpyDeviceToHost));
  return FMT_OK;
}

int fmt_mt_fetch_regen(fmt_ctx* c, uint32_t doc, fmt_mt_op* ops, uint32_t capOps, uint16_t* text, uint32_t capText,
                       uint32_t* nOps, uint32_t* nText) {
  if (const int rc = mtReadEntry(c, c && doc < c->mtDocs && !(ops == nullptr && capOps > 0) && !(text == nullptr && capText > 0),
                                 "fmt_mt_fetch_regen", "fmt_mt_fetch_regen: bad arguments"))
    return rc;
  uint32_t cnt[2] = {0, 0};
  if (c->mtPlan.local) FMT_HIP(c, hipMemcpy(cnt, c->mtLocRegenCount.p + 2ull * doc, sizeof cnt, hipMemcpyDeviceToHost));
  if (nOps) *nOps = cnt[0];
  if (nText) *nText = cnt[1];
  const uint32_t m = cnt[0] < capOps ? cnt[0] : capOps, t = cnt[1] < capText ? cnt[1] : capText;
  if (m) FMT_HIP(c, hipMemcpy(ops, c->mtLocRegen.p + c->mtPlan.locSlabOffs(fmt_plan::kLocRegen)[doc], m * sizeof(fmt_mt_op), hipMemcpyDeviceToHost));
  if (t) FMT_HIP(c, hipMemcpy(text, c->mtLocRegenText.p + c->mtPlan.locSlabOffs(fmt_plan::kLocRegenText)[doc], t * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return FMT_OK;
}

// Internal diagnostic (not part of fmt.h): shader-clock totals per phase of a huge document's last
// replay (huge_engine.h HugeDoc::prof), HugeDoc::kProf values; FMT_E_USAGE if `doc` is not a huge document.
int fmt_internal_huge_profile(fmt_ctx* c, uint32_t doc, uint64_t* out) {
  if (c == nullptr || out == nullptr || doc >= c->mtHugeSlot.size() || c->mtHugeSlot[doc] < 0) return FMT_E_USAGE;
  FMT_HIP(c, hipMemcpy(out, c->huge[static_cast<size_t>(c->mtHugeSlot[doc])].out.prof, fmt_huge::HugeDoc::kProf * sizeof(uint64_t),
                       hipMemcpyDeviceToHost));
  return FMT_OK;
}

// Test hook (not part of fmt.h): the summary formatters' JSON.stringify of a number (jsnum.h).
int fmt_internal_js_number(double x, char* out, int cap) { return out == nullptr || cap < 0 ? 0 : fmt_json::jsNumber(x, out, cap); }

// Test hook (not part of fmt.h): fmt_mt_load's host half (mt_plan.h planMergeTreeLoad) with the large
// tier's capacities, no device needed. Returns the plan's status, *err its message (NULL: FMT_OK). The
// plan goes to a holder the calling thread keeps, and *out / *n_words describe the holder: a refused
// batch leaves there the plan of the thread's last valid batch, as fmt_mt_load leaves its context. Words
// 0..5: insertChars, initChars, catchupOps, rmOrderOps, flags (1 obliterates, 2 local, 4 hiClients, 8
// anyAdjust), number of documents; then 14 arrays, each its length and its elements: cuOffs, rmOffs,
// numOffs, pmOffs, locOffs, numSorted (the doubles' bits), numSortedId, numSortedOffs, loadSegs, segProps,
// docChars, startSeg (text, len, props), hugeDocs, refused (doc, status, fail_seq, cur_seq, min_seq; signed
// values sign-extended). Valid until the calling thread's next call.
int fmt_internal_mt_plan(const fmt_mt_batch* b, const char** err, const uint64_t** out, uint64_t* nWords) {
  static thread_local fmt_plan::MtPlan held;
  static thread_local std::vector<uint64_t> w;
  if (err == nullptr || out == nullptr || nWords == nullptr) return FMT_E_USAGE;
  *err = nullptr;
  const int rc = fmt_plan::planMergeTreeLoad(b, fmt_kernels::mergeTreeCaps(true), held, err);
  const fmt_plan::MtPlan& P = held;
  w.assign({P.insertChars, P.initChars, P.catchupOps, P.rmOrderOps,
            (P.obliterates ? 1ull : 0) | (P.local ? 2ull : 0) | (P.hiClients ? 4ull : 0) | (P.anyAdjust ? 8ull : 0),
            P.docChars.size()});
  auto put = [&](const auto& v) {
    w.push_back(v.size());
    w.insert(w.end(), v.begin(), v.end());
  };
  put(P.cuOffs);
  put(P.rmOffs);
  put(P.numOffs);
  put(P.pmOffs);
  put(P.locOffs);
  w.push_back(P.numSorted.size());
  for (double x : P.numSorted) {
    uint64_t bits;
    std::memcpy(&bits, &x, sizeof bits);
    w.push_back(bits);
  }
  put(P.numSortedId);
  put(P.numSortedOffs);
  put(P.loadSegs);
  put(P.segProps);
  put(P.docChars);
  w.push_back(P.startSeg.size());
  for (const fmt_mt_snapshot_seg& sg : P.startSeg) w.insert(w.end(), {sg.text, sg.len, sg.props});
  put(P.hugeDocs);
  w.push_back(P.refused.size());
  for (size_t i = 0; i < P.refused.size(); i++) {
    const fmt_mt_doc_result& h = P.refusedHdr[i];
    for (int64_t x : {int64_t{P.refused[i]}, int64_t{h.status}, int64_t{h.fail_seq}, int64_t{h.cur_seq}, int64_t{h.min_seq}})
      w.push_back(static_cast<uint64_t>(x));
  }
  *out = w.data();
  *nWords = w.size();
  return rc;
}

// Test hook (not part of fmt.h): the route fmt_mt_load plans for `b` with or without the checkpoint and step-down
// slabs, as mt_route_words.h lays it out; no device needed. rounds <= 0 / local_path < 0: this build's. Returns the
// plan's status (refused: *err says why, no words). Valid until the calling thread's next call.
int fmt_internal_mt_route(const fmt_mt_batch* b, int ckptSlab, int descSlab, int rounds, int localPath, const char** err,
                          const uint32_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint32_t> w;
  fmt_plan::MtPlan P;
  if (err == nullptr || out == nullptr || nWords == nullptr || rounds > fmt_plan::kMaxDescendRounds) return FMT_E_USAGE;
  *err = nullptr;
  const int rc = fmt_plan::planMergeTreeLoad(b, fmt_kernels::mergeTreeCaps(true), P, err);
  w.clear();
  if (rc == FMT_OK)
    w = fmt_plan::routeWords(fmt_plan::planRoute(P, ckptSlab != 0, descSlab != 0, rounds > 0 ? rounds : fmt_plan::kDescendRounds,
                                                 localPath >= 0 ? localPath : FMT_LOCAL_PATH));
  *out = w.data();
  *nWords = w.size();
  return rc;
}

// Test hook (not part of fmt_text.h): fmt_mt_fetch_text_all's host half (text_plan.h) over host headers,
// no device needed. tile_leaves 0: the kernels' tile. Words: the number of items; the items (doc, first
// leaf, leaves each); each document's first item (n_docs + 1); and, when tile_units (one per item, so
// from a second call) is given, the offsets (n_docs + 1) and every item's base. Valid until the calling
// thread's next call.
int fmt_internal_text_plan(const fmt_mt_doc_result* hdrs, uint32_t nDocs, uint32_t tileLeaves, const uint64_t* tileUnits,
                           const uint64_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint64_t> w;
  if ((nDocs && hdrs == nullptr) || out == nullptr || nWords == nullptr) return FMT_E_USAGE;
  fmt_plan::TextPlan P;
  fmt_plan::planTextTiles(hdrs, nDocs, tileLeaves, P);
  w.assign(1, P.items.size());
  for (const fmt_plan::TextItem& it : P.items) w.insert(w.end(), {it.doc, it.firstLeaf, it.nLeaves});
  w.insert(w.end(), P.docFirst.begin(), P.docFirst.end());
  if (tileUnits != nullptr) {
    std::vector<uint64_t> offs(nDocs + 1ull), base(P.items.size() + 1);
    fmt_plan::textOffsets(P, tileUnits, offs.data(), base.data());
    w.insert(w.end(), offs.begin(), offs.end());
    w.insert(w.end(), base.begin(), base.end() - 1);
  }
  *out = w.data();
  *nWords = w.size();
  return FMT_OK;
}

// Test hook (not part of fmt_runs.h): fmt_mt_fetch_prop_runs_all's host half (runs_plan.h stitchRuns) over
// host headers and one pass-1 report per work item of planTextTiles(hdrs, tileLeaves) (5 words each: units,
// heads, tail, first, last), no device needed. Words: the number of items; the offsets (n_docs + 1); per
// item its run base, position base, open start and flags. Valid until the calling thread's next call.
int fmt_internal_runs_plan(const fmt_mt_doc_result* hdrs, uint32_t nDocs, uint32_t tileLeaves, const uint32_t* tiles,
                           uint64_t nTiles, const uint64_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint64_t> w;
  if ((nDocs && hdrs == nullptr) || out == nullptr || nWords == nullptr) return FMT_E_USAGE;
  fmt_plan::TextPlan P;
  fmt_plan::planTextTiles(hdrs, nDocs, tileLeaves, P);
  if (nTiles != P.items.size() || (nTiles && tiles == nullptr)) return FMT_E_USAGE;
  static_assert(sizeof(fmt_plan::RunTile) == 5 * sizeof(uint32_t), "RunTile is five words");
  std::vector<fmt_plan::RunTile> t(P.items.size() + 1);
  if (nTiles) std::memcpy(t.data(), tiles, nTiles * sizeof(fmt_plan::RunTile));
  std::vector<uint64_t> offs(nDocs + 1ull);
  std::vector<fmt_plan::RunTileBase> base(P.items.size() + 1);
  fmt_plan::stitchRuns(P, t.data(), offs.data(), base.data());
  w.assign(1, P.items.size());
  w.insert(w.end(), offs.begin(), offs.end());
  for (size_t k = 0; k < P.items.size(); k++) w.insert(w.end(), {base[k].runBase, base[k].posBase, base[k].openStart, base[k].flags});
  *out = w.data();
  *nWords = w.size();
  return FMT_OK;
}

// Test hook (not part of fmt_pos.h): fmt_mt_query_positions' host half (pos_plan.h) over host headers, no
// device needed. tile_leaves 0: the kernels' tile. hits[n_queries] receives the records as the host leaves
// them. Words: the number of views; the views (doc, ref_seq, client, first item; signed values
// sign-extended); the number of items; the items (doc, first leaf, leaves, view); and, when tile_units (two
// per item: view, local; so from a second call) is given, the number of device queries and the queries (doc,
// first leaf, leaves, pos, ref_seq, client, view base, local base, out). Returns planPosViews' status. Valid
// until the calling thread's next call.
int fmt_internal_pos_plan(const fmt_mt_doc_result* hdrs, uint32_t nDocs, uint32_t obliterates, uint32_t tileLeaves,
                          const uint64_t* qOffsets, const fmt_mt_pos_query* q, uint64_t nQueries, const uint64_t* tileUnits,
                          uint64_t nTileUnits, fmt_mt_pos_hit* hits, const uint64_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint64_t> w;
  if ((nDocs && hdrs == nullptr) || qOffsets == nullptr || (nQueries && (q == nullptr || hits == nullptr)) || out == nullptr ||
      nWords == nullptr)
    return FMT_E_USAGE;
  fmt_plan::TextPlan T;
  fmt_plan::planTextTiles(hdrs, nDocs, tileLeaves, T);
  fmt_plan::PosPlan P;
  const int rc = fmt_plan::planPosViews(hdrs, nDocs, obliterates != 0, T, qOffsets, q, nQueries, hits, P);
  if (rc != FMT_OK) return rc;
  auto sx = [](int32_t x) { return static_cast<uint64_t>(static_cast<int64_t>(x)); };
  w.assign(1, P.views.size());
  for (const fmt_plan::PosView& v : P.views) w.insert(w.end(), {uint64_t{v.doc}, sx(v.refSeq), sx(v.client), v.firstItem});
  w.push_back(P.items.size());
  for (const fmt_plan::PosItem& it : P.items) w.insert(w.end(), {it.doc, it.firstLeaf, it.nLeaves, it.view});
  if (tileUnits != nullptr) {
    if (nTileUnits != P.items.size()) return FMT_E_USAGE;
    static_assert(sizeof(fmt_plan::PosTileUnits) == 2 * sizeof(uint64_t), "PosTileUnits is two words");
    std::vector<fmt_plan::PosTileUnits> u(P.items.size() + 1);
    std::memcpy(u.data(), tileUnits, P.items.size() * sizeof(fmt_plan::PosTileUnits));
    fmt_plan::resolvePosQueries(P, T, hdrs, u.data(), q, nQueries, hits);
    w.push_back(P.dev.size());
    for (const fmt_plan::PosDevQuery& d : P.dev)
      w.insert(w.end(), {uint64_t{d.doc}, uint64_t{d.firstLeaf}, uint64_t{d.nLeaves}, uint64_t{d.pos}, sx(d.refSeq), sx(d.client),
                         uint64_t{d.viewBase}, uint64_t{d.localBase}, d.out});
  }
  *out = w.data();
  *nWords = w.size();
  return FMT_OK;
}

// Test hook (not part of fmt_range.h): fmt_mt_fetch_text_ranges' host half (range_plan.h) over host headers, no
// device needed. tile_leaves 0: the kernels' tile. hits[n_queries] receives the records as the host leaves
// them. Words: the number of views; the views (doc, ref_seq, client, first item; signed values
// sign-extended); the number of (view, tile) items; those items (doc, first leaf, leaves, view); when
// tile_units (two per such item: view, local; so from a second call) is given, the number of range items
// and the items (doc, first leaf, leaves, lo, hi, ref_seq, client, query); and, when placeholder != 0 or
// item_units (one per range item, so from a third call) is given, every item's base and *total. Returns the
// plan's status. Valid until the calling thread's next call.
int fmt_internal_range_plan(const fmt_mt_doc_result* hdrs, uint32_t nDocs, uint32_t obliterates, uint32_t tileLeaves,
                            uint32_t placeholder, const uint64_t* qOffsets, const fmt_mt_range_query* q, uint64_t nQueries,
                            const uint64_t* tileUnits, uint64_t nTileUnits, const uint64_t* itemUnits, uint64_t nItemUnits,
                            fmt_mt_range_hit* hits, uint64_t* total, const uint64_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint64_t> w;
  if ((nDocs && hdrs == nullptr) || qOffsets == nullptr || (nQueries && (q == nullptr || hits == nullptr)) || total == nullptr ||
      out == nullptr || nWords == nullptr)
    return FMT_E_USAGE;
  fmt_plan::TextPlan T;
  fmt_plan::planTextTiles(hdrs, nDocs, tileLeaves, T);
  fmt_plan::RangePlan P;
  int rc = fmt_plan::planRangeViews(hdrs, nDocs, obliterates != 0, T, qOffsets, q, nQueries, hits, P);
  if (rc != FMT_OK) return rc;
  *total = 0;
  auto sx = [](int32_t x) { return static_cast<uint64_t>(static_cast<int64_t>(x)); };
  w.assign(1, P.views.views.size());
  for (const fmt_plan::PosView& v : P.views.views) w.insert(w.end(), {uint64_t{v.doc}, sx(v.refSeq), sx(v.client), v.firstItem});
  w.push_back(P.views.items.size());
  for (const fmt_plan::PosItem& it : P.views.items) w.insert(w.end(), {it.doc, it.firstLeaf, it.nLeaves, it.view});
  if (tileUnits != nullptr) {
    if (nTileUnits != P.views.items.size()) return FMT_E_USAGE;
    std::vector<fmt_plan::PosTileUnits> u(P.views.items.size() + 1);
    std::memcpy(u.data(), tileUnits, P.views.items.size() * sizeof(fmt_plan::PosTileUnits));
    rc = fmt_plan::cutRanges(P, T, u.data(), q, nQueries, hits);
    if (rc != FMT_OK) return rc;
    w.push_back(P.items.size());
    for (size_t k = 0; k < P.items.size(); k++) {
      const fmt_plan::RangeItem& it = P.items[k];
      w.insert(w.end(), {uint64_t{it.doc}, uint64_t{it.firstLeaf}, uint64_t{it.nLeaves}, uint64_t{it.lo}, uint64_t{it.hi}, sx(it.refSeq),
                         sx(it.client), P.itemQuery[k]});
    }
    if (placeholder != 0 || itemUnits != nullptr) {
      if (placeholder == 0 && nItemUnits != P.items.size()) return FMT_E_USAGE;
      *total = fmt_plan::rangeOffsets(P, placeholder == 0 ? itemUnits : nullptr, nQueries, hits);
      w.insert(w.end(), P.itemBase.begin(), P.itemBase.end());
    }
  }
  *out = w.data();
  *nWords = w.size();
  return FMT_OK;
}

// Test hook (not part of fmt.h): the HBM map tier's host half (map_plan.h planMapLarge) over a batch's
// doc_op_offsets and a list of overflowing documents, no device needed. Returns FMT_OK, or FMT_E_USAGE with
// *err the reason. Words 0..11: tile size, scratch bytes, slots, ops, then the region starts in words (key,
// first, D, last, value, op slot, tile counts, last clear); then three arrays, each its length and its
// elements: documents (doc, n_ops, slots, table_off, op_slot_off, first_tile, n_tiles, shift each), tileDoc,
// tileFirst. Valid until the calling thread's next call.
int fmt_internal_map_large_plan(const uint64_t* docOpOffsets, uint32_t nDocs, const uint32_t* overflow, uint32_t nOverflow,
                                const char** err, const uint64_t** out, uint64_t* nWords) {
  static thread_local std::vector<uint64_t> w;
  if (docOpOffsets == nullptr || (nOverflow && overflow == nullptr) || err == nullptr || out == nullptr || nWords == nullptr)
    return FMT_E_USAGE;
  fmt_plan::MapLargePlan P;
  *err = fmt_plan::planMapLarge(docOpOffsets, nDocs, overflow, nOverflow, P);
  w.assign({fmt_plan::kMapLargeTile, P.scratchBytes(), P.slots, P.ops, P.keyAt(), P.firstAt(), P.delAt(), P.lastAt(),
            P.valueAt(), P.opSlotAt(), P.tileCountAt(), P.clearAt()});
  w.push_back(P.docs.size());
  for (const fmt_plan::MapLargeDoc& d : P.docs)
    w.insert(w.end(), {d.doc, d.nOps, uint64_t{d.mask} + 1, d.tableOff, d.opSlotOff, d.firstTile, d.nTiles, d.shift});
  w.push_back(P.tileDoc.size());
  w.insert(w.end(), P.tileDoc.begin(), P.tileDoc.end());
  w.push_back(P.tileFirst.size());
  w.insert(w.end(), P.tileFirst.begin(), P.tileFirst.end());
  *out = w.data();
  *nWords = w.size();
  return *err ? FMT_E_USAGE : FMT_OK;
}

// Test hook (not part of fmt_v1.h): fmt_mt_summarize_v1's host formatter (v1Blobs) over one document
// given as host arrays, no device needed. segs: n_segs fmt_kernels::SumV1Seg records (kernels.h) and
// their text back to back; rm: the remove-order entries (later stamps); numbers: the document's
// computed annotate-adjust numbers or NULL; names[k]: JSON-quoted name of short client k. *out: the
// header blob then the bodies, ends[0 .. *n_blobs) where each ends; both stay valid until the calling
// thread's next call. Returns the document's V1 status (FMT_E_DATA: a prop set outside the tables).
int fmt_internal_v1_format(const void* segs, uint32_t nSegs, const uint16_t* text, const fmt_mt_propset* props,
                           uint32_t nProps, const fmt_mt_remove_order* rm, uint32_t nRm, const double* numbers,
                           uint32_t nNumbers, const char* const* keys, uint32_t nKeys, const char* const* values,
                           uint32_t nValues, const char* const* names, uint32_t nNames, int32_t minSeq, int32_t curSeq,
                           uint32_t chunk, const char** out, const uint64_t** ends, uint32_t* nBlobs) {
  static thread_local std::string blob;
  static thread_local std::vector<uint64_t> blobEnds;
  if (out == nullptr || ends == nullptr || nBlobs == nullptr || (nSegs && segs == nullptr)) return FMT_E_USAGE;
  blob.clear();
  blobEnds.clear();
  const auto* S = static_cast<const fmt_kernels::SumV1Seg*>(segs);
  SumDict D;
  makeDict(D, keys, nKeys, values, nValues);
  const std::vector<double> numVec(numbers, numbers + (numbers ? nNumbers : 0));
  const std::vector<double>* nums = numbers ? &numVec : nullptr;
  int rc = FMT_OK;
  for (uint32_t i = 0; i < nSegs && rc == FMT_OK; i++)
    if (!propSetInTables(props, nProps, S[i].props, nKeys, 0u, nValues, nums)) rc = FMT_E_DATA;
  if (rc == FMT_OK) rc = v1Blobs(blob, blobEnds, S, nSegs, text, props, rm, nRm, names, nNames, minSeq, curSeq,
                                 chunk ? chunk : 10000u, D, nums, 0u);
  *out = blob.data();
  *ends = blobEnds.data();
  *nBlobs = rc == FMT_OK ? static_cast<uint32_t>(blobEnds.size()) : 0u;
  return rc;
}

// Test hook (not part of fmt.h): fmt_mt_summarize_legacy's host formatter (legacyBlobs) over one
// document given as host arrays, no device needed. runs: n_runs fmt_kernels::SumRun records
// (kernels.h) and their text back to back; numbers: the document's computed annotate-adjust numbers or
// NULL. *out: the header blob then the body, ends[0 .. *n_blobs) where each ends (one blob: no body);
// both stay valid until the calling thread's next call. Returns FMT_E_DATA for a prop set outside the
// tables.
int fmt_internal_legacy_format(const void* runs, uint32_t nRuns, const uint16_t* text, const fmt_mt_propset* props,
                               uint32_t nProps, const double* numbers, uint32_t nNumbers, const char* const* keys,
                               uint32_t nKeys, const char* const* values, uint32_t nValues, int32_t minSeq,
                               uint32_t chunk, const char** out, const uint64_t** ends, uint32_t* nBlobs) {
  static thread_local std::string blob;
  static thread_local std::vector<uint64_t> blobEnds;
  if (out == nullptr || ends == nullptr || nBlobs == nullptr || (nRuns && runs == nullptr)) return FMT_E_USAGE;
  blob.clear();
  blobEnds.clear();
  const auto* R = static_cast<const fmt_kernels::SumRun*>(runs);
  SumDict D;
  makeDict(D, keys, nKeys, values, nValues);
  const std::vector<double> numVec(numbers, numbers + (numbers ? nNumbers : 0));
  const std::vector<double>* nums = numbers ? &numVec : nullptr;
  int rc = FMT_OK;
  for (uint32_t i = 0; i < nRuns && rc == FMT_OK; i++)
    if (!propSetInTables(props, nProps, R[i].props, nKeys, 0u, nValues, nums)) rc = FMT_E_DATA;
  if (rc == FMT_OK) {
    uint32_t split = 0;
    legacyBlobs(blob, &split, R, nRuns, text, props, minSeq, chunk ? chunk : 10000u, D, nums, 0u);
    blobEnds.push_back(split);
    if (blob.size() > split) blobEnds.push_back(blob.size());
  }
  *out = blob.data();
  *ends = blobEnds.data();
  *nBlobs = static_cast<uint32_t>(blobEnds.size());
  return rc;
}

// Test hook (not part of fmt_map_summary.h): fmt_map_summarize's host half (map_sum_plan.h) over fetched
// sparse entries (fmt_map_fetch_sparse's counts and packed birth-ordered entries), no device needed:
// tables, ordering, blob scan and formatter on `threads` host threads (0: 1). ordered / tags (the live
// entries each), n_blobs / status (n_docs each) may be NULL. *docs: per document where its header
// starts, its blobs following; *piece_at (n_docs + 1) and *ends as MapSumBlobs. A document with status
// FMT_E_USAGE has no pieces. All valid until the calling thread's next call.
int fmt_internal_map_summary_format(const uint32_t* counts, const fmt_map_entry* entries, uint32_t nDocs,
                                    const char* const* keys, uint32_t nKeys, const char* const* values, uint32_t nValues,
                                    uint32_t threads, fmt_map_entry* ordered, uint32_t* tags, uint32_t* nBlobs, int32_t* status,
                                    const char* const** docs, const uint64_t** pieceAt, const uint64_t** ends) {
  static thread_local fmt_plan::MapSumBlobs B;
  static thread_local std::vector<const char*> docPtr;
  if ((nDocs && counts == nullptr) || (nKeys && keys == nullptr) || (nValues && values == nullptr) || docs == nullptr ||
      pieceAt == nullptr || ends == nullptr)
    return FMT_E_USAGE;
  const uint32_t nt = threads ? threads : 1u;
  std::vector<uint64_t> at(nDocs + 1ull, 0);
  for (uint32_t d = 0; d < nDocs; d++) at[d + 1] = at[d] + counts[d];
  const uint64_t n = at[nDocs];
  if (n && entries == nullptr) return FMT_E_USAGE;
  fmt_plan::MapSumTables T;
  fmt_plan::mapSumBuildTables(keys, nKeys, values, nValues, nt, T);
  std::vector<fmt_map_entry> ord(n);
  std::vector<uint32_t> tg(n), nb(nDocs);
  std::vector<int32_t> st(nDocs, FMT_OK);
  fmt_plan::mapSumOrderDocs(entries, at.data(), ord.data(), tg.data(), nb.data(), counts, at.data(), nDocs, T, nt,
                            [](uint32_t) { return true; });
  for (uint32_t d = 0; d < nDocs; d++)
    if (!fmt_plan::mapSumInTables(ord.data() + at[d], counts[d], nKeys, nValues)) st[d] = FMT_E_USAGE;
  fmt_plan::mapSumFormat(ord.data(), tg.data(), nb.data(), counts, at.data(), st.data(), nDocs, keys, values, T, nt, B);
  docPtr.assign(nDocs, nullptr);
  for (uint32_t d = 0; d < nDocs; d++) docPtr[d] = B.buf[B.docThread[d]].data() + B.docAt[d];
  if (ordered && n) std::memcpy(ordered, ord.data(), n * sizeof(fmt_map_entry));
  if (tags && n) std::memcpy(tags, tg.data(), n * sizeof(uint32_t));
  if (nBlobs && nDocs) std::memcpy(nBlobs, nb.data(), nDocs * sizeof(uint32_t));
  if (status && nDocs) std::memcpy(status, st.data(), nDocs * sizeof(int32_t));
  *docs = docPtr.data();
  *pieceAt = B.pieceAt.data();
  *ends = B.ends.data();
  return FMT_OK;
}

// Test hook: the ordered entries, tags (the live entries each) and blob counts (n_docs) of the last
// fmt_map_summarize as they came back from the device (documents past the device tier: as the host
// ordered them), packed in document order.
int fmt_internal_map_summary_arrays(fmt_ctx* c, fmt_map_entry* ordered, uint32_t* tags, uint32_t* nBlobs, uint64_t cap) {
  if (c == nullptr || !c->mapSumDone) return setErr(c, FMT_E_USAGE, "fmt_internal_map_summary_arrays before fmt_map_summarize");
  const uint32_t nd = c->mapDocs;
  const uint64_t n = c->mapSumN;
  if (cap < n) return setErr(c, FMT_E_USAGE, "fmt_internal_map_summary_arrays: cap below the live entries");
  const uint32_t* host = c->mapSumHost.p;
  if (ordered && n) std::memcpy(ordered, host, n * sizeof(fmt_map_entry));
  if (tags && n) std::memcpy(tags, host + 3 * n, n * sizeof(uint32_t));
  if (nBlobs && nd) std::memcpy(nBlobs, host + 4 * n, nd * sizeof(uint32_t));
  return FMT_OK;
}

// Measurement switch (tools/bench_map_summary.py only): on != 0 makes fmt_map_summarize skip the device
// tier and order every document with map_sum_plan.h on its host threads.
int fmt_internal_map_summary_host_only(fmt_ctx* c, int on) {
  if (c == nullptr) return FMT_E_USAGE;
  c->mapSumHostOnly = on != 0;
  return FMT_OK;
}

// Internal diagnostic (not part of fmt.h): per-phase cycle totals of a FMT_PROFILE=1 build.
int fmt_internal_mt_profile(uint64_t* out, int n, int reset) {
  return fmt_kernels::mergeTreeProfile(out, n, reset != 0);
}

}  // extern "C"

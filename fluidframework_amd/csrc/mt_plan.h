// mt_plan.h — the host-only half of fmt_mt_load: everything a merge-tree batch decides before the
// device is touched. planMergeTreeLoad validates the batch (every refusal of fmt_mt_load that is not a
// device error, in a fixed order), sizes the per-document slabs, sorts the host numbers of an
// annotate-adjust batch and routes summary-loaded documents past the large tier to the huge tier.
// runtime.cpp stages the result on the device; tests reach it without one (fmt_internal_mt_plan), and
// the host emulations (tests/emu) share prepareSortedNumbers. No HIP include, no fmt_ctx.
#pragma once

#include <algorithm>
#include <cstdint>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/fmt.h"

namespace fmt_plan {

// Host threads for the passes over a batch (validation, per-document sizing).
inline unsigned hostWorkers() { return std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// fn(begin, end, worker) over hostWorkers() contiguous shares of [0, n) (one share below 2^16 items).
template <class F>
void parallelChunks(uint64_t n, F&& fn) {
  const unsigned T = n < (1u << 16) ? 1u : hostWorkers();
  if (T == 1) {
    fn(0, n, 0u);
    return;
  }
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < T; t++) pool.emplace_back([&, t] { fn(n * t / T, n * (t + 1) / T, t); });
  for (auto& th : pool) th.join();
}

// Per-document slab sizes (a document that needs more reports FMT_E_CAPACITY at replay); 0 for a
// document without the feature.
// Catch-up ranges: 16 per flagged op + 16.
constexpr uint64_t kCatchupPerOp = 16, kCatchupPerDoc = 16;
inline uint64_t catchupSlab(uint64_t flagged) { return flagged ? flagged * kCatchupPerOp + kCatchupPerDoc : 0; }
// Remove-order entries (split copies included): 64 per flagged remove + 256.
constexpr uint64_t kRmPerOp = 64, kRmPerDoc = 256;
inline uint64_t rmOrderSlab(uint64_t flagged) { return flagged ? flagged * kRmPerOp + kRmPerDoc : 0; }
// Computed numbers: 64 per adjust entry of the document's annotates + 64, at most 0x7fff (the computed id
// range: one adjust over a range can compute a new number per leaf it hits).
constexpr uint64_t kNumPerAdjust = 64, kNumPerDoc = 64, kNumMax = 0x7FFF;
inline uint64_t numberSlab(uint64_t adjusts) { return adjusts ? std::min(kNumPerAdjust * adjusts + kNumPerDoc, kNumMax) : 0; }
// PropertiesManager records (mt_engine.h Doc::pm*): 32 per kv word of the document's annotates + 256.
constexpr uint64_t kPmPerWord = 32, kPmPerDoc = 256, kPmMax = 1u << 20;
inline uint64_t pmSlab(uint64_t kvWords) { return kvWords ? std::min(kPmPerWord * kvWords + kPmPerDoc, kPmMax) : 0; }
// f4, a document's local records (mt_engine.h LocalTables), in the order of MtPlan::locOffs: 4 + 2
// pending groups per submission (a reconnect replaces a group by one per segment), 32 group records per
// submission (hits and split copies; deleted ones compact away), 64 PropertiesManager records per key
// of a local annotate (annotate-adjust batches: + 32 per key of any annotate, whose remote changes stay
// listed until minSeq passes them), regenerated ops / text per reconnect, and normalization scratch for
// a document that reconnects. leaves / chars: the large tier's.
enum { kLocGroups, kLocRecs, kLocPm, kLocRegen, kLocRegenText, kLocScratch, kLocSlabs };
inline void localSlabs(uint64_t sub, uint64_t keys, uint64_t regens, uint64_t text, uint64_t leaves, uint64_t chars,
                       uint64_t cap[kLocSlabs]) {
  cap[kLocGroups] = sub ? std::min<uint64_t>(6 * sub + 64 + (regens ? leaves : 0), 1u << 22) : 0;
  cap[kLocRecs] = sub ? std::min<uint64_t>(32 * sub + 1024, 1u << 24) : 0;
  cap[kLocPm] = keys ? std::min<uint64_t>(64 * keys + 512, 1u << 22) : 0;
  cap[kLocRegen] = regens ? std::min<uint64_t>(regens * std::min<uint64_t>(8 * sub + 64, leaves), 1u << 22) : 0;
  cap[kLocRegenText] = regens ? std::min<uint64_t>(regens * std::min<uint64_t>(text, chars) + 64, 1u << 26) : 0;
  cap[kLocScratch] = regens ? 15ull * leaves + chars / 2 + 64 : 0;
}

// The host's numbers ascending (NaN skipped, -0 as 0), each once with the first value id that holds it:
// one list of ids 0 .. nValues for the batch, or per document with its local ids 1 .. (docValueBase; value
// id v of document d is valueNum[docValueBase[d] + v]) and numSortedOffs[d] where document d's list
// starts (empty for batch-global ids).
inline void prepareSortedNumbers(const double* valueNum, uint32_t nValues, const uint32_t* docValueBase, uint32_t nDocs,
                                 std::vector<double>& numSorted, std::vector<uint32_t>& numSortedId,
                                 std::vector<uint32_t>& numSortedOffs) {
  numSorted.clear();
  numSortedId.clear();
  numSortedOffs.clear();
  auto sortNumbers = [&](uint32_t lo, uint32_t hi, uint32_t base) {
    std::vector<std::pair<double, uint32_t>> nums;
    for (uint32_t i = lo; valueNum && i < hi; i++)
      if (valueNum[base + i] == valueNum[base + i]) nums.emplace_back(valueNum[base + i] == 0.0 ? 0.0 : valueNum[base + i], i);
    std::stable_sort(nums.begin(), nums.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    const size_t first = numSorted.size();
    for (const auto& [x, i] : nums) {
      if (numSorted.size() > first && numSorted.back() == x) continue;  // (one text per number: the first id)
      numSorted.push_back(x);
      numSortedId.push_back(i);
    }
  };
  if (docValueBase == nullptr) {
    sortNumbers(0, nValues, 0);
    return;
  }
  numSortedOffs.assign(1, 0);
  for (uint32_t d = 0; d < nDocs; d++) {
    sortNumbers(1, docValueBase[d + 1] - docValueBase[d] + 1, docValueBase[d]);
    numSortedOffs.push_back(static_cast<uint32_t>(numSorted.size()));
  }
}

struct MtPlan {
  // totals and flags of the op scan, the snapshot segments and the props ops
  uint64_t insertChars = 0;  // units of every insert op and snapshot segment
  uint64_t initChars = 0;    // units of doc_init
  uint64_t catchupOps = 0, rmOrderOps = 0;  // FMT_MT_F_CATCHUP / FMT_MT_F_RMORDER ops
  bool obliterates = false;  // launch the Doc<true> kernels
  bool local = false;        // f4: some op has a FMT_MT_F_LOCAL_ANY flag
  bool hiClients = false;    // some op or merge-info stamp names a short client id 64..253 (huge tier only)
  bool anyAdjust = false;    // the props ops hold annotate-adjust entries
  // slab offsets, n_docs + 1 each; empty when the batch lacks the feature
  std::vector<uint64_t> cuOffs, rmOffs, numOffs, pmOffs;
  std::vector<uint64_t> locOffs;  // kLocSlabs arrays of n_docs + 1, back to back
  // annotate-adjust batches: prepareSortedNumbers
  std::vector<double> numSorted;
  std::vector<uint32_t> numSortedId, numSortedOffs;
  // per document
  std::vector<uint32_t> loadSegs;           // its FMT_MT_F_LOADSEG ops (V1 body segments)
  std::vector<uint8_t> segProps;            // a loaded segment has properties
  std::vector<uint64_t> docChars;           // start units + inserted units (its most text)
  std::vector<fmt_mt_snapshot_seg> startSeg;  // its doc_init text as one segment (len 0: none)
  // routing: summary-loaded documents past the large tier, ascending. They start in the huge tier
  // (hugeDocs), except in a local batch, whose records the huge tier lacks: those fail alone
  // (refused, with the headers they report)
  std::vector<uint32_t> hugeDocs, refused;
  std::vector<fmt_mt_doc_result> refusedHdr;

  bool hasCatchup() const { return catchupOps > 0; }
  bool hasRmOrder() const { return rmOrderOps > 0; }
  const uint64_t* locSlabOffs(int slab) const { return locOffs.data() + slab * (locOffs.size() / kLocSlabs); }
};

// The header of a summary-loaded document that fails alone at load.
inline fmt_mt_doc_result refusalHeader(const fmt_mt_snapshot_doc& sd, int status) {
  fmt_mt_doc_result h{};
  h.status = status;
  h.fail_seq = sd.seq;
  h.cur_seq = sd.seq;
  h.min_seq = sd.min_seq;
  return h;
}

// Validates `b` and plans its load. Returns FMT_OK, or the refusal's status with *err naming it (a
// string literal); `out` is assigned only on FMT_OK. large: the large tier's capacities (anything with
// .leaves and .chars: fmt_kernels::MtCaps, whose header needs HIP).
template <class Caps>
int planMergeTreeLoad(const fmt_mt_batch* b, const Caps& large, MtPlan& out, const char** err) {
  auto refuse = [&](int code, const char* what) {
    *err = what;
    return code;
  };
  if (b == nullptr || b->doc_op_offsets == nullptr || (b->n_ops && b->ops == nullptr))
    return refuse(FMT_E_USAGE, "fmt_mt_load: bad arguments");
  const uint32_t n = b->n_docs;
  if (b->doc_op_offsets[0] != 0 || b->doc_op_offsets[n] != b->n_ops)
    return refuse(FMT_E_USAGE, "doc_op_offsets do not cover ops");
  // (a document's op count is offsets[d + 1] - offsets[d] on the device: a descending pair would wrap)
  for (uint32_t d = 0; d < n; d++)
    if (b->doc_op_offsets[d + 1] < b->doc_op_offsets[d]) return refuse(FMT_E_USAGE, "doc_op_offsets not ascending");
  MtPlan P;
  // one pass over the op records on host threads: totals, and the first invalid record
  struct OpScan {
    uint64_t insertChars = 0, catchupOps = 0, rmOrderOps = 0;
    bool obliterates = false, local = false, hiClients = false;
    uint64_t errAt = ~0ull;
    int errCode = FMT_OK;
    const char* err = nullptr;
  };
  std::vector<OpScan> scans(hostWorkers());
  parallelChunks(b->n_ops, [&](uint64_t lo, uint64_t hi, unsigned t) {
    OpScan& S = scans[t];
    auto bad = [&](uint64_t i, int code, const char* what) {
      S.errAt = i;
      S.errCode = code;
      S.err = what;
    };
    for (uint64_t i = lo; i < hi; i++) {
      const fmt_mt_op& op = b->ops[i];
      if (op.flags & FMT_MT_F_CATCHUP) S.catchupOps++;
      if (op.flags & FMT_MT_F_RMORDER) S.rmOrderOps++;
      if (op.flags & FMT_MT_F_LOCAL_ANY) S.local = true;
      if (op.client > 63 && op.client != FMT_MT_CLIENT_NONCOLLAB) S.hiClients = true;
      if (op.flags & FMT_MT_F_LOADSEG) {  // a SnapshotV1 body segment: its merge info row in range
        if (op.type != FMT_MT_INSERT || b->snapshot_info == nullptr || op.pos1 < 0 ||
            static_cast<uint64_t>(op.pos1) >= b->n_snapshot_segs ||
            b->snapshot_info[op.pos1].rm_first + static_cast<uint64_t>(b->snapshot_info[op.pos1].rm_count) > b->n_snapshot_stamps)
          return bad(i, FMT_E_DATA, "a loader segment (FMT_MT_F_LOADSEG) without a valid merge-info row");
      }
      if (op.type == FMT_MT_INSERT) {
        if (static_cast<uint64_t>(op.payload) + fmt_mt_op_len(&op) > b->text_len)
          return bad(i, FMT_E_DATA, "insert payload outside the text arena");
        S.insertChars += fmt_mt_op_len(&op);
      } else if (op.type == FMT_MT_ANNOTATE) {
        if (op.payload >= b->n_props_ops) return bad(i, FMT_E_DATA, "annotate props op id out of range");
      } else if (op.type == FMT_MT_OBLITERATE || op.type == FMT_MT_OBLITERATE_SIDED) {
        S.obliterates = true;
      } else if (op.type != FMT_MT_REMOVE) {
        return bad(i, FMT_E_UNSUPPORTED, "op type not supported by this engine build");
      }
    }
  });
  const OpScan* firstBad = nullptr;
  for (const OpScan& S : scans) {
    P.insertChars += S.insertChars;
    P.catchupOps += S.catchupOps;
    P.rmOrderOps += S.rmOrderOps;
    P.obliterates = P.obliterates || S.obliterates;
    P.local = P.local || S.local;
    P.hiClients = P.hiClients || S.hiClients;
    if (S.err != nullptr && (firstBad == nullptr || S.errAt < firstBad->errAt)) firstBad = &S;
  }
  if (firstBad != nullptr) return refuse(firstBad->errCode, firstBad->err);
  // f4 batches run the Loc variants (annotate-adjust and remote ops with relative positions too):
  // features they do not combine with are refused
  if (P.local && (P.obliterates || P.catchupOps || P.rmOrderOps || b->snapshot_info != nullptr))
    return refuse(FMT_E_UNSUPPORTED,
                  "local-client records (FMT_MT_F_LOCAL_ANY) do not combine with obliterate, catch-up, remove order "
                  "or SnapshotV1 merge info");
  if (b->snapshots) {
    for (uint32_t d = 0; d < n; d++) {
      const fmt_mt_snapshot_doc& sd = b->snapshots[d];
      if (!sd.loaded) continue;
      if (b->snapshot_segs == nullptr || sd.first_seg + sd.n_header + sd.n_body > b->n_snapshot_segs)
        return refuse(FMT_E_USAGE, "snapshot segments out of range");
      for (uint64_t k = sd.first_seg; k < sd.first_seg + sd.n_header + sd.n_body; k++) {
        const fmt_mt_snapshot_seg& sg = b->snapshot_segs[k];
        const uint32_t len = sg.len & ~FMT_MT_SEG_MARKER;
        if ((sg.len & FMT_MT_SEG_MARKER) != 0 && len != 1) return refuse(FMT_E_DATA, "a marker segment has length 1");
        if (static_cast<uint64_t>(sg.text) + len > b->text_len)
          return refuse(FMT_E_DATA, "snapshot segment text outside the text arena");
        if (sg.props != FMT_MT_NO_PROPS && sg.props >= b->n_props_ops)
          return refuse(FMT_E_DATA, "snapshot segment props op id out of range");
        P.insertChars += len;
      }
    }
  }
  if (b->doc_init) {
    for (uint32_t d = 0; d < n; d++) {
      if (static_cast<uint64_t>(b->doc_init[2 * d]) + b->doc_init[2 * d + 1] > b->text_len)
        return refuse(FMT_E_DATA, "initial text outside the text arena");
      P.initChars += b->doc_init[2 * d + 1];
    }
  }
  // Annotate-adjust entries (FMT_MT_VALUE_ADJUST + row index) in the props ops: per document they size
  // its computed-number slab and decide whether its legacy summary is exact.
  const uint32_t nKv = b->props_off ? b->props_off[b->n_props_ops] : 0;
  std::vector<uint32_t> adjCount(b->n_props_ops, 0);  // adjust entries per props op
  for (uint32_t op = 0; b->props_off && op < b->n_props_ops; op++) {
    const uint32_t a = b->props_off[op], e = b->props_off[op + 1];
    if (a > e || e > nKv) return refuse(FMT_E_USAGE, "props_off is not ascending");
    for (uint32_t t = a; t < e; t++) {
      if ((b->props_kv[t] & 0xFFFFu) != FMT_MT_VALUE_ADJUST) continue;
      if (t + 1 >= e || b->adjusts == nullptr || b->props_kv[t + 1] >= b->n_adjusts)
        return refuse(FMT_E_DATA, "annotate-adjust entry without a valid adjust row");
      adjCount[op]++;
      P.anyAdjust = true;
      t++;
    }
  }
  if (b->doc_value_base != nullptr) {
    for (uint32_t d = 0; d < n; d++)
      if (b->doc_value_base[d + 1] < b->doc_value_base[d]) return refuse(FMT_E_USAGE, "doc_value_base is not ascending");
    if (b->value_num != nullptr && b->doc_value_base[n] >= b->n_values)
      return refuse(FMT_E_USAGE, "doc_value_base reaches past value_num");
  }
  if (P.anyAdjust) {
    if (b->value_num == nullptr && b->n_values > 0) return refuse(FMT_E_USAGE, "adjusts need value_num");
    for (uint32_t t = 0; t < nKv; t++) {
      const uint32_t v = b->props_kv[t] & 0xFFFFu;
      if (v == FMT_MT_VALUE_ADJUST) t++;
      else if (v >= FMT_MT_VALUE_COMPUTED)
        return refuse(FMT_E_USAGE, "host value ids must stay below FMT_MT_VALUE_COMPUTED in a batch with adjusts");
    }
    prepareSortedNumbers(b->value_num, b->n_values, b->doc_value_base, n, P.numSorted, P.numSortedId, P.numSortedOffs);
  }
  if (b->snapshots != nullptr && b->snapshot_info != nullptr) {
    for (uint64_t k = 0; k < b->n_snapshot_stamps && !P.hiClients; k++) P.hiClients = b->snapshot_stamps[k].client > 63;
    for (uint64_t k = 0; k < b->n_snapshot_segs && !P.hiClients; k++) P.hiClients = b->snapshot_info[k].ins_client > 63;
  }
  // The batch is valid. One walk over each document's ops and start, on host threads: every slab's
  // size goes to the document's place in its offset array (summed below), the per-document facts of
  // the huge tier to theirs.
  const uint64_t n1 = n + 1ull;
  if (P.hasCatchup()) P.cuOffs.assign(n1, 0);
  if (P.hasRmOrder()) P.rmOffs.assign(n1, 0);
  if (P.anyAdjust) P.numOffs.assign(n1, 0);
  if (P.anyAdjust) P.pmOffs.assign(n1, 0);
  if (P.local) P.locOffs.assign(kLocSlabs * n1, 0);
  P.loadSegs.assign(n, 0);
  P.segProps.assign(n, 0);
  P.docChars.assign(n, 0);
  P.startSeg.assign(n, fmt_mt_snapshot_seg{0, 0, FMT_MT_NO_PROPS});
  std::vector<uint8_t> pastLarge(n, 0);  // a summary-loaded document with more than the large tier holds
  // (the props ops of the annotates are looked up only where a slab is sized from them)
  const bool sizeAnnotates = (P.anyAdjust || P.local) && b->props_off != nullptr;
  constexpr uint32_t kSizingFlags = FMT_MT_F_CATCHUP | FMT_MT_F_RMORDER | FMT_MT_F_REGEN | FMT_MT_F_LOADSEG | FMT_MT_F_LOCAL;
  parallelChunks(n, [&](uint64_t d0, uint64_t d1, unsigned) {
    for (uint64_t d = d0; d < d1; d++) {
      uint64_t cu = 0, rm = 0, adj = 0, kvWords = 0, sub = 0, keys = 0, regens = 0, text = 0, chars = 0;
      uint32_t loadSegs = 0;
      // the document's text and the flags it holds: a loop without a branch on the op type, which is as
      // good as random (this is all a plain document costs, as before the split); then the counts, for a
      // document that holds something a slab or the huge tier counts, over ops that are still in cache
      uint32_t seen = 0;
      for (uint64_t i = b->doc_op_offsets[d]; i < b->doc_op_offsets[d + 1]; i++) {
        const fmt_mt_op& op = b->ops[i];
        chars += op.type == FMT_MT_INSERT ? fmt_mt_op_len(&op) : 0;
        seen |= op.flags;
      }
      const bool counted = (seen & kSizingFlags) != 0 || sizeAnnotates;
      for (uint64_t i = b->doc_op_offsets[d]; counted && i < b->doc_op_offsets[d + 1]; i++) {
        const fmt_mt_op& op = b->ops[i];
        const bool sent = (op.flags & FMT_MT_F_LOCAL) != 0;  // a submission of the local client
        cu += (op.flags & FMT_MT_F_CATCHUP) ? 1 : 0;
        rm += (op.flags & FMT_MT_F_RMORDER) ? 1 : 0;
        regens += (op.flags & FMT_MT_F_REGEN) ? 1 : 0;
        loadSegs += (op.flags & FMT_MT_F_LOADSEG) ? 1 : 0;
        sub += sent ? 1 : 0;
        if (sent && op.type == FMT_MT_INSERT) text += fmt_mt_op_len(&op);
        if (sizeAnnotates && op.type == FMT_MT_ANNOTATE) {
          const uint64_t words = b->props_off[op.payload + 1] - b->props_off[op.payload];
          adj += adjCount[op.payload];
          kvWords += words;
          if (sent) keys += words;
          else if (P.anyAdjust && !(op.flags & FMT_MT_F_ROLLBACK)) keys += (words + 1) / 2;
        }
      }
      if (P.hasCatchup()) P.cuOffs[d + 1] = catchupSlab(cu);
      if (P.hasRmOrder()) P.rmOffs[d + 1] = rmOrderSlab(rm);
      if (P.anyAdjust) P.numOffs[d + 1] = numberSlab(adj);
      if (P.anyAdjust) P.pmOffs[d + 1] = pmSlab(kvWords);
      if (P.local) {
        uint64_t cap[kLocSlabs];
        localSlabs(sub, keys, regens, text, large.leaves, large.chars, cap);
        for (int k = 0; k < kLocSlabs; k++) P.locOffs[k * n1 + d + 1] = cap[k];
      }
      P.loadSegs[d] = loadSegs;
      if (b->snapshots && b->snapshots[d].loaded) {
        const fmt_mt_snapshot_doc& sd = b->snapshots[d];
        uint64_t segChars = 0;
        for (uint64_t k = sd.first_seg; k < sd.first_seg + sd.n_header + sd.n_body; k++) {
          if (b->snapshot_segs[k].props != FMT_MT_NO_PROPS) P.segProps[d] = 1;
          segChars += b->snapshot_segs[k].len & ~FMT_MT_SEG_MARKER;
        }
        chars += segChars;
        // (a V1 summary with merge info brings its body as loader-segment ops: they count as loaded)
        const uint64_t loaded = static_cast<uint64_t>(sd.n_header) + sd.n_body + loadSegs;
        pastLarge[d] = loaded > large.leaves || (loadSegs > 0 ? chars : segChars) > large.chars;
      } else if (b->doc_init && b->doc_init[2 * d + 1] > 0) {
        P.startSeg[d] = fmt_mt_snapshot_seg{b->doc_init[2 * d], b->doc_init[2 * d + 1], FMT_MT_NO_PROPS};
        chars += b->doc_init[2 * d + 1];
      }
      P.docChars[d] = chars;
    }
  });
  for (std::vector<uint64_t>* offs : {&P.cuOffs, &P.rmOffs, &P.numOffs, &P.pmOffs})
    for (uint64_t d = 1; d < offs->size(); d++) (*offs)[d] += (*offs)[d - 1];
  for (uint64_t k = 0; k < P.locOffs.size(); k += n1)
    for (uint64_t d = 1; d < n1; d++) P.locOffs[k + d] += P.locOffs[k + d - 1];
  for (uint32_t d = 0; d < n; d++) {
    if (!pastLarge[d]) continue;
    if (P.local) {
      P.refused.push_back(d);
      P.refusedHdr.push_back(refusalHeader(b->snapshots[d], FMT_E_UNSUPPORTED));
    } else {
      P.hugeDocs.push_back(d);
    }
  }
  out = std::move(P);
  return FMT_OK;
}

}  // namespace fmt_plan

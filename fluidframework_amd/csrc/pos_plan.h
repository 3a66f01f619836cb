// pos_plan.h — the host-only half of fmt_mt_query_positions (include/fmt_pos.h): what the bulk position
// read decides without a device.
//
//   views     planPosViews checks q_offsets, gives every query the status the headers and the batch's flags
//             decide (a failed document's status, the limits of a remote view) and collects, per document,
//             the distinct views (ref_seq, client) of the queries that stay FMT_OK, ordered by (ref_seq,
//             client); the local view's client is ignored, so every local query of a document shares one
//             view. One sizing item per (view, tile), the tiles being the text read's (text_plan.h
//             planTextTiles): pass 1 (pos.hip) sums each item's units in its view and in the local view.
//   queries   resolvePosQueries takes the exclusive prefix of each view's tile sums, which is every tile's
//             position base in the view and in the local view, and finds each query's tile by binary
//             search. A position at the view's length is answered here (FMT_MT_POS_F_END), one past it is
//             FMT_E_DATA, so the device never sees a position outside its tile. Every other query goes to
//             pass 2 as a PosDevQuery; its record in `out` is pre-filled with FMT_E_DATA, which a wave
//             that finds no leaf leaves standing.
//
// No HIP include, no fmt_ctx.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fmt_pos.h"
#include "text_plan.h"

namespace fmt_plan {

struct PosItem {  // pass 1's work item: one tile of one view
  uint32_t doc, firstLeaf, nLeaves, view;
  int32_t refSeq, client;
  uint32_t pad[2];
};

struct PosTileUnits {  // pass 1's output per item
  uint64_t view, local;
};

struct PosDevQuery {  // pass 2's work item: one query and the one tile that holds its position
  uint32_t doc, firstLeaf, nLeaves;
  uint32_t pos;  // the position, counted from the tile's first leaf
  int32_t refSeq, client;
  uint32_t viewBase, localBase;  // positions of the tile's first leaf in the view and in the local view
  uint64_t out;                  // index of the query's record
};

struct PosView {
  uint32_t doc;
  int32_t refSeq, client;
  uint32_t pad;
  uint64_t firstItem;  // its items are items[firstItem .. firstItem + the document's tiles)
};

constexpr uint32_t kPosNoView = 0xFFFFFFFFu;

struct PosPlan {
  std::vector<PosView> views;
  std::vector<PosItem> items;
  std::vector<uint32_t> qView;  // per query: its view, or kPosNoView (its record holds its status already)
  std::vector<uint64_t> viewBase, localBase;  // per item: the exclusive prefixes within its view
  std::vector<PosDevQuery> dev;
};

inline uint64_t posViewKey(int32_t refSeq, int32_t client) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(refSeq)) << 32) | static_cast<uint32_t>(client);
}

// The status of query x of a document with header h (fmt_pos.h, in its order).
inline int32_t posQueryStatus(const fmt_mt_doc_result& h, bool obliterates, const fmt_mt_pos_query& x) {
  if (h.status != FMT_OK) return h.status;
  if (x.ref_seq == FMT_MT_VIEW_LOCAL) return FMT_OK;
  if (obliterates) return FMT_E_UNSUPPORTED;
  if (x.client < 0 || x.client >= 64) return FMT_E_UNSUPPORTED;
  if (x.ref_seq < h.min_seq || x.ref_seq > h.cur_seq) return FMT_E_USAGE;
  return FMT_OK;
}

// q_offsets[nDocs + 1] ascends from 0 to nQueries.
inline bool posOffsetsValid(const uint64_t* qOffsets, uint32_t nDocs, uint64_t nQueries) {
  if (qOffsets == nullptr || qOffsets[0] != 0 || qOffsets[nDocs] != nQueries) return false;
  for (uint32_t d = 0; d < nDocs; d++)
    if (qOffsets[d] > qOffsets[d + 1]) return false;
  return true;
}

// Zeroes out[0 .. nQueries) and writes the statuses known from the headers; fills P.views, P.items and P.qView
// over `tiles`, the text read's plan of these headers (text_plan.h planTextTiles). Returns FMT_E_USAGE for malformed offsets (nothing written), FMT_E_CAPACITY for more than
// 2^32 - 1 views or items.
inline int planPosViews(const fmt_mt_doc_result* hdrs, uint32_t nDocs, bool obliterates, const TextPlan& tiles,
                        const uint64_t* qOffsets, const fmt_mt_pos_query* q, uint64_t nQueries, fmt_mt_pos_hit* out,
                        PosPlan& P) {
  if (!posOffsetsValid(qOffsets, nDocs, nQueries)) return FMT_E_USAGE;
  P.views.clear();
  P.items.clear();
  P.dev.clear();
  P.qView.assign(nQueries, kPosNoView);
  if (nQueries) std::memset(out, 0, nQueries * sizeof(fmt_mt_pos_hit));
  std::vector<uint64_t> keys;
  for (uint32_t d = 0; d < nDocs; d++) {
    const uint64_t a = qOffsets[d], b = qOffsets[d + 1];
    if (a == b) continue;
    keys.clear();
    for (uint64_t i = a; i < b; i++) {
      const int32_t st = posQueryStatus(hdrs[d], obliterates, q[i]);
      out[i].status = st;
      if (st == FMT_OK) keys.push_back(posViewKey(q[i].ref_seq, q[i].ref_seq == FMT_MT_VIEW_LOCAL ? 0 : q[i].client));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint64_t firstView = P.views.size();
    if (firstView + keys.size() >= kPosNoView) return FMT_E_CAPACITY;
    for (const uint64_t k : keys) {
      const int32_t refSeq = static_cast<int32_t>(static_cast<uint32_t>(k >> 32));
      const int32_t client = static_cast<int32_t>(static_cast<uint32_t>(k));
      const uint32_t v = static_cast<uint32_t>(P.views.size());
      P.views.push_back(PosView{d, refSeq, client, 0u, P.items.size()});
      for (uint64_t t = tiles.docFirst[d]; t < tiles.docFirst[d + 1]; t++) {
        const TextItem& it = tiles.items[t];
        P.items.push_back(PosItem{d, it.firstLeaf, it.nLeaves, v, refSeq, client, {0u, 0u}});
      }
    }
    if (P.items.size() > 0xFFFFFFFFull) return FMT_E_CAPACITY;
    for (uint64_t i = a; i < b; i++) {
      if (out[i].status != FMT_OK) continue;
      const uint64_t k = posViewKey(q[i].ref_seq, q[i].ref_seq == FMT_MT_VIEW_LOCAL ? 0 : q[i].client);
      P.qView[i] = static_cast<uint32_t>(firstView + static_cast<uint64_t>(std::lower_bound(keys.begin(), keys.end(), k) - keys.begin()));
    }
  }
  return FMT_OK;
}

// From units[P.items.size()] and the tiles planPosViews took: every query's final record (end, past end) or its PosDevQuery in P.dev, in
// query order, with its record pre-filled FMT_E_DATA.
inline void resolvePosQueries(PosPlan& P, const TextPlan& tiles, const fmt_mt_doc_result* hdrs, const PosTileUnits* units,
                              const fmt_mt_pos_query* q, uint64_t nQueries, fmt_mt_pos_hit* out) {
  const size_t ni = P.items.size();
  P.viewBase.assign(ni + 1, 0);
  P.localBase.assign(ni + 1, 0);
  std::vector<uint64_t> viewLen(P.views.size()), localLen(P.views.size());
  for (size_t v = 0; v < P.views.size(); v++) {
    const PosView& V = P.views[v];
    const uint64_t nt = tiles.docFirst[V.doc + 1] - tiles.docFirst[V.doc];
    uint64_t at = 0, lat = 0;
    for (uint64_t k = V.firstItem; k < V.firstItem + nt; k++) {
      P.viewBase[k] = at;
      P.localBase[k] = lat;
      at += units[k].view;
      lat += units[k].local;
    }
    viewLen[v] = at;
    localLen[v] = lat;
  }
  P.dev.clear();
  for (uint64_t i = 0; i < nQueries; i++) {
    const uint32_t v = P.qView[i];
    if (v == kPosNoView) continue;
    const PosView& V = P.views[v];
    const uint64_t pos = q[i].pos;
    fmt_mt_pos_hit& o = out[i];
    if (pos >= viewLen[v]) {
      if (pos == viewLen[v]) {
        o.leaf = hdrs[V.doc].n_leaves;
        o.leaf_start = static_cast<uint32_t>(viewLen[v]);
        o.local_pos = static_cast<uint32_t>(localLen[v]);
        o.props = 0xFFFFu;
        o.flags = FMT_MT_POS_F_END;
      } else {
        o.status = FMT_E_DATA;
      }
      continue;
    }
    // the last tile whose base is at or below pos: the next base is above it, so the tile holds the position
    const uint64_t nt = tiles.docFirst[V.doc + 1] - tiles.docFirst[V.doc];
    const uint64_t* first = P.viewBase.data() + V.firstItem;
    const uint64_t k = V.firstItem + static_cast<uint64_t>(std::upper_bound(first, first + nt, pos) - first) - 1;
    const PosItem& it = P.items[k];
    P.dev.push_back(PosDevQuery{it.doc, it.firstLeaf, it.nLeaves, static_cast<uint32_t>(pos - P.viewBase[k]), V.refSeq, V.client,
                                static_cast<uint32_t>(P.viewBase[k]), static_cast<uint32_t>(P.localBase[k]), i});
    o.status = FMT_E_DATA;
  }
}

}  // namespace fmt_plan

// range_plan.h — the host-only half of fmt_mt_fetch_text_ranges (include/fmt_range.h): what the bulk range
// read decides without a device.
//
//   views     planRangeViews checks q_offsets and hands the queries' views to pos_plan.h planPosViews, so the
//             statuses the headers decide, the distinct views per document and the (view, tile) sizing items
//             are the position read's own: pass A is pos.hip's posTileUnitsKernel over them.
//   items     cutRanges takes the exclusive prefix of each view's tile units (every tile's position base in
//             its view), resolves FMT_MT_RANGE_TO_END, settles FMT_E_DATA, and cuts every surviving non-empty
//             range into RangeItems: one range, one tile, [lo, hi) in view units counted from the tile's
//             first leaf. The first and last tile come from binary search over the bases; a tile without
//             units in the view gets no item. Items are in query order, then tile order.
//   offsets   rangeOffsets takes the exclusive prefix of the items' text units (pass B's output, or hi - lo
//             with a placeholder): every item's base in `out`, every hit's text_off and units, the total.
//
// No HIP include, no fmt_ctx.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fmt_range.h"
#include "pos_plan.h"

namespace fmt_plan {

struct RangeItem {  // the work item of passes B and C (range.hip): one range clipped to one tile
  uint32_t doc, firstLeaf, nLeaves;
  uint32_t lo, hi;  // [lo, hi) in units of the view, counted from the tile's first leaf; lo < hi
  int32_t refSeq, client;
  uint32_t pad;
};

struct RangePlan {
  PosPlan views;  // the views, their (view, tile) items and each query's view (pos_plan.h)
  std::vector<RangeItem> items;
  std::vector<uint64_t> itemQuery;  // per item: its query
  std::vector<uint64_t> itemBase;   // per item: its first unit in `out`
};

// Zeroes hits[0 .. nQueries) and writes the statuses known from the headers; fills P.views over `tiles`.
// Returns FMT_E_USAGE for malformed offsets (nothing written), FMT_E_CAPACITY as planPosViews does.
inline int planRangeViews(const fmt_mt_doc_result* hdrs, uint32_t nDocs, bool obliterates, const TextPlan& tiles,
                          const uint64_t* qOffsets, const fmt_mt_range_query* q, uint64_t nQueries, fmt_mt_range_hit* hits,
                          RangePlan& P) {
  if (!posOffsetsValid(qOffsets, nDocs, nQueries)) return FMT_E_USAGE;
  P.items.clear();
  P.itemQuery.clear();
  P.itemBase.clear();
  std::vector<fmt_mt_pos_query> pq(nQueries);
  std::vector<fmt_mt_pos_hit> ph(nQueries);
  for (uint64_t i = 0; i < nQueries; i++) pq[i] = fmt_mt_pos_query{0u, q[i].ref_seq, q[i].client, 0u};
  const int rc = planPosViews(hdrs, nDocs, obliterates, tiles, qOffsets, pq.data(), nQueries, ph.data(), P.views);
  if (rc != FMT_OK) return rc;
  if (nQueries) std::memset(hits, 0, nQueries * sizeof(fmt_mt_range_hit));
  for (uint64_t i = 0; i < nQueries; i++) hits[i].status = ph[i].status;
  return FMT_OK;
}

// From units[P.views.items.size()] (pass A) and the tiles planRangeViews took: every FMT_OK query's span or its
// FMT_E_DATA, and P.items / P.itemQuery. Returns FMT_E_CAPACITY for more than 2^32 - 1 items.
inline int cutRanges(RangePlan& P, const TextPlan& tiles, const PosTileUnits* units, const fmt_mt_range_query* q,
                     uint64_t nQueries, fmt_mt_range_hit* hits) {
  PosPlan& V = P.views;
  const size_t ni = V.items.size();
  V.viewBase.assign(ni + 1, 0);
  std::vector<uint64_t> viewLen(V.views.size());
  for (size_t v = 0; v < V.views.size(); v++) {
    const PosView& W = V.views[v];
    const uint64_t nt = tiles.docFirst[W.doc + 1] - tiles.docFirst[W.doc];
    uint64_t at = 0;
    for (uint64_t k = W.firstItem; k < W.firstItem + nt; k++) {
      V.viewBase[k] = at;
      at += units[k].view;
    }
    viewLen[v] = at;
  }
  P.items.clear();
  P.itemQuery.clear();
  for (uint64_t i = 0; i < nQueries; i++) {
    const uint32_t v = V.qView[i];
    if (v == kPosNoView) continue;
    const PosView& W = V.views[v];
    const uint64_t len = viewLen[v];
    const uint64_t start = q[i].start, end = q[i].end == FMT_MT_RANGE_TO_END ? len : q[i].end;
    if (start > end || end > len) {
      hits[i].status = FMT_E_DATA;
      continue;
    }
    hits[i].span = static_cast<uint32_t>(end - start);
    if (start == end) continue;
    // the last tile whose base is at or below a position holds it: the next base is above the position
    const uint64_t nt = tiles.docFirst[W.doc + 1] - tiles.docFirst[W.doc];
    const uint64_t* first = V.viewBase.data() + W.firstItem;
    const uint64_t kf = W.firstItem + static_cast<uint64_t>(std::upper_bound(first, first + nt, start) - first) - 1;
    const uint64_t kl = W.firstItem + static_cast<uint64_t>(std::upper_bound(first, first + nt, end - 1) - first) - 1;
    for (uint64_t k = kf; k <= kl; k++) {
      const uint64_t base = V.viewBase[k], n = units[k].view;
      if (n == 0) continue;
      const PosItem& it = V.items[k];
      const uint64_t lo = std::max(start, base) - base, hi = std::min(end, base + n) - base;
      P.items.push_back(RangeItem{it.doc, it.firstLeaf, it.nLeaves, static_cast<uint32_t>(lo), static_cast<uint32_t>(hi), W.refSeq,
                                  W.client, 0u});
      P.itemQuery.push_back(i);
    }
    if (P.items.size() > 0xFFFFFFFFull) return FMT_E_CAPACITY;
  }
  return FMT_OK;
}

// itemUnits[P.items.size()]: the text units of every item (pass B), or nullptr: hi - lo (a placeholder stands
// for every Marker). Fills P.itemBase and every FMT_OK hit's text_off and units; returns the total.
inline uint64_t rangeOffsets(RangePlan& P, const uint64_t* itemUnits, uint64_t nQueries, fmt_mt_range_hit* hits) {
  const size_t ni = P.items.size();
  P.itemBase.assign(ni, 0);
  uint64_t at = 0;
  size_t k = 0;
  for (uint64_t i = 0; i < nQueries; i++) {
    if (hits[i].status != FMT_OK) continue;
    hits[i].text_off = at;
    for (; k < ni && P.itemQuery[k] == i; k++) {
      P.itemBase[k] = at;
      const uint64_t span = P.items[k].hi - P.items[k].lo;  // (an item never holds more text than positions)
      at += itemUnits != nullptr ? std::min(itemUnits[k], span) : span;
    }
    hits[i].units = static_cast<uint32_t>(at - hits[i].text_off);
  }
  return at;
}

}  // namespace fmt_plan

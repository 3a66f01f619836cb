// text_plan.h — the host-only half of fmt_mt_fetch_text_all (include/fmt_text.h): what the bulk text
// read decides without a device.
//
//   tiles     the work items of the two text kernels (text.hip): a document's leaves cut into runs of
//             tileLeaves consecutive leaves, in document order, then tile order. A document that
//             failed, or has no leaf, has no item.
//   offsets   from the units each tile contributes (pass 1's output): the exclusive 64-bit prefix,
//             which is every tile's base in the packed text and, at a document's first tile, the
//             document's offset.
//
// No HIP include, no fmt_ctx.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/fmt.h"

namespace fmt_plan {

constexpr uint32_t kTextTileLeaves = 1024;  // leaves per work item

struct TextItem {
  uint32_t doc;
  uint32_t firstLeaf;
  uint32_t nLeaves;  // 1 .. tileLeaves
  uint32_t pad;
};

struct TextPlan {
  std::vector<TextItem> items;
  std::vector<uint64_t> docFirst;  // nDocs + 1: document d's items are items[docFirst[d] .. docFirst[d + 1])
};

inline void planTextTiles(const fmt_mt_doc_result* hdrs, uint32_t nDocs, uint32_t tileLeaves, TextPlan& P) {
  P.items.clear();
  P.docFirst.assign(nDocs + 1ull, 0);
  if (tileLeaves == 0) tileLeaves = kTextTileLeaves;
  for (uint32_t d = 0; d < nDocs; d++) {
    P.docFirst[d] = P.items.size();
    if (hdrs[d].status != FMT_OK) continue;
    const uint32_t n = hdrs[d].n_leaves;
    for (uint32_t first = 0; first < n;) {
      const uint32_t m = n - first < tileLeaves ? n - first : tileLeaves;
      P.items.push_back(TextItem{d, first, m, 0u});
      first += m;
    }
  }
  P.docFirst[nDocs] = P.items.size();
}

// offsets[nDocs + 1] and tileBase[items] from tileUnits[items]; returns the total (offsets[nDocs]).
inline uint64_t textOffsets(const TextPlan& P, const uint64_t* tileUnits, uint64_t* offsets, uint64_t* tileBase) {
  const size_t nDocs = P.docFirst.size() - 1;
  uint64_t at = 0;
  for (size_t d = 0; d < nDocs; d++) {
    offsets[d] = at;
    for (uint64_t k = P.docFirst[d]; k < P.docFirst[d + 1]; k++) {
      tileBase[k] = at;
      at += tileUnits[k];
    }
  }
  offsets[nDocs] = at;
  return at;
}

}  // namespace fmt_plan

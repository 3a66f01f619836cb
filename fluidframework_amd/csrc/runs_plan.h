// runs_plan.h — the host-only half of fmt_mt_fetch_prop_runs_all (include/fmt_runs.h): what the bulk
// property-run read decides without a device.
//
// The work items are the text read's (text_plan.h planTextTiles). Pass 1 (runs.hip) reports per tile what
// its leaves look like from outside (RunTile); the stitch below walks each document's tiles once, O(tiles)
// and no per-leaf work, and gives pass 2 each tile's bases (RunTileBase):
//
//   A tile's first visible leaf is a head inside its tile whatever came before it. It continues the open
//   run of the nearest earlier tile that has a visible leaf iff both are text of one class; then it is no
//   head after all, the tile has one new run fewer, and the open run's length keeps growing: a tile
//   without another head passes the run on whole. The tile that sees a run's end writes its len as
//   end - start, so a tile needs the start of the run that is open where it begins (openStart) and
//   whether its own last run ends with it (kRunCloses: the next tile with a visible leaf does not
//   continue it, or there is none).
//
// No HIP include, no fmt_ctx.
#pragma once

#include <cstdint>
#include <vector>

#include "text_plan.h"

namespace fmt_plan {

// RunTile::first / last: the class of the tile's first / last visible leaf, and
constexpr uint32_t kRunEndMarker = 1u << 16;  // that leaf is a Marker
constexpr uint32_t kRunEndHas = 1u << 17;     // the tile has a visible leaf at all

struct RunTile {     // pass 1's report of one work item
  uint32_t units;    // positions of its visible leaves
  uint32_t heads;    // heads, its first visible leaf counted
  uint32_t tail;     // positions from its last head to its end
  uint32_t first;
  uint32_t last;
};

constexpr uint32_t kRunContinues = 1;  // the first visible leaf continues the run open at the tile's start
constexpr uint32_t kRunCloses = 2;     // the tile's last run ends with the tile

struct RunTileBase {  // pass 2's input for one work item
  uint64_t runBase;   // packed index of the tile's first new run
  uint32_t posBase;   // position of the tile's first leaf in its document's local view
  uint32_t openStart; // kRunContinues: start of the run it continues
  uint32_t flags;
  uint32_t pad;
};

// offsets[nDocs + 1] and base[items] from tiles[items]; returns the total number of runs (offsets[nDocs]).
inline uint64_t stitchRuns(const TextPlan& P, const RunTile* tiles, uint64_t* offsets, RunTileBase* base) {
  const size_t nDocs = P.docFirst.size() - 1;
  uint64_t at = 0;
  for (size_t d = 0; d < nDocs; d++) {
    offsets[d] = at;
    uint32_t pos = 0, openStart = 0, openEnd = 0;
    int64_t open = -1;  // the nearest earlier tile with a visible leaf
    for (uint64_t k = P.docFirst[d]; k < P.docFirst[d + 1]; k++) {
      const RunTile& t = tiles[k];
      RunTileBase b{at, pos, 0u, 0u, 0u};
      if ((t.first & kRunEndHas) != 0) {
        const bool cont = open >= 0 && ((openEnd | t.first) & kRunEndMarker) == 0 && (openEnd & 0xFFFFu) == (t.first & 0xFFFFu);
        if (open >= 0 && !cont) base[open].flags |= kRunCloses;
        if (cont) {
          b.flags = kRunContinues;
          b.openStart = openStart;
        }
        const uint32_t fresh = t.heads - (cont ? 1u : 0u);
        if (fresh > 0) openStart = pos + t.units - t.tail;
        at += fresh;
        openEnd = t.last;
        open = static_cast<int64_t>(k);
      }
      base[k] = b;
      pos += t.units;
    }
    if (open >= 0) base[open].flags |= kRunCloses;
  }
  offsets[nDocs] = at;
  return at;
}

}  // namespace fmt_plan

// map_plan.h — the host-only half of fmt_map_run_sparse_tiered's HBM tier (map_sparse_large.hip):
// what the documents the LDS tier refused need, decided before any of their kernels is launched.
// planMapLarge takes the batch's doc_op_offsets and the overflowing documents (ascending) and lays
// out, per overflowing document, a hash table of S slots (the smallest power of two >= 2 x its ops,
// so the load stays <= 1/2 whatever the keys are; Fibonacci hashing as spHash in map_sparse.hip) and
// one op-slot word per op, and cuts the documents' op ranges into tiles of kMapLargeTile ops (the last
// tile of a document short), the unit the kernels' passes grid-stride over.
//
// Scratch, in 32-bit words (S = all documents' slots, N = their ops, T = tiles, n = documents):
//     [0, S) key   [S, 2S) first   [2S, 3S) D   [3S, 4S) last   [4S, 5S) value
//     [5S, 5S + N) op slot   [.., + T) tile birth counts   [.., + n) last clear
// A document's table starts at its tableOff in each of the five slot regions, its op-slot words at
// opSlotOff. Bound: S_d < 4 x ops_d, so fewer than 80 B of tables + 4 B of op slot per op, 4 B per
// tile (1/64 B per op, + 4 B per document for its short tile) and 4 B per document: under 84.02 B per
// op + 8 B per document. A 10^6-op document takes 2^21 slots: 40 MiB of tables, 4 MB of op slots.
// Limits: a document of fewer than 2^30 ops (S <= 2^31, ordinals and slots are uint32) and the
// device memory for the scratch. runtime.cpp uploads docs / tileDoc / tileFirst; tests reach the
// plan without a device (fmt_internal_map_large_plan). No HIP include, no fmt_ctx.
#pragma once

#include <cstdint>
#include <vector>

namespace fmt_plan {

constexpr uint32_t kMapLargeTile = 256;           // ops per tile: one wave, four chunks of 64 lanes
constexpr uint64_t kMapLargeMaxOps = 1ull << 30;  // per document (exclusive)

// One overflowing document as the kernels see it.
struct MapLargeDoc {
  uint64_t opBegin;    // doc_op_offsets[doc]: its records, and its entries in the output
  uint64_t tableOff;   // first slot of its table within each slot region
  uint64_t opSlotOff;  // first of its words within the op-slot region
  uint32_t doc, nOps;
  uint32_t shift, mask;  // S = mask + 1 = 2^(32 - shift)
  uint32_t firstTile, nTiles;
};

struct MapLargePlan {
  std::vector<MapLargeDoc> docs;               // the overflowing documents, ascending
  std::vector<uint32_t> tileDoc, tileFirst;    // tile -> index into docs, first op (within the document)
  uint64_t slots = 0, ops = 0;                 // S and N above
  uint64_t words() const { return 5 * slots + ops + tileDoc.size() + docs.size(); }
  uint64_t scratchBytes() const { return 4 * words(); }
  // region starts, in words
  uint64_t keyAt() const { return 0; }
  uint64_t firstAt() const { return slots; }
  uint64_t delAt() const { return 2 * slots; }
  uint64_t lastAt() const { return 3 * slots; }
  uint64_t valueAt() const { return 4 * slots; }
  uint64_t opSlotAt() const { return 5 * slots; }
  uint64_t tileCountAt() const { return 5 * slots + ops; }
  uint64_t clearAt() const { return 5 * slots + ops + tileDoc.size(); }
};

// Fills `plan` (emptied first). Returns NULL, or why the list cannot be planned: a document out of
// range or out of order, one without ops (it cannot have overflowed), or one of 2^30 ops or more.
inline const char* planMapLarge(const uint64_t* docOpOffsets, uint32_t nDocs, const uint32_t* overflow, uint32_t nOverflow,
                                MapLargePlan& plan) {
  plan = MapLargePlan{};
  for (uint32_t j = 0; j < nOverflow; j++) {
    const uint32_t d = overflow[j];
    if (d >= nDocs || (j > 0 && d <= overflow[j - 1])) return "overflowing documents must be ascending and below n_docs";
    const uint64_t n = docOpOffsets[d + 1] - docOpOffsets[d];
    if (n == 0) return "an overflowing document without ops";
    if (n >= kMapLargeMaxOps) return "a document of 2^30 ops or more (ordinals and slots are 32-bit)";
    MapLargeDoc D{};
    D.opBegin = docOpOffsets[d];
    D.tableOff = plan.slots;
    D.opSlotOff = plan.ops;
    D.doc = d;
    D.nOps = static_cast<uint32_t>(n);
    D.shift = 31;
    while ((1ull << (32 - D.shift)) < 2 * n) D.shift--;
    D.mask = static_cast<uint32_t>((1ull << (32 - D.shift)) - 1);
    D.firstTile = static_cast<uint32_t>(plan.tileDoc.size());
    D.nTiles = static_cast<uint32_t>((n + kMapLargeTile - 1) / kMapLargeTile);
    for (uint32_t t = 0; t < D.nTiles; t++) {
      plan.tileDoc.push_back(j);
      plan.tileFirst.push_back(t * kMapLargeTile);
    }
    plan.slots += uint64_t{D.mask} + 1;
    plan.ops += n;
    plan.docs.push_back(D);
  }
  if (plan.tileDoc.size() >= 0xFFFFFFFFull) return "too many tiles";
  return nullptr;
}

}  // namespace fmt_plan

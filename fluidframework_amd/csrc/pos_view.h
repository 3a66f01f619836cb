// pos_view.h — fmt_pos.h's view rule on the device, shared by the readers that count positions in a view
// (pos.hip, range.hip): a leaf's units, and whether the local view or a remote view (ref_seq, client) sees it.
// Clients are 0..63 (the host refuses the others), so the shift is defined.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/fmt.h"
#include "../../include/fmt_pos.h"

namespace fmt_kernels {

__device__ __forceinline__ uint32_t posUnitsOf(const fmt_mt_leaf& L) { return (L.pad & FMT_MT_LEAF_MARKER) != 0 ? 1u : L.len; }

__device__ __forceinline__ bool posVisibleLocal(const fmt_mt_leaf& L) { return L.rm_seq == FMT_NOT_REMOVED; }

__device__ __forceinline__ bool posVisible(const fmt_mt_leaf& L, int32_t refSeq, int32_t client) {
  if (refSeq == FMT_MT_VIEW_LOCAL) return posVisibleLocal(L);
  const uint32_t c = static_cast<uint32_t>(client) & 63u;
  const bool inserted = L.ins_seq <= refSeq || static_cast<int32_t>(L.ins_client) == client;
  const bool removed = L.rm_seq <= refSeq || ((L.rm_clients >> c) & 1ull) != 0;
  return inserted && !removed;
}

}  // namespace fmt_kernels

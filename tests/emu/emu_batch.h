// emu_batch.h — TEST INFRASTRUCTURE ONLY: a host batch as the view a launch takes (csrc/mt_bind.h
// MtDeviceBatch, what fmt_mt_run builds from its device buffers), so that the emulations bind
// documents with the kernel's own bindDoc. The emulations' catch-up and remove-order slabs have one
// fixed capacity per document; here they become the offset arrays the binding reads.
#pragma once
#include <vector>

#include "../../fluidframework_amd/csrc/mt_bind.h"

struct EmuBatch {
  std::vector<uint64_t> cuOffs, rmOffs;
  fmt_kernels::MtDeviceBatch view;

  // catchup / rmOrder: whether the call has such slabs (capCatchup / capRm entries per document)
  EmuBatch(const fmt_mt_batch* b, bool catchup, uint32_t capCatchup, bool rmOrder, uint32_t capRm,
           const fmt_mt::AdjustTables* adj = nullptr, const fmt_mt::LocalTables* loc = nullptr) {
    auto slabs = [&](std::vector<uint64_t>& v, uint64_t cap) {
      v.resize(b->n_docs + 1ull);
      for (uint32_t d = 0; d <= b->n_docs; d++) v[d] = d * cap;
      return v.data();
    };
    view = fmt_kernels::MtDeviceBatch{b->ops, b->doc_op_offsets, b->n_docs, b->text, b->doc_init, b->props_off, b->props_kv,
                                      b->n_props_ops, catchup ? slabs(cuOffs, capCatchup) : nullptr, b->snapshots,
                                      b->snapshot_segs, rmOrder ? slabs(rmOffs, capRm) : nullptr, b->snapshot_info,
                                      b->snapshot_stamps, b->n_snapshot_segs, b->relpos, b->n_relpos, b->marker_id_key,
                                      adj, loc};
  }
};

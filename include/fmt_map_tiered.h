/*
 * fmt_map_tiered.h — the sparse SharedMap path without per-document limits, the peer of fmt.h's
 * fmt_map_run_sparse. The conventions of fmt.h hold.
 */
#ifndef FMT_MAP_TIERED_H_
#define FMT_MAP_TIERED_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Valid wherever fmt_map_run_sparse is (after fmt_map_load_sparse). Runs fmt_map_run_sparse's LDS
 * tier, then every document that tier refused again in the HBM tier (hash tables in
 * device memory, 32-bit ordinals), into the same buffers; returns when both are done. Afterwards
 * fmt_map_fetch_sparse has every document's entries (FMT_OK; a key id >= key_bound anywhere is
 * still FMT_E_DATA) and fmt_map_pending_run may follow. If the HBM tier's tables cannot be
 * allocated the call fails (FMT_E_DEVICE, fmt_last_error says how much was needed) and those
 * documents stay refused as after fmt_map_run_sparse. fmt_get_stats covers both tiers; a batch
 * without such documents costs what fmt_map_run_sparse costs, plus one 4-byte read back. */
int fmt_map_run_sparse_tiered(fmt_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* FMT_MAP_TIERED_H_ */

/*
 * fmt_runs.h — bulk formatted-text reads, the peer of fmt_text.h for the other half of the converged-state
 * readout: where each formatting starts and ends (the reference reads it a position at a time through
 * getPropertiesAtPosition, client.ts:1667-1670). Every document's property runs come from one device
 * pass and are copied back packed, in one call; a second call returns every document's prop-set table.
 * The conventions of fmt.h hold.
 *
 * The view is fmt_text.h's, the local perspective:
 *   visible   a leaf is visible iff rm_seq == FMT_NOT_REMOVED (in a local batch this shows a pending
 *             local insert and hides a pending local remove).
 *   position  getLength() coordinates: a visible text leaf occupies `len` positions, a visible Marker 1.
 *   class     the match class of a leaf's `props` (matchProperties, properties.ts): 0xffff when props
 *             are undefined or the set is empty (n == 0); otherwise the lowest first-record id of a set
 *             in the document's table with the same (key, value) entries in any order. Value ids
 *             compare as ids (computed annotate-adjust numbers are interned per value, so equal ids
 *             mean equal values).
 *   run       a maximal sequence of consecutive visible leaves that are all text leaves of one class;
 *             invisible leaves in between are ignored and do not break a run. A visible Marker is
 *             always a run of its own. A visible leaf with len == 0 (none is expected in engine
 *             output) contributes nothing and breaks nothing.
 */
#ifndef FMT_RUNS_H_
#define FMT_RUNS_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMT_MT_RUN_MARKER 1u /* fmt_mt_prop_run.flags: the run is one Marker */

typedef struct fmt_mt_prop_run { /* 16 bytes */
  uint32_t start;      /* first position of the run in the document's local view */
  uint32_t len;        /* positions it covers; a document's lens sum to its header's visible_len */
  uint32_t first_leaf; /* index of the run's first leaf in the document's leaf list */
  uint16_t props;      /* the run's class: a first-record id in the document's prop-set table, 0xffff = none */
  uint16_t flags;      /* FMT_MT_RUN_MARKER */
} fmt_mt_prop_run;

/* Every document's runs, packed in document order, one call.
 * offsets[n_docs + 1] (required): document d's runs are out[offsets[d] .. offsets[d+1]). A document whose
 *   status is not FMT_OK has none.
 * out == NULL: offsets only (the sizing call). Otherwise cap is out's capacity in runs; FMT_E_USAGE, and
 *   nothing written to out, when cap < offsets[n_docs] (offsets are still returned).
 * Two calls on the same state return equal bytes. Needs a completed fmt_mt_run since the last fmt_mt_load
 * (FMT_E_USAGE otherwise, as every other fmt_mt_fetch_*). Synchronizes the ctx stream. */
int fmt_mt_fetch_prop_runs_all(fmt_ctx* ctx, uint64_t* offsets, fmt_mt_prop_run* out, uint64_t cap);

/* Every document's prop-set table (its header's n_props records, as fmt_mt_fetch_doc returns them), packed
 * in document order: what a run's `props` names. Same contract as above, cap in records. Computed values
 * (ids at or above FMT_MT_VALUE_COMPUTED) are resolved through fmt_mt_fetch_numbers, per document. */
int fmt_mt_fetch_props_all(fmt_ctx* ctx, uint64_t* offsets, fmt_mt_propset* out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* FMT_RUNS_H_ */

/*
 * fmt_text.h — bulk SharedString text reads, the peer of fmt.h's per-document fmt_mt_fetch_doc for the
 * commonest read after a replay: every string's getText() (sequence.ts SharedString.getText →
 * MergeTreeTextHelper.ts:28-87), gathered on the device and copied back packed, in one call.
 * The conventions of fmt.h hold.
 */
#ifndef FMT_TEXT_H_
#define FMT_TEXT_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every document's text from the local perspective, packed in document order, one call.
 * placeholder == 0: SharedString.getText() — the units of every leaf that is not removed
 *   (rm_seq == FMT_NOT_REMOVED, which in a local batch hides a pending local remove and shows a
 *   pending local insert) and is not a Marker, in document order.
 * placeholder != 0: SharedString.getTextWithPlaceholders() with that one UTF-16 unit — as above, and
 *   every Marker that is not removed contributes `placeholder` once (a Marker's cachedLength is 1), so
 *   a document's unit count equals its header's visible_len.
 * offsets[n_docs + 1] (required): document d's units are out[offsets[d] .. offsets[d+1]). A document
 *   whose status is not FMT_OK has none.
 * out == NULL: offsets only (the sizing call). Otherwise cap is out's capacity in units; FMT_E_USAGE,
 *   and nothing written to out, when cap < offsets[n_docs] (offsets are still returned).
 * Needs a completed fmt_mt_run since the last fmt_mt_load (FMT_E_USAGE otherwise, as every other
 * fmt_mt_fetch_*). Synchronizes the ctx stream. */
int fmt_mt_fetch_text_all(fmt_ctx* ctx, uint16_t placeholder, uint64_t* offsets, uint16_t* out, uint64_t cap);
/* Leaves per work item of the text kernels (for tests that aim at its edges). */
uint32_t fmt_mt_text_tile_leaves(void);

#ifdef __cplusplus
}
#endif
#endif /* FMT_TEXT_H_ */

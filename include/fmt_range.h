/*
 * fmt_range.h — bulk range reads, the peer of fmt_text.h, fmt_runs.h and fmt_pos.h for the reference's
 * commonest read: SharedString.getText(start, end) and getTextWithPlaceholders(start, end)
 * (MergeTreeTextHelper.ts) of many (document, start, end, view) ranges. Every range of every document is
 * gathered in one device pass and copied back in one call; only the units of the ranges cross the bus.
 * The conventions of fmt.h hold.
 *
 * View. A query names a view (ref_seq, client) exactly as fmt_pos.h does: the same visibility rule, the
 * same position counting (a visible text leaf counts len, a visible Marker 1), the same limits of a remote
 * view with the same statuses, tested in the same order. A range query and a position query with the same
 * (ref_seq, client) are refused identically.
 */
#ifndef FMT_RANGE_H_
#define FMT_RANGE_H_

#include "fmt.h"
#include "fmt_pos.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMT_MT_RANGE_TO_END 0xffffffffu /* fmt_mt_range_query.end: the view's length */

typedef struct fmt_mt_range_query { /* 16 bytes */
  uint32_t start;  /* [start, end) in positions of the view */
  uint32_t end;    /* FMT_MT_RANGE_TO_END: the view's length */
  int32_t ref_seq; /* FMT_MT_VIEW_LOCAL, or the remote view's reference sequence number */
  int32_t client;  /* the remote view's short client id (ignored for the local view) */
} fmt_mt_range_query;

typedef struct fmt_mt_range_hit { /* 24 bytes */
  uint64_t text_off; /* the range's units are out[text_off .. text_off + units) */
  uint32_t units;    /* units written: span minus the Markers in the range when placeholder == 0, span otherwise */
  uint32_t span;     /* end - start after FMT_MT_RANGE_TO_END is resolved ((0, TO_END) reports the view's length) */
  int32_t status;    /* FMT_OK or a per-query FMT_E_* */
  uint32_t pad;      /* 0 */
} fmt_mt_range_hit;

/* Reads n_queries ranges, packed per document: document d's queries are q[q_offsets[d] .. q_offsets[d+1]),
 * q_offsets[n_docs + 1] ascending from 0 to n_queries (anything else is FMT_E_USAGE for the call, nothing
 * written). hits[i] answers q[i]. Ranges of one document may overlap, repeat and come in any order; the text
 * is packed in query order, so text_off ascends with the query index.
 *   status       of one query: the document's own status; then the limits of a remote view (fmt_pos.h); then
 *                FMT_E_DATA unless start <= end <= the view's length, FMT_MT_RANGE_TO_END standing for that
 *                length. Whenever status != FMT_OK every other field is zero and the query has no units.
 *   empty        start == end (the view's length included), or a range of Markers only with placeholder == 0:
 *                FMT_OK, units == 0.
 *   placeholder  fmt_text.h's: 0 drops Markers, anything else writes that unit once per visible Marker.
 *                Positions count Markers either way.
 *   sizing       out == NULL: hits and *total are filled, no text is gathered. Otherwise cap < *total is
 *                FMT_E_USAGE with nothing written to out (the hits are still returned). Nothing is cached
 *                between the two calls.
 * n_queries == 0 is FMT_OK and launches nothing. Two calls on the same state return equal bytes. The call
 * disturbs no later text, runs, positions, summary or digest call and no later run. Needs a completed
 * fmt_mt_run since the last fmt_mt_load (FMT_E_USAGE otherwise). Synchronizes the ctx stream.
 * A host that wants the leaf extents of a range asks fmt_mt_query_positions for start and end - 1. */
int fmt_mt_fetch_text_ranges(fmt_ctx* ctx, uint16_t placeholder, const uint64_t* q_offsets, const fmt_mt_range_query* q,
                             uint64_t n_queries, fmt_mt_range_hit* hits, uint64_t* total, uint16_t* out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* FMT_RANGE_H_ */

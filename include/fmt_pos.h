/*
 * fmt_pos.h — bulk position queries, the peer of fmt_text.h and fmt_runs.h for positional reads of the
 * converged state: which segment holds position p of document d, what are its properties, and where does
 * another client's position land in the local view (the reference's getContainingSegment,
 * getPropertiesAtPosition, getRangeExtentsOfPosition and resolveRemoteClientPosition, client.ts). Every
 * query of every document is answered in one device pass and copied back in one call.
 * The conventions of fmt.h hold.
 *
 * View. A query names a view (ref_seq, client).
 *   local     ref_seq == FMT_MT_VIEW_LOCAL; client is ignored. A leaf is visible iff
 *             rm_seq == FMT_NOT_REMOVED: exactly the view of fmt_text.h and fmt_runs.h (in a local batch it
 *             shows a pending local insert and hides a pending local remove).
 *   remote    any other ref_seq. Leaf L is inserted in the view iff L.ins_seq <= ref_seq ||
 *             L.ins_client == client; it is removed in the view iff L.rm_seq <= ref_seq ||
 *             (L.rm_clients >> client) & 1; it is visible iff it is inserted and not removed. Stamps of
 *             pending local ops (>= FMT_MT_LOCAL_SEQ_BASE) need no special case: they exceed every
 *             ref_seq, so only their own client sees them.
 *   position  a visible text leaf contributes `len` units, a visible Marker 1.
 *
 * Limits of a remote view. Each is the status of the one query, not a failed call; they are tested in
 * this order, after the document's own status:
 *   FMT_E_UNSUPPORTED  any remote view when the loaded batch holds obliterates. A leaf record keeps only
 *                      its first remove stamp, and how an obliterate's stamps decide visibility from
 *                      another client's perspective has not been checked against the reference; the
 *                      rule is not guessed here.
 *   FMT_E_UNSUPPORTED  client < 0 || client >= 64: below the huge tier the remover words of ids 64..253
 *                      are not part of a leaf record.
 *   FMT_E_USAGE        ref_seq outside [header.min_seq, header.cur_seq]: below minSeq zamboni has already
 *                      merged or dropped the stamps the rule reads.
 * Local-view queries have none of these limits.
 */
#ifndef FMT_POS_H_
#define FMT_POS_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMT_MT_VIEW_LOCAL 0x7fffffff /* fmt_mt_pos_query.ref_seq: the local view */

#define FMT_MT_POS_F_MARKER 1u         /* the leaf is a Marker */
#define FMT_MT_POS_F_END 2u            /* pos is the view's length: no leaf */
#define FMT_MT_POS_F_HIDDEN_LOCALLY 4u /* the leaf is not visible in the local view */

typedef struct fmt_mt_pos_query { /* 16 bytes */
  uint32_t pos;    /* position in the view */
  int32_t ref_seq; /* FMT_MT_VIEW_LOCAL, or the remote view's reference sequence number */
  int32_t client;  /* the remote view's short client id */
  uint32_t pad;
} fmt_mt_pos_query;

typedef struct fmt_mt_pos_hit { /* 32 bytes */
  uint32_t leaf;       /* index in the document's leaf list (fmt_mt_fetch_doc order) */
  uint32_t offset;     /* units into that leaf */
  uint32_t leaf_start; /* position of the leaf's first unit in the query's view */
  uint32_t leaf_len;   /* its units in the view (1 for a Marker) */
  uint32_t local_pos;  /* the same unit's position in the local view: units visible locally before the
                          leaf, plus offset when the leaf is visible locally, plus 0 when it is not */
  uint16_t props;      /* the leaf's prop-set id, 0xffff undefined (resolve with fmt_mt_fetch_props_all) */
  uint16_t unit;       /* the UTF-16 unit at the position (a Marker's one char unit) */
  int32_t status;      /* FMT_OK or a per-query FMT_E_* */
  uint32_t flags;      /* FMT_MT_POS_F_MARKER | FMT_MT_POS_F_END | FMT_MT_POS_F_HIDDEN_LOCALLY */
} fmt_mt_pos_hit;

/* Answers n_queries position queries, packed per document: document d's queries are
 * q[q_offsets[d] .. q_offsets[d+1]), q_offsets[n_docs + 1] ascending from 0 to n_queries (anything else is
 * FMT_E_USAGE for the call). out[i] answers q[i].
 *   hit       the first visible leaf with leaf_start <= pos < leaf_start + leaf_len.
 *   end       pos == the view's length: status FMT_OK, flags FMT_MT_POS_F_END, leaf = the header's n_leaves,
 *             offset = 0, leaf_len = 0, leaf_start = that length, local_pos = the local view's length,
 *             props = 0xffff, unit = 0.
 *   past end  pos > the view's length: FMT_E_DATA.
 *   A query of a document whose status is not FMT_OK gets that status; then the limits of a remote view
 *   above. Whenever status != FMT_OK every other field is zero.
 * local_pos adds nothing for a leaf hidden locally (FMT_MT_POS_F_HIDDEN_LOCALLY says so): a host that
 * wants getPosition(segment) + offset adds the offset itself.
 * n_queries == 0 is FMT_OK and launches nothing. Two calls on the same state return equal bytes. The call
 * disturbs no later text, runs, summary or digest call and no later run. Needs a completed fmt_mt_run since
 * the last fmt_mt_load (FMT_E_USAGE otherwise, as every fmt_mt_fetch_*). Synchronizes the ctx stream. */
int fmt_mt_query_positions(fmt_ctx* ctx, const uint64_t* q_offsets, const fmt_mt_pos_query* q, uint64_t n_queries,
                           fmt_mt_pos_hit* out);

#ifdef __cplusplus
}
#endif
#endif /* FMT_POS_H_ */

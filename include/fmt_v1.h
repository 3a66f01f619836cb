/*
 * fmt_v1.h — bulk SnapshotV1 SharedString summaries, the peer of fmt.h's fmt_mt_summarize_legacy.
 *
 * SnapshotV1 (newMergeTreeSnapshotFormat, client.ts:1569-1580) is the summary format that keeps the
 * collaboration window: segments above minSeq carry seq / client, removedSeq / removedClient /
 * removedClientIds and movedSeq / movedSeqs / movedClientIds (merge-tree/src/snapshotV1.ts:90-276).
 * The conventions of fmt.h hold.
 */
#ifndef FMT_V1_H_
#define FMT_V1_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bulk SnapshotV1 summaries of every document of the last fmt_mt_run (replaces Client.summarize →
 * SnapshotV1.extractSync + emit, snapshotV1.ts:126-276, for all documents at once). The segmentation
 * (extractSync, snapshotV1.ts:170-276: skip what is removed at/below minSeq, merge acked segments
 * while canAppend && matchProperties, write every other segment alone), the text and the first
 * remove stamp of each removed segment (the op whose seq is its removedSeq / movedSeq) run on the
 * device, one wave per document; the later stamps are the documents' remove-order entries
 * (fmt_mt_remove_order, ops flagged FMT_MT_F_RMORDER), fetched in one copy and joined per segment on
 * the host; the JSON and the chunking by chunk_size units (emit, snapshotV1.ts:126-168; 0 = 10000,
 * SnapshotV1.chunkSize) run on `threads` host threads (0 = up to 16). keys / values: as
 * fmt_mt_summarize_legacy; segment properties are the segments' own (snapshotV1.ts:211).
 * client_names: every document's long client ids JSON-quoted, flattened; document d's are
 * client_names[doc_client_offsets[d] .. doc_client_offsets[d + 1]), entry k the name of short client
 * id k (getLongClientId, client.ts:857-863). Per document (fmt_mt_summary_v1_blobs): the replay's
 * status when it failed; FMT_E_UNSUPPORTED when a removed segment above minSeq has no removing op in
 * the batch (a stamp loaded from a summary); FMT_E_USAGE when a stamp's client has no name. The whole
 * call: FMT_E_USAGE before fmt_mt_run; FMT_E_UNSUPPORTED after a batch with local-client records
 * (FMT_MT_F_LOCAL_ANY: pending stamps have no SnapshotV1 form here). */
int fmt_mt_summarize_v1(fmt_ctx* ctx, const char* const* keys, uint32_t n_keys, const char* const* values,
                        uint32_t n_values, const char* const* client_names, const uint64_t* doc_client_offsets,
                        uint32_t chunk_size, uint32_t threads, fmt_summary_timing* timing);
/* Document d's header blob from the last fmt_mt_summarize_v1 and the number of its body blobs (what
 * SnapshotV1.emit adds to the summary tree as "header", snapshotV1.ts:126-168). Valid until the next
 * fmt_mt_summarize_v1, independent of the legacy blobs. The document's V1 status when it has none. */
int fmt_mt_summary_v1_blobs(fmt_ctx* ctx, uint32_t doc, const char** header, size_t* header_len, uint32_t* n_bodies);
/* Body blob k of document d ("body_k", snapshotV1.ts:150-158), k < n_bodies. */
int fmt_mt_summary_v1_body(fmt_ctx* ctx, uint32_t doc, uint32_t k, const char** body, size_t* body_len);

#ifdef __cplusplus
}
#endif
#endif /* FMT_V1_H_ */

/*
 * fmt_map_summary.h — bulk SharedMap summaries (SharedMap.summarizeCore, map.ts:176-246) of the sparse
 * map path, the peer of fmt.h's fmt_mt_summarize_legacy. The conventions of fmt.h hold.
 */
#ifndef FMT_MAP_SUMMARY_H_
#define FMT_MAP_SUMMARY_H_

#include "fmt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmt_map_summary_timing {
  double kernel_ms;            /* device ordering + blob assignment (events) */
  double fetch_ms;             /* device -> host */
  double format_ms;            /* host tables + JSON */
  uint64_t bytes;              /* blob bytes produced */
  uint32_t threads;
  uint32_t host_ordered_docs;  /* documents past the device tier, ordered on host threads */
} fmt_map_summary_timing;

/* Every document's summary from the sequenced entries of the last fmt_map_run_sparse or
 * fmt_map_run_sparse_tiered (pending local state is not summarised: summarizeCore reads
 * sequencedData only). keys[k]: key id k's string, JSON-quoted; values[v]: value id v's JSON text
 * (UTF-8), as fmt_mt_summarize_legacy takes them. The entries are put into JS object order (array-index
 * keys ascending, then birth order) and split into blobs on the device for documents of at most 2048
 * live entries, on the host threads for the rest (timing->host_ordered_docs); the JSON is written on
 * `threads` host threads (0: up to 16). The replay's own results are left as they are:
 * fmt_map_fetch_sparse and fmt_map_pending_run return afterwards what they returned before.
 * fmt_get_stats then describes this call (ops: live entries).
 * FMT_E_USAGE before a sparse run or on null arguments; FMT_E_DATA when the run saw a key id >=
 * key_bound; FMT_E_CAPACITY when a plain fmt_map_run_sparse refused a document (it cannot be told
 * from an empty one: run fmt_map_run_sparse_tiered). */
int fmt_map_summarize(fmt_ctx* ctx, const char* const* keys, uint32_t n_keys, const char* const* values,
                      uint32_t n_values, uint32_t threads, fmt_map_summary_timing* timing);
/* Document doc's header blob and its number of blobs ("blob0" ...), from the last fmt_map_summarize;
 * valid until the next one or the next map load. FMT_E_USAGE for a document with a live entry whose
 * key id is >= n_keys or whose value id is neither FMT_MAP_VALUE_UNDEFINED nor < n_values (the other
 * documents are unaffected). */
int fmt_map_summary_blobs(fmt_ctx* ctx, uint32_t doc, const char** header, size_t* header_len, uint32_t* n_blobs);
/* Blob k of document doc. */
int fmt_map_summary_blob(fmt_ctx* ctx, uint32_t doc, uint32_t k, const char** blob, size_t* blob_len);

#ifdef __cplusplus
}
#endif

#endif /* FMT_MAP_SUMMARY_H_ */

"""Measurement of the bulk SnapshotV1 summary path (fmt_mt_summarize_v1, csrc/summary_v1.hip) on T1
with remove order flagged: kernel, fetch and format ms and summaries/s, beside the bulk legacy path
(fmt_mt_summarize_legacy) on the same replay in the same process, and the per-document Python V1 path
(fmt_mt_fetch_doc + fmt_mt_fetch_remove_order + summary.v1_summary) on a sample of documents, whose
blobs are compared with the bulk ones byte for byte before anything is reported. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]


def _median(rows, key):
    return float(np.median([r[key] for r in rows]))


def _timed(call, steps):
    call()  # warm-up: code objects, the ctx's device and pinned buffers
    rows = []
    for _ in range(steps):
        t0 = time.perf_counter()
        r = call()
        r["wall_ms"] = (time.perf_counter() - t0) * 1e3
        rows.append(r)
    out = {k: _median(rows, k) for k in ("kernel_ms", "fetch_ms", "format_ms", "wall_ms")}
    out["bytes"], out["threads"] = rows[-1]["bytes"], rows[-1]["threads"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--ops-per-doc", type=int, default=2000)
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0, help="formatter threads (0: the library's default)")
    ap.add_argument("--sample", type=int, default=200, help="documents of the per-document Python path")
    args = ap.parse_args()

    import torch  # (torch's HIP runtime first: conftest / DESIGN note on the load order)

    torch.cuda.init()
    from fluidframework_amd import native, summary, workloads
    from fluidframework_amd.streams import flag_remove_order

    t0 = time.time()
    batch = workloads.conflict_farm(args.docs, n_clients=args.clients, ops_per_doc=args.ops_per_doc, seed=args.seed)
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    names = [f"c{k}" for k in range(args.clients + 1)]  # (generated farms carry no names; short ids 1..clients)
    clients = [names] * args.docs
    print(f"[v1] generated {args.docs} docs, {len(batch.ops)} ops in {time.time() - t0:.1f}s", flush=True)
    e = native.Engine(0)
    e.mt_load(batch)
    e.mt_run()
    hdrs = e.mt_headers(raise_on_failed_docs=False)
    ok_docs = np.nonzero(hdrs["status"] == 0)[0]  # (a failed replay has no summary in either format)
    print(f"[v1] replay {e.stats().kernel_ms:.1f} ms (remove order recorded), {args.docs - len(ok_docs)} documents failed",
          flush=True)
    legacy = _timed(lambda: e.mt_summarize_legacy(batch.keys, batch.values, threads=args.threads), args.steps)
    v1 = _timed(lambda: e.mt_summarize_v1(batch.keys, batch.values, clients, threads=args.threads), args.steps)
    for name, r in (("legacy", legacy), ("v1", v1)):
        r["total_ms"] = r["kernel_ms"] + r["fetch_ms"] + r["format_ms"]
        r["summaries_per_s"] = len(ok_docs) / (r["total_ms"] / 1e3)
        print(f"[v1] bulk {name}: kernel {r['kernel_ms']:.2f} fetch {r['fetch_ms']:.2f} format {r['format_ms']:.2f} ms, "
              f"{r['summaries_per_s']:.0f} summaries/s, {r['bytes']} blob bytes, {r['threads']} threads", flush=True)
    # the per-document Python path on a sample, and its blobs against the bulk ones
    sample = [int(d) for d in ok_docs[:: max(1, len(ok_docs) // args.sample)][: args.sample]]
    equal, merge_info = 0, 0
    t0 = time.perf_counter()
    py = []
    for d in sample:
        lv, ch, pr = e.mt_doc(d, hdrs[d])
        a, b = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
        rm = summary.removers_from_engine(lv, int(hdrs[d]["n_leaves"]), e.mt_remove_order(d, hdrs[d]), batch.ops[a:b])
        py.append(summary.v1_summary(hdrs[d], lv, ch, pr, batch.keys, batch.values, names, rm))
    py_s = time.perf_counter() - t0
    for d, want in zip(sample, py):
        equal += e.mt_summary_v1(d) == want
        merge_info += want[0].count('"removedClientIds"') + sum(b.count('"removedClientIds"') for b in want[1])
    e.close()
    ok = equal == len(sample) and merge_info > 0
    line = {
        "metric": "SnapshotV1 summaries written/sec (bulk: device segmentation + host JSON)",
        "value": v1["summaries_per_s"], "unit": "summaries/s", "n_gpus": 1, "steps": args.steps,
        "higher_is_better": True, "data": "synthetic",
        "config": {"workload": "T1 conflict farm, remove order flagged", "docs": args.docs,
                   "ops_per_doc": args.ops_per_doc, "clients": args.clients, "seed": args.seed,
                   "docs_summarized": int(len(ok_docs)),
                   "docs_failed_in_replay": {native.STATUS_NAMES.get(int(c), int(c)): int(n) for c, n in
                                             zip(*np.unique(hdrs["status"][hdrs["status"] != 0], return_counts=True))}},
        "v1": v1, "legacy": legacy,
        "python_per_document": {"docs": len(sample), "seconds": py_s, "summaries_per_s": len(sample) / py_s},
        "sample_equal": equal, "sample_removed_segments": merge_info, "equal": bool(ok),
    }
    print(json.dumps(line), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""Measurement of the bulk SharedMap summaries (fmt_map_summarize, csrc/map_summary.hip) at the
benchmarked sparse shape: the documents of `bench.py --workload map --sparse --key-pool 1048576`
replayed once, then every document's summary produced `steps` times each way, alternating:

  device   ordering and blob assignment on the device (map_summary.hip), JSON on the host threads
  host     the same call with the device tier switched off (fmt_internal_map_summary_host_only): every
           document ordered by csrc/map_sum_plan.h on the same host threads

The host figure is the reference the device ordering is judged against. Both produce the same bytes
(checked: a digest of every header and blob of a sample, and the total). Prints one JSON line with the
median and the range of kernel_ms / fetch_ms / format_ms and summaries/s of both."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def _digest(eng, docs):
    h = hashlib.sha256()
    for d in docs:
        head, blobs = eng.map_summary_doc(d)
        h.update(head.encode())
        for b in blobs:
            h.update(b"\0" + b.encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--ops-per-doc", type=int, default=1000)
    ap.add_argument("--key-pool", type=int, default=1 << 20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch  # (torch's HIP runtime first: DESIGN note on the load order)

    torch.cuda.init()
    from fluidframework_amd import native, workloads

    t0 = time.time()
    batch = workloads.map_stream(args.docs, args.ops_per_doc, key_pool=args.key_pool, seed=args.seed)
    values = [workloads.map_value_json(i) for i in range(50 + args.ops_per_doc + 1)]
    print(f"[map-summary] generated {args.docs} docs, {len(batch.ops)} ops in {time.time() - t0:.1f}s", flush=True)
    e = native.Engine(0)
    e.map_load_sparse(batch)
    e.map_run_sparse_tiered()
    counts, _ = e.map_fetch_sparse()
    live = int(counts.sum())
    sample = range(0, args.docs, max(1, args.docs // 1000))
    runs = {"device": [], "host": []}
    digests = {}
    for step in range(args.warmup + args.steps):
        for mode in ("device", "host") if step % 2 == 0 else ("host", "device"):  # alternate, and who goes first
            e.map_summary_host_only(mode == "host")
            t0 = time.time()
            t = e.map_summarize(batch.keys, values, threads=args.threads)
            t["call_ms"] = (time.time() - t0) * 1e3  # (with the Python side's key quoting: not part of either figure)
            t["ms"] = t["kernel_ms"] + t["fetch_ms"] + t["format_ms"]
            digests.setdefault(mode, set()).add((_digest(e, sample), t["bytes"]))
            if step >= args.warmup:
                runs[mode].append(t)
            print(f"[map-summary] {mode:6s} kernel {t['kernel_ms']:.2f} fetch {t['fetch_ms']:.2f} format {t['format_ms']:.2f} ms; "
                  f"{t['host_ordered_docs']} documents ordered on the host", flush=True)
    e.map_summary_host_only(False)
    e.close()
    equal = len(digests["device"] | digests["host"]) == 1

    def stat(mode, field):
        x = [r[field] for r in runs[mode]]
        return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))}

    line = {
        "metric": "SharedMap summaries/sec (sparse entries to blobs, one call)",
        "config": {"docs": args.docs, "ops_per_doc": args.ops_per_doc, "key_pool": args.key_pool, "threads": args.threads,
                   "live_entries": live, "max_live": int(counts.max()), "steps": args.steps, "warmup": args.warmup},
        "bytes": runs["device"][0]["bytes"],
        "equal": bool(equal),
    }
    for mode in ("device", "host"):
        line[mode] = {f: stat(mode, f) for f in ("kernel_ms", "fetch_ms", "format_ms", "ms")}
        line[mode]["summaries_per_s"] = args.docs / (line[mode]["ms"]["median"] / 1e3)
        line[mode]["host_ordered_docs"] = runs[mode][0]["host_ordered_docs"]
    line["device_over_host"] = line["host"]["ms"]["median"] / line["device"]["ms"]["median"]
    print(json.dumps(line), flush=True)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())

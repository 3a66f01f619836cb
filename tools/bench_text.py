#!/usr/bin/env python3
"""Bulk getText against the per-document read it replaces, in one process on one GPU.

One load and one run of the T1-shaped batch (conflict farm, 20,000 documents x 2000 ops by default),
then each of these `--repeats` times:
  (a) Engine.mt_text_strings(): fmt_mt_fetch_text_all, two kernels and one packed copy;
  (b) mt_doc(d) + visible_text for every document: fmt_mt_fetch_doc and a host walk over the leaves.
(a) == (b) is checked for every document. --bulk-only leaves (b) and the check out: the form to trace,
`rocprofv3 --kernel-trace --stats -- python tools/bench_text.py --bulk-only`, since (b)'s 80,000 copies
only slow a traced run down. Prints one JSON line: the times, the units and leaves read,
and the gather pass's algorithmic bytes (32 per leaf + 2 per unit read + 2 per unit written)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    from fluidframework_amd import native, workloads
    from mt_compare import visible_text

    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--unique", type=int, default=2000)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bulk-only", action="store_true", help="time (a) alone (for a kernel trace)")
    a = ap.parse_args()
    batch = workloads.conflict_farm(a.unique, n_clients=8, ops_per_doc=a.ops, seed=5, replicas=a.docs // a.unique)
    eng = native.Engine(0)
    try:
        eng.mt_load(batch)
        eng.mt_run()
        hdrs = eng.mt_headers()
        bulk, per_doc, texts, ref = [], [], None, None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            texts = eng.mt_text_strings()
            bulk.append(time.perf_counter() - t0)
            if a.bulk_only:
                continue
            t0 = time.perf_counter()
            ref = []
            for d in range(batch.n_docs):
                leaves, chars, _ = eng.mt_doc(d, hdrs[d])
                ref.append(visible_text(hdrs[d], leaves, chars))
            per_doc.append(time.perf_counter() - t0)
            assert texts == ref, "bulk text differs from the per-document read"
        units = sum(len(t.encode("utf-16-le", "surrogatepass")) // 2 for t in texts)
        leaves = int(hdrs["n_leaves"].sum(dtype="uint64"))
        print(json.dumps({"docs": batch.n_docs, "ops": len(batch.ops), "repeats": a.repeats, "leaves": leaves,
                          "units": units, "gather_bytes": 32 * leaves + 4 * units,
                          "bulk_s": bulk, "per_doc_s": per_doc,
                          "bulk_slowest_below_per_doc_fastest": max(bulk) < min(per_doc) if per_doc else None}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Bulk property runs against the per-document read they replace, in one process on one GPU.

One load and one run of the T1-shaped batch (conflict farm, 20,000 documents x 2000 ops by default),
then each of these `--repeats` times:
  (a) Engine.mt_prop_runs() + Engine.mt_props_all(): fmt_mt_fetch_prop_runs_all (three kernels, one
      packed copy) and fmt_mt_fetch_props_all (one gather, one packed copy);
  (b) mt_doc(d) + expected_runs (tests/runs_cases.py) for every document: fmt_mt_fetch_doc and a host walk
      over the leaves.
(a) == (b) is checked for every document, runs and tables, byte for byte. --bulk-only leaves (b) and the
check out: the form to trace, `rocprofv3 --kernel-trace --stats -- python tools/bench_runs.py --bulk-only`.
Prints one JSON line: the times, run counts, leaves per run and the algorithmic bytes of each pass (32 per
leaf read, 2 per prop record's class, 16 per run written)."""
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
        bulk, per_doc = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            offs, runs = eng.mt_prop_runs()
            poffs, props = eng.mt_props_all()
            bulk.append(time.perf_counter() - t0)
            if a.bulk_only:
                continue
            from runs_cases import expected_runs

            t0 = time.perf_counter()
            ref = []
            for d in range(batch.n_docs):
                leaves, _, table = eng.mt_doc(d, hdrs[d])
                ref.append((expected_runs(hdrs[d], leaves, table), table))
            per_doc.append(time.perf_counter() - t0)
            for d, (r, table) in enumerate(ref):
                assert runs[int(offs[d]) : int(offs[d + 1])].tobytes() == r.tobytes(), f"document {d}: runs differ"
                assert props[int(poffs[d]) : int(poffs[d + 1])].tobytes() == table.tobytes(), f"document {d}: tables differ"
        leaves = int(hdrs["n_leaves"].sum(dtype="uint64"))
        visible = int(hdrs["visible_len"].sum(dtype="uint64"))
        n_runs, n_props = int(offs[-1]), int(poffs[-1])
        print(json.dumps({"docs": batch.n_docs, "ops": len(batch.ops), "repeats": a.repeats, "leaves": leaves,
                          "positions": visible, "runs": n_runs, "prop_records": n_props,
                          "leaves_per_run": round(leaves / max(n_runs, 1), 3),
                          "positions_per_run": round(visible / max(n_runs, 1), 3),
                          "class_bytes": 2 * n_props, "pass1_bytes": 32 * leaves, "pass2_bytes": 32 * leaves + 16 * n_runs,
                          "bulk_s": bulk, "per_doc_s": per_doc,
                          "bulk_slowest_below_per_doc_fastest": max(bulk) < min(per_doc) if per_doc else None}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()

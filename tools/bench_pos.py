#!/usr/bin/env python3
"""Bulk position queries against the per-document read they replace, in one process on one GPU.

One load and one run of the T1-shaped batch (conflict farm, 20,000 documents x 2000 ops by default). Per
document 8 local-view queries and 8 remote-view queries (4 at cur_seq for a client that wrote nothing, 4 in
the middle of the collab window for writer 1), positions drawn from [0, visible_len] with a fixed seed. Then
each of these `--repeats` times:
  (a) Engine.mt_positions(): fmt_mt_query_positions (two kernels, one copy back);
  (b) mt_doc(d) + expected_hits (tests/pos_cases.py) for every document: fmt_mt_fetch_doc and a host walk
      over the leaves.
(a) == (b) is checked byte for byte. --bulk-only leaves (b) and the check out: the form to trace,
`rocprofv3 --kernel-trace --stats -- python tools/bench_pos.py --bulk-only`.
Prints one JSON line: the times, the counts (queries, views, leaves) and the algorithmic bytes of each pass
(pass 1 reads 32 per leaf per view of its document; pass 2 reads at most one tile's leaves per query and
writes 32 per query)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import numpy as np

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
        n = batch.n_docs
        rng = np.random.default_rng(11)
        q = np.zeros((n, 16), dtype=native.POS_QUERY_DTYPE)
        q["pos"] = (rng.random((n, 16)) * (hdrs["visible_len"].astype(np.float64)[:, None] + 1)).astype(np.uint32)
        q["ref_seq"][:, :8] = native.VIEW_LOCAL
        q["ref_seq"][:, 8:12] = hdrs["cur_seq"][:, None]
        q["client"][:, 8:12] = 63
        q["ref_seq"][:, 12:] = ((hdrs["min_seq"].astype(np.int64) + hdrs["cur_seq"]) // 2)[:, None]
        q["client"][:, 12:] = 1
        q = q.reshape(-1)
        offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(16)
        bulk, per_doc = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            hits = eng.mt_positions(q, offs)
            bulk.append(time.perf_counter() - t0)
            if a.bulk_only:
                continue
            from pos_cases import expected_hits

            t0 = time.perf_counter()
            ref = []
            for d in range(n):
                leaves, chars, _ = eng.mt_doc(d, hdrs[d])
                ref.append(expected_hits(hdrs[d], leaves, chars, q[16 * d : 16 * d + 16]))
            per_doc.append(time.perf_counter() - t0)
            assert hits.tobytes() == np.concatenate(ref).tobytes(), "bulk and per-document hits differ"
        leaves = int(hdrs["n_leaves"].sum(dtype="uint64"))
        print(json.dumps({"docs": n, "ops": len(batch.ops), "repeats": a.repeats, "leaves": leaves, "queries": len(q),
                          "views": 3 * n, "ok": int((hits["status"] == 0).sum()), "past_end": int((hits["status"] == native.FMT_E_DATA).sum()),
                          "hidden_locally": int(((hits["flags"] & native.POS_F_HIDDEN_LOCALLY) != 0).sum()),
                          "pass1_bytes": 3 * 32 * leaves, "pass2_bytes_at_most": 16 * 32 * leaves + 32 * len(q),
                          "bulk_s": bulk, "per_doc_s": per_doc,
                          "bulk_slowest_below_per_doc_fastest": max(bulk) < min(per_doc) if per_doc else None}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()

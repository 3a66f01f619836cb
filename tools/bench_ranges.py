#!/usr/bin/env python3
"""Bulk range reads against the routes they replace, in one process on one GPU.

(a) One load and one run of the T1-shaped batch (conflict farm, 20,000 documents x 2000 ops by default). Per
    document 16 ranges drawn with a fixed seed: 8 in the local view, 4 at cur_seq for a client that wrote
    nothing, 4 in the middle of the collab window for writer 1. Then each of these `--repeats` times:
      bulk      Engine.mt_text_ranges(): fmt_mt_fetch_text_ranges, sizing call and fill;
      existing  for the local ranges mt_texts() and host slices; for the remote ones mt_doc(d) and
                expected_ranges (tests/range_cases.py) for every document: fmt_mt_fetch_doc and a host walk.
    bulk == existing is checked byte for byte.
(b) --segments N: one document of N segments (workloads.t3_stream with --large-ops ops). One 1,024-unit window
    in the middle of the local view through mt_text_ranges() against mt_texts() of the whole and a host slice,
    `--repeats` times each, equality checked.
--bulk-only leaves the existing routes and the checks out: the form to trace,
`rocprofv3 --kernel-trace --stats -- python tools/bench_ranges.py --bulk-only`.
Prints one JSON line per part: the times and the counts (queries, units read, units of the whole text)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def part_a(eng, a, np, native, workloads):
    batch = workloads.conflict_farm(a.unique, n_clients=8, ops_per_doc=a.ops, seed=5, replicas=a.docs // a.unique)
    eng.mt_load(batch)
    eng.mt_run()
    hdrs = eng.mt_headers()
    n = batch.n_docs
    rng = np.random.default_rng(11)
    q = np.zeros((n, 16), dtype=native.RANGE_QUERY_DTYPE)
    # local ranges inside [0, visible_len]; remote ones start in the first quarter and run to the view's end or a short way
    vis = hdrs["visible_len"].astype(np.float64)[:, None]
    x, y = rng.random((n, 8)) * (vis + 1), rng.random((n, 8)) * (vis + 1)
    q["start"][:, :8], q["end"][:, :8] = np.minimum(x, y).astype(np.uint32), np.maximum(x, y).astype(np.uint32)
    q["ref_seq"][:, :8] = native.VIEW_LOCAL
    q["start"][:, 8:] = (rng.random((n, 8)) * (vis / 4)).astype(np.uint32)
    q["end"][:, 8:] = native.RANGE_TO_END
    q["end"][:, 8::2] = q["start"][:, 8::2] + np.uint32(3)  # (past a short view's end: FMT_E_DATA on both sides)
    q["ref_seq"][:, 8:12] = hdrs["cur_seq"][:, None]
    q["client"][:, 8:12] = 63
    q["ref_seq"][:, 12:] = ((hdrs["min_seq"].astype(np.int64) + hdrs["cur_seq"]) // 2)[:, None]
    q["client"][:, 12:] = 1
    q = q.reshape(-1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(16)
    bulk, existing = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        hits, units = eng.mt_text_ranges(q, offs)
        bulk.append(time.perf_counter() - t0)
        if a.bulk_only:
            continue
        from range_cases import expected_ranges

        t0 = time.perf_counter()
        toffs, text = eng.mt_texts()
        parts = []
        for d in range(n):
            whole = text[int(toffs[d]) : int(toffs[d + 1])]
            mine = q[16 * d : 16 * d + 16]
            parts += [whole[int(s) : int(e)] for s, e in zip(mine["start"][:8], mine["end"][:8])]
            leaves, chars, _ = eng.mt_doc(d, hdrs[d])
            parts.append(expected_ranges(hdrs[d], leaves, chars, mine[8:], 0)[1])
        existing.append(time.perf_counter() - t0)
        assert units.tobytes() == np.concatenate(parts).tobytes(), "bulk and existing routes differ"
    print(json.dumps({"part": "a", "docs": n, "ops": len(batch.ops), "repeats": a.repeats, "queries": len(q),
                      "ok": int((hits["status"] == 0).sum()), "past_end": int((hits["status"] == native.FMT_E_DATA).sum()),
                      "units": len(units), "leaves": int(hdrs["n_leaves"].sum(dtype="uint64")), "bulk_s": bulk, "existing_s": existing,
                      "bulk_slowest_below_existing_fastest": max(bulk) < min(existing) if existing else None}))


def part_b(eng, a, np, native, workloads):
    batch = workloads.t3_stream(n_segments=a.segments, n_ops=a.large_ops)
    t0 = time.perf_counter()
    eng.mt_load(batch)
    eng.mt_run()
    load_run = time.perf_counter() - t0
    hdr = eng.mt_headers()[0]
    mid = int(hdr["visible_len"]) // 2
    q = np.zeros(1, dtype=native.RANGE_QUERY_DTYPE)
    q["start"], q["end"], q["ref_seq"] = mid, mid + 1024, native.VIEW_LOCAL
    offs = np.array([0, 1], dtype=np.uint64)
    bulk, existing = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        hits, units = eng.mt_text_ranges(q, offs)
        bulk.append(time.perf_counter() - t0)
        if a.bulk_only:
            continue
        t0 = time.perf_counter()
        _, text = eng.mt_texts()
        window = text[mid : mid + 1024]
        existing.append(time.perf_counter() - t0)
        assert int(hits[0]["status"]) == 0 and units.tobytes() == window.tobytes(), "the window and the slice of the whole text differ"
    print(json.dumps({"part": "b", "segments": a.segments, "ops": len(batch.ops), "leaves": int(hdr["n_leaves"]),
                      "visible_len": int(hdr["visible_len"]), "load_run_s": load_run, "units": len(units), "bulk_s": bulk,
                      "existing_s": existing, "bulk_slowest_below_existing_fastest": max(bulk) < min(existing) if existing else None}))


def main():
    import numpy as np

    from fluidframework_amd import native, workloads

    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--unique", type=int, default=2000)
    ap.add_argument("--ops", type=int, default=2000)
    ap.add_argument("--segments", type=int, default=1_000_000, help="part (b): segments of the one large document (0: skip)")
    ap.add_argument("--large-ops", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--bulk-only", action="store_true", help="time the bulk read alone (for a kernel trace)")
    a = ap.parse_args()
    eng = native.Engine(0)
    try:
        if not a.skip_a:
            part_a(eng, a, np, native, workloads)
        if a.segments:
            part_b(eng, a, np, native, workloads)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

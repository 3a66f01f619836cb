"""Bulk property runs (include/fmt_runs.h): the reference the runs tests compare against, and the batches
they share (tests only).

expected_runs restates the header's definition over one document's state as the oracle dumps it (header,
leaves, prop-set table), leaf by leaf. tile_reports / emit_tiles restate the two device passes at any tile
size in the same plain way, so that the host stitch between them (csrc/runs_plan.h through
native.runs_plan) can be checked without a device."""
import numpy as np

import text_cases
from fluidframework_amd import native, workloads
from fluidframework_amd.native import PROP_RUN_DTYPE, PROPS_CONT, propset_entries
from fluidframework_amd.streams import MergeTreeStreamBuilder
from text_cases import LEAF_MARKER, NOT_REMOVED, msg

NO_CLASS = 0xFFFF


def classes_of(props) -> list:
    """Per record of a document's prop-set table its match class: 0xffff for an empty set, else the lowest
    first-record id holding the same entries in any order (continuation records: their own id, no leaf
    names them)."""
    out, seen = [], {}
    for p in range(len(props)):
        n = int(props[p]["n"])
        if n == 0:
            out.append(NO_CLASS)
        elif n == PROPS_CONT:
            out.append(p)
        else:
            out.append(seen.setdefault(frozenset(propset_entries(props, p)), p))
    return out


def _visible(hdr, leaves):
    """(leaf index, units, class key source) of every leaf that counts, in document order."""
    for i, L in enumerate(leaves[: int(hdr["n_leaves"])]):
        if int(L["rm_seq"]) != NOT_REMOVED or int(L["len"]) == 0:
            continue
        marker = bool(int(L["pad"]) & LEAF_MARKER)
        yield i, (1 if marker else int(L["len"])), int(L["props"]), marker


def expected_runs(hdr, leaves, props) -> np.ndarray:
    if int(hdr["status"]) != 0:
        return np.zeros(0, dtype=PROP_RUN_DTYPE)
    cls = classes_of(props[: int(hdr["n_props"])])
    runs, pos = [], 0
    for i, units, p, marker in _visible(hdr, leaves):
        c = NO_CLASS if p == NO_CLASS else cls[p]
        if runs and not marker and not runs[-1][4] and runs[-1][3] == c:
            runs[-1][1] += units
        else:
            runs.append([pos, units, i, c, 1 if marker else 0])
        pos += units
    out = np.zeros(len(runs), dtype=PROP_RUN_DTYPE)
    for k, r in enumerate(runs):
        out[k] = tuple(r)
    return out


def expected_batch(hdrs, leaves, props, ok=None):
    """(offsets uint64[n + 1], runs) over mt_replay_batch's arrays: what Engine.mt_prop_runs returns."""
    parts = [expected_runs(hdrs[d], leaves[d], props[d]) if ok is None or ok[d] else np.zeros(0, PROP_RUN_DTYPE)
             for d in range(len(hdrs))]
    offs = np.zeros(len(hdrs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return offs, (np.concatenate(parts) if parts else np.zeros(0, PROP_RUN_DTYPE))


# ---- the two device passes restated per tile (the stitch between them is native.runs_plan)
def _tile_leaves(hdr, leaves, props, first, n):
    cls = classes_of(props[: int(hdr["n_props"])])
    for i, units, p, marker in _visible(hdr, leaves):
        if first <= i < first + n:
            yield i, units, (NO_CLASS if p == NO_CLASS else cls[p]), marker


def tile_reports(hdrs, docs, T) -> np.ndarray:
    """Pass 1 over documents docs[d] = (leaves, props) cut into tiles of T leaves: one RUN_TILE_DTYPE each."""
    plan = native.text_plan(hdrs, tile_leaves=T)
    out = np.zeros(len(plan.items), dtype=native.RUN_TILE_DTYPE)
    for k, (d, first, n) in enumerate(plan.items.tolist()):
        prev = None
        for i, units, c, marker in _tile_leaves(hdrs[d], docs[d][0], docs[d][1], first, n):
            key = c | (native.RUN_END_MARKER if marker else 0) | native.RUN_END_HAS
            if prev is None:
                out[k]["first"] = key
            if prev is None or marker or prev[1] or prev[0] != c:
                out[k]["heads"] += 1
                out[k]["tail"] = 0
            out[k]["tail"] += units
            out[k]["units"] += units
            out[k]["last"] = key
            prev = (c, marker)
    return out


def emit_tiles(hdrs, docs, T, plan) -> tuple:
    """Pass 2 with the stitch's bases (native.runs_plan's result): (offsets, runs); every field of every
    run must have been written exactly once."""
    items = native.text_plan(hdrs, tile_leaves=T).items.tolist()
    total = int(plan.offsets[-1])
    runs = np.zeros(total, dtype=PROP_RUN_DTYPE)
    wrote_head, wrote_len = np.zeros(total, int), np.zeros(total, int)
    for k, (d, first, n) in enumerate(items):
        flags, base = int(plan.flags[k]), int(plan.run_base[k])
        continues = bool(flags & native.RUN_CONTINUES)
        pos, open_start, rank, prev = int(plan.pos_base[k]), int(plan.open_start[k]), 0, None
        for i, units, c, marker in _tile_leaves(hdrs[d], docs[d][0], docs[d][1], first, n):
            head = (prev is None and not continues) or (prev is not None and (marker or prev[1] or prev[0] != c))
            if head:
                r = base + rank
                runs[r]["start"], runs[r]["first_leaf"], runs[r]["props"], runs[r]["flags"] = pos, i, c, int(marker)
                wrote_head[r] += 1
                if rank or continues:
                    runs[r - 1]["len"] = pos - open_start
                    wrote_len[r - 1] += 1
                open_start = pos
                rank += 1
            pos += units
            prev = (c, marker)
        if flags & native.RUN_CLOSES and (rank or continues):
            runs[base + rank - 1]["len"] = pos - open_start
            wrote_len[base + rank - 1] += 1
    assert (wrote_head == 1).all() and (wrote_len == 1).all()
    return plan.offsets, runs


# ---- shared batches
FARM_SEED = 23


def farm_batch():
    """64 documents x 200 ops, the shape of test_gpu_text.farm_batch."""
    return workloads.conflict_farm(64, n_clients=8, ops_per_doc=200, seed=FARM_SEED)


def vacuity(offs, runs, hdrs, leaves):
    """(runs made of two or more leaves, documents with two or more runs) of a batch's expected runs."""
    multi = docs2 = 0
    for d in range(len(hdrs)):
        r = runs[int(offs[d]) : int(offs[d + 1])]
        docs2 += len(r) >= 2
        vis = [i for i, _, _, _ in _visible(hdrs[d], leaves[d])]
        firsts = [int(x) for x in r["first_leaf"]] + [1 << 62]
        multi += sum(1 for a, b in zip(firsts[:-1], firsts[1:]) if sum(1 for i in vis if a <= i < b) >= 2)
    return multi, docs2


A, B = {"k": 1}, {"k": 2}
MARK = "marker"


def _build(d, specs, removed=(), annotate=()):
    """One insert per spec, appended: spec = props dict, None (no props) or MARK; every leaf one position.
    Then `annotate` = [(leaf, props)], then leaves `removed` (one remove each, last first)."""
    seq = 1
    for k, p in enumerate(specs):
        if p == MARK:
            seg = {"marker": {"refType": 1}, "props": {"markerId": f"m{k}"}}
        else:
            seg = "x" if p is None else {"text": "x", "props": p}
        d.add_message(msg("AB"[k % 2], seq, {"type": 0, "pos1": k, "seg": seg}))
        seq += 1
    for leaf, p in annotate:
        d.add_message(msg("A", seq, {"type": 2, "pos1": leaf, "pos2": leaf + 1, "props": p}))
        seq += 1
    for leaf in sorted(removed, reverse=True):
        d.add_message(msg("B", seq, {"type": 1, "pos1": leaf, "pos2": leaf + 1}))
        seq += 1


def edge_documents():
    """[(name, intended leaf count, specs, removed leaves, annotates, intended run count or None)]: every
    document of the chunk-edge batch. Inserts stay above minSeq (msn 0), so zamboni merges nothing."""
    alt = lambda n: [A if k % 2 else B for k in range(n)]  # noqa: E731
    docs = [("empty", [], (), (), 0)]
    for n in (63, 64, 65, 129):
        docs.append((f"one_class_{n}", [A] * n, (), (), 1))
        docs.append((f"alternating_{n}", alt(n), (), (), n))
    docs += [
        ("change_63_64", [A] * 64 + [B] * 65, (), (), 2),
        ("change_64_65", [A] * 65 + [B] * 64, (), (), 2),
        ("removed_between", [A] * 65, (10,), (), 1),
        ("removed_lane_63", [A] * 129, (63,), (), 1),
        ("removed_lane_0", [A] * 129, (0, 64), (), 1),
        ("removed_63_then_change", [A] * 63 + [B] + [B] * 65, (63,), (), 2),
        ("removed_64_then_same", [A] * 64 + [B] + [A] * 64, (64,), (), 1),
        ("markers_ends_and_64", [MARK] + [A] * 63 + [MARK] + [A] * 63 + [MARK], (), (), 5),
        ("markers_adjacent", [A, MARK, MARK, A], (), (), 4),
        ("marker_removed_between", [A, MARK, A], (1,), (), 1),
        ("all_removed", [A, B, A], (0, 1, 2), (), 0),
        ("ab_ba", [{"a": 1, "b": 2}, {"b": 2, "a": 1}], (), (), 1),
        ("null_annotated", [A, None], (), ((0, {"k": None}),), 1),
    ]
    return [(name, len(specs), specs, rm, an, n_runs) for name, specs, rm, an, n_runs in docs]


def edge_batch():
    b = MergeTreeStreamBuilder()
    docs = edge_documents()
    for name, n, specs, rm, an, n_runs in docs:
        _build(b.begin_doc("", observer="observer"), specs, rm, an)
    return b.finish(), docs


def tile_documents(T):
    """Three documents of T + 40 one-position leaves of alternating classes around the tile edge: leaves
    T-3 .. T+3 one class; the same with leaf T-1 removed; Markers at T-1 and T."""
    n = T + 40
    alt = [A if k % 2 else B for k in range(n)]
    C = {"k": 7}
    span = [C if T - 3 <= k <= T + 3 else alt[k] for k in range(n)]
    marks = [MARK if k in (T - 1, T) else alt[k] for k in range(n)]
    return [("span", span, ()), ("span_removed", span, (T - 1,)), ("markers", marks, ())]


def tile_batch(T):
    b = MergeTreeStreamBuilder()
    docs = tile_documents(T)
    for name, specs, rm in docs:
        _build(b.begin_doc("", observer="observer"), specs, rm)
    return b.finish(), docs


def huge_middle_batch(T):
    """A small document, then one summary-loaded document of 2T + 52 one-unit segments (the huge tier):
    alternating classes, but segments T-5 .. 2T+5 all of one class, so that its middle tile lies wholly
    inside one run; one insert at its end."""
    n = 2 * T + 52
    b = MergeTreeStreamBuilder()
    _build(b.begin_doc("", observer="observer"), [A, A, B])
    texts = [{"text": chr(0x4E00 + i), "props": {"k": 7} if T - 5 <= i <= 2 * T + 5 else {"k": i % 2}} for i in range(n)]
    h = b.begin_doc_from_summary(text_cases.summary_header(texts), observer="observer")
    h.add_message(msg("B", 1, {"type": 0, "pos1": n, "seg": "!"}))
    return b.finish(), 1


def pending_local_batch():
    """text_cases.pending_local_batch with a pending local annotate added to the hand-made view (last)."""
    import local_farm

    b = MergeTreeStreamBuilder()
    for sd in (41, 42):
        local_farm.LocalFarm(sd, builder=b).run(150)
    d = b.begin_doc(initial_text="0123456789", observer="A")
    d.add_message(msg("B", 1, {"type": 0, "pos1": 5, "seg": "remote"}))
    d.local_op({"type": 0, "pos1": 2, "seg": "PENDING"})
    d.local_op({"type": 1, "pos1": 12, "pos2": 15})
    d.local_op({"type": 2, "pos1": 1, "pos2": 4, "props": {"bold": True}})
    d.add_message(msg("B", 2, {"type": 0, "pos1": 0, "seg": ">"}, ref=1))
    return b.finish()

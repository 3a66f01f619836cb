"""Bulk range reads (include/fmt_range.h): the reference the range tests compare against, and the helpers
they share (tests only).

expected_ranges restates the header's definitions over one document's state as the oracle (or the engine's
per-document fetch) dumps it: header, leaves, chars; views and statuses are pos_cases'. item_units /
gather_items restate the two device passes per work item in the same plain way, so that the host plan around
them (csrc/range_plan.h through native.range_plan) can be checked without a device."""
import numpy as np

import pos_cases
from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_DATA, RANGE_HIT_DTYPE, RANGE_QUERY_DTYPE, RANGE_TO_END, VIEW_LOCAL
from text_cases import LEAF_MARKER


def view_text(leaves, chars, ref_seq, client, placeholder):
    """(units, position of every unit in the view, the view's length): a visible text leaf gives its chars
    at consecutive positions, a visible Marker the placeholder at its one position when there is one."""
    u, _ = pos_cases.view_units(leaves, ref_seq, client)
    start = np.cumsum(u) - u
    marker = (leaves["pad"] & LEAF_MARKER) != 0
    text = (u > 0) & ~marker
    lens = u[text]
    first = np.cumsum(lens) - lens  # each text leaf's first unit among the text units
    k = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(first, lens)  # each unit's index in its leaf
    units = np.asarray(chars, dtype="<u2")[np.repeat(leaves["char_off"][text].astype(np.int64), lens) + k]
    where = np.repeat(start[text], lens) + k
    if placeholder:
        at = start[(u > 0) & marker]
        where = np.concatenate([where, at])
        units = np.concatenate([units, np.full(len(at), placeholder, dtype="<u2")])
        order = np.argsort(where, kind="stable")  # (positions are distinct)
        units, where = units[order], where[order]
    return units, where.astype(np.int64), int(u.sum())


def expected_ranges(hdr, leaves, chars, queries, placeholder, obliterates=False):
    """(RANGE_HIT_DTYPE per query of one document, the packed units): text_off counts from the document's
    first unit."""
    queries = np.asarray(queries, dtype=RANGE_QUERY_DTYPE)
    hits = np.zeros(len(queries), dtype=RANGE_HIT_DTYPE)
    L = leaves[: int(hdr["n_leaves"])]
    views, parts, at = {}, [], 0
    for k, q in enumerate(queries):
        st = pos_cases.query_status(hdr, q, obliterates)
        if st != 0:
            hits[k]["status"] = st
            continue
        ref = int(q["ref_seq"])
        key = (ref, 0 if ref == VIEW_LOCAL else int(q["client"]))
        if key not in views:
            views[key] = view_text(L, chars, *key, placeholder)
        units, where, length = views[key]
        start, end = int(q["start"]), int(q["end"])
        if end == RANGE_TO_END:
            end = length
        if not start <= end <= length:
            hits[k]["status"] = FMT_E_DATA
            continue
        a, b = np.searchsorted(where, [start, end], side="left")
        hits[k]["text_off"], hits[k]["units"], hits[k]["span"] = at, b - a, end - start
        parts.append(units[a:b])
        at += int(b - a)
    return hits, (np.concatenate(parts) if parts else np.zeros(0, "<u2"))


def expected_batch(hdrs, leaves, chars, queries, q_offsets, placeholder, obliterates=False):
    """expected_ranges over per-document arrays: what Engine.mt_text_ranges returns."""
    all_hits, all_units, at = [], [], 0
    for d in range(len(hdrs)):
        hits, units = expected_ranges(hdrs[d], leaves[d], chars[d], queries[int(q_offsets[d]) : int(q_offsets[d + 1])], placeholder,
                                      obliterates)
        hits["text_off"][hits["status"] == 0] += np.uint64(at)
        at += len(units)
        all_hits.append(hits)
        all_units.append(units)
    return (np.concatenate(all_hits) if all_hits else np.zeros(0, RANGE_HIT_DTYPE),
            np.concatenate(all_units) if all_units else np.zeros(0, "<u2"))


def pack(per_doc):
    """[(start, end, ref_seq, client) lists per document] -> (queries, q_offsets)."""
    offs = np.zeros(len(per_doc) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in per_doc], dtype=np.uint64)
    q = np.zeros(int(offs[-1]), dtype=RANGE_QUERY_DTYPE)
    at = 0
    for x in per_doc:
        for start, end, ref, client in x:
            q[at]["start"], q[at]["end"], q[at]["ref_seq"], q[at]["client"] = start, end, ref, client
            at += 1
    return q, offs


# ---- the device passes restated per work item (the plan around them is native.range_plan)
def tile_units(plan, docs) -> np.ndarray:
    """Pass A over documents docs[d] = (hdr, leaves, chars): (n_view_items, 2) units in the view and locally."""
    views = plan.views.tolist()
    out = np.zeros((len(plan.view_items), 2), dtype=np.uint64)
    for k, (d, first, n, v) in enumerate(plan.view_items.tolist()):
        _, ref, client, _ = views[v]
        u, ul = pos_cases.view_units(docs[d][1][first : first + n], ref, client)
        out[k] = (int(u.sum()), int(ul.sum()))
    return out


def _item_text(docs, row, placeholder):
    d, first, n, lo, hi, ref, client, _ = row
    hdr, leaves, chars = docs[d]
    assert first + n <= int(hdr["n_leaves"]) and 0 <= lo < hi
    units, where, length = view_text(leaves[first : first + n], chars, ref, client, placeholder)
    assert hi <= length, "an item lies inside its tile"
    a, b = np.searchsorted(where, [lo, hi], side="left")
    return units[a:b]


def item_units(plan, docs) -> np.ndarray:
    """Pass B: the text units of every item (Markers give none)."""
    return np.array([len(_item_text(docs, row, 0)) for row in plan.items.tolist()], dtype=np.uint64)


def gather_items(plan, docs, placeholder) -> np.ndarray:
    """Pass C: every item's units at its base; every unit of the packed text written exactly once."""
    out = np.zeros(plan.total, dtype="<u2")
    wrote = np.zeros(plan.total, int)
    for row, base in zip(plan.items.tolist(), plan.item_base.tolist()):
        t = _item_text(docs, row, placeholder)
        out[base : base + len(t)] = t
        wrote[base : base + len(t)] += 1
    assert (wrote == 1).all()
    return out


def run_plan(docs, queries, q_offsets, T, placeholder=0, obliterates=False):
    """native.range_plan around the restated passes at tile size T: what the engine returns, and the plan."""
    hdrs = np.array([h for h, _, _ in docs], dtype=native.DOC_RESULT_DTYPE)
    kw = dict(placeholder=placeholder, obliterates=obliterates, tile_leaves=T)
    first = native.range_plan(hdrs, queries, q_offsets, **kw)
    tu = tile_units(first, docs)
    cut = native.range_plan(hdrs, queries, q_offsets, tile_units=tu, **kw)
    if placeholder == 0:
        cut = native.range_plan(hdrs, queries, q_offsets, tile_units=tu, item_units=item_units(cut, docs), **kw)
    return cut.hits, gather_items(cut, docs, placeholder), cut

"""Bulk position queries (include/fmt_pos.h): the reference the position tests compare against, and the
helpers they share (tests only).

expected_hits restates the header's definitions over one document's state as the oracle (or the engine's
per-document fetch) dumps it: header, leaves, chars. tile_units / resolve_tiles restate the two device passes
at any tile size in the same plain way, so that the host plan between them (csrc/pos_plan.h through
native.pos_plan) can be checked without a device."""
import numpy as np

from fluidframework_amd import native
from fluidframework_amd.native import (FMT_E_DATA, FMT_E_UNSUPPORTED, FMT_E_USAGE, POS_F_END, POS_F_HIDDEN_LOCALLY, POS_F_MARKER,
                                       POS_HIT_DTYPE, POS_QUERY_DTYPE, VIEW_LOCAL)
from text_cases import LEAF_MARKER, NOT_REMOVED


def query_status(hdr, q, obliterates=False) -> int:
    """The status the header and the batch's flags decide for one query, in fmt_pos.h's order."""
    if int(hdr["status"]) != 0:
        return int(hdr["status"])
    if int(q["ref_seq"]) == VIEW_LOCAL:
        return 0
    if obliterates:
        return FMT_E_UNSUPPORTED
    if not 0 <= int(q["client"]) < 64:
        return FMT_E_UNSUPPORTED
    if not int(hdr["min_seq"]) <= int(q["ref_seq"]) <= int(hdr["cur_seq"]):
        return FMT_E_USAGE
    return 0


def view_units(leaves, ref_seq, client):
    """Per leaf its units in the view (ref_seq, client) and in the local view (int64 arrays)."""
    L = leaves
    units = np.where((L["pad"] & LEAF_MARKER) != 0, 1, L["len"]).astype(np.int64)
    local = L["rm_seq"] == NOT_REMOVED
    if ref_seq == VIEW_LOCAL:
        vis = local
    else:
        inserted = (L["ins_seq"] <= ref_seq) | (L["ins_client"] == client)
        removed = (L["rm_seq"] <= ref_seq) | (((L["rm_clients"] >> np.uint64(client)) & np.uint64(1)) != 0)
        vis = inserted & ~removed
    return units * vis, units * local


def _hit(rec, L, chars, i, offset, start, units, before_local, local_units):
    marker = bool(int(L["pad"]) & LEAF_MARKER)
    rec["leaf"], rec["offset"], rec["leaf_start"], rec["leaf_len"] = i, offset, start, units
    rec["local_pos"] = before_local + (offset if local_units else 0)
    rec["props"] = int(L["props"])
    rec["unit"] = int(chars[int(L["char_off"]) + (0 if marker else offset)])
    rec["flags"] = (POS_F_MARKER if marker else 0) | (0 if local_units else POS_F_HIDDEN_LOCALLY)


def expected_hits(hdr, leaves, chars, queries, obliterates=False) -> np.ndarray:
    """One POS_HIT_DTYPE per query of one document."""
    queries = np.asarray(queries, dtype=POS_QUERY_DTYPE)
    out = np.zeros(len(queries), dtype=POS_HIT_DTYPE)
    n = int(hdr["n_leaves"])
    L = leaves[:n]
    views = {}
    for k, q in enumerate(queries):
        st = query_status(hdr, q, obliterates)
        if st != 0:
            out[k]["status"] = st
            continue
        ref = int(q["ref_seq"])
        key = (ref, 0 if ref == VIEW_LOCAL else int(q["client"]))
        if key not in views:
            u, ul = view_units(L, *key)
            views[key] = (u, ul, np.cumsum(u), np.cumsum(ul))
        u, ul, cum, cum_local = views[key]
        length = int(cum[-1]) if n else 0
        pos = int(q["pos"])
        if pos > length:
            out[k]["status"] = FMT_E_DATA
        elif pos == length:
            out[k]["leaf"], out[k]["leaf_start"], out[k]["local_pos"] = n, length, int(cum_local[-1]) if n else 0
            out[k]["props"], out[k]["flags"] = 0xFFFF, POS_F_END
        else:
            i = int(np.searchsorted(cum, pos, side="right"))  # the first leaf whose units end past pos: it has some
            start = int(cum[i] - u[i])
            _hit(out[k], L[i], chars, i, pos - start, start, int(u[i]), int(cum_local[i] - ul[i]), int(ul[i]))
    return out


def expected_batch(hdrs, leaves, chars, queries, q_offsets, obliterates=False) -> np.ndarray:
    """expected_hits over per-document arrays (mt_replay_batch's, or lists): what Engine.mt_positions returns."""
    parts = [expected_hits(hdrs[d], leaves[d], chars[d], queries[int(q_offsets[d]) : int(q_offsets[d + 1])], obliterates)
             for d in range(len(hdrs))]
    return np.concatenate(parts) if parts else np.zeros(0, POS_HIT_DTYPE)


def pack(per_doc):
    """[(pos, ref_seq, client) lists per document] -> (queries, q_offsets)."""
    offs = np.zeros(len(per_doc) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in per_doc], dtype=np.uint64)
    q = np.zeros(int(offs[-1]), dtype=POS_QUERY_DTYPE)
    at = 0
    for x in per_doc:
        for pos, ref, client in x:
            q[at]["pos"], q[at]["ref_seq"], q[at]["client"] = pos, ref, client
            at += 1
    return q, offs


def view_length(hdr, leaves, ref_seq, client=0) -> int:
    return int(view_units(leaves[: int(hdr["n_leaves"])], ref_seq, client)[0].sum())


# ---- the two device passes restated per tile (the plan between them is native.pos_plan)
def tile_units(plan, docs) -> np.ndarray:
    """Pass 1 over documents docs[d] = (hdr, leaves, chars): (n_items, 2) units in the view and locally."""
    views = plan.views.tolist()
    out = np.zeros((len(plan.items), 2), dtype=np.uint64)
    for k, (d, first, n, v) in enumerate(plan.items.tolist()):
        _, ref, client, _ = views[v]
        u, ul = view_units(docs[d][1][first : first + n], ref, client)
        out[k] = (int(u.sum()), int(ul.sum()))
    return out


def resolve_tiles(plan, docs) -> np.ndarray:
    """Pass 2 over the plan's device queries: the records as the host left them, each device query's record
    written at most once, by the leaf of its one tile that holds the position."""
    out = plan.hits.copy()
    wrote = np.zeros(len(out), int)
    for d, first, n, pos, ref, client, view_base, local_base, at in plan.dev.tolist():
        hdr, leaves, chars = docs[d]
        assert first + n <= int(hdr["n_leaves"]) and int(out[at]["status"]) == FMT_E_DATA
        L = leaves[first : first + n]
        u, ul = view_units(L, ref, client)
        cum, cum_local = np.cumsum(u), np.cumsum(ul)
        assert 0 <= pos < int(cum[-1]), "a device query's position lies inside its tile"
        i = int(np.searchsorted(cum, pos, side="right"))
        start = int(cum[i] - u[i])
        out[at]["status"] = 0
        _hit(out[at], L[i], chars, first + i, pos - start, view_base + start, int(u[i]), local_base + int(cum_local[i] - ul[i]), int(ul[i]))
        wrote[at] += 1
    assert (wrote <= 1).all()
    return out


def run_plan(docs, queries, q_offsets, T, obliterates=False) -> np.ndarray:
    """native.pos_plan around the two restated passes at tile size T: what the engine returns."""
    hdrs = np.array([h for h, _, _ in docs], dtype=native.DOC_RESULT_DTYPE)
    first = native.pos_plan(hdrs, queries, q_offsets, obliterates=obliterates, tile_leaves=T)
    plan = native.pos_plan(hdrs, queries, q_offsets, tile_units=tile_units(first, docs), obliterates=obliterates, tile_leaves=T)
    return resolve_tiles(plan, docs), plan

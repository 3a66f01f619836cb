"""Bulk getText (include/fmt_text.h): the reference the text tests compare against, and the batches
they share (tests only).

expected_units restates the header's definition over one document's state as the oracle dumps it
(header, leaves, chars): the units of every leaf that is not removed and is not a Marker, in document
order; with a placeholder, every Marker that is not removed contributes that unit once."""
import numpy as np

from fluidframework_amd.streams import MergeTreeStreamBuilder

NOT_REMOVED = 0x7FFFFFFF
LEAF_MARKER = 0x8000
LOCAL_SEQ_BASE = 0x40000000  # fmt.h FMT_MT_LOCAL_SEQ_BASE: stamps of pending local ops


def expected_units(hdr, leaves, chars, placeholder=0) -> np.ndarray:
    if int(hdr["status"]) != 0:
        return np.zeros(0, dtype="<u2")
    out = []
    for L in leaves[: int(hdr["n_leaves"])]:
        if int(L["rm_seq"]) != NOT_REMOVED:
            continue
        if int(L["pad"]) & LEAF_MARKER:
            if placeholder:
                out.append(np.array([placeholder], dtype="<u2"))
            continue
        o = int(L["char_off"])
        out.append(np.asarray(chars[o : o + int(L["len"])], dtype="<u2"))
    return np.concatenate(out) if out else np.zeros(0, dtype="<u2")


def expected_batch(hdrs, leaves, chars, placeholder=0):
    """(offsets uint64[n + 1], units) over mt_replay_batch's arrays: what Engine.mt_texts returns."""
    parts = [expected_units(hdrs[d], leaves[d], chars[d], placeholder) for d in range(len(hdrs))]
    offs = np.zeros(len(hdrs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return offs, (np.concatenate(parts) if parts else np.zeros(0, dtype="<u2"))


def units_of(s: str) -> np.ndarray:
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype="<u2")


def oracle_doc(orc, batch, d):
    """Document d of a batch without summary loads replayed in one oracle client: text() and dump()."""
    doc = orc.MergeTreeDoc()
    o, n = (int(x) for x in batch.doc_init[d])
    if n:
        doc.insert_local(0, batch.text[o : o + n].tobytes().decode("utf-16-le", "surrogatepass"))
    doc.start_collab(0)
    rel = getattr(batch, "relpos", None)
    if rel is not None and len(rel):
        doc.set_relpos(rel, int(batch.marker_id_key))
    a, b = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
    doc.apply(batch.ops[a:b], batch.text, batch.props_off, batch.props_kv)
    return doc


def msg(client, seq, contents, ref=None, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": seq - 1 if ref is None else ref,
            "minimumSequenceNumber": msn, "contents": contents}


def pending_local_batch():
    """Writer views (local-client records): two local farms (local_farm.LocalFarm: submissions, acks,
    reconnects, rollbacks) and, last, one hand-made view whose stream ends with one pending insert and
    one pending remove over sequenced text."""
    import local_farm

    b = MergeTreeStreamBuilder()
    for sd in (41, 42):
        local_farm.LocalFarm(sd, builder=b).run(150)
    d = b.begin_doc(initial_text="0123456789", observer="A")
    d.add_message(msg("B", 1, {"type": 0, "pos1": 5, "seg": "remote"}))
    d.local_op({"type": 0, "pos1": 2, "seg": "PENDING"})
    d.local_op({"type": 1, "pos1": 12, "pos2": 15})
    d.add_message(msg("B", 2, {"type": 0, "pos1": 0, "seg": ">"}, ref=1))
    return b.finish()


def pending_counts(hdr, leaves):
    """(visible leaves of pending local inserts, leaves hidden by a pending local remove)."""
    L = leaves[: int(hdr["n_leaves"])]
    ins = (L["ins_seq"] >= LOCAL_SEQ_BASE) & (L["rm_seq"] == NOT_REMOVED)
    rm = (L["rm_seq"] >= LOCAL_SEQ_BASE) & (L["rm_seq"] != NOT_REMOVED)
    return int(ins.sum()), int(rm.sum())


# ---- hand-built documents for the chunk and copy edges (test_gpu_text.py). Consecutive inserts carry
# differing props, so no two leaves merge (zamboni needs matching props; minSeq stays 0 anyway).
def _distinct_inserts(d, texts, first_seq=1):
    seq = first_seq
    for k, t in enumerate(texts):
        seg = t if isinstance(t, dict) else {"text": t, "props": {"k": k % 2}}
        d.add_message(msg("AB"[k % 2], seq, {"type": 0, "pos1": _append_pos(texts[:k]), "seg": seg}))
        seq += 1
    return seq


def _append_pos(before):
    return sum(1 if isinstance(t, dict) else len(t) for t in before)


MARKER = {"marker": {"refType": 1}, "props": {"markerId": "m"}}


def edge_documents():
    """[(name, intended leaf count, build(doc builder))]: every document of the chunk-edge batch."""
    def leaves_of(n):
        def build(d):
            _distinct_inserts(d, ["x"] * n)
        return build

    def removed_ends(d):
        seq = _distinct_inserts(d, [chr(ord("a") + k % 26) for k in range(64)])
        d.add_message(msg("A", seq, {"type": 1, "pos1": 0, "pos2": 1}))
        d.add_message(msg("B", seq + 1, {"type": 1, "pos1": 62, "pos2": 63}))

    def all_removed(d):
        seq = _distinct_inserts(d, ["p", "q", "r"])
        d.add_message(msg("A", seq, {"type": 1, "pos1": 0, "pos2": 3}))

    def long_leaf(d):
        _distinct_inserts(d, ["a", "".join(chr(0x100 + i) for i in range(300)), "z"])

    def markers_at_ends(d):
        _distinct_inserts(d, [MARKER, "one", "two", dict(MARKER, props={"markerId": "n"})])

    def odd_units(d):
        _distinct_inserts(d, ["a\ud800b", "\udfff", "c\uffffd", "e\u0000f", "\u0000"])

    return [("empty", 0, lambda d: None), ("one", 1, leaves_of(1)), ("63", 63, leaves_of(63)), ("64", 64, leaves_of(64)),
            ("65", 65, leaves_of(65)), ("removed_ends", 64, removed_ends), ("all_removed", 3, all_removed),
            ("long_leaf", 3, long_leaf), ("markers", 4, markers_at_ends), ("odd_units", 5, odd_units)]


def edge_batch():
    b = MergeTreeStreamBuilder()
    docs = edge_documents()
    for name, n, build in docs:
        build(b.begin_doc("", observer="observer"))
    return b.finish(), docs


def summary_header(texts):
    """A legacy summary header holding one segment per entry: a text, or {"text", "props"}."""
    import json

    n = sum(len(t["text"] if isinstance(t, dict) else t) for t in texts)
    return json.dumps({
        "chunkStartSegmentIndex": 0, "chunkSegmentCount": len(texts), "chunkLengthChars": n, "totalLengthChars": n,
        "totalSegmentCount": len(texts), "chunkSequenceNumber": 0, "segmentTexts": list(texts),
        "headerMetadata": {"orderedChunkMetadata": [{"id": "header"}], "sequenceNumber": 0, "totalLength": n,
                           "totalSegmentCount": len(texts)}})

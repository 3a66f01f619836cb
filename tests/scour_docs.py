"""Directed documents for zamboni's leaf-block scour (csrc/mt_engine.h scourLeafBlock: two ballots decide
whether a block needs the serial pass at all), shared by the CPU and GPU halves of test_scour_fastpath.py.

Every document is built leaf by leaf. A leaf spec is (kind, text[, props]):
  old     inserted at or below the final minSeq (can be appended onto, can append)
  new     inserted above it
  marker  a Marker inserted at or below it (never appends, nothing appends onto it)
  dead    an old leaf removed at or below it (dropped by the scour)
  tomb    an old leaf removed above it (a tombstone the scour keeps)
  held    (local documents) an old leaf the local client annotated and never had acknowledged
Messages, all with minimumSequenceNumber 0 until the tail: the leaves that are not `new` appended one by
one in document order (so their indices are their positions in the spec); the removes of the `dead`
leaves; then `slots` empty messages; the `new` leaves, each inserted in front of its successor; the
removes of the `tomb` leaves and the local annotates. The tail is `slots` empty messages whose
minimumSequenceNumber goes up one by one from the last `dead` remove: each runs zamboni once (two heap
pops), with every old stamp at or below minSeq and every new one above it.
"""
from fluidframework_amd.streams import MergeTreeStreamBuilder


def _seg(kind, text, props):
    if kind == "marker":
        return {"marker": {"refType": 1}, **({"props": props} if props else {})}
    return {"text": text, "props": props} if props else text


def add_doc(b, specs, slots=None, local=False, obliterate=None, adjust=None):
    """obliterate: (first, last) spec indices of old leaves obliterated above the final minSeq (they
    become tombstones kept by the scour); adjust: (index, key, delta) annotate-adjust of an old leaf."""
    specs = [(s + (None,))[:3] for s in specs]
    slots = slots if slots is not None else len(specs) // 2 + 8
    d = b.begin_doc("", observer="A")
    seq = 0

    def send(op, msn=0):
        nonlocal seq
        seq += 1
        d.add_message({"clientId": "B", "sequenceNumber": seq, "referenceSequenceNumber": seq - 1,
                       "minimumSequenceNumber": msn, "type": "op", "contents": op})

    present = [False] * len(specs)  # inserted and not removed: what a position counts
    ln = [1 if k == "marker" else len(t) for k, t, _ in specs]

    def pos(i):
        return sum(ln[j] for j in range(i) if present[j])

    for i, (k, t, p) in enumerate(specs):
        if k != "new":
            send({"type": 0, "pos1": pos(i), "seg": _seg(k, t, p)})
            present[i] = True
    for i, (k, t, p) in enumerate(specs):
        if k == "dead":
            send({"type": 1, "pos1": pos(i), "pos2": pos(i) + ln[i]})
            present[i] = False
    floor = seq
    for _ in range(slots):
        send({"type": 3, "ops": []})
    for i, (k, t, p) in enumerate(specs):
        if k == "new":
            send({"type": 0, "pos1": pos(i), "seg": _seg(k, t, p)})
            present[i] = True
    for i, (k, t, p) in enumerate(specs):
        if k == "tomb":
            send({"type": 1, "pos1": pos(i), "pos2": pos(i) + ln[i]})
            present[i] = False
    if obliterate is not None:
        a, z = obliterate
        send({"type": 4, "pos1": pos(a), "pos2": pos(z) + ln[z]})
        for i in range(a, z + 1):
            present[i] = False
    if adjust is not None:
        i, key, delta = adjust
        send({"type": 2, "pos1": pos(i), "pos2": pos(i) + ln[i], "adjust": {key: {"delta": delta}}})
    if local:
        for i, (k, t, p) in enumerate(specs):
            if k == "held":
                d.local_op({"type": 2, "pos1": pos(i), "pos2": pos(i) + ln[i], "props": {"held": i}})
    for k in range(slots):
        send({"type": 3, "ops": []}, msn=floor + k)
    return d


def alternating(n, start=0, kind="old"):
    """n one-unit leaves whose props alternate, so that no two neighbours match"""
    return [(kind, "abcdefgh"[(start + k) % 8], {"alt": (start + k) % 2}) for k in range(n)]


def markers(n):
    return [("marker", "")] * n


def straddle(pair_kind, mid):
    """67+ leaves, all markers but four: leaves 62..66 are one block (the leaves appended as 60..63, after
    two `new` leaves put in front of leaf 0 and one in front of the marker at the block's end). Leaves 63
    and 64 are `pair_kind`; 65 is `mid`."""
    body = markers(60) + [("marker", ""), (pair_kind[0], "pq"), (pair_kind[1], "rs"), mid, ("marker", "")] + markers(8)
    return [("new", "x", {"front": 1}), ("new", "y", {"front": 2})] + body


def plain_cases():
    """name -> (specs, oracle's final leaf count relative to the spec: leaves that go away)"""
    sep = lambda mid: alternating(9) + [("old", "ab"), mid, ("old", "cd")] + alternating(9, 1)  # noqa: E731
    return {
        # every leaf of most blocks above minSeq; the four old ones in front merge, their block shrinks and
        # packParent scours the siblings, none of which can change
        "all_above_min_seq": ([("old", "a"), ("old", "b"), ("old", "c"), ("old", "d")] + alternating(28, kind="new"), 3),
        "drops_only": (alternating(6) + [("dead", "D"), ("dead", "E")] + alternating(6, 1) + [("dead", "F")] + alternating(5), 5),  # (and the neighbours of each dropped run merge once it is gone)
        "drops_between_new": (alternating(4, kind="new") + [("dead", "D")] + alternating(7, kind="new") + [("dead", "E")], 2),
        "apart_by_marker": (sep(("marker", "")), 0),
        "apart_by_tombstone": (sep(("tomb", "T")), 0),
        "apart_by_new": (sep(("new", "N")), 0),
        "empty_insert_between": (sep(("old", "")), 2),  # (an empty insert creates no leaf: "ab" and "cd" are neighbours)
        "apart_by_dropped": (sep(("dead", "X")), 2),  # (the dropped leaf goes, and then its neighbours merge)
        "straddle_pair_63_64": (straddle(("old", "old"), ("new", "n", {"mid": 1})), 1),
        "straddle_no_pair": (straddle(("old", "new"), ("new", "n", {"mid": 1})), 0),
        "straddle_drop_64": (straddle(("new", "dead"), ("new", "n", {"mid": 1})), 1),
        # the first block loses three of its four leaves; its siblings hold alternating old leaves (no-ops)
        # and the parent is redistributed
        "noop_siblings_then_pack": ([("dead", "a"), ("dead", "b"), ("dead", "c"), ("old", "d", {"k": 9})] + alternating(27), 3),
        "noop_siblings_two_levels": ([("dead", "a"), ("dead", "b"), ("dead", "c")] + alternating(70), 3),
    }


def plain_batch():
    b = MergeTreeStreamBuilder()
    cases = plain_cases()
    for specs, _ in cases.values():
        add_doc(b, specs)
    return b.finish(), list(cases)


def obliterate_batch():
    """An obliterate above minSeq over old leaves (tombstones the scours keep: runs of no-op scours), and a
    mergeable pair right behind them."""
    b = MergeTreeStreamBuilder()
    specs = alternating(14) + [("old", "ab"), ("old", "cd")] + alternating(14, 1)
    add_doc(b, specs, obliterate=(3, 9))
    add_doc(b, alternating(20, kind="new") + [("old", "ab"), ("old", "cd")] + alternating(6), obliterate=(22, 24))
    return b.finish()


def adjust_batch():
    b = MergeTreeStreamBuilder()
    num = lambda k: ("old", "abcdefgh"[k % 8], {"n": k})  # noqa: E731
    specs = [num(k) for k in range(14)] + [("old", "ab", {"n": 50}), ("old", "cd", {"n": 50})] + [num(k) for k in range(14, 26)]
    add_doc(b, specs, adjust=(5, "n", 1))
    add_doc(b, specs, adjust=(14, "n", 1))  # the pair's head adjusted above minSeq
    return b.finish()


def local_batch():
    """Two old leaves with one set of props and a held leaf (a pending local annotate) between them"""
    b = MergeTreeStreamBuilder()
    add_doc(b, alternating(9) + [("old", "ab"), ("held", "H"), ("old", "cd")] + alternating(9, 1), local=True)
    add_doc(b, alternating(9) + [("old", "ab"), ("old", "H"), ("old", "cd")] + alternating(9, 1), local=True)  # nothing held: merges
    add_doc(b, alternating(3) + [("held", "G"), ("dead", "D"), ("held", "H")] + alternating(9, 1), local=True)
    return b.finish()

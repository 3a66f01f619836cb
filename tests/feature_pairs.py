"""Streams and checks for merge-tree feature PAIRS (shared by test_feature_pairs_emulated.py and
test_gpu_feature_pairs.py): annotate-adjust x remove order, annotate-adjust x obliterate, obliterate x
remove order past the small tier, catch-up x remove order and catch-up x annotate-adjust.

Every pair selects separately compiled instantiations of the engine (Doc<Ob, tier, Rm, Adj>,
hugeDocKernel<Adj, Rm>, the large -> huge checkpoint); the builders rewrite the pinned fixtures and
generators of the single-feature tests, so the oracle's own replay of the same batch is the reference.
"""
import random
from dataclasses import replace

import numpy as np

from fluidframework_amd import summary
from fluidframework_amd.streams import (MT_F_CATCHUP, MT_INSERT, MT_OBLITERATE, MT_REMOVE, VALUE_COMPUTED,
                                        MergeTreeStreamBuilder, flag_catchup, flag_remove_order)
from mt_compare import compare_doc, resolve_props, visible_text

ADJUSTED_KEYS = ("n", "w", "weight")  # the keys the builders' adjust ops name
CAP_CU = 1 << 15  # catch-up ranges / remove-order entries of room per document, every route
CAP_RM = 1 << 16


# ------------------------------------------------------------------------------------------ streams
def adjust_rm_batch(narrow):
    """The annotate-adjust conflict farms (test_annotate_adjust.adjust_fixture_batch) flagged for
    remove-order recording: (batch, final texts). narrow: the documents stay in the small tier; else
    most escalate to the large tier through the 32-prop-set limit. The farms hold overlapping removes,
    so stamp lists with more than one remover exist."""
    from test_annotate_adjust import adjust_fixture_batch

    batch, finals = adjust_fixture_batch(narrow=narrow)
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch, finals


def _ob_messages(rnd, init_len, n_ops, annotate_share, rewrite, hot=None, remove_share=0.05):
    """test_huge_checkpoint._ob_growth's stream shape (inserts of 3..12 units, obliterates of 1..6,
    writers w0..w4, minSeq trailing by 40) with annotates of 2..9 units mixed in at annotate_share and
    plain removes at remove_share (5 %), in rounds of three writers who all reference the round's start: their ops
    are concurrent, so obliterates meet concurrent inserts, removes and annotates. Positions stay below
    a lower bound of the visible length (a round's inserts count only when it holds no obliterate,
    which could swallow them). hot: annotates, removes and obliterates start in the first `hot` units,
    so they overlap in a long document too."""
    init = "".join(rnd.choice("abcdefgh") for _ in range(init_len))
    msgs, bound, seq = [], init_len, 0
    while seq < n_ops:
        ref, added, removed, obl = seq, 0, 0, False
        span = min(bound, hot) if hot else bound
        for c in rnd.sample(range(5), 3):
            r = rnd.random()
            if r < annotate_share and bound > 20:
                a = rnd.randrange(span - 10)
                op = rewrite({"type": 2, "pos1": a, "pos2": a + rnd.randint(2, 9), "props": {"client": f"w{c}"}})
            elif r < annotate_share + remove_share and bound > 200:
                a = rnd.randrange(span - 10)
                op = {"type": MT_REMOVE, "pos1": a, "pos2": a + rnd.randint(1, 6)}
                removed += op["pos2"] - op["pos1"]
            elif r < annotate_share + remove_share + 0.2 and bound > 200:
                a = rnd.randrange(span - 10)
                op = {"type": MT_OBLITERATE, "pos1": a, "pos2": a + rnd.randint(1, 6)}
                removed += op["pos2"] - op["pos1"]
                obl = True
            else:
                s = "".join(rnd.choice("XYZ") for _ in range(rnd.randint(3, 12)))
                op = {"type": MT_INSERT, "pos1": rnd.randrange(bound + 1), "seg": s}
                added += len(s)
            seq += 1
            msgs.append({"clientId": f"w{c}", "sequenceNumber": seq, "referenceSequenceNumber": ref,
                         "minimumSequenceNumber": max(0, ref - 40), "type": "op", "contents": op})
        bound += (0 if obl else added) - removed
    return init, msgs


def adjust_ob_batch(long, n_docs=12, n_ops=300):
    """Annotate-adjust x real obliterate ops: (batch, None). The 2.3.0 obliterate fixtures exist only
    as packed ops (tests/golden/replay_obliterate_2.3.0.npz holds no messages), so this takes the
    issue's second route: _ob_growth-style message streams (_ob_messages) whose annotates (15 % of
    ops) go through the rewrite adjust_fixture_batch applies (test_annotate_adjust.annotate_rewriter,
    its narrow form unless long). long: 6000 more units of initial text, as long_obliterate_farms
    appends, so every document outgrows the small tier's 6144 units while obliterates are live."""
    from test_annotate_adjust import annotate_rewriter

    b = MergeTreeStreamBuilder(keep_messages=True)
    for d in range(n_docs):
        rnd = random.Random(7001 + d)
        init, msgs = _ob_messages(rnd, 400 + (6000 if long else 0), n_ops, 0.15, annotate_rewriter(rnd, narrow=not long))
        doc = b.begin_doc(init, observer="observer")
        for m in msgs:
            doc.add_message(m)
    return b.finish(), None


def ob_rm_long_batch():
    """long_obliterate_farms(6000) flagged for remove order: the large tier's Ob x Rm variant from op 0
    (remove-order batches take no small -> large checkpoint)."""
    from test_obliterate import long_obliterate_farms

    batch = long_obliterate_farms(extra=6000)
    batch = replace(batch, ops=batch.ops.copy(), clients=[[f"client-{i}" for i in range(64)]] * batch.n_docs)
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch, None


ADJUST_RM_TAIL = 2086  # adjust_rm_growth: the original op its overlapping removes follow


def adjust_rm_growth(catchup=False):
    """marker_batch(1, 2099, seed=5, adjust=True)'s document flagged for remove order. That stream
    holds no remove (its relative positions must find their markers), so after its op 2086 — before
    the large tier's prop sets run out (it stops before op index 2102 of this stream's 2104) — it inserts
    six units at the front, adjusts "weight" on them, and three writers remove overlapping parts of them
    from the same view; the visible text is then what it was, so the later positions stand. From
    there on minSeq stays below the inserted ops: the removes recorded by the large tier are still above
    the final minSeq when the huge tier finishes. catchup: every op flagged for catch-up instead of the
    remove-order flags (catch-up x annotate-adjust across the checkpoint)."""
    from marker_docs import doc_messages

    init, msgs = doc_messages(0, 2099, 5, adjust=True)
    out, seqmap, tail_msn = [], {0: 0}, None

    def push(m):
        out.append(dict(m, sequenceNumber=len(out) + 1))

    for m in msgs:
        msn = seqmap[m["minimumSequenceNumber"]]
        if tail_msn is not None:  # the collab window lags behind the inserted ops
            msn = min(msn, tail_msn)
        push(dict(m, referenceSequenceNumber=seqmap[m["referenceSequenceNumber"]], minimumSequenceNumber=msn))
        if m["sequenceNumber"] == ADJUST_RM_TAIL:
            s, tail_msn = len(out), msn

            def mk(c, ref, op):
                return {"clientId": c, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn, "contents": op}

            push(mk("A", s, {"type": 0, "pos1": 0, "seg": "qrstuv"}))
            push(mk("B", s + 1, {"type": 2, "pos1": 0, "pos2": 6, "adjust": {"weight": {"delta": 2}}}))
            push(mk("A", s + 2, {"type": 1, "pos1": 0, "pos2": 4}))
            push(mk("wd", s + 2, {"type": 1, "pos1": 2, "pos2": 6}))
            push(mk("we", s + 2, {"type": 1, "pos1": 1, "pos2": 5}))
        seqmap[m["sequenceNumber"]] = len(out)
    b = MergeTreeStreamBuilder(keep_messages=True)
    doc = b.begin_doc(init, observer="observer")
    for m in out:
        doc.add_message(m)
    batch = b.finish()
    if catchup:
        batch.ops["flags"] |= MT_F_CATCHUP
    else:
        flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch


def _ob_growth_batch(seed, annotate_share, dup_share, n_msgs):
    """test_huge_checkpoint._ob_growth's document (128,000 units, writers w0..w4 one after another, 20 %
    obliterates of 1..6 units, inserts of 3..12, minSeq trailing by 40), n_msgs messages long: the callers
    end it 17 messages after the large tier's stop (its text limit), so what the large tier recorded just
    before its checkpoint is still above the final minSeq. annotate_share: annotates in the first 600 units, where
    half of the obliterates fall too, rewritten into adjusts (annotate_rewriter). dup_share: after an
    obliterate, writer "wd" removes the same range from the same view (as _rm_growth duplicates
    removes): leaves with a sliceRemove and a setRemove stamp."""
    from test_annotate_adjust import annotate_rewriter

    rnd = random.Random(seed)
    init = "".join(rnd.choice("abcdefgh") for _ in range(128000))
    rewrite = annotate_rewriter(random.Random(seed + 1))
    b = MergeTreeStreamBuilder(keep_messages=True)
    d = b.begin_doc(init, observer="observer")
    length, seq = len(init), 0

    def send(c, ref, op):
        nonlocal seq
        seq += 1
        d.add_message({"clientId": c, "sequenceNumber": seq, "referenceSequenceNumber": ref,
                       "minimumSequenceNumber": max(0, seq - 40), "type": "op", "contents": op})

    while seq < n_msgs:
        c, r = f"w{rnd.randrange(5)}", rnd.random()
        if r < annotate_share:
            a = rnd.randrange(600)
            send(c, seq, rewrite({"type": 2, "pos1": a, "pos2": a + rnd.randint(2, 9), "props": {"client": c}}))
        elif r < annotate_share + 0.2:
            a = rnd.randrange(600 if annotate_share and r < annotate_share + 0.1 else length - 10)
            op = {"type": MT_OBLITERATE, "pos1": a, "pos2": a + rnd.randint(1, 6)}
            length -= op["pos2"] - op["pos1"]
            send(c, seq, op)
            if rnd.random() < dup_share:
                send("wd", seq - 1, dict(op, type=MT_REMOVE))
        else:
            t = "".join(rnd.choice("XYZ") for _ in range(rnd.randint(3, 12)))
            send(c, seq, {"type": MT_INSERT, "pos1": rnd.randrange(length + 1), "seg": t})
            length += len(t)
    return b.finish()


def ob_rm_growth():
    """Obliterate x remove order across the checkpoint: _ob_growth's document with half of its
    obliterates followed by a concurrent remove of the same range, flagged for remove order (the large
    tier stops before op index 597 of 614)."""
    batch = _ob_growth_batch(21, 0.0, 0.5, 614)
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch


def ob_adjust_growth():
    """Obliterate x annotate-adjust across the checkpoint: _ob_growth's document with annotate-adjust
    ops at about 10 % of ops; the checkpoint carries live obliterates and PropertiesManager records (the
    large tier stops before op index 628 of 645)."""
    return _ob_growth_batch(23, 0.1, 0.0, 645)


def catchup_pair_batches(only=None):
    """{"adjust": (batch, finals), "rm": (batch, finals), "adjust_growth": batch, "rm_growth": batch}
    (only: that entry alone): catch-up x annotate-adjust — the narrow adjust farms with
    FMT_MT_F_CATCHUP set by window (as test_catchup.fixture_batch) and no remove order; catch-up x remove
    order — the plain 0.40 fixture batch with both; and one growth document of each kind for the
    checkpoint, every op flagged for catch-up (as test_emulated_checkpoint_carries_catchup_ranges flags
    its document)."""
    def adjust():
        from test_annotate_adjust import adjust_fixture_batch

        batch, finals = adjust_fixture_batch(narrow=True)
        flag_catchup(batch.ops, batch.doc_op_offsets)
        return batch, finals

    def rm():
        from test_catchup import fixture_batch

        batch, finals = fixture_batch()
        flag_remove_order(batch.ops, batch.doc_op_offsets)
        return batch, finals

    def rm_growth():
        from test_huge_checkpoint import _rm_growth

        batch = _rm_growth()
        batch.ops["flags"] |= MT_F_CATCHUP
        batch.clients = [["observer"] + [f"client-{i}" for i in range(1, 64)]]
        return batch

    build = {"adjust": adjust, "rm": rm, "adjust_growth": lambda: adjust_rm_growth(catchup=True), "rm_growth": rm_growth}
    return {k: f() for k, f in build.items() if only in (None, k)}


def load_time_huge(kind):
    """One document that is over the large tier when the batch is loaded: it starts from a legacy
    summary (begin_doc_from_summary: one header chunk of 200 segments, 131,600 units), so the runtime
    sets it up for the huge tier at load (mtHugeLoaded) and hugeDocKernel<Adj, true> replays its 300
    messages from the first, beside the small tier's launch. Flagged for remove order. kind "adjust_rm" —
    _ob_messages with 25 % annotates (rewritten into adjusts) and its obliterates turned into removes;
    "ob_rm" — _ob_messages without annotates, with as many removes as obliterates. Both with the ranged ops in the first 16 units,
    so their ranges overlap."""
    import json

    from test_annotate_adjust import annotate_rewriter

    rnd = random.Random(911 if kind == "adjust_rm" else 912)
    n_segs, seg_len = 200, 658
    if kind == "adjust_rm":
        init, msgs = _ob_messages(rnd, n_segs * seg_len, 300, 0.25, annotate_rewriter(rnd), hot=16)
        for m in msgs:  # (no obliterates in this one: they become removes)
            if m["contents"]["type"] == MT_OBLITERATE:
                m["contents"]["type"] = MT_REMOVE
    else:
        init, msgs = _ob_messages(rnd, n_segs * seg_len, 300, 0.0, lambda op: op, hot=16, remove_share=0.2)
    texts = [init[k * seg_len: (k + 1) * seg_len] for k in range(n_segs)]
    header = json.dumps({
        "chunkStartSegmentIndex": 0, "chunkSegmentCount": n_segs, "chunkLengthChars": len(init),
        "totalLengthChars": len(init), "totalSegmentCount": n_segs, "chunkSequenceNumber": 0, "segmentTexts": texts,
        "headerMetadata": {"orderedChunkMetadata": [{"id": "header"}], "sequenceNumber": 0, "totalLength": len(init),
                           "totalSegmentCount": n_segs}})
    b = MergeTreeStreamBuilder(keep_messages=True)
    doc = b.begin_doc_from_summary(header, observer="observer")
    for m in msgs:
        doc.add_message(m)
    batch = b.finish()
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch


# ------------------------------------------------------------------------------------------- oracle
class Oracle:
    """The oracle's replay of a batch, once: headers, leaves, chars, props (rows per document), the
    computed numbers of annotate-adjust batches and the catch-up ranges when cap_catchup > 0."""

    def __init__(self, orc, batch, caps, cap_catchup=0, index=False):
        self.orc, self.batch = orc, batch
        self.numbers = [] if batch.adjusts is not None else None
        orc.set_index(index)
        try:
            r = orc.mt_replay_batch(batch, threads=8, cap_leaves=caps[0], cap_chars=caps[1], cap_props=caps[2],
                                    cap_catchup=cap_catchup, numbers=self.numbers)
        finally:
            orc.set_index(False)
        assert r[0] == 0, r[0]
        self.h, self.lv, self.ch, self.pr = r[1:5]
        self.cu = r[6] if cap_catchup else None
        self._removers = {}

    def doc(self, d):
        h = self.h[d]
        return h, self.lv[d][: int(h["n_leaves"])], self.ch[d][: int(h["n_chars"])], self.pr[d][: int(h["n_props"])]

    def removers(self, d):
        if d not in self._removers:
            self._removers[d] = self.orc.mt_removers(self.batch, d)
        return self._removers[d]

    def names(self, d):
        return self.batch.clients[d]

    def leaf_adjusted(self, d, i):
        """Leaf i of document d holds the result of an adjust: one of ADJUSTED_KEYS with a computed
        number (value ids from FMT_MT_VALUE_COMPUTED on; a raw set of the key has a host value id)."""
        h, lv, _, pr = self.doc(d)
        kv = resolve_props(int(lv[i]["props"]), pr) or ()
        return any(self.batch.keys[x >> 16] in ADJUSTED_KEYS and (x & 0xFFFF) >= VALUE_COMPUTED for x in kv)


LARGE_CAPS = (4096, 1 << 18, 4096)  # oracle output room for documents up to the large tier
HUGE_CAPS = (1 << 16, 1 << 19, 1 << 15)


def live_adjust_rm(o):
    """(computed numbers in the batch, leaves removed above minSeq that carry an adjusted key and more
    than one remover) on the oracle's result."""
    multi = 0
    for d in range(o.batch.n_docs):
        ms = int(o.h[d]["min_seq"])
        for i, stamps in o.removers(d).items():
            if len(stamps) > 1 and stamps[0][1] > ms and o.leaf_adjusted(d, i):
                multi += 1
    return sum(len(x) for x in o.numbers), multi


def live_adjust_ob(o):
    """(computed numbers, leaves with an obliterate stamp that carry an adjusted key)."""
    hit = 0
    for d in range(o.batch.n_docs):
        for i, stamps in o.removers(d).items():
            if any(k == 1 for _, _, k in stamps) and o.leaf_adjusted(d, i):
                hit += 1
    return sum(len(x) for x in o.numbers), hit


def live_both_stamps(o):
    """Leaves removed above minSeq whose stamp list holds a setRemove and a sliceRemove (obliterate) stamp."""
    return sum(1 for d in range(o.batch.n_docs) for st in o.removers(d).values()
               if {k for _, _, k in st} == {0, 1} and st[0][1] > int(o.h[d]["min_seq"]))


def assert_catchup_live(o, kind):
    """A catch-up pair batch (catchup_pair_batches "adjust" / "rm"): catch-up ranges in at least a third
    of the documents, beside computed numbers / beside stamp lists with more than one remover."""
    assert int((o.h["n_catchup"] > 0).sum()) * 3 >= o.batch.n_docs
    if kind == "adjust":
        assert sum(len(x) for x in o.numbers) > 0
    else:
        assert sum(len(s) > 1 for d in range(o.batch.n_docs) for s in o.removers(d).values()) > 0


def assert_growth_live(o, kind):
    """A growth document (feature_pairs' *_growth builders) holds its pair, on the oracle's result."""
    if kind == "adjust_rm":
        nums, multi = live_adjust_rm(o)
        assert nums > 0 and multi > 0, (nums, multi)
    elif kind == "ob_adjust":
        nums, hit = live_adjust_ob(o)
        assert nums > 0 and hit > 0, (nums, hit)
    elif kind == "ob_rm":
        assert live_both_stamps(o) > 0
    else:
        assert int(o.h[0]["n_catchup"]) > 0
        if kind == "catchup_adjust":
            assert len(o.numbers[0]) > 0


def assert_carried(o, kind, at):
    """The large tier, which stopped before op `at`, recorded something the final result needs: a
    later remove stamp of a leaf still above minSeq (remove-order kinds), an adjust above minSeq
    (adjust kinds), a catch-up range (catch-up kinds: every op is flagged)."""
    ops = o.batch.ops
    ms, stop = int(o.h[0]["min_seq"]), int(ops["seq"][at])
    assert 0 < at < len(ops) and ms < stop
    if kind in ("adjust_rm", "ob_rm", "catchup_rm"):
        assert any(len(st) > 1 and st[0][1] > ms and st[1][1] < stop for st in o.removers(0).values())
    if kind in ("adjust_rm", "ob_adjust", "catchup_adjust"):
        adj = o.batch.adjusts is not None and ((ops["type"][:at] == 2) & (ops["seq"][:at] > ms)).any()
        assert adj


# ------------------------------------------------------------------------------------------- checks
def check_doc(o, d, got, *, nums=None, legacy=None, engine_summary=None, rm=None, cu=None, final=None):
    """Document d of the engine (got = header, leaves, chars, props) against the oracle o: status,
    header fields, every leaf field, text and prop sets; then, as given,
      nums / legacy   annotate-adjust: computed numbers, and the legacy summary read through the
                      engine's getAtSeq prop sets == orc.mt_replay_summary (engine_summary: the bulk
                      summarizer's blobs, the same);
      rm              remove-order entries: the stamp list of every leaf removed above minSeq ==
                      orc.mt_removers, and the SnapshotV1 summary built from each side byte-equal;
      cu              catch-up ranges == the oracle's, up to n_catchup;
      final           the fixture's resultText."""
    batch = o.batch
    h, lv, ch, pr = got
    exp = o.doc(d)
    assert int(h["status"]) == int(exp[0]["status"]) == 0, (d, int(h["status"]), int(exp[0]["status"]))
    diffs = compare_doc(exp, (h, lv, ch, pr))
    assert not diffs, f"doc {d}: {diffs[:5]}"
    if final is not None:
        assert visible_text(h, lv, ch) == final, d
    if o.numbers is not None:
        assert nums is not None and np.array_equal(nums, o.numbers[d]), (d, nums, o.numbers[d])
        want = o.orc.mt_replay_summary(batch, d, batch.keys, batch.values)
        vals = summary.values_with_numbers(batch.values, nums)
        assert summary.legacy_summary(h, lv, ch, pr, batch.keys, vals, legacy_props=legacy) == want, d
        if engine_summary is not None:
            assert engine_summary == want, d
    if rm is not None:
        a, b = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
        n = int(h["n_leaves"])
        assert int(h["n_rm_order"]) == len(rm)
        mine = summary.removers_from_engine(lv, n, rm, batch.ops[a:b])
        want = o.removers(d)
        ms = int(h["min_seq"])
        for i in range(n):
            r = int(lv[i]["rm_seq"])
            if r != summary.NOT_REMOVED and r > ms:
                assert mine.get(i) == want.get(i), (d, i, mine.get(i), want.get(i))
        vals = batch.values if o.numbers is None else summary.values_with_numbers(batch.values, nums)
        v_en = summary.v1_summary(h, lv, ch, pr, batch.keys, vals, o.names(d), mine)
        v_or = summary.v1_summary(*exp, batch.keys, vals, o.names(d), want)
        assert v_en == v_or, d
    if cu is not None:
        n = int(exp[0]["n_catchup"])
        assert int(h["n_catchup"]) == n and np.array_equal(cu[:n], o.cu[d][:n]), d

"""Directed documents for the bulk summary path (summaryRunsKernel, summaryV1Kernel and the C++ JSON
writers), their census and their references (used by test_summary_edges.py and
test_gpu_summary_edges.py).

Every document is loaded from a hand-written summary header (each spec becomes one leaf) and followed
by at most a few messages. The messages keep minimumSequenceNumber at the header's until the last
one raises it: zamboni then runs once, scours the two blocks with the oldest stamps (the first two
messages of such a document are there to be scoured, in its first and last block) and leaves the rest
of the layout alone. What a builder intends is still not what the kernel sees, so every family names
the decisions it exists for (PROMISES) and `census` finds them in a FINAL state (the oracle's, or the
engine's): test_summary_edges.py fails when a family no longer reaches its decisions.

`census` is plain Python written from the rule text: a leaf is in the legacy summary iff it is
present at PriorPerspective(minSeq, NonCollabClient); it is appended onto the open run while
prev.canAppend(seg) && matchProperties (textSegment.ts:76-83: both TextSegments, the run not ending
in '\\n', the run or the leaf at most TextSegmentGranularity = 256 long; properties.ts:32-61:
undefined ≡ {}). The only constants it shares with the kernels are 256 and the 64-leaf chunk.

Expected bytes never come from the code under test: oracle.mt_replay_summary (an independent C++
replay and summary) and summary.legacy_summary / summary.v1_summary over a state must agree.
"""
import functools
import json
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from fluidframework_amd import summary
from fluidframework_amd.native import propset_entries
from fluidframework_amd.streams import MT_LEAF_MARKER, MergeTreeStreamBuilder

GRANULARITY = 256  # TextSegmentGranularity (textSegment.ts:21)
WAVE = 64          # leaves per chunk of the kernels' scan
S = 10             # sequenceNumber (= minSeq) of every loaded header

TIERS = ["asis", "large", "huge"]
LARGE_PREFIX = 6200    # units: past the small tier's text, within the large tier's
HUGE_PREFIX = 140000   # units: past the large tier's 131071 (tests/test_long_inserts.py)


# ------------------------------------------------------------------------------------------ census
def _same_props(a, b):
    """matchProperties (properties.ts:32-61) on (key << 16 | value) entries; None ≡ ()."""
    return sorted(a or ()) == sorted(b or ())


def census(hdr, leaves, chars, props, min_seq, legacy_props=None):
    """(Counter of decisions and facts, run lengths) of one final state under the legacy rule.

    For every adjacent pair of present leaves the first clause that decides it, in the order the rule
    reads: marker_prev, marker_next, newline, granularity_stop, class_mismatch, append. An append also
    counts its sub-reasons as "append:<reason>". Facts about single leaves and 64-leaf chunks are
    counted under their own names (see PROMISES). The run lengths are the summary's segment lengths.
    """
    c = Counter()
    n = int(hdr["n_leaves"])
    run = None  # [units, last unit, marker, props entries, props id, leaves in it]
    runs = []
    prev_i = None
    chunk_units = Counter()
    chunk_present = Counter()
    first_present = last_present = None
    for i in range(n):
        L = leaves[i]
        ins, rm, ln = int(L["ins_seq"]), int(L["rm_seq"]), int(L["len"])
        c["ins_eq_min"] += ins == min_seq
        c["ins_eq_min_plus_1"] += ins == min_seq + 1
        c["rm_eq_min"] += rm == min_seq
        c["rm_eq_min_plus_1"] += rm == min_seq + 1
        c["v1_skipped"] += rm <= min_seq
        c["v1_solo"] += rm > min_seq and (ins > min_seq or rm != summary.NOT_REMOVED)
        if ins > min_seq or rm <= min_seq:
            continue
        o = int(L["char_off"])
        units = chars[o : o + ln]
        marker = (int(L["pad"]) & MT_LEAF_MARKER) != 0
        pid = int(L["props"]) if legacy_props is None else int(legacy_props[i])
        ent = None if pid == 0xFFFF else propset_entries(props, pid)
        last = int(units[-1]) if ln else 0
        chunk_units[i // WAVE] += ln
        chunk_present[i // WAVE] += 1
        if first_present is None:
            first_present = marker
        last_present = marker
        c["leaf_gt_64"] += ln > WAVE
        c["leaf_gt_4096"] += ln > WAVE * WAVE
        c["marker_with_props"] += marker and bool(ent)
        c["marker_without_props"] += marker and not ent
        c["wide_set"] += ent is not None and len(ent) > 8
        if run is None:
            why = None
        elif run[2]:
            why = "marker_prev"
            c["marker_marker"] += marker
        elif marker:
            why = "marker_next"
        elif run[1] == 10:
            why = "newline"
            c["newline:after_append"] += run[5] > 1
            c["newline:leaf_is_only_newline"] += run[0] == 1
        elif run[0] > GRANULARITY and ln > GRANULARITY:
            why = "granularity_stop"
            c["granularity_stop:grown_run"] += run[5] > 1
        elif not _same_props(run[3], ent):
            why = "class_mismatch"
            c["class_mismatch:wide"] += bool(run[3]) and bool(ent) and len(run[3]) > 8 and len(ent) > 8
        else:
            why = "append"
            c["append:run_gt_256_leaf_le_256"] += run[0] > GRANULARITY
            c["append:run_le_256_leaf_gt_256"] += ln > GRANULARITY
            c["append:same_class_different_id"] += bool(ent) and run[4] != pid
            c["append:same_class_different_id_wide"] += bool(ent) and run[4] != pid and len(ent) > 8
            c["append:empty_vs_undefined"] += not ent and run[4] != pid
            c["append:across_64_boundary"] += prev_i // WAVE != i // WAVE
            c["append:across_127_128"] += prev_i // WAVE == 1 and i // WAVE == 2
            c["append:across_skipped_chunk"] += i // WAVE - prev_i // WAVE >= 2
            c["append:gains_newline"] += last == 10
            c["append:newline_inside"] += run[6]  # a '\n' that is not the run's last unit stops nothing
            c["append:run_last_0x010a"] += run[1] == 0x010A
            c["append:run_last_0x0a00"] += run[1] == 0x0A00
            c["append:joins_surrogate_pair"] += 0xD800 <= run[1] <= 0xDBFF and ln > 0 and 0xDC00 <= int(units[0]) <= 0xDFFF
        if why is not None:
            c[why] += 1
            if why != "append":
                c["split_surrogate_pair"] += 0xD800 <= run[1] <= 0xDBFF and ln > 0 and 0xDC00 <= int(units[0]) <= 0xDFFF
                c["run_ends_lone_high"] += 0xD800 <= run[1] <= 0xDBFF and not (ln > 0 and 0xDC00 <= int(units[0]) <= 0xDFFF)
                c["run_starts_lone_low"] += (ln > 0 and 0xDC00 <= int(units[0]) <= 0xDFFF) and not 0xD800 <= run[1] <= 0xDBFF
        if why == "append":
            run[0] += ln
            run[1] = last
            run[5] += 1
            run[6] = run[6] or 10 in units.tolist()[:-1]
        else:
            if run is not None:
                runs.append(run[0])
            run = [ln, last, marker, ent, pid, 1, 10 in units.tolist()[:-1]]
        prev_i = i
    if run is not None:
        runs.append(run[0])
    c["leaves"] = n
    c["present"] = sum(chunk_present.values())
    c["leaves_ge_130"] += n >= 130
    c["no_leaves"] += n == 0
    c["nothing_present"] += n > 0 and not runs
    c["marker_first"] += bool(first_present)
    c["marker_last"] += bool(last_present)
    c["single_255"] += runs == [255] and c["present"] == 1
    c["single_256"] += runs == [256] and c["present"] == 1
    c["single_257"] += runs == [257] and c["present"] == 1
    c["chunk_units_not_multiple_of_64"] += sum(u % WAVE != 0 for u in chunk_units.values())
    return +c, runs


# --------------------------------------------------------------------------------------- documents
@dataclass
class Case:
    name: str
    specs: list                 # the header's segment specs (legacy "segmentTexts")
    msgs: list = field(default_factory=list)  # messages; positions are relative to the specs' start
    v1_load: tuple = None       # (header dict, [body dicts]) of a SnapshotV1 load in place of `specs`


def T(n, ch="t"):
    """n units of text that ends in no newline: ch repeated with a counter mixed in."""
    s = "".join(chr(ord("a") + (k * 7 + n) % 26) for k in range(n))
    return (ch + s)[:n]


def M(ref_type=1, props=None):
    m = {"marker": {"refType": ref_type}}
    if props is not None:
        m["props"] = props
    return m


def P(text, **props):
    return {"text": text, "props": props}


def msg(client, seq, msn, op, ref=None):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": seq - 1 if ref is None else ref,
            "minimumSequenceNumber": msn, "type": "op", "contents": op}


def ins(pos, seg):
    return {"type": 0, "pos1": pos, "seg": seg}


def rem(a, b):
    return {"type": 1, "pos1": a, "pos2": b}


def ann(a, b, props=None, adjust=None):
    op = {"type": 2, "pos1": a, "pos2": b}
    if props is not None:
        op["props"] = props
    if adjust is not None:
        op["adjust"] = adjust
    return op


def group(*ops):
    return {"type": 3, "ops": list(ops)}


def _len(spec):
    if isinstance(spec, str):
        return len(spec.encode("utf-16-le", "surrogatepass")) // 2
    return 1 if "marker" in spec else _len(spec["text"])


PAD = 12  # padding leaves on either side of a padded document's middle (more than one block each)


def padded(name, mid, ops, final_msn):
    """`mid` between two stretches of PAD one-unit leaves whose props alternate (so that neither the
    summary nor zamboni merges them). Messages: S+1 and S+2 insert into the first and the last
    stretch (the two blocks zamboni scours when the last message raises minSeq), then `ops`
    (client, op) at S+3, S+4, ... with positions relative to `mid`, then an empty message that raises
    minSeq to `final_msn`."""
    front = [P("f", pad=k % 2) for k in range(PAD)]
    back = [P("b", pad=k % 2) for k in range(PAD)]
    n_mid = sum(_len(s) for s in mid)
    msgs = [msg("Z", S + 1, S, ins(1, P("y", pad=7))), msg("Z", S + 2, S, ins(PAD + 1 + n_mid + PAD - 1, P("z", pad=8)))]
    seq = S + 2
    for client, op in ops:
        seq += 1
        op = dict(op)
        for k in ("pos1", "pos2"):
            if k in op:
                op[k] += PAD + 1
        if op["type"] == 3:
            op["ops"] = [{**m, **{k: m[k] + PAD + 1 for k in ("pos1", "pos2") if k in m}} for m in op["ops"]]
        msgs.append(msg(client, seq, S, op))
    msgs.append(msg("Z", seq + 1, final_msn, group()))
    return Case(name, front + mid + back, msgs)


def _shift(op, k):
    if op is None or k == 0:
        return op
    op = dict(op)
    for f in ("pos1", "pos2"):
        if isinstance(op.get(f), int):
            op[f] += k
    if op.get("type") == 3:
        op["ops"] = [_shift(m, k) for m in op["ops"]]
    return op


def legacy_header(specs, seq=S):
    total = sum(_len(s) for s in specs)
    return json.dumps({"chunkStartSegmentIndex": 0, "chunkSegmentCount": len(specs), "chunkLengthChars": total,
                       "totalLengthChars": total, "totalSegmentCount": len(specs), "chunkSequenceNumber": seq,
                       "segmentTexts": specs,
                       "headerMetadata": {"orderedChunkMetadata": [{"id": "header"}], "sequenceNumber": seq,
                                          "totalLength": total, "totalSegmentCount": len(specs)}})


def _prefix(tier):
    """The leaf that escalates a copy: its props keep it from merging into the case."""
    if tier == "large":
        return [P("L" * LARGE_PREFIX, tier="large")]
    if tier == "huge":
        return [P("H" * HUGE_PREFIX, tier="huge")]
    return []


def add_case(b, case, tier):
    pre = _prefix(tier)
    k = sum(_len(s) for s in pre)
    if case.v1_load is not None:
        head, bodies = case.v1_load
        head = dict(head, segments=pre + head["segments"], segmentCount=head["segmentCount"] + len(pre),
                    length=head["length"] + k)
        md = dict(head["headerMetadata"])
        md["totalLength"] += k
        md["totalSegmentCount"] += len(pre)
        head["headerMetadata"] = md
        bodies = [dict(bd, startIndex=bd["startIndex"] + len(pre)) for bd in bodies]
        d = b.begin_doc_from_summary(json.dumps(head), [json.dumps(bd) for bd in bodies])
    else:
        d = b.begin_doc_from_summary(legacy_header(pre + case.specs))
    for m in case.msgs:
        d.add_message(dict(m, contents=_shift(m["contents"], k)))


# ---------------------------------------------------------------------------------------- families
def _newline():
    return [Case("ends_in_newline", ["ab\n", "cd"]),
            Case("only_newline", ["\n", "cd", "ef"]),
            Case("gains_newline", ["ab", "\n", "cd", "ef"]),
            Case("newline_inside", ["a\nb", "cd", "e\n\nf", "gh"]),
            Case("unit_010a", ["ab" + chr(0x010A), "cd"]),
            Case("unit_0a00", ["ab" + chr(0x0A00), "cd"]),
            Case("newline_then_props", ["ab\n", P("cd", x=1), P("ef\n", x=1), P("gh", x=1)])]


def _granularity():
    return [Case("256_257", [T(256), T(257, "u")]),
            Case("257_256", [T(257), T(256, "u")]),
            Case("257_257", [T(257), T(257, "u")]),
            Case("grown_300_257_256", [T(150), T(150, "u"), T(257, "v"), T(256, "w")]),
            Case("alone_255", [T(255)]),
            Case("alone_256", [T(256)]),
            Case("alone_257", [T(257)]),
            Case("256_1_257", [T(256), "x", T(257, "u"), "y"])]


WIDE = {f"k{k:02d}": 1 for k in range(20)}  # 20 keys: three records of FMT_MT_PROPS_MAX = 8
INDEX_KEYS = {"b": 7, "10": 1, "9": 2, "0": 3, "01": 4, "4294967294": 5, "4294967295": 6, "a": 8}


def _props():
    wide_first = {k: WIDE[k] for k in list(WIDE)[:10]}
    wide_rest = {k: WIDE[k] for k in list(WIDE)[10:]}
    return [padded("other_key_order", [P("aa", x=1, y=2), P("bb", q=0), P("cc")],
                   [("B", ann(2, 4, {"q": None})), ("B", ann(2, 6, {"y": 2})), ("C", ann(2, 6, {"x": 1}))], S + 5),
            Case("other_value", [P("aa", x=1), P("bb", x=2), P("cc", x=1)]),
            padded("emptied_next_to_none", [P("aa", x=1), "bb", P("cc", x=1)],
                   [("B", ann(0, 2, {"x": None})), ("B", ann(4, 6, {"x": None}))], S + 4),
            padded("wide_equal", [P("aa", **wide_rest), P("bb", **WIDE), P("cc", **dict(WIDE, k19=2))],
                   [("B", ann(0, 2, wide_first))], S + 3),
            Case("wide_last_key_differs", [P("aa", **WIDE), P("bb", **dict(WIDE, k19=2)), P("cc", **dict(WIDE, k19=2))]),
            Case("index_keys", [P("aa", **INDEX_KEYS), P("bb", **INDEX_KEYS), P("cc", **dict(INDEX_KEYS, a=9))]),
            Case("index_keys_marker", [M(2, dict(INDEX_KEYS)), P("aa", **{"1": 1, "00": 2, "4294967296": 3, "-1": 4, "1.5": 5})]),
            padded("annotate_above_min_seq", [P("aa", x=1), P("bb", x=1), P("cc", x=1)],
                   [("B", ann(2, 4, {"x": 2}))], S + 2)]


def _props_adjust():
    """The same pair in a batch with annotate-adjust: the legacy summary reads getAtSeq(minSeq), the
    engine's per-leaf legacy prop sets; SnapshotV1 reads the leaf's own."""
    return [padded("annotate_above_min_seq", [P("aa", x=1), P("bb", x=1), P("cc", x=1)],
                   [("B", ann(2, 4, {"x": 2}))], S + 2),
            padded("adjust_above_min_seq", [P("aa", n=5), P("bb", n=5), P("cc", n=5)],
                   [("B", ann(2, 4, adjust={"n": {"delta": 1}}))], S + 2),
            padded("adjust_below_min_seq", [P("aa", n=5), P("bb", n=5), P("cc", n=6)],
                   [("B", ann(2, 4, adjust={"n": {"delta": 1}}))], S + 3)]


def _markers():
    return [Case("between_texts", ["ab", M(1), "cd"]),
            Case("adjacent", ["ab", M(1), M(2), "cd"]),
            Case("first", [M(1), "ab", "cd"]),
            Case("last", ["ab", "cd", M(0)]),
            Case("with_props", ["ab", M(1, {"k": 1}), M(1, {"k": 1}), P("cd", k=1), M(3, {"k": 1, "j": "x"})]),
            Case("only_markers", [M(1), M(1)])]


def _presence():
    mid = [P("aa", m=0), P("bb", m=1), P("cc", m=0), P("dd", m=1), P("ee", m=0), P("ff", m=1)]
    return [padded("inserted_at_min_seq", mid, [("B", ins(2, P("I", i=1))), ("C", ins(7, P("J", i=2)))], S + 3),
            padded("removed_at_min_seq", mid, [("B", rem(2, 4)), ("C", rem(6, 8))], S + 3),
            padded("inserted_and_removed", mid, [("B", ins(2, P("I", i=1))), ("C", rem(2, 3)), ("B", rem(5, 7))], S + 4),
            Case("all_removed", [P("a", m=k % 2) for k in range(200)],  # (scouring spreads over two parents: some stay)
                 [msg("B", S + 1, S, rem(0, 200)), msg("B", S + 2, S + 1, group())]),
            Case("no_leaves", [])]


def _wave():
    rng = np.random.default_rng(7)
    many = ["".join(chr(0x4E00 + int(x)) for x in rng.integers(0, 500, int(n))) for n in rng.integers(1, 4, 140)]
    classes = [P(chr(0x3041 + k), c=(k // 3) % 2) for k in range(135)]  # runs of three, never at a multiple of 64
    removed = [chr(0x0400 + k) for k in range(270)]
    return [Case("140_appends", many),
            Case("135_in_runs_of_3", classes),
            Case("long_leaves", [P(T(70), w=0), P(T(5000, "u"), w=1), "a", "b", T(65, "v"), P(T(4097, "w"), w=0)]),
            Case("chunk_removed", removed, [msg("B", S + 1, S, rem(40, 200)), msg("B", S + 2, S + 1, group())])]


SPECIAL = '"\\' + "".join(chr(k) for k in [*range(0x20), 0x7F, 0x80, 0x7FF, 0x800, 0x2028, 0x2029, 0xFFFF]) + "end"


def _text():
    hi, lo = chr(0xD83D), chr(0xDE00)
    return [Case("special_units", [SPECIAL, P(SPECIAL, x=1)]),
            Case("intact_pair", ["a" + hi + lo + "b"]),
            Case("pair_joined_by_append", ["a" + hi, lo + "b"]),
            Case("pair_split_by_props", [P("a" + hi, h=1), P(lo + "b", h=2)]),
            Case("lone_high_ends_run", [P("x" + hi, h=1), P("y", h=2)]),
            Case("lone_low_starts_run", [P("x", h=1), P(lo + "y", h=2)]),
            Case("lone_halves_in_one_run", [lo + "x" + hi + "y" + lo + lo + hi])]


def _chunks():
    return [Case("one_run", ["abcdef"]),
            Case("two_runs", [P("abc", x=1), P("defgh", x=2)]),
            Case("five_runs", [P(T(3 + k), x=k) for k in range(5)]),
            Case("marker_runs", ["ab", M(1), "cd", M(2, {"k": 1}), "e"]),
            Case("last_run_of_one_unit", [P("abcd", x=1), P("e", x=2)])]


def _v1_loaded():
    """A SnapshotV1 load whose header holds merge info, so that its body segments arrive as
    FMT_MT_F_LOADSEG records ahead of the messages; then removes above minSeq."""
    head = {"version": "1", "segmentCount": 2, "length": 6, "startIndex": 0,
            "segments": [{"text": "head", "props": {"v": 1}}, {"json": "hh", "seq": S + 1, "client": "B"}],
            "headerMetadata": {"minSequenceNumber": S, "sequenceNumber": S + 1,
                               "orderedChunkMetadata": [{"id": "header"}, {"id": "body_0"}],
                               "totalLength": 14, "totalSegmentCount": 5}}
    body = {"version": "1", "segmentCount": 3, "length": 8, "startIndex": 2,
            "segments": [{"json": {"text": "bod", "props": {"v": 2}}, "seq": S + 1, "client": "B"},
                         {"json": {"text": "yyy", "props": {"v": 3}}, "seq": S + 1, "client": "B"},
                         {"json": "zz", "seq": S + 1, "client": "B"}]}
    msgs = [msg("C", S + 2, S, rem(7, 10)), msg("B", S + 3, S, ann(0, 2, {"v": 4})), msg("C", S + 4, S, rem(12, 13))]
    return Case("loaded_then_removed", [], msgs, v1_load=(head, [body]))


def _remover_doc(n_records):
    """n_records op records, none at or below minSeq: removes at the first, a middle and the last seq,
    annotates of one leaf between them."""
    specs = [P("aaa", r=0), P("bbb", r=1), P("ccc", r=2), P("ddd", r=3), P("eee", r=4)]
    mid = n_records // 2
    msgs = []
    for k in range(n_records):
        seq = S + 1 + k
        if k == 0:
            op, who = rem(0, 3), "B"
        elif k == mid:
            op, who = rem(3, 6), "C"
        elif k == n_records - 1:
            op, who = rem(6, 9), "D"
        else:
            op, who = ann(12, 15, {"r": 4 + k % 2}), "BCD"[k % 3]
        msgs.append(msg(who, seq, S, op))
    return Case(f"{n_records}_records", specs, msgs)


def _first_remover():
    grouped = Case("remover_second_in_group", [P("aaa", r=0), P("bbb", r=1), P("ccc", r=2)],
                   [msg("B", S + 1, S, ann(0, 3, {"r": 5})),
                    msg("C", S + 2, S, group(ann(6, 9, {"r": 6}), ins(9, "tail"), rem(3, 6), rem(0, 1))),
                    msg("B", S + 3, S, ann(6, 9, {"r": 7}))])
    return [_remover_doc(64), _remover_doc(65), _remover_doc(4097), grouped, _v1_loaded()]


FAMILIES = {"newline": _newline, "granularity": _granularity, "props": _props, "props_adjust": _props_adjust,
            "markers": _markers, "presence": _presence, "wave": _wave, "text": _text, "chunks": _chunks,
            "first_remover": _first_remover}

# the decisions and facts each family exists for: census keys, each found at least once among the
# family's documents (in every tier, except where a tier's prefix leaf takes the place named)
PROMISES = {
    "newline": ["newline", "newline:after_append", "newline:leaf_is_only_newline", "append:gains_newline",
                "append:newline_inside", "append:run_last_0x010a", "append:run_last_0x0a00"],
    "granularity": ["append:run_le_256_leaf_gt_256", "append:run_gt_256_leaf_le_256", "granularity_stop",
                    "granularity_stop:grown_run", "single_255", "single_256", "single_257"],
    "props": ["append:same_class_different_id", "class_mismatch", "append:empty_vs_undefined",
              "append:same_class_different_id_wide", "class_mismatch:wide", "wide_set", "append"],
    "props_adjust": ["append", "class_mismatch"],
    "markers": ["marker_prev", "marker_next", "marker_marker", "marker_first", "marker_last", "marker_with_props",
                "marker_without_props"],
    "presence": ["ins_eq_min", "ins_eq_min_plus_1", "rm_eq_min", "rm_eq_min_plus_1", "nothing_present", "no_leaves"],
    "wave": ["leaves_ge_130", "append:across_64_boundary", "append:across_127_128", "leaf_gt_64", "leaf_gt_4096",
             "chunk_units_not_multiple_of_64", "append:across_skipped_chunk", "class_mismatch"],
    "text": ["append:joins_surrogate_pair", "split_surrogate_pair", "run_ends_lone_high", "run_starts_lone_low"],
    "chunks": ["class_mismatch", "marker_prev"],
    "first_remover": ["v1_solo"],
}
ONLY_ASIS = {"marker_first", "no_leaves", "nothing_present", "single_255", "single_256", "single_257"}


def promises(family, tier):
    return [k for k in PROMISES[family] if tier == "asis" or k not in ONLY_ASIS]


@functools.lru_cache(maxsize=None)
def batch(family, tier="asis"):
    """(MergeTreeBatch, [case names]) of one family in one tier, remove order flagged as
    tests/v1_bulk.py does."""
    b = MergeTreeStreamBuilder()
    cases = FAMILIES[family]()
    for case in cases:
        add_case(b, case, tier)
    return b.finish(remove_order=True), [c.name for c in cases]


@functools.lru_cache(maxsize=None)
def neighbours_batch():
    """A document whose replay fails (an insert past the end of an empty document) between two good ones."""
    b = MergeTreeStreamBuilder()
    add_case(b, _granularity()[3], "asis")
    d = b.begin_doc("", observer="A")
    d.add_message(msg("B", 1, 0, ins(5, "x"), ref=0))
    add_case(b, _markers()[4], "asis")
    return b.finish(remove_order=True)


# -------------------------------------------------------------------------------------- references
CAP_LEAVES, CAP_PROPS = 1024, 256


@functools.lru_cache(maxsize=None)
def oracle_state(family, tier="asis"):
    """[(header, leaves, chars, props, removers)] of the oracle's replay, and the batch's computed
    annotate-adjust numbers per document (or None)."""
    import oracle as orc

    import v1_bulk

    bt, _ = batch(family, tier)
    numbers = [] if bt.adjusts is not None else None
    cap_chars = {"asis": 1 << 14, "large": 1 << 14, "huge": HUGE_PREFIX + (1 << 14)}[tier]
    state = v1_bulk.oracle_state(orc, bt, cap_leaves=CAP_LEAVES, cap_chars=cap_chars, cap_props=CAP_PROPS, numbers=numbers)
    return state, numbers


def doc_values(bt, numbers, d):
    return bt.values if numbers is None else summary.values_with_numbers(bt.values, numbers[d])


def totals(state, legacy_props=None):
    """Every document's own total: the units its legacy summary holds, from the reference's segments."""
    out = []
    for d, (h, l, c, p, _) in enumerate(state):
        segs = summary.legacy_segments(h, l, c, p, int(h["min_seq"]), None if legacy_props is None else legacy_props[d])
        out.append(sum(summary._utf16_len(t) for t, _, _ in segs))
    return out


def chunk_sizes(total):
    """The chunk sizes a document is summarised with: 1, its total - 1, its total and the default."""
    return sorted({1, max(total - 1, 1), max(total, 1), summary.SIZE_OF_FIRST_CHUNK})


def remover_census(bt, d, state):
    """Where the first remover of each leaf removed above minSeq sits among document d's op records:
    Counter of n_records, loadseg_prefix (records), first / middle / last (the record with the leaf's
    rm_seq is the first, an inner or the last one past the prefix) and not_first_of_seq (records of
    that seq come before the removing one)."""
    from fluidframework_amd.streams import MT_F_LOADSEG, MT_OBLITERATE, MT_OBLITERATE_SIDED, MT_REMOVE

    h, l, *_ = state[d]
    ops = bt.ops[int(bt.doc_op_offsets[d]) : int(bt.doc_op_offsets[d + 1])]
    pre = int(((ops["flags"] & MT_F_LOADSEG) != 0).sum())
    rest = ops[pre:]
    c = Counter(n_records=len(ops), loadseg_prefix=pre)
    ms = int(h["min_seq"])
    for i in range(int(h["n_leaves"])):
        rm = int(l[i]["rm_seq"])
        if rm == summary.NOT_REMOVED or rm <= ms:
            continue
        at = np.nonzero(rest["seq"] == rm)[0]
        removing = [int(k) for k in at if int(rest["type"][k]) in (MT_REMOVE, MT_OBLITERATE, MT_OBLITERATE_SIDED)]
        c["first"] += removing[0] == 0
        c["last"] += removing[0] == len(rest) - 1
        c["middle"] += 0 < removing[0] < len(rest) - 1
        c["not_first_of_seq"] += removing[0] != int(at[0])
    return c


@functools.lru_cache(maxsize=None)
def legacy_view_state(family, tier):
    """[(header, leaves, chars, props, legacy props or None)] per document: the state summary.legacy_summary
    reads on the CPU. A plain batch: the oracle's. A batch with annotate-adjust: the state of the engine
    source under host emulation with its per-leaf getAtSeq(minSeq) prop sets, which index that state's
    own prop-set table (the emulation's state equals the oracle's leaf for leaf, tests/test_annotate_adjust.py)."""
    from mt_compare import emu_legacy_props, emu_replay

    bt, _ = batch(family, tier)
    if bt.adjusts is None:
        return [(h, l, c, p, None) for h, l, c, p, _ in oracle_state(family, tier)[0]]
    hdr, lv, ch, pr = emu_replay(bt, large=tier != "asis")
    assert (hdr["status"] == 0).all()
    return [(hdr[d], lv[d], ch[d], pr[d], emu_legacy_props(d)) for d in range(bt.n_docs)]


@functools.lru_cache(maxsize=None)
def legacy_reference(family, tier="asis"):
    """{(document, chunk size): (header, body or None)} from oracle.mt_replay_summary, each document
    at 1, its own total - 1, its own total and 10000."""
    import oracle as orc

    bt, _ = batch(family, tier)
    state, _ = oracle_state(family, tier)
    out = {}
    for d in range(bt.n_docs):
        total = json.loads(orc.mt_replay_summary(bt, d, bt.keys, bt.values)[0])["totalLengthChars"]
        for chunk in chunk_sizes(total):
            out[d, chunk] = orc.mt_replay_summary(bt, d, bt.keys, bt.values, chunk)
    return out


@functools.lru_cache(maxsize=None)
def v1_reference(family, tier="asis"):
    """{(document, chunk size): (header, [bodies])} from summary.v1_summary over the oracle's state and
    stamps (v1_bulk.reference), each document at 1, its own total - 1, its own total and 10000."""
    import v1_bulk

    bt, _ = batch(family, tier)
    state, numbers = oracle_state(family, tier)
    values = None if numbers is None else [doc_values(bt, numbers, d) for d in range(bt.n_docs)]
    out = {}
    for d in range(bt.n_docs):
        one = lambda chunk: v1_bulk.reference(_OneDoc(bt, d), [state[d]], chunk, None if values is None else [values[d]])[0]
        total = json.loads(one(summary.V1_CHUNK_SIZE)[0])["headerMetadata"]["totalLength"]
        for chunk in chunk_sizes(total):
            out[d, chunk] = one(chunk)
    return out


class _OneDoc:
    """Document d of a batch as v1_bulk.reference reads a batch (keys, values, clients)."""

    def __init__(self, bt, d):
        self.keys, self.values, self.clients = bt.keys, bt.values, [bt.clients[d]]

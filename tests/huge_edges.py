"""Streams that take the huge-document engine (csrc/huge_engine.h) across the thresholds T3's own
shape stays just inside of, with proofs from the ops and the oracle alone that they do:

  - kWinLds: window entries past the LDS mirror live only in HBM. hold_min_seq turns a T3 stream's
    minSeq into a sawtooth (sampled every `period` ops and held), so the collab window grows through
    kWinLds during a hold and one op releases it all (a mass graduation of swap-removes back down
    through the boundary). window_lower_bound / window_upper_bound bound the window size from the op
    records alone.
  - kSlotCap: a group splits when its slot list fills. A document loaded as one group (at most kFill
    full leaf blocks) whose oracle replay ends with more than kSlotCap leaf blocks must have split.
  - the merge area under the runtime's own sizing (compaction_stream).

engine_constants reads the thresholds from the header; nothing here copies them."""
import copy
import dataclasses
import os
import re

import numpy as np

from fluidframework_amd import workloads
from fluidframework_amd.streams import (ADJUST_DTYPE, MT_ANNOTATE, MT_INSERT, MT_OP_DTYPE, MT_REMOVE, SNAPSHOT_DOC_DTYPE,
                                        SNAPSHOT_SEG_DTYPE, VALUE_ADJUST, value_numbers)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "fluidframework_amd", "csrc")


def engine_constants():
    """kWinLds, kSlotCap and kFill as huge_engine.h defines them for the device build."""
    src = open(os.path.join(CSRC, "huge_engine.h"), encoding="utf-8").read()
    out = {"kWinLds": int(re.search(r"constexpr uint32_t kWinLds = (\d+);", src).group(1))}
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (FMT_HUGE_SLOTCAP|FMT_HUGE_FILL) (\d+)$", src, re.M)}
    for name, macro in (("kSlotCap", "FMT_HUGE_SLOTCAP"), ("kFill", "FMT_HUGE_FILL")):
        assert re.search(rf"constexpr int {name} = {macro};", src)
        out[name] = macros[macro]
    return out


def merge_area_units(batch, n_ops=None):
    """The merge area the runtime gives a document that is huge at load (runtime.cpp setupHugeDoc:
    max(textPerOp * nOps + 65536, 4 * docChars + 131072), textPerOp read from its call for such loads)."""
    src = open(os.path.join(CSRC, "runtime.cpp"), encoding="utf-8").read()
    assert "std::max<uint64_t>(textPerOp * nOps + 65536, 4 * docChars + 131072)" in src
    per_op = int(re.search(r"for \(uint32_t d : P\.hugeDocs\) \{.*?FMT_NON_COLLAB_CLIENT, (\d+), P\.docChars\[d\]\);", src,
                           re.S).group(1))
    n_ops = len(batch.ops) if n_ops is None else n_ops
    ins = batch.ops[batch.ops["type"] == MT_INSERT]
    doc_chars = int(batch.snapshot_segs["len"].sum()) + int(ins["len"].sum())
    return max(per_op * n_ops + 65536, 4 * doc_chars + 131072)


# ------------------------------------------------------------------ batches
def one_doc(batch, d):
    """Document d of a batch as a batch of its own (same text, props and segment tables)."""
    b = copy.copy(batch)
    o0, o1 = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
    b.ops = batch.ops[o0:o1]
    b.doc_op_offsets = np.array([0, o1 - o0], dtype=np.uint64)
    b.doc_init = batch.doc_init[d : d + 1]
    if batch.snapshots is not None:
        b.snapshots = batch.snapshots[d : d + 1]
    return b


def concat_batches(batches):
    """One batch holding every document of `batches` (same props table: conflict farm and T3 share it)."""
    ops, offs, texts, init, snaps, segs = [], [0], [], [], [], []
    tbase, sbase = 0, 0
    for b in batches:
        o = b.ops.copy()
        o["payload"][o["type"] == 0] += tbase
        ops.append(o)
        offs.extend((np.asarray(b.doc_op_offsets[1:], dtype=np.int64) + offs[-1]).tolist())
        texts.append(b.text)
        di = b.doc_init.copy()
        di[:, 0] += tbase
        init.append(di)
        if b.snapshots is not None:
            sd = b.snapshots.copy()
            sd["first_seg"] += sbase
            sg = b.snapshot_segs.copy()
            sg["text"] += tbase
            snaps.append(sd)
            segs.append(sg)
            sbase += len(sg)
        else:
            snaps.append(np.zeros(b.n_docs, dtype=SNAPSHOT_DOC_DTYPE))
        tbase += len(b.text)
    first = batches[0]
    return first.__class__(
        ops=np.concatenate(ops), doc_op_offsets=np.asarray(offs, dtype=np.uint64), text=np.concatenate(texts),
        doc_init=np.concatenate(init), props_off=first.props_off, props_kv=first.props_kv, keys=first.keys,
        values=first.values, snapshots=np.concatenate(snaps),
        snapshot_segs=np.concatenate(segs) if segs else np.zeros(0, dtype=SNAPSHOT_SEG_DTYPE))


def prefix(batch, n):
    """The first n ops of a one-document batch."""
    return dataclasses.replace(batch, ops=batch.ops[:n].copy(), doc_op_offsets=np.array([0, n], dtype=np.uint64))


def hold_min_seq(batch, period):
    """A copy of a one-document batch whose minSeq is sampled every `period` ops and held:
    min_seq'[i] = min_seq[i - i % period]. Still non-decreasing, never above the original (so never
    above a later refSeq): the stream stays valid and the oracle replays the same ops."""
    ops = batch.ops.copy()
    i = np.arange(len(ops))
    ops["min_seq"] = batch.ops["min_seq"][i - i % period]
    return dataclasses.replace(batch, ops=ops)


# ------------------------------------------------------------------ window bounds from the ops alone
def _span_start(ops):
    """Per op i, the index of the first op whose seq is above min_seq[i] (the ops in (min_seq[i], seq_i]
    are [that index, i])."""
    return np.searchsorted(ops["seq"], ops["min_seq"], side="right")


def window_lower_bound(ops):
    """Per op i, a lower bound of the window table's size after it: the insert ops with seq in
    (min_seq[i], seq_i]. Each leaves at least one leaf with ins > minSeq, which zamboni cannot take and
    a remove keeps in the window."""
    cum = np.concatenate([[0], np.cumsum(ops["type"] == MT_INSERT)])
    return cum[1:] - cum[_span_start(ops)]


def window_upper_bound(ops, max_range):
    """Per op i, an upper bound: (max_range + 3) per op in that span (a range op touches at most
    max_range leaves of at least one unit plus two splits, an insert makes at most three leaves)."""
    return (np.arange(1, len(ops) + 1) - _span_start(ops)) * (max_range + 3)


def crossings(ops, period, max_range, threshold):
    """(up, down): how often the window provably rises through `threshold` and falls back below it.
    Checkpoints in op order: the first op of every hold (below, when the upper bound says so) and the
    last op of every full hold (above, when the lower bound says so)."""
    lo, hi = window_lower_bound(ops), window_upper_bound(ops, max_range)
    state, up, down = None, 0, 0
    for k in range(0, len(ops), period):
        marks = [(k, "below" if hi[k] < threshold else None)]
        if k + period <= len(ops):
            marks.append((k + period - 1, "above" if lo[k + period - 1] > threshold else None))
        for _, s in marks:
            if s is None or s == state:
                continue
            up += state == "below" and s == "above"
            down += state == "above" and s == "below"
            state = s
    return up, down


# ------------------------------------------------------------------ the streams
@dataclasses.dataclass(frozen=True)
class WindowStream:
    n_segments: int
    n_ops: int
    n_clients: int
    max_lag: int
    max_range: int
    seed: int
    period: int

    def batch(self, period=None):
        return hold_min_seq(workloads.t3_stream(self.n_segments, self.n_ops, n_clients=self.n_clients, max_lag=self.max_lag,
                                                max_range=self.max_range, seed=self.seed), period or self.period)


# Three full holds and the release after the third (3 * period < n_ops). About a third of the ops are
# inserts, so a hold of 4,200 ops keeps ~1,400 leaves above minSeq at its end; after a release the span
# is the original stream's own lag (the refSeq lag plus the wait for the least recent writer), and the
# upper bound charges it (max_range + 3) entries per op, which is what limits the writers, the lag and
# the ranges of both shapes. The wide one is as wide as that bound lets it be: every op sees the
# document as of up to 12 ops back, from one of 12 clients, with ranges up to 12 units. Deep refSeq lag,
# many writers and long ranges (overlapping removers, writers 64 and up) cannot show a provable trough:
# with them the original minSeq trails by hundreds of ops. They are in DEEP_STREAMS below, which need
# only the lower bound.
WINDOW_STREAMS = {
    "window_sawtooth": WindowStream(3000, 12700, 8, 32, 8, 71, 4200),
    "window_sawtooth_wide": WindowStream(6000, 12700, 12, 12, 12, 72, 4200),
}

# Deep shapes: one full hold, the release, and a second hold the stream ends in (n_ops = 2 * period), so
# the window is past the mirror at the end of the first hold (the release then swaps tail entries down
# through kWinLds) and again at the last op: the final state still holds more than kWinLds entries above
# minSeq, with their removers. Only the lower bound is claimed for them.
#   window_deep: 31 writers seeing the document as of up to 1,000 ops back, ranges up to 24 units:
#     concurrent removes overlap, so leaves past the mirror carry several removers (the remove-order
#     variant's stream: a leaf's stamp list then comes from the recorded entries, not from the leaf).
#   window_many_writers: 100 writers (short ids past 63: the per-leaf side table that perspectives of
#     those clients read, on entries past the mirror too), lag up to 2,000, ranges up to 20.
DEEP_STREAMS = {
    "window_deep": WindowStream(9000, 8400, 31, 1000, 24, 76, 4200),
    "window_many_writers": WindowStream(9000, 8400, 100, 2000, 20, 77, 4200),
}


def window_sawtooth():
    return WINDOW_STREAMS["window_sawtooth"].batch()


def window_sawtooth_wide():
    return WINDOW_STREAMS["window_sawtooth_wide"].batch()


def window_deep():
    return DEEP_STREAMS["window_deep"].batch()


def window_many_writers():
    return DEEP_STREAMS["window_many_writers"].batch()


def leaf_blocks(leaves):
    """The number of leaf blocks of a dumped document: its last leaf's block ordinal + 1 (fmt_mt_leaf:
    block = the ordinal's low 16 bits, pad = its high bits beside the marker flag)."""
    from fluidframework_amd.streams import MT_LEAF_MARKER
    last = leaves[-1]
    return (int(last["block"]) | (int(last["pad"]) & ~MT_LEAF_MARKER) << 16) + 1


GROUP_SPLIT_OPS = 5000


def group_split():
    """7,000 segments load as one group of 1,000 leaf blocks (the oracle's tree with no op replayed
    says how many); minSeq stays at 0 for the whole stream (one hold), so zamboni packs nothing while
    the ops split leaves and blocks."""
    return hold_min_seq(workloads.t3_stream(7000, GROUP_SPLIT_OPS, n_clients=8, max_lag=64, max_range=2, seed=73),
                        GROUP_SPLIT_OPS)


# split_with_tail: one hold over the whole stream. SPLIT_TAIL_BEFORE ops in, the window already holds
# more than kWinLds entries (lower bound) while the oracle's tree has at most kSlotCap leaf blocks; by
# SPLIT_TAIL_AFTER ops it has more, in the same hold: the one group split with entries past the mirror.
SPLIT_TAIL_OPS, SPLIT_TAIL_BEFORE, SPLIT_TAIL_AFTER = 5500, 4000, 5500


def split_with_tail():
    return hold_min_seq(workloads.t3_stream(4000, SPLIT_TAIL_OPS, n_clients=8, max_lag=64, max_range=2, seed=74),
                        SPLIT_TAIL_OPS)


def compaction_stream(n_segments=3000, n_ops=3000):
    """Churn at the end of a loaded document, minSeq trailing by one op: two writers append three units
    by turns, every seventh op removes four units from inside what was appended, every thirty-first
    removes the last hundred. Each acked insert is appended onto the run before it by zamboni, which
    copies the whole run into the merge area again; the removes split the run and their release lets
    the halves merge once more."""
    base = workloads.t3_stream(n_segments, 1, n_clients=2, max_lag=1, seed=75)
    total = int(base.snapshot_segs["len"].sum())
    text = base.text.tolist()
    ops = np.zeros(n_ops, dtype=MT_OP_DTYPE)
    length = total
    for i in range(n_ops):
        seq = i + 1
        client = 1 + i % 2
        grown = length - total
        if i % 31 == 30 and grown > 200:
            ops[i] = (seq, seq - 1, seq - 1, length - 100, length, 0, 0, client, MT_REMOVE, 0)
            length -= 100
        elif i % 7 == 6 and grown > 40:
            p = total + (i * 13) % (grown - 8)
            ops[i] = (seq, seq - 1, seq - 1, p, p + 4, 0, 0, client, MT_REMOVE, 0)
            length -= 4
        else:
            ops[i] = (seq, seq - 1, seq - 1, length, -1, len(text), 3, client, MT_INSERT, 0)
            text += [ord("x") + client] * 3
            length += 3
    return dataclasses.replace(base, ops=ops, doc_op_offsets=np.array([0, n_ops], dtype=np.uint64),
                               text=np.asarray(text, dtype="<u2"))


STREAMS = {"window_sawtooth": window_sawtooth, "window_sawtooth_wide": window_sawtooth_wide, "group_split": group_split,
           "split_with_tail": split_with_tail, "compaction": compaction_stream, "window_deep": window_deep,
           "window_many_writers": window_many_writers}


# ------------------------------------------------------------------ Rm and Adj variants of the sawtooth
def with_remove_order(batch):
    """FMT_MT_F_RMORDER on every op (the remove-order instantiation records each remove's stamps)."""
    from fluidframework_amd.streams import MT_F_RMORDER
    ops = batch.ops.copy()
    ops["flags"] |= MT_F_RMORDER
    return dataclasses.replace(batch, ops=ops)


def with_adjusts(batch):
    """Every second annotate becomes an annotate-adjust of "weight" (delta by client, one in three
    clamped to [-4, 6]): the batch gains the key, the fmt_mt_adjust rows, one props op per row and the
    per-value number table, as MergeTreeStreamBuilder.finish packs them."""
    n_props = len(batch.props_off) - 1
    key = len(batch.keys)
    rows = [(float(d), -4.0 if k % 3 == 0 else 0.0, 6.0 if k % 3 == 0 else 0.0, 5 if k % 3 == 0 else 0, 0)
            for k, d in enumerate((1, -2, 3, -1, 2, -3, 0.5))]
    kv = batch.props_kv.tolist()
    off = batch.props_off.tolist()
    for r in range(len(rows)):
        kv += [(key << 16) | VALUE_ADJUST, r]
        off.append(len(kv))
    ops = batch.ops.copy()
    ann = np.nonzero(ops["type"] == MT_ANNOTATE)[0][::2]
    ops["payload"][ann] = n_props + ops["client"][ann].astype(np.uint32) % len(rows)
    return dataclasses.replace(batch, ops=ops, props_off=np.asarray(off, dtype=np.uint32),
                               props_kv=np.asarray(kv, dtype=np.uint32), keys=list(batch.keys) + ["weight"],
                               adjusts=np.array(rows, dtype=ADJUST_DTYPE), value_num=value_numbers(batch.values))


# ------------------------------------------------------------------ the oracle's state, computed once
_batches, _expected = {}, {}


def stream(name):
    """The named stream's batch (built once; treat it as read-only)."""
    if name not in _batches:
        _batches[name] = STREAMS[name]()
    return _batches[name]


def oracle_state(orc, batch, numbers=None):
    """(rc, (header, leaves, chars, props)) of a one-document batch replayed by the oracle with its
    remote-length index; `numbers` (a list) receives the computed annotate-adjust numbers."""
    sd = batch.snapshots[0] if batch.snapshots is not None else None
    n_segs = int(sd["n_header"]) + int(sd["n_body"]) if sd is not None and sd["loaded"] else 1
    orc.set_index(True)
    try:
        kw = {} if numbers is None else {"numbers": numbers}
        rc, oh, ol, oc, op, *_ = orc.mt_replay_batch(batch, cap_leaves=n_segs + 3 * len(batch.ops) + 8,
                                                     cap_chars=len(batch.text) + 8, cap_props=4096, **kw)
    finally:
        orc.set_index(False)
    h = oh[0]
    return rc, (h, ol[0][: int(h["n_leaves"])], oc[0][: int(h["n_chars"])], op[0][: int(h["n_props"])])


def expected_digest(orc, name):
    """The oracle's state digest of the named stream's own replay (remove clients past 63 included)."""
    orc.set_index(True)
    try:
        rc, dig, st, _ = orc.mt_replay_digest(stream(name), 0, 1, threads=1)
    finally:
        orc.set_index(False)
    assert rc == 0 and int(st[0]) == 0
    return int(dig[0])


def expected(orc, name):
    """The oracle's final state of the named stream (computed once, shared by every test)."""
    if name not in _expected:
        rc, exp = oracle_state(orc, stream(name))
        assert rc == 0
        _expected[name] = exp
    return _expected[name]

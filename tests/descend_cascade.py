"""The plain-batch cascade with stepping down under host emulation (tests/emu/mt_emu_tiers.cpp through
micro_cascade.lib(): one launch per call, the step-down switch and both lists exposed), the steps of the
route launchMergeTree walks (csrc/mt_route.h) run from here, and the documents the step-down tests are built
from. Shared by test_descend_emulated.py (CPU) and test_gpu_descend.py (the same batches on the device)."""
import ctypes

import numpy as np

from fluidframework_amd.native import batch_struct
from micro_cascade import CKPT, COMPACT, E_CAPACITY, LARGE, MICRO, SMALL, Cascade, _msg, lib, route
from mt_compare import _p

ROUNDS = int(lib().emu_descend_rounds())  # csrc/mt_route.h kDescendRounds
TIERS = {"micro": MICRO, "compact": COMPACT, "small": SMALL, "large": LARGE}


def consts():
    """(kCkptDescend, kDescendLeaves4, kDescendChars4, kDescendMinOps) of mt_engine.h"""
    v = (ctypes.c_int32 * 4)()
    lib().emu_descend_consts(v)
    return tuple(int(x) for x in v)


DESC = consts()[0]


class DescendCascade(Cascade):
    """micro_cascade.Cascade driven launch by launch: launch() is one tier over a list with the
    step-down switch, rounds() the whole of launchMergeTree. ops_in[tier] counts the ops each tier
    replayed, hops[d] the launches that took document d over from another tier, and routes the kinds of
    hop taken."""

    def __init__(self, batch, cap_catchup=0, checkpoints=True):
        super().__init__(batch, cap_catchup, checkpoints)
        self.ops_in = [0, 0, 0, 0]
        self.hops = np.zeros(self.n, dtype=int)
        self.downs = np.zeros(self.n, dtype=int)      # downward hops taken
        self.up_after_down = np.zeros(self.n, dtype=bool)
        self.routes = {"small->compact": 0}

    def new_list(self):
        return np.zeros(self.n + 1, dtype=np.uint32)

    def _next_op(self, d):
        st = int(self.hdr[d]["status"])
        if self.ck is not None and st in (CKPT, DESC):
            return self.head(d)[0]
        return None

    def launch(self, tier, docs=None, descend=False, up=None, down=None):
        """docs: a list array ([0] = n, then ids) or None (every document, none resumed). Returns the
        statuses of the documents replayed, in list order."""
        b, keep = batch_struct(self.batch)
        cu = _p(self.cu) if self.cap_catchup else None
        ck = _p(self.ck) if self.ck is not None else None
        ids = np.arange(self.n) if docs is None else docs[1:1 + int(docs[0])].astype(int)
        offs = self.batch.doc_op_offsets
        start = {}
        for d in ids:  # where each document's replay starts in this launch
            nxt = self._next_op(d) if docs is not None or tier == SMALL else None
            start[d] = int(offs[d]) if nxt is None else nxt
        up = self.new_list() if up is None else up
        if tier == LARGE:
            if self.big is None:
                from fluidframework_amd.native import LEAF_DTYPE, PROPSET_DTYPE
                self.big = (np.zeros(self.n * self.bl, dtype=LEAF_DTYPE), np.zeros(self.n * self.bc, dtype="<u2"),
                            np.zeros(self.n * self.bp, dtype=PROPSET_DTYPE))
            lv, ch, pr = self.big
            small = (_p(self.leaves), _p(self.chars))
        else:
            lv, ch, pr, small = self.leaves, self.chars, self.props, (None, None)
        rc = lib().emu_tier_launch(ctypes.addressof(b), tier, _p(self.hdr), _p(lv), _p(ch), _p(pr), cu, self.cap_catchup, ck,
                                   _p(docs) if docs is not None else None, int(descend), _p(up),
                                   _p(down) if down is not None else None, small[0], small[1])
        del keep
        assert rc == len(ids)
        st = self.hdr["status"][ids].copy()
        for d, s in zip(ids, st):
            nxt = self._next_op(d)
            end = int(offs[d + 1]) if nxt is None else nxt
            if s == E_CAPACITY:  # restarts from its first op in the next tier: these ops are replayed twice
                end = int(offs[d + 1]) if self.ck is None else end
            self.ops_in[tier] += end - start[d]
            if s not in (CKPT, DESC, E_CAPACITY):
                self.done_in[d] = tier
            if s == DESC:
                self.downs[d] += 1
                self.routes["small->compact"] += 1
            if s == CKPT and self.downs[d] > 0:
                self.up_after_down[d] = True
        if docs is not None:
            self.hops[ids] += 1
        return st

    def rounds(self, rounds=0, descend=True, docs=None):
        """The register tiers of the route the runtime plans for the batch (csrc/mt_route.h planRoute, read
        through micro_cascade.route), step by step as launchMergeTree walks it; a step's reordering of its
        list is left out (no result depends on list order). rounds: other than the build's; descend False: no
        step-down slab; docs: the caller's list. Returns the list of the documents left for the large tier."""
        program = route(self.batch, ckpt_slab=self.ck is not None, desc_slab=descend, rounds=rounds)
        lists = {"none": None, "every": None, "caller": docs}
        for s in program.steps:
            assert s["variant"] == 0 and (s["in"] != "caller" or s["tier"] == "micro"), s  # (micro resumes nothing)
            src, up, down = (lists[k] if k in lists else lists.setdefault(k, self.new_list())
                             for k in (s["in"], s["up"], s["down"]))
            self.launch(TIERS[s["tier"]], src, s["descend"], up=up, down=down)
        return lists["toLarge"]


def held_by_last_round(batch, rounds=ROUNDS):
    """Documents the last round kept in a tier although they met the step-down condition there: those
    that stop once more when the cascade is given one more round."""
    a, b = DescendCascade(batch), DescendCascade(batch)
    a.rounds(rounds)
    b.rounds(rounds + 1)
    return np.nonzero(b.downs > a.downs)[0]


# ---- documents --------------------------------------------------------------------------------------

def grow_then_shrink_batch(peaks=(300,), tail_ops=400, piece=1, keep=8):
    """One document per peak. Phase 1, minSeq pinned at 0 so nothing is merged or dropped: `peak`
    inserts of `piece` units at position 0 (one leaf each). Phase 2, minSeq still pinned: one remove per
    op of the last visible `piece` units (the oldest leaf left), all but `keep` of them; the tombstones
    stay. Phase 3: `tail_ops` one-unit inserts at position 0 whose minSeq follows seq, so zamboni merges
    and drops a few leaves an op. Returns (batch, per document: the ops of phases 1 and 2)."""
    from fluidframework_amd.streams import MergeTreeStreamBuilder

    b = MergeTreeStreamBuilder()
    mids = []
    for peak in peaks:
        d = b.begin_doc()
        seq, length = 0, 0
        for k in range(peak):
            seq += 1
            d.add_message(_msg(seq, 0, {"type": 0, "pos1": 0, "seg": "abcdefgh"[k % 8] * piece}))
            length += piece
        for _ in range(peak - keep):
            seq += 1
            d.add_message(_msg(seq, 0, {"type": 1, "pos1": length - piece, "pos2": length}))
            length -= piece
        mids.append(seq)
        for k in range(tail_ops):
            seq += 1
            d.add_message(_msg(seq, seq - 1, {"type": 0, "pos1": 0, "seg": "z"}))
            length += 1
    return b.finish(), mids


def leaves_after_each_op(orc, batch, d, lo, hi):
    """[(leaves, text units) after document d's first k ops, by the oracle] for k in [lo, hi)."""
    from micro_cascade import prefix_leaves

    return [prefix_leaves(orc, batch, d, k) for k in range(lo, hi)]


def replicate(batch, copies):
    """`copies` documents with the ops of the one-document batch."""
    from dataclasses import replace

    n = len(batch.ops)
    assert batch.n_docs == 1
    return replace(batch, ops=np.tile(batch.ops, copies), doc_op_offsets=np.arange(copies + 1, dtype=np.uint64) * np.uint64(n),
                   doc_init=np.tile(batch.doc_init, (copies, 1)) if batch.doc_init is not None else None,
                   clients=[], messages=[])

"""The plain-batch tier cascade micro → compact → small → large under host emulation, one launch per
call (tests/emu/mt_emu_tiers.cpp: the engine and the kernel's own launch binding, csrc/mt_bind.h,
compiled for the host), and the documents the micro-tier tests are built from. Shared by
test_micro_tier_emulated.py (CPU) and test_gpu_micro_tier.py (the same batches on the device); lib() is
also what descend_cascade.py drives."""
import ctypes
import os

import numpy as np

from fluidframework_amd.native import CATCHUP_DTYPE, DOC_RESULT_DTYPE, LEAF_DTYPE, PROPSET_DTYPE, batch_struct
from mt_compare import _build_atomic, _p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libmt_emu_tiers.so")
MICRO, COMPACT, SMALL, LARGE = 0, 1, 2, 3
OK, E_CAPACITY, CKPT = 0, -3, -34  # header statuses (CKPT: fmt_mt::kCkptEscalate, stopped at a checkpoint)
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emu", "mt_emu_tiers.cpp")
        csrc = os.path.join(HERE, "..", "fluidframework_amd", "csrc")
        deps = [src, os.path.join(HERE, "emu", "emu_batch.h"), os.path.join(HERE, "emu", "emu_route.h"),
                os.path.join(HERE, "..", "include", "fmt.h")] + \
               [os.path.join(csrc, f) for f in ("mt_bind.h", "mt_engine.h", "wave.h", "huge_ckpt.h", "adjust.h", "mt_plan.h",
                                                "mt_route.h", "mt_route_words.h")]
        if not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
            _build_atomic(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas"], LIB_PATH, src)
        L = ctypes.CDLL(LIB_PATH)
        L.emu_micro_ckpt_words.restype = ctypes.c_uint32
        L.emu_micro_ckpt_layout.argtypes = [ctypes.POINTER(ctypes.c_uint32)] * 4
        L.emu_micro_caps.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_uint32)] * 2
        L.emu_descend_consts.argtypes = [ctypes.POINTER(ctypes.c_int32)]
        L.emu_tier_launch.argtypes = ([ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 +
                                      [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4)
        L.emu_mt_route.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_uint32]
        L.emu_bind_resumes.argtypes = [ctypes.c_int] * 6
        L.emu_bind_collect.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
        _lib = L
    return _lib


def caps(tier):
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib().emu_micro_caps(tier, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def route(batch, ckpt_slab=True, desc_slab=True, rounds=0, local_path=-1):
    """The route the runtime plans for `batch` (csrc/mt_route.h), read from the emulation library: a
    native.MtRouteResult. rounds: other than the build's kDescendRounds."""
    from fluidframework_amd.native import parse_mt_route

    b, keep = batch_struct(batch)
    w = np.zeros(1024, dtype=np.uint32)
    n = lib().emu_mt_route(ctypes.addressof(b), int(ckpt_slab), int(desc_slab), rounds, local_path, _p(w), len(w))
    del keep
    assert n > 0, "the plan refuses the batch"
    return parse_mt_route(w[:n])


def ckpt_layout():
    """(head words, rows of the leaf area, words of the text area, first word of the obliterate table)"""
    v = [ctypes.c_uint32() for _ in range(4)]
    lib().emu_micro_ckpt_layout(*[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


class Cascade:
    """A batch's result slabs and checkpoint slots, as the runtime holds them, and the tiers run so far."""

    def __init__(self, batch, cap_catchup=0, checkpoints=True):
        self.batch = batch
        n = self.n = batch.n_docs
        self.words = int(lib().emu_micro_ckpt_words())
        (self.cl, self.cc), self.cp = caps(SMALL), 32
        (self.bl, self.bc), self.bp = caps(LARGE), 1024
        self.hdr = np.zeros(n, dtype=DOC_RESULT_DTYPE)
        self.leaves = np.zeros(n * self.cl, dtype=LEAF_DTYPE)
        self.chars = np.zeros(n * self.cc, dtype="<u2")
        self.props = np.zeros(n * self.cp, dtype=PROPSET_DTYPE)
        self.big = None
        self.cap_catchup = cap_catchup
        self.cu = np.zeros(max(n * cap_catchup, 1), dtype=CATCHUP_DTYPE)
        self.ck = np.zeros((n, self.words), dtype=np.uint32) if checkpoints else None
        self.done_in = np.full(n, -1)  # the tier each document finished in

    def run(self, tier, only_escalated=None):
        """One tier: the micro tier over every document, any other over the documents the tier before
        it left (checkpointed or overflowed). Returns the statuses after it."""
        only = tier != MICRO if only_escalated is None else only_escalated
        docs = None  # the overflow list a launch before this one built: [0] = n, then ids in document order
        if only:
            ids = np.nonzero(np.isin(self.hdr["status"], (E_CAPACITY, CKPT)))[0]
            docs = np.concatenate(([len(ids)], ids)).astype(np.uint32)
        b, keep = batch_struct(self.batch)
        cu = _p(self.cu) if self.cap_catchup else None
        ck = _p(self.ck) if self.ck is not None else None
        pending = self.done_in < 0
        if tier == LARGE:
            if self.big is None:
                self.big = (np.zeros(self.n * self.bl, dtype=LEAF_DTYPE), np.zeros(self.n * self.bc, dtype="<u2"),
                            np.zeros(self.n * self.bp, dtype=PROPSET_DTYPE))
            lv, ch, pr = self.big
            small = (_p(self.leaves), _p(self.chars))
        else:
            lv, ch, pr, small = self.leaves, self.chars, self.props, (None, None)
        rc = lib().emu_tier_launch(ctypes.addressof(b), tier, _p(self.hdr), _p(lv), _p(ch), _p(pr), cu, self.cap_catchup, ck,
                                   _p(docs) if docs is not None else None, 0, None, None, small[0], small[1])
        del keep
        assert rc >= 0
        st = self.hdr["status"]
        self.done_in[pending & (st != CKPT) & (st != E_CAPACITY)] = tier
        return st.copy()

    def head(self, d):
        """Document d's checkpoint head: (next op, leaves, text units)."""
        h = self.ck[d]
        return int(h[0]) | (int(h[1]) << 32), int(h[2]), int(h[3])

    def poison_unwritten(self, d, value=0xA5A5A5A5):
        """Overwrite what the saver of document d's checkpoint did not write: the leaf rows at and
        above its live rows, the text words past its text, the obliterate table."""
        head, rows, char_words, ob_off = ckpt_layout()
        _, n, n_chars = self.head(d)
        live = (n + 63) // 64
        slot = self.ck[d]
        for f in range(5):
            for r in range(live, rows):
                o = head + (f * rows + r) * 64
                slot[o:o + 64] = value
        text = head + 5 * rows * 64
        slot[text + (n_chars + 1) // 2:text + char_words] = value
        slot[ob_off:] = value

    def doc(self, d, cap_catchup=False):
        """(header, leaves, chars, props) of document d, from the slabs of the tier it finished in."""
        if self.done_in[d] == LARGE:
            (lv, ch, pr), cl, cc, cp = self.big, self.bl, self.bc, self.bp
        else:
            lv, ch, pr, cl, cc, cp = self.leaves, self.chars, self.props, self.cl, self.cc, self.cp
        return (self.hdr[d], lv[d * cl:(d + 1) * cl], ch[d * cc:(d + 1) * cc], pr[d * cp:(d + 1) * cp])

    def catchup(self, d):
        n = int(self.hdr[d]["n_catchup"])
        return self.cu[d * self.cap_catchup:d * self.cap_catchup + n]


# ---- documents --------------------------------------------------------------------------------------

def _msg(seq, min_seq, contents):
    return {"clientId": "B", "sequenceNumber": seq, "referenceSequenceNumber": seq - 1,
            "minimumSequenceNumber": min_seq, "contents": contents}


GROW_OPS, SHRINK_OPS, REGROW_OPS = 40, 10, 12


def leaf_boundary_batch(orc, peaks=(126, 127, 128), seed=5):
    """One document per peak. Phase 1, minSeq pinned at 0 so nothing is merged or dropped: GROW_OPS
    two-char inserts at random positions (a split adds two leaves), then one-char inserts at position
    0 (one leaf each) up to exactly `peak` leaves. Phase 2: SHRINK_OPS inserts at 0 with minSeq
    following seq, so zamboni merges and drops leaves. Phase 3: REGROW_OPS random inserts with minSeq
    pinned again. Returns (batch, per document: the op index phase 1 ends at)."""
    from fluidframework_amd.streams import MergeTreeStreamBuilder

    def build(fill):
        rng = np.random.default_rng(seed)
        b = MergeTreeStreamBuilder()
        ends = []
        for k in range(len(peaks)):
            d = b.begin_doc()
            seq, length = 0, 0
            for _ in range(GROW_OPS):
                seq += 1
                d.add_message(_msg(seq, 0, {"type": 0, "pos1": int(rng.integers(0, length + 1)), "seg": "xy"}))
                length += 2
            for _ in range(fill[k]):
                seq += 1
                d.add_message(_msg(seq, 0, {"type": 0, "pos1": 0, "seg": "z"}))
                length += 1
            ends.append(seq)
            for _ in range(SHRINK_OPS):
                seq += 1
                d.add_message(_msg(seq, seq - 1, {"type": 0, "pos1": 0, "seg": "w"}))
                length += 1
            pinned = seq - 1
            for _ in range(REGROW_OPS):
                seq += 1
                d.add_message(_msg(seq, pinned, {"type": 0, "pos1": int(rng.integers(0, length + 1)), "seg": "uv"}))
                length += 2
        return b.finish(), ends

    probe, _ = build([0] * len(peaks))
    fill = []
    for k, peak in enumerate(peaks):  # leaves after the random inserts alone
        n0 = int(orc.mt_replay_batch(_prefix(probe, k, GROW_OPS), threads=1, cap_leaves=4096, cap_chars=1 << 16,
                                     cap_props=64)[1][0]["n_leaves"])
        assert n0 <= peak
        fill.append(peak - n0)
    return build(fill)


def _prefix(batch, d, n_ops):
    """Document d's first n_ops ops as a batch of one document."""
    from dataclasses import replace

    o0 = int(batch.doc_op_offsets[d])
    return replace(batch, ops=batch.ops[o0:o0 + n_ops].copy(), doc_op_offsets=np.array([0, n_ops], dtype=np.uint64),
                   doc_init=batch.doc_init[d:d + 1] if batch.doc_init is not None else None, clients=[], messages=[])


def prefix_leaves(orc, batch, d, n_ops):
    """(leaves, text units) of document d after its first n_ops ops, by the oracle."""
    h = orc.mt_replay_batch(_prefix(batch, d, n_ops), threads=1, cap_leaves=4096, cap_chars=1 << 16, cap_props=64)[1][0]
    assert int(h["status"]) == 0
    return int(h["n_leaves"]), int(h["n_chars"])


def text_boundary_batch(piece=48, n_ops=40):
    """One writer appending `piece` units per op with minSeq following seq: zamboni keeps the document
    at a few leaves of up to 256 units while its text passes the micro tier's 1024 units."""
    from fluidframework_amd.streams import MergeTreeStreamBuilder

    b = MergeTreeStreamBuilder()
    d = b.begin_doc()
    for k in range(n_ops):
        seq = k + 1
        d.add_message(_msg(seq, seq - 1, {"type": 0, "pos1": k * piece, "seg": "abcdefgh"[k % 8] * piece}))
    return b.finish()


def two_hop_batch():
    """Conflict-farm documents kept above 3000 units (their text passes 1024, 2048 and 6144), with
    insert props and the catch-up window's ops flagged."""
    from fluidframework_amd import workloads
    from fluidframework_amd.streams import flag_catchup

    batch = workloads.with_insert_props(workloads.conflict_farm(24, n_clients=8, ops_per_doc=2000, min_length=3000,
                                                                seed=33))
    flag_catchup(batch.ops, batch.doc_op_offsets)
    return batch

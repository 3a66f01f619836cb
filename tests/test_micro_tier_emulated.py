"""The micro tier (2 register rows, 1024 text units) and the checkpoints between neighbouring register
tiers, under host emulation vs the oracle (CPU only): the cascade micro → compact → small → large as
the runtime runs plain batches, one tier per call so that the checkpoint slots can be inspected and
scribbled over between two tiers."""
import numpy as np
import pytest

from fluidframework_amd import workloads
from micro_cascade import (CKPT, COMPACT, E_CAPACITY, GROW_OPS, LARGE, MICRO, OK, SMALL, Cascade, caps, leaf_boundary_batch,
                           prefix_leaves, text_boundary_batch, two_hop_batch)
from mt_compare import compare_doc


def _oracle(orc, batch, cap_catchup=0):
    cl, cc = caps(LARGE)
    return orc.mt_replay_batch(batch, threads=8, cap_leaves=cl, cap_chars=cc, cap_props=1024, cap_catchup=cap_catchup)


def _assert_equal(orc_out, cas, docs=None):
    rc, oh, ol, oc, op = orc_out[:5]
    assert rc == 0
    for d in range(cas.n) if docs is None else docs:
        diffs = compare_doc((oh[d], ol[d], oc[d], op[d]), cas.doc(d))
        assert not diffs, f"doc {d} (finished in tier {cas.done_in[d]}): {diffs[:5]}"


@pytest.fixture(scope="module")
def t1_batch():
    return workloads.conflict_farm(512, n_clients=8, ops_per_doc=2000, seed=1)


def test_t1_cascade_matches_oracle_and_takes_every_route(orc, t1_batch):
    """512 T1 documents through micro → compact → small: every document == oracle, and the batch
    exercises all three routes (measured with the emulated tiers when the thresholds were set: 43 %
    of the documents finish in the micro tier, 57 % stop there, 18 % stop in the compact tier too;
    these are conditions on the inputs)."""
    n = t1_batch.n_docs
    cas = Cascade(t1_batch)
    micro = cas.run(MICRO)
    assert set(np.unique(micro)) <= {OK, CKPT}
    print(f"micro tier: {np.mean(micro == OK):.3f} finish, {np.mean(micro == CKPT):.3f} stop")
    assert (micro == OK).sum() >= 0.25 * n
    assert (micro == CKPT).sum() >= 0.25 * n
    compact = cas.run(COMPACT)
    print(f"compact tier: {np.mean(compact == CKPT):.3f} stop")
    assert set(np.unique(compact)) <= {OK, CKPT}
    assert (compact == CKPT).sum() >= 0.05 * n
    small = cas.run(SMALL)
    assert (small == OK).all()
    assert {int(t) for t in np.unique(cas.done_in)} == {MICRO, COMPACT, SMALL}
    _assert_equal(_oracle(orc, t1_batch), cas)
    # a compact-only run of the same batch (what the cascade was before the micro tier) stops the same documents
    alone = Cascade(t1_batch)
    alone.run(COMPACT, only_escalated=False)
    assert np.array_equal(alone.hdr["status"] == CKPT, compact == CKPT)


def test_leaf_boundary_stops_before_the_overflowing_op(orc):
    """Documents that peak at exactly 126, 127 and 128 leaves, shrink by zamboni and grow again. An op
    adds at most two leaves, so the micro tier stops before the first op that finds more than 126:
    the 126-leaf document never stops; the other two stop with 127 leaves, before the op after the one
    that made them, and resume in the compact tier with the state the oracle has there."""
    batch, ends = leaf_boundary_batch(orc)
    exp = _oracle(orc, batch)
    oh = exp[1]
    for d, peak in enumerate((126, 127, 128)):  # the inputs are what they are meant to be
        assert prefix_leaves(orc, batch, d, ends[d])[0] == peak
        assert prefix_leaves(orc, batch, d, ends[d] + 10)[0] < peak - 30  # zamboni shrinks it
        assert int(oh[d]["n_leaves"]) < 120  # and it grows again, but not back to the boundary
    cas = Cascade(batch)
    micro = cas.run(MICRO)
    assert micro.tolist() == [OK, CKPT, CKPT]
    for d in (1, 2):
        nxt, n, n_chars = cas.head(d)
        at = nxt - int(batch.doc_op_offsets[d])
        first_127 = ends[d] - (d - 1)  # ops after which the document holds 127 leaves
        assert at == first_127 and n == 127
        assert (n, n_chars) == prefix_leaves(orc, batch, d, at)
        assert prefix_leaves(orc, batch, d, at - 1)[0] == 126  # one op earlier it was not yet due
    compact = cas.run(COMPACT)
    assert (compact == OK).all() and cas.done_in.tolist() == [MICRO, COMPACT, COMPACT]
    _assert_equal(exp, cas)


def test_text_boundary_stops_before_the_insert_that_outgrows_the_text(orc):
    """A document of a handful of leaves whose text passes 1024 units: the micro tier stops before the
    insert that would not fit, the compact tier resumes it."""
    batch = text_boundary_batch(piece=48, n_ops=40)
    exp = _oracle(orc, batch)
    assert int(exp[1][0]["n_chars"]) == 48 * 40 and int(exp[1][0]["n_leaves"]) < 100
    cas = Cascade(batch)
    assert cas.run(MICRO).tolist() == [CKPT]
    nxt, n, n_chars = cas.head(0)
    assert n < 100 and n_chars == 48 * 21 and nxt == 21  # 21 × 48 = 1008 fit, the 22nd insert does not
    assert cas.run(COMPACT).tolist() == [OK]
    _assert_equal(exp, cas)


def test_two_hops_through_one_slot_keep_catchup_and_props(orc):
    """Documents that grow through micro → compact → small → large: the compact tier saves into the
    slot it resumed from; catch-up ranges recorded before and after each checkpoint and the prop sets
    equal the oracle's."""
    batch = two_hop_batch()
    exp = _oracle(orc, batch, cap_catchup=4096)
    ocu = exp[6]
    cas = Cascade(batch, cap_catchup=4096)
    stops = np.zeros(batch.n_docs, dtype=int)
    for tier in (MICRO, COMPACT, SMALL):
        st = cas.run(tier)
        assert set(np.unique(st)) <= {OK, CKPT}, np.unique(st)
        stops += st == CKPT
    assert (stops == 3).sum() >= 2, stops  # through every tier by checkpoint
    assert (cas.run(LARGE) == OK).all()
    assert (cas.done_in == LARGE).sum() == (stops == 3).sum()
    _assert_equal(exp, cas)
    assert exp[1]["n_catchup"].max() > 0
    for d in range(batch.n_docs):
        n = int(exp[1][d]["n_catchup"])
        assert int(cas.hdr[d]["n_catchup"]) == n and np.array_equal(cas.catchup(d), ocu[d][:n]), d


def test_resume_reads_only_what_the_saver_wrote(orc, t1_batch):
    """A checkpoint holds the live rows and the live text only. With everything else in the slot
    overwritten after each save, the next tier still resumes to the oracle's state."""
    from dataclasses import replace

    k = 96
    o1 = int(t1_batch.doc_op_offsets[k])
    batch = replace(t1_batch, ops=t1_batch.ops[:o1], doc_op_offsets=t1_batch.doc_op_offsets[:k + 1],
                    doc_init=t1_batch.doc_init[:k] if t1_batch.doc_init is not None else None, clients=[], messages=[])
    cas = Cascade(batch)
    cas.ck[:] = 0xA5A5A5A5  # (a fresh allocation holds anything)
    micro = cas.run(MICRO)
    stopped = np.nonzero(micro == CKPT)[0]
    assert len(stopped) >= 10
    assert any(cas.head(d)[1] <= 128 for d in stopped)  # two live rows of the slot's four
    for d in stopped:
        cas.poison_unwritten(d)
    compact = cas.run(COMPACT)
    again = np.nonzero(compact == CKPT)[0]
    assert len(again) >= 3
    for d in again:
        cas.poison_unwritten(d)
    assert (cas.run(SMALL) == OK).all()
    _assert_equal(_oracle(orc, batch), cas)


def test_cascade_without_checkpoints_restarts_in_the_next_tier(orc):
    """No checkpoint slab (the allocation failed): a document that outgrows a tier reports
    FMT_E_CAPACITY and the next tier replays it from its first op."""
    batch = workloads.conflict_farm(48, n_clients=8, ops_per_doc=2000, seed=3)
    cas = Cascade(batch, checkpoints=False)
    micro = cas.run(MICRO)
    assert set(np.unique(micro)) == {OK, E_CAPACITY}
    compact = cas.run(COMPACT)
    assert set(np.unique(compact)) <= {OK, E_CAPACITY} and (compact == E_CAPACITY).any()
    assert (cas.run(SMALL) == OK).all()
    _assert_equal(_oracle(orc, batch), cas)

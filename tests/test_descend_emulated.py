"""Stepping down a tier (fmt_mt::kCkptDescend: a small-tier document that shrank to half of the compact
tier stops at a checkpoint the compact tier resumes), under host emulation vs the oracle (CPU
only): the rounds of launchMergeTree's plain cascade, one launch per call so that lists and checkpoint
slots can be inspected and scribbled over between two launches."""
import numpy as np
import pytest

from descend_cascade import DESC, ROUNDS, DescendCascade, consts, grow_then_shrink_batch, held_by_last_round
from fluidframework_amd import workloads
from micro_cascade import CKPT, COMPACT, E_CAPACITY, LARGE, MICRO, OK, SMALL, Cascade, caps, prefix_leaves, two_hop_batch
from mt_compare import compare_doc

_, D4, C4, MIN_OPS = consts()


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


def test_thresholds_leave_room_to_double():
    """Half of the tier below: a document that stepped down must double before the upward check
    (n + 2 > rows × 64, text past the tier's) sends it up again."""
    assert 2 * D4 <= caps(COMPACT)[0] and 2 * C4 <= caps(COMPACT)[1]


def test_t1_rounds_match_oracle_and_take_every_route(orc, t1_batch):
    """512 T1 documents through the rounds: every document == oracle on every compared field, and
    every route is taken: small → compact, up again after stepping down, and held by the last round
    (a document that would step down once more if there were another round)."""
    cas = DescendCascade(t1_batch)
    esc = cas.rounds()
    assert int(esc[0]) == 0 and (cas.hdr["status"] == OK).all()
    print(f"ops per tier {cas.ops_in}, routes {cas.routes}, hops per document {np.bincount(cas.hops).tolist()}")
    assert cas.routes["small->compact"] >= 1
    assert cas.up_after_down.any()
    assert cas.downs.max() <= ROUNDS - 1
    assert len(held_by_last_round(t1_batch)) >= 1
    _assert_equal(_oracle(orc, t1_batch), cas)


def test_switch_off_equals_the_upward_cascade(t1_batch):
    """With the switch off the launches leave what micro_cascade.Cascade (the cascade before stepping
    down) leaves: statuses, checkpoint heads and outputs, after every tier."""
    k = 128
    from dataclasses import replace

    o1 = int(t1_batch.doc_op_offsets[k])
    batch = replace(t1_batch, ops=t1_batch.ops[:o1], doc_op_offsets=t1_batch.doc_op_offsets[:k + 1],
                    doc_init=t1_batch.doc_init[:k] if t1_batch.doc_init is not None else None, clients=[], messages=[])
    old, new = Cascade(batch), DescendCascade(batch)
    lists = [None, new.new_list(), new.new_list(), new.new_list()]
    for tier in (MICRO, COMPACT, SMALL):
        st_old = old.run(tier)
        new.launch(tier, lists[tier], descend=False, up=lists[tier + 1])
        assert np.array_equal(st_old, new.hdr["status"]), tier
        assert np.array_equal(old.hdr, new.hdr) and np.array_equal(old.ck, new.ck), tier
        assert np.array_equal(old.leaves, new.leaves) and np.array_equal(old.chars, new.chars), tier
        assert np.array_equal(old.props, new.props), tier
    assert (new.hdr["status"] == OK).all()


def test_without_checkpoints_nothing_steps_down(orc):
    batch = workloads.conflict_farm(48, n_clients=8, ops_per_doc=2000, seed=3)
    cas = DescendCascade(batch, checkpoints=False)
    up1, up2, down = cas.new_list(), cas.new_list(), cas.new_list()
    st = cas.launch(MICRO, None, True, up=up1)
    assert set(np.unique(st)) == {OK, E_CAPACITY}
    st = cas.launch(COMPACT, up1, True, up=up2, down=down)
    assert set(np.unique(st)) <= {OK, E_CAPACITY} and (st == E_CAPACITY).any()
    st = cas.launch(SMALL, up2, True, up=cas.new_list(), down=down)
    assert (st == OK).all() and int(down[0]) == 0
    _assert_equal(_oracle(orc, batch), cas)


def test_stops_at_the_op_that_reaches_the_threshold(orc):
    """Hand-built documents that grow past 254 leaves one leaf an op and then shrink 15 leaves an op.
    Document 0 passes through exactly D4 leaves, document 1 through D4 + 1 and then D4 - 14: each stops
    in the small tier after the first op that leaves at most D4, not one op earlier. The compact tier
    resumes at the next op; the documents grow again and go up once more with 255 leaves."""
    peaks = (2 * D4 + 37, 2 * D4 + 38)
    batch, mids = grow_then_shrink_batch(peaks=peaks, tail_ops=280)
    exp = _oracle(orc, batch)
    offs = batch.doc_op_offsets
    first = []
    for d, before in enumerate((D4 + 15, D4 + 1)):
        k = next(k for k in range(mids[d], mids[d] + 30) if prefix_leaves(orc, batch, d, k)[0] <= D4)
        assert prefix_leaves(orc, batch, d, k - 1)[0] == before  # the inputs are what they are meant to be
        assert prefix_leaves(orc, batch, d, k)[0] == (D4 if d == 0 else D4 - 14)
        first.append(k)
    cas = DescendCascade(batch)
    up1, up2, up3, down = (cas.new_list() for _ in range(4))
    assert (cas.launch(MICRO, None, True, up=up1) == CKPT).all()
    assert (cas.launch(COMPACT, up1, True, up=up2) == CKPT).all()  # every peak is past 254
    st = cas.launch(SMALL, up2, True, up=up3, down=down)
    assert (st == DESC).all() and int(down[0]) == 2 and int(up3[0]) == 0
    for d in (0, 1):
        nxt, n, n_chars = cas.head(d)
        assert nxt - int(offs[d]) == first[d] and (n, n_chars) == prefix_leaves(orc, batch, d, first[d])
    assert cas.head(0)[1] == D4 and cas.head(1)[1] == D4 - 14
    up4 = cas.new_list()
    assert (cas.launch(COMPACT, down, False, up=up4) == CKPT).all()
    for d in (0, 1):
        assert cas.head(d)[1] == caps(COMPACT)[0] - 1  # 255 leaves: doubled since the step down
    assert (cas.launch(SMALL, up4, False, up=up3) == OK).all() and int(up3[0]) == 0
    _assert_equal(exp, cas)


def test_text_over_the_margin_keeps_a_document_up(orc):
    """Leaves under D4 but text over the compact tier's margin: the small tier keeps the document."""
    batch, mids = grow_then_shrink_batch(peaks=(280,), piece=12, keep=100, tail_ops=200)
    n, chars = prefix_leaves(orc, batch, 0, mids[0] + 14)
    assert n <= D4 and chars > C4 and chars <= caps(COMPACT)[1]
    cas = DescendCascade(batch)
    up1, up2, down = cas.new_list(), cas.new_list(), cas.new_list()
    assert cas.launch(MICRO, None, True, up=up1).tolist() == [CKPT]
    assert cas.launch(COMPACT, up1, True, up=up2).tolist() == [CKPT]
    assert cas.launch(SMALL, up2, True, up=cas.new_list(), down=down).tolist() == [OK] and int(down[0]) == 0
    _assert_equal(_oracle(orc, batch), cas)
    # the same document with one-unit pieces (text under the margin) does step down
    small_text, _ = grow_then_shrink_batch(peaks=(280,), piece=1, keep=100, tail_ops=200)
    cas = DescendCascade(small_text)
    up1, up2, down = cas.new_list(), cas.new_list(), cas.new_list()
    cas.launch(MICRO, None, True, up=up1)
    cas.launch(COMPACT, up1, True, up=up2)
    assert cas.launch(SMALL, up2, True, up=cas.new_list(), down=down).tolist() == [DESC]


def test_too_few_ops_left_keeps_a_document_up(orc):
    batch, mids = grow_then_shrink_batch(peaks=(300,), tail_ops=MIN_OPS)  # reaches D4 with fewer than MIN_OPS left
    cas = DescendCascade(batch)
    up1, up2, down = cas.new_list(), cas.new_list(), cas.new_list()
    cas.launch(MICRO, None, True, up=up1)
    cas.launch(COMPACT, up1, True, up=up2)
    assert cas.launch(SMALL, up2, True, up=cas.new_list(), down=down).tolist() == [OK] and int(down[0]) == 0
    _assert_equal(_oracle(orc, batch), cas)


def test_downward_resume_reads_only_what_the_saver_wrote(orc, t1_batch):
    """As test_resume_reads_only_what_the_saver_wrote for the upward hop: everything in the slot that a
    save did not write is overwritten before the next launch, at every hop of every round."""
    from dataclasses import replace

    k = 96
    o1 = int(t1_batch.doc_op_offsets[k])
    batch = replace(t1_batch, ops=t1_batch.ops[:o1], doc_op_offsets=t1_batch.doc_op_offsets[:k + 1],
                    doc_init=t1_batch.doc_init[:k] if t1_batch.doc_init is not None else None, clients=[], messages=[])
    cas = DescendCascade(batch)
    cas.ck[:] = 0xA5A5A5A5
    poisoned_down = 0
    launch = cas.launch

    def poisoning(tier, docs=None, descend=False, up=None, down=None):
        nonlocal poisoned_down
        st = launch(tier, docs, descend, up, down)
        ids = np.arange(cas.n) if docs is None else docs[1:1 + int(docs[0])].astype(int)
        for d, s in zip(ids, st):
            if s in (CKPT, DESC):
                cas.poison_unwritten(d)
                poisoned_down += s == DESC
        return st

    cas.launch = poisoning
    cas.rounds()
    assert poisoned_down >= 1
    assert (cas.hdr["status"] == OK).all()
    _assert_equal(_oracle(orc, batch), cas)


def test_catchup_ranges_across_a_downward_hop(orc):
    """Flagged ops and insert props as in micro_cascade.two_hop_batch, on conflict-farm documents without
    its 3000-unit floor (text kept over 3000 units never fits half of the compact tier, so those
    documents cannot step down): catch-up ranges recorded before and after downward hops, and the prop
    sets, equal the oracle's. two_hop_batch itself goes through the rounds too, unchanged by them."""
    from fluidframework_amd.streams import flag_catchup

    for batch in (workloads.with_insert_props(workloads.conflict_farm(64, n_clients=8, ops_per_doc=2000, seed=33)),
                  two_hop_batch()):
        flag_catchup(batch.ops, batch.doc_op_offsets)
        _catchup_case(orc, batch, expect_down=batch.n_docs == 64)


def _catchup_case(orc, batch, expect_down):
    exp = _oracle(orc, batch, cap_catchup=4096)
    ocu = exp[6]
    cas = DescendCascade(batch, cap_catchup=4096)
    esc = cas.rounds()
    print(f"routes {cas.routes}, for the large tier {int(esc[0])}")
    assert (cas.downs.sum() >= 1) == expect_down
    if int(esc[0]) > 0:
        assert (cas.launch(LARGE, esc, False) == OK).all()
    _assert_equal(exp, cas)
    assert exp[1]["n_catchup"].max() > 0
    down = np.nonzero(cas.downs > 0)[0]
    assert not expect_down or any(int(exp[1][d]["n_catchup"]) > 0 for d in down)
    for d in range(batch.n_docs):
        n = int(exp[1][d]["n_catchup"])
        assert int(cas.hdr[d]["n_catchup"]) == n and np.array_equal(cas.catchup(d), ocu[d][:n]), d

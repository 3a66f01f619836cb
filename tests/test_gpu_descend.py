"""Stepping down a tier on the device: the batches of test_descend_emulated.py through Engine.mt_load /
mt_run (plain batches with checkpoints run the rounds of launchMergeTree), headers, leaves, text and
prop sets against the oracle's, and a second run on the loaded batch (lists and counters are reset)."""
import numpy as np
import pytest

from descend_cascade import grow_then_shrink_batch, replicate
from fluidframework_amd import native, workloads
from mt_compare import compare_doc

pytestmark = pytest.mark.gpu

HEADER_FIELDS = ["status", "cur_seq", "min_seq", "n_leaves", "n_chars", "n_blocks", "depth", "visible_len", "n_catchup"]


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _run(engine):
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    return hdrs, [engine.mt_doc(d, hdrs[d]) for d in range(len(hdrs))]


def _check(orc, engine, batch, ref=None):
    """ref: the one-document batch that `batch` repeats (the oracle replays only that)."""
    engine.mt_load(batch)
    hdrs, docs = _run(engine)
    assert (hdrs["status"] == 0).all(), np.unique(hdrs["status"])
    rc, oh, ol, oc, op = orc.mt_replay_batch(ref or batch, threads=16, cap_leaves=8192, cap_chars=1 << 17, cap_props=1024)[:5]
    assert rc == 0
    for d in range(batch.n_docs):
        o = d if ref is None else 0
        for f in HEADER_FIELDS:
            assert hdrs[f][d] == oh[f][o], (d, f)
        lv, ch, pr = docs[d]
        assert not compare_doc((oh[o], ol[o], oc[o], op[o]), (hdrs[d], lv, ch, pr)), d
    hdrs2, docs2 = _run(engine)  # the same loaded batch again
    assert np.array_equal(hdrs, hdrs2)
    for a, b in zip(docs, docs2):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_t1_documents_through_the_rounds(orc, engine):
    _check(orc, engine, workloads.conflict_farm(512, n_clients=8, ops_per_doc=2000, seed=1))


def test_grow_then_shrink_documents(orc, engine):
    one, _ = grow_then_shrink_batch(peaks=(293,), tail_ops=280)
    _check(orc, engine, replicate(one, 300), ref=one)

"""The micro tier on the device: the batches of test_micro_tier_emulated.py through Engine.mt_load /
mt_run (plain batches start in the micro tier; its overflow goes on in the compact, small and large
tiers from checkpoints), headers and state digests against the oracle's."""
import numpy as np
import pytest

from fluidframework_amd import native, workloads
from micro_cascade import leaf_boundary_batch, text_boundary_batch, two_hop_batch
from mt_compare import compare_doc

pytestmark = pytest.mark.gpu

HEADER_FIELDS = ["status", "cur_seq", "min_seq", "n_leaves", "n_chars", "n_blocks", "depth", "visible_len", "n_catchup"]


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _check(orc, engine, batch, full_docs=()):
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    assert (hdrs["status"] == 0).all(), np.unique(hdrs["status"])
    got = engine.mt_digests()
    rc, exp, st, _ = orc.mt_replay_digest(batch, threads=16)
    assert rc == 0
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, f"{len(bad)} documents differ, first {bad[:8].tolist()}"
    cl, cc, cp = native.capacity()
    out = orc.mt_replay_batch(batch, threads=16, cap_leaves=8192, cap_chars=1 << 17, cap_props=1024, cap_catchup=4096)
    rc, oh, ol, oc, op = out[:5]
    assert rc == 0
    for f in HEADER_FIELDS:
        assert np.array_equal(hdrs[f], oh[f]), f
    for d in full_docs:
        lv, ch, pr = engine.mt_doc(d, hdrs[d])
        assert not compare_doc((oh[d], ol[d], oc[d], op[d]), (hdrs[d], lv, ch, pr)), d
    return hdrs, out


def test_t1_documents_through_the_cascade(orc, engine):
    batch = workloads.conflict_farm(512, n_clients=8, ops_per_doc=2000, seed=1)
    hdrs, _ = _check(orc, engine, batch, full_docs=range(0, 512, 37))
    # documents on every route: at most 126 leaves at the end, and past the compact tier's 256
    assert (hdrs["n_leaves"] <= 126).any() and (hdrs["n_leaves"] > 256).any()


def test_leaf_and_text_boundaries(orc, engine):
    batch, _ = leaf_boundary_batch(orc)
    _check(orc, engine, batch, full_docs=range(3))
    _check(orc, engine, text_boundary_batch(piece=48, n_ops=40), full_docs=[0])


def test_two_hops_through_one_slot(orc, engine):
    batch = two_hop_batch()
    hdrs, out = _check(orc, engine, batch, full_docs=range(batch.n_docs))
    ocu = out[6]
    for d in range(batch.n_docs):
        n = int(hdrs[d]["n_catchup"])
        assert np.array_equal(engine.mt_catchup(d, hdrs[d]), ocu[d][:n]), d

"""The planned route on the device (csrc/mt_route.h through Engine.mt_load / mt_run): the batches of
route_cases.py, one document finishing in each tier of its route and one going on to the large tier,
headers, leaves, text and prop sets against the host emulation executing the same exported route
(route_cases.run_route; test_mt_route.py checks on the CPU that each document finishes in the intended
tier), and fmt_stats.launches against the route's nominalLaunches."""
import numpy as np
import pytest

from descend_cascade import grow_then_shrink_batch
from fluidframework_amd import native
from mt_compare import compare_doc
from mt_compare import emu_replay, emu_replay_local
from route_cases import huge_batch, plain_batch, run_route, variant_batch

pytestmark = pytest.mark.gpu

HEADER_FIELDS = ["status", "cur_seq", "min_seq", "n_leaves", "n_chars", "n_blocks", "depth", "visible_len", "n_catchup"]


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _check(engine, batch, skip=()):
    emu, large_ran = run_route(batch, skip)
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    assert (hdrs["status"] == 0).all(), np.unique(hdrs["status"])
    for d in range(batch.n_docs):
        if d in skip:
            continue
        eh, el, ec, ep = emu.doc(d)
        for f in HEADER_FIELDS:
            assert hdrs[f][d] == eh[f], (d, f)
        lv, ch, pr = engine.mt_doc(d, hdrs[d])
        assert not compare_doc((eh, el, ec, ep), (hdrs[d], lv, ch, pr)), d
    assert engine.stats().launches == native.mt_route(batch).nominal_launches[(large_ran, False)]
    return emu


def test_plain_route_one_document_per_tier(engine):
    emu = _check(engine, plain_batch())
    assert emu.done_in.tolist() == [0, 1, 2, 3]


def test_plain_route_with_descent(engine):
    batch, _ = grow_then_shrink_batch(peaks=(100, 200, 293, 300), tail_ops=280)
    emu = _check(engine, batch)
    assert emu.routes["small->compact"] >= 1


def test_plain_route_from_the_callers_list(engine):
    """A summary-loaded document past the large tier runs in the huge tier: the register tiers take the others
    from the caller's list (MtListKind::kCaller)."""
    batch, huge = huge_batch()
    emu = _check(engine, batch, skip=(huge,))
    assert emu.done_in.tolist() == [0, 1, 2, 3, -1]
    assert int(engine.mt_headers()["n_leaves"][huge]) > 2048


def _check_variant(engine, batch, emu, large_ran=True):
    """emu: (headers, leaves, chars, props) of the emulation executing the batch's route and its large pass."""
    eh, el, ec, ep = emu[:4]
    assert (eh["status"] == 0).all()
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    for d in range(batch.n_docs):
        for f in HEADER_FIELDS:
            assert hdrs[f][d] == eh[f][d], (d, f)
        lv, ch, pr = engine.mt_doc(d, hdrs[d])
        assert not compare_doc((eh[d], el[d], ec[d], ep[d]), (hdrs[d], lv, ch, pr)), d
    assert engine.stats().launches == native.mt_route(batch).nominal_launches[(large_ran, False)]
    return hdrs


def test_obliterate_route(engine):
    batch = variant_batch("ob")
    _check_variant(engine, batch, emu_replay(batch, large=4))


def test_remove_order_route(engine):
    batch = variant_batch("rm")
    emu = emu_replay(batch, large=4, cap_rm=512)
    hdrs = _check_variant(engine, batch, emu)
    for d in range(batch.n_docs):
        n = int(emu[0]["n_rm_order"][d])  # (a lone remove adds no later stamp: the slabs may be empty)
        assert int(hdrs["n_rm_order"][d]) == n and np.array_equal(engine.mt_remove_order(d, hdrs[d]), emu[4][d][:n]), d


def test_local_route(engine):
    batch = variant_batch("local")
    _check_variant(engine, batch, emu_replay_local(batch))


def test_adjust_route(engine):
    batch = variant_batch("adjust")
    _check_variant(engine, batch, emu_replay(batch, large=4))

"""Merge-tree feature pairs on the device against the oracle's replay of the same batch: the batches
and checks of test_feature_pairs_emulated.py (feature_pairs.py) through Engine.mt_load / mt_run, so
the compiled instantiations themselves run — small and large Doc<true, ., Rm, Adj>, large Doc<true, G,
true>, hugeDocKernel<Adj, Rm> (resumed from the large tier's checkpoint and loaded at its first op).
"""
import pytest

import feature_pairs as fp
from fluidframework_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = native.Engine(0)
    yield eng
    eng.close()


def _run(engine, batch):
    engine.mt_load(batch)
    engine.mt_run()
    return engine.mt_headers(raise_on_failed_docs=False)


def _check_all(engine, o, finals=None, rm=False, cu=False):
    """Every document of the loaded batch against the oracle (fp.check_doc)."""
    batch = o.batch
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    adjust = batch.adjusts is not None
    if adjust:
        engine.mt_summarize_legacy(batch.keys, batch.values)
    for d in range(batch.n_docs):
        h = hdrs[d]
        assert int(h["status"]) == 0, (d, int(h["status"]), int(h["fail_seq"]))
        lv, ch, pr = engine.mt_doc(d, h)
        fp.check_doc(o, d, (h, lv, ch, pr), nums=engine.mt_numbers(d) if adjust else None,
                     legacy=engine.mt_legacy_props(d, h) if adjust else None,
                     engine_summary=engine.mt_summary(d) if adjust else None,
                     rm=engine.mt_remove_order(d, h) if rm else None, cu=engine.mt_catchup(d, h) if cu else None,
                     final=finals[d] if finals else None)
    return hdrs


def _state(engine, n_docs):
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    return hdrs, [engine.mt_doc(d, hdrs[d]) for d in range(n_docs)]


def _second_run_is_identical(engine, batch):
    """mt_run() again on the loaded batch: identical headers and documents (slabs and counters reset)."""
    h1, d1 = _state(engine, batch.n_docs)
    engine.mt_run()
    h2, d2 = _state(engine, batch.n_docs)
    assert h1.tobytes() == h2.tobytes()
    for a, b in zip(d1, d2):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("narrow", [True, False])
def test_adjust_x_remove_order_on_gpu(orc, engine, narrow):
    batch, finals = fp.adjust_rm_batch(narrow)
    o = fp.Oracle(orc, batch, fp.LARGE_CAPS)
    nums, multi = fp.live_adjust_rm(o)
    assert nums > 0 and multi > 0, (nums, multi)
    _run(engine, batch)
    _check_all(engine, o, finals, rm=True)
    if not narrow:
        assert engine.stats().launches >= 2  # (the large tier ran: Doc<true, G, true, Adj>)
        _second_run_is_identical(engine, batch)
        _check_all(engine, o, finals, rm=True)


@pytest.mark.parametrize("long", [False, True])
def test_adjust_x_obliterate_on_gpu(orc, engine, long):
    batch, _ = fp.adjust_ob_batch(long)
    o = fp.Oracle(orc, batch, fp.LARGE_CAPS)
    nums, hit = fp.live_adjust_ob(o)
    assert nums > 0 and hit > 0, (nums, hit)
    _run(engine, batch)
    _check_all(engine, o)
    if long:
        _second_run_is_identical(engine, batch)
        _check_all(engine, o)


def test_obliterate_x_remove_order_past_small_tier_on_gpu(orc, engine):
    batch, _ = fp.ob_rm_long_batch()
    o = fp.Oracle(orc, batch, fp.LARGE_CAPS)
    assert fp.live_both_stamps(o) > 0
    assert int((o.h["n_chars"] > 6144).sum()) >= 15  # end past the small tier's text (SmallTier::kCapChars)
    _run(engine, batch)
    assert engine.stats().launches >= 2  # (the large tier ran: Doc<true, G, true>)
    _check_all(engine, o, rm=True)
    _second_run_is_identical(engine, batch)
    _check_all(engine, o, rm=True)


@pytest.mark.parametrize("kind", ["adjust", "rm"])
def test_catchup_pairs_on_gpu(orc, engine, kind):
    batch, finals = fp.catchup_pair_batches(only=kind)[kind]
    o = fp.Oracle(orc, batch, fp.LARGE_CAPS, cap_catchup=fp.CAP_CU)
    fp.assert_catchup_live(o, kind)
    _run(engine, batch)
    _check_all(engine, o, finals, rm=kind == "rm", cu=True)
    _second_run_is_identical(engine, batch)
    _check_all(engine, o, finals, rm=kind == "rm", cu=True)


GROWTH = {
    "adjust_rm": (fp.adjust_rm_growth, True, False),
    "ob_rm": (fp.ob_rm_growth, True, False),
    "ob_adjust": (fp.ob_adjust_growth, False, False),
    "catchup_adjust": (lambda: fp.catchup_pair_batches(only="adjust_growth")["adjust_growth"], False, True),
    "catchup_rm": (lambda: fp.catchup_pair_batches(only="rm_growth")["rm_growth"], True, True),
}


@pytest.mark.parametrize("kind", list(GROWTH))
def test_pair_resumes_in_the_huge_tier_on_gpu(orc, engine, kind):
    build, rm, cu = GROWTH[kind]
    batch = build()
    o = fp.Oracle(orc, batch, fp.HUGE_CAPS, cap_catchup=fp.CAP_CU if cu else 0, index=True)
    fp.assert_growth_live(o, kind)
    _run(engine, batch)
    _check_all(engine, o, rm=rm, cu=cu)
    at = int(engine.huge_profile(0)["resumed_at"])
    assert at > 0
    fp.assert_carried(o, kind, at)


@pytest.mark.parametrize("kind", ["adjust_rm", "ob_rm"])
def test_pair_loaded_in_the_huge_tier_on_gpu(orc, engine, kind):
    """A summary-loaded document over the large tier at load (131,600 units in 200 segments): the
    load-time huge path, hugeDocKernel<Adj, true> from its first message."""
    batch = fp.load_time_huge(kind)
    sd = batch.snapshots[0]
    assert sd["loaded"] and int(batch.snapshot_segs["len"][: int(sd["n_header"])].sum()) > 131071
    o = fp.Oracle(orc, batch, fp.HUGE_CAPS, index=True)
    if kind == "adjust_rm":
        nums, multi = fp.live_adjust_rm(o)
        assert nums > 0 and multi > 0, (nums, multi)
    else:
        assert fp.live_both_stamps(o) > 0
    _run(engine, batch)
    # (set up for the huge tier at load: no large-tier pass and no pass over grown documents, which a
    # restart after the small and large tiers' -3 would add)
    assert engine.stats().launches == 1
    _check_all(engine, o, rm=True)
    assert int(engine.huge_profile(0)["resumed_at"]) == 0

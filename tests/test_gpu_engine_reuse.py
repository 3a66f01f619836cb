"""Engine reuse on the device: does a batch give the same bytes on an engine that has just served
another batch as on a fresh one? The stations and the tour are tests/engine_reuse.py's (held to their
rows by test_engine_reuse_stations.py).

  fresh      each station on its own fresh Engine, everything fetched against the oracle with the
             helpers of the feature's own suite (feature_pairs.check_doc, mt_compare.compare_doc, the
             map and summary byte comparisons); the fetched bytes are kept
  tour       one engine walks a closed tour holding every ordered pair of stations; after every step
             the same fetches against the oracle again, then bit-equal to the kept fresh ones; every
             fifth step runs twice before it fetches
  failed load, call order, shared scratch: directed tests below

Run with `pytest -m gpu`.
"""
from dataclasses import replace

import numpy as np
import pytest

import engine_reuse as er
from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_DATA, FMT_E_USAGE

pytestmark = pytest.mark.gpu

NAMES = [s.name for s in er.STATIONS]
SEGMENTS = er.tour_segments(len(er.STATIONS), 4 * len(er.STATIONS))  # about 8 steps each: a few seconds at the most
_fresh = {}


def fresh(orc, name):
    """The kept fetches of station `name` from a fresh engine of its own, checked against the oracle."""
    if name not in _fresh:
        s = er.BY_NAME[name]
        e = native.Engine(0)
        try:
            er.run_station(e, s)
            got = er.fetch_station(e, s)
            if s.family == "mt":
                er.check_mt_full(orc, e, s, got)
            else:
                er.check_map(orc, s, got)
        finally:
            e.close()
        _fresh[name] = got
    return _fresh[name]


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def visit(orc, engine, s, twice=False):
    """One tour step: load and run s, fetch, compare with the oracle directly, then bit-equal to fresh."""
    er.run_station(engine, s, twice=twice)
    got = er.fetch_station(engine, s)
    er.check_station(orc, s, got)
    assert er.same(got, fresh(orc, s.name)) == [], s.name
    return got


@pytest.mark.parametrize("name", NAMES)
def test_fresh_reference(orc, name):
    fresh(orc, name)


@pytest.mark.parametrize("k", range(len(SEGMENTS)))
def test_tour_segment(orc, engine, k):
    """Segment k of the tour on the module's engine: the station before its first step is replayed
    first, so every pair of the segment is a real succession whichever tests ran before."""
    seg = SEGMENTS[k]
    step0 = sum(len(x) - 1 for x in SEGMENTS[:k])
    visit(orc, engine, er.STATIONS[seg[0]])
    for i, v in enumerate(seg[1:]):
        visit(orc, engine, er.STATIONS[v], twice=(step0 + i) % 5 == 4)


def _raises(code, f, *a):
    with pytest.raises(native.EngineError) as ei:
        f(*a)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def test_failed_load_keeps_the_previous_merge_tree_batch(orc, engine):
    """fmt_mt_load's comment: mtPlan is "replaced only by a batch that passes validation". After three
    stations, a load with descending doc_op_offsets and one with a value id an annotate-adjust batch may
    not hold return their codes; the previous station's fetches still match, without a run and after one."""
    bad = er.bad_mt_batches()
    for name in ("rm_order", "local"):
        visit(orc, engine, er.BY_NAME[name])
    s = er.BY_NAME["catchup_rm_order"]
    visit(orc, engine, s)
    for which, code in (("offsets", FMT_E_USAGE), ("value_id", FMT_E_DATA)):
        _raises(code, engine.mt_load, bad[which])
        got = er.fetch_station(engine, s)
        er.check_station(orc, s, got)
        # (the stats read before the fetches are the last summarize call's here, not a run's)
        assert [k for k in er.same(got, fresh(orc, s.name)) if k != "stats_run"] == []
        engine.mt_run()
        got = er.fetch_station(engine, s)
        assert er.same(got, fresh(orc, s.name)) == []


def test_failed_load_keeps_the_previous_map_batch(orc, engine):
    """The map loads validate offsets and seq order on the host (a key id >= key_bound is found by the
    run on the device, so such a batch does load): descending offsets and a seq of 0 return their codes,
    and the previous station's fetches still match, without a run and after one."""
    for name in ("map_tiered_keys", "map_summary"):
        visit(orc, engine, er.BY_NAME[name])
    s = er.BY_NAME["map_pending"]
    visit(orc, engine, s)
    b = s.batch
    offs = np.asarray(b.doc_op_offsets).copy()
    offs[1], offs[2] = offs[2], offs[1]
    ops = b.ops.copy()
    ops["seq"][0] = 0
    for batch, code in ((replace(b, doc_op_offsets=offs), FMT_E_USAGE), (replace(b, ops=ops), FMT_E_DATA)):
        _raises(code, engine.map_load_sparse, batch)
        _raises(code, engine.map_load, batch)
        got = er.fetch_station(engine, s)
        er.check_station(orc, s, got)
        # (the last run before these fetches was the pending run: the stats read before it, after the run
        # and after the sparse fetch, which adds its bytes to the last run's, differ by design)
        assert [k for k in er.same(got, fresh(orc, s.name)) if k not in ("stats_run", "stats_fetch")] == []
        engine.map_run_sparse()
        assert er.same(er.fetch_station(engine, s), fresh(orc, s.name)) == []


def test_a_bad_key_id_does_not_outlive_its_batch(orc, engine):
    """A key id >= key_bound passes the load (the run finds it and sets errWord): fmt_map_check returns
    FMT_E_DATA after the run, on the sparse and the dense path, and the next station on the same engine is
    bit-equal to fresh, its own fmt_map_check clean."""
    for load, run, base, nxt in ((engine.map_load_sparse, engine.map_run_sparse, "map_pending", "map_sparse3"),
                                 (engine.map_load, engine.map_run, "map_dense_lds", "map_dense_hbm")):
        b = er.BY_NAME[base].batch
        ops = b.ops.copy()
        ops["key"][len(ops) // 2] = b.key_bound
        load(replace(b, ops=ops))
        run()
        _raises(FMT_E_DATA, engine.map_check)
        visit(orc, engine, er.BY_NAME[nxt])
        engine.map_check()


def test_refused_headers_before_and_after_the_run(orc, engine):
    """fmt_mt_fetch_headers between load and run (fmt.h "Call order") with a refused document first and
    last in its batch, after a 48-document station: the plan's refusal header for it, every other header
    zero; after the run every fetch is the fresh engine's."""
    for name in ("refused_first", "refused_last"):
        visit(orc, engine, er.BY_NAME["plain"])
        s = er.BY_NAME[name]
        want = er.refused_headers(s.batch)
        assert int((want["status"] == native.FMT_E_UNSUPPORTED).sum()) == 1
        engine.mt_load(s.batch)
        assert engine.mt_headers(raise_on_failed_docs=False).tobytes() == want.tobytes()
        engine.mt_run()
        got = er.fetch_station(engine, s)
        er.check_station(orc, s, got)
        assert er.same(got, fresh(orc, s.name)) == []


def test_merge_tree_fetches_before_a_run_are_refused(orc, engine):
    """After a 48-document station, the 3-document one is loaded and not run: every fetch, the digest
    and both summarize calls return FMT_E_USAGE (runtime.cpp mtNeedsRun: a host check ahead of the first
    HIP call of each), fmt_mt_fetch_headers returns the load's own view (all zero: nothing refused), the
    blobs of the last summarize are still served (fmt.h: valid until the next one), and after the run
    everything is the fresh engine's."""
    import v1_bulk

    big, small = er.BY_NAME["plain"], er.BY_NAME["plain3"]
    before = visit(orc, engine, big)
    b = small.batch
    engine.mt_load(b)
    hdrs = engine.mt_headers()
    assert len(hdrs) == 3 and hdrs.tobytes() == bytes(hdrs.nbytes)
    h = fresh(orc, small.name)["_arrays"]["headers"]
    for call in (lambda: engine.mt_doc(0, h[0]), engine.mt_digests, engine.mt_catchup_all,
                 lambda: engine.mt_catchup(0, {"n_catchup": 1}), lambda: engine.mt_remove_order(0, {"n_rm_order": 1}),
                 lambda: engine.mt_numbers(0), lambda: engine.mt_regen(0), lambda: engine.mt_legacy_props(0, h[0]),
                 lambda: engine.mt_rm_clients_hi(0, h[0]), lambda: engine.mt_rm_clients_hi2(0, h[0]),
                 lambda: engine.mt_summarize_legacy(b.keys, b.values),
                 lambda: engine.mt_summarize_v1(b.keys, b.values, v1_bulk.all_names(b))):
        assert "fmt_mt_run" in _raises(FMT_E_USAGE, call)
    for d in (0, 47):
        assert engine.mt_summary(d) == before[f"legacy{d}"] and engine.mt_summary_v1(d) == before[f"v1_{d}"]
    engine.mt_run()
    got = er.fetch_station(engine, small)
    er.check_station(orc, small, got)
    assert er.same(got, fresh(orc, small.name)) == []


def test_map_fetches_before_a_run(orc, engine):
    """After a 48-document sparse station, the 3-document one is loaded and not run: the pending run,
    the summary and fmt_map_check are refused (FMT_E_USAGE); fmt_map_fetch_sparse and, after a dense
    load, fmt_map_fetch return the batch with no op applied from the host (fmt.h "Call order": the two
    calls bench.py makes before its first run with --warmup 0), not the last batch's counts and slots."""
    big, small = er.BY_NAME["map_pending"], er.BY_NAME["map_sparse3"]
    visit(orc, engine, big)
    b = small.batch
    engine.map_load_sparse(b)
    counts, entries = engine.map_fetch_sparse()
    assert counts.tolist() == [0, 0, 0] and len(entries) == 0
    _raises(FMT_E_USAGE, engine.map_pending, b)
    _raises(FMT_E_USAGE, engine.map_summarize, b.keys, b.values)
    _raises(FMT_E_USAGE, engine.map_check)
    engine.map_run_sparse()
    engine.map_check()
    got = er.fetch_station(engine, small)
    er.check_station(orc, small, got)
    assert er.same(got, fresh(orc, small.name)) == []
    dense = er.BY_NAME["map_dense_lds"]
    visit(orc, engine, er.BY_NAME["map_dense_hbm"])
    engine.map_load(dense.batch)
    slots = engine.map_fetch()
    assert (slots["value"] == 0xFFFFFFFF).all() and (slots["birth_seq"] == 0).all()
    _raises(FMT_E_USAGE, engine.map_check)
    engine.map_run()
    got = er.fetch_station(engine, dense)
    er.check_station(orc, dense, got)
    assert er.same(got, fresh(orc, dense.name)) == []


def test_fetches_share_their_scratch_without_disturbing_each_other(orc, engine):
    """mapPackedOff / mapPacked serve the sparse fetch, the pending fetch and the summary: interleaved
    on one loaded station, each result equals the first of its kind."""
    s = er.BY_NAME["map_tiered_none"]
    b = s.batch
    er.run_station(engine, s)
    f0 = engine.map_fetch_sparse()
    p0 = engine.map_pending(b)
    f1 = engine.map_fetch_sparse()
    engine.map_summarize(b.keys, b.values)
    s0 = [engine.map_summary_doc(d) for d in range(b.n_docs)]
    p1 = engine.map_pending(b)  # (a fresh pending run, then its fetch)
    f2 = engine.map_fetch_sparse()
    want = er.map_oracle(orc, s.name)
    for f in (f0, f1, f2):
        assert all(np.array_equal(g, w) for g, w in zip(f, want["sparse"]))
    for p in (p0, p1):
        assert all(np.array_equal(g, w) for g, w in zip(p, want["pending"]))
    assert s0 == [orc.map_summary(b, d) for d in range(b.n_docs)]

"""GPU: the read frame of the merge-tree bulk reads (csrc/runtime.cpp readFrame / invalidateReads, DESIGN.md
section 4.15). The seven bulk reads share one host copy of the headers, one upload of the per-document views
and one tile plan, built by whichever read comes first after a run and stale from the next load or run on.
Every comparison is byte for byte against the same reads on a fresh engine."""
from dataclasses import replace

import numpy as np
import pytest

import test_gpu_text
import v1_bulk
from fluidframework_amd import native, workloads

pytestmark = pytest.mark.gpu
OBJ = 0xFFFC


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _queries(engine, n_docs):
    """Two local queries per document: its first position and its last (or its end, twice, when empty)."""
    vis = engine.mt_headers(raise_on_failed_docs=False)["visible_len"]
    q = np.zeros(2 * n_docs, dtype=native.POS_QUERY_DTYPE)
    q["ref_seq"] = native.VIEW_LOCAL
    q["pos"][1::2] = np.maximum(vis.astype(np.int64) - 1, 0)
    return q, np.arange(0, 2 * n_docs + 1, 2, dtype=np.uint64)


def _blobs(engine, fetch, n_docs):
    out = []
    for d in range(n_docs):
        try:
            out.append(repr(fetch(d)))
        except native.EngineError as e:
            out.append(f"status {e.code}")
    return "\n".join(out).encode("utf-8")


def _readers(engine, batch):
    """The seven bulk reads by name, each returning its result as bytes."""
    n = batch.n_docs

    def pair(f, *a):
        offs, data = f(*a)
        return offs.tobytes() + data.tobytes()

    def legacy():
        engine.mt_summarize_legacy(batch.keys, batch.values)
        return _blobs(engine, engine.mt_summary, n)

    def v1():
        engine.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
        return _blobs(engine, engine.mt_summary_v1, n)

    def positions():
        q, offs = _queries(engine, n)
        return engine.mt_positions(q, offs).tobytes()

    return [("digests", lambda: engine.mt_digests().tobytes()), ("legacy", legacy), ("v1", v1),
            ("texts", lambda: pair(engine.mt_texts, 0)), ("runs", lambda: pair(engine.mt_prop_runs)),
            ("props", lambda: pair(engine.mt_props_all)), ("positions", positions)]


def _read_all(engine, batch, first=0):
    readers = _readers(engine, batch)
    return {name: f() for name, f in readers[first:] + readers[:first]}


def _fresh(batch):
    e = native.Engine(0)
    try:
        e.mt_load(batch)
        e.mt_run()
        return _read_all(e, batch)
    finally:
        e.close()


@pytest.fixture(scope="module")
def tiers():
    batch, _ = test_gpu_text.tier_batch(native.text_tile_leaves())
    return batch, _fresh(batch)


def test_whichever_read_comes_first_builds_the_frame(engine, tiers):
    """Documents of the micro, compact, small, large and huge tiers, one of them across a tile edge: after
    each of seven runs another of the seven reads goes first, and every result equals the fresh engine's."""
    batch, want = tiers
    assert all(len(v) > 0 for v in want.values())
    engine.mt_load(batch)
    for first in range(7):
        engine.mt_run()
        got = _read_all(engine, batch, first)
        assert [k for k in want if got[k] != want[k]] == [], first


def test_a_frame_does_not_outlive_its_batch(engine, tiers):
    """After the tier batch was read by all seven, five farm documents (another count, other tiers at the
    same indices) read as on a fresh engine; so they do after a load the host refuses."""
    batch, want = tiers
    engine.mt_load(batch)
    engine.mt_run()
    assert _read_all(engine, batch) == want
    small = workloads.conflict_farm(5, n_clients=4, ops_per_doc=150, seed=31)
    want_small = _fresh(small)
    engine.mt_load(small)
    engine.mt_run()
    got = _read_all(engine, small)
    assert [k for k in want_small if got[k] != want_small[k]] == []
    offs = np.asarray(small.doc_op_offsets).copy()
    offs[1], offs[2] = offs[2], offs[1]
    with pytest.raises(native.EngineError) as e:
        engine.mt_load(replace(small, doc_op_offsets=offs))
    assert e.value.code == native.FMT_E_USAGE
    for first in (0, 3):
        got = _read_all(engine, small, first)
        assert [k for k in want_small if got[k] != want_small[k]] == [], first


def test_shared_tiles_separate_sizing(engine):
    """Sizing and fill calls of two placeholders, the runs and the position queries interleaved: the tile plan
    they share knows no placeholder, the units of each sizing call do."""
    batch = v1_bulk.farm_batch()
    n = batch.n_docs
    fresh = native.Engine(0)
    try:
        fresh.mt_load(batch)
        fresh.mt_run()
        want_text = {ph: fresh.mt_texts(ph) for ph in (OBJ, 0)}
        want_runs = fresh.mt_prop_runs()
        q, q_offs = _queries(fresh, n)
        want_hits = fresh.mt_positions(q, q_offs)
    finally:
        fresh.close()
    engine.mt_load(batch)
    engine.mt_run()
    L, h, ptr = engine.L, engine.h, native._ptr

    def text(ph, out):
        offs = np.zeros(n + 1, dtype=np.uint64)
        assert L.fmt_mt_fetch_text_all(h, ph, ptr(offs), None if out is None else ptr(out), 0 if out is None else len(out)) == native.FMT_OK
        assert np.array_equal(offs, want_text[ph][0]), ph
        if out is not None:
            assert np.array_equal(out, want_text[ph][1]), ph

    def runs(out):
        offs = np.zeros(n + 1, dtype=np.uint64)
        assert L.fmt_mt_fetch_prop_runs_all(h, ptr(offs), None if out is None else ptr(out), 0 if out is None else len(out)) == native.FMT_OK
        assert np.array_equal(offs, want_runs[0])
        if out is not None:
            assert out.tobytes() == want_runs[1].tobytes()

    assert len(want_text[OBJ][1]) > 0 and len(want_runs[1]) > 0
    text(OBJ, None)
    runs(None)
    text(0, None)
    runs(np.zeros(len(want_runs[1]), dtype=native.PROP_RUN_DTYPE))
    text(OBJ, np.zeros(len(want_text[OBJ][1]), dtype="<u2"))
    assert engine.mt_positions(q, q_offs).tobytes() == want_hits.tobytes()
    text(0, np.zeros(len(want_text[0][1]), dtype="<u2"))

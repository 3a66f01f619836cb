"""GPU parity of the bulk SharedMap summaries (fmt_map_summarize, csrc/map_summary.hip): after
map_load_sparse + map_run_sparse_tiered + map_summarize every document's header and blobs equal
oracle.map_summary byte for byte, and the device's ordered entries, tags and blob counts equal the
host half's (native.map_summary_order, csrc/map_sum_plan.h). The documents are those of
tests/map_summary_cases.py: the directed ones of the host tests, every live count at which the device
takes another path (one wave in registers up to 64, the LDS sort up to 2048, the host beyond), flush
boundaries on the edges of the scan's 64-entry tiles, and the benchmarked sparse shape.

Run with `pytest -m gpu`.
"""
import numpy as np
import pytest

import map_summary_cases as cases
from fluidframework_amd import native, workloads
from fluidframework_amd.native import FMT_E_CAPACITY, FMT_E_USAGE
from fluidframework_amd.streams import MapStreamBuilder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _summarize(engine, batch, keys=None, values=None, tiered=True):
    engine.map_load_sparse(batch)
    engine.map_run_sparse_tiered() if tiered else engine.map_run_sparse()
    return engine.map_summarize(batch.keys if keys is None else keys, batch.values if values is None else values)


def _assert_arrays(engine, batch, keys=None, values=None):
    """The device's ordered entries, tags and blob counts against the host hook over the fetched entries."""
    counts, entries = engine.map_fetch_sparse()
    keys, values = batch.keys if keys is None else keys, batch.values if values is None else values
    ho, ht, hb, _ = native.map_summary_order(counts, entries, keys, values, threads=8)
    do, dt, db = engine.map_summary_arrays(len(entries))
    assert np.array_equal(db, hb), np.flatnonzero(db != hb)[:5]
    if not (np.array_equal(do, ho) and np.array_equal(dt, ht)):
        at = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        for d in range(batch.n_docs):
            s = slice(at[d], at[d + 1])
            if not (np.array_equal(do[s], ho[s]) and np.array_equal(dt[s], ht[s])):
                k = next(i for i in range(int(counts[d])) if do[s][i] != ho[s][i] or dt[s][i] != ht[s][i])
                pytest.fail(f"document {d} ({counts[d]} entries): rank {k}: {do[s][k]} tag {dt[s][k]}, "
                            f"host {ho[s][k]} tag {ht[s][k]}")
    return counts


def _assert_oracle(orc, engine, batch, docs):
    bad = [d for d in docs if engine.map_summary_doc(d) != orc.map_summary(batch, d)]
    assert not bad, bad[:5]


def test_directed_documents(orc, engine):
    batch, docs = cases.directed()
    t = _summarize(engine, batch)
    assert t["host_ordered_docs"] == 0 and t["threads"] >= 1
    _assert_oracle(orc, engine, batch, range(batch.n_docs))
    _assert_arrays(engine, batch)
    assert t["bytes"] == sum(len(h.encode()) + sum(len(b.encode()) for b in bl)
                             for h, bl in (engine.map_summary_doc(d) for d in range(batch.n_docs)))
    s = engine.stats()
    assert s.ops == len(engine.map_fetch_sparse()[1]) and s.docs == batch.n_docs and s.bytes_written > 0


def test_randomised_documents(orc, engine):
    batch = cases.randomised()
    _summarize(engine, batch)
    _assert_oracle(orc, engine, batch, range(batch.n_docs))
    _assert_arrays(engine, batch)


@pytest.mark.parametrize("with_2049", [False, True])
def test_live_counts_at_each_path_edge(orc, engine, with_2049):
    batch = cases.edges(with_2049)
    t = _summarize(engine, batch)
    assert t["host_ordered_docs"] == (1 if with_2049 else 0)  # 2048 stays on the device, 2049 does not
    counts = _assert_arrays(engine, batch)
    n = len(cases.EDGE_COUNTS)
    assert [int(c) for c in counts[0 : 4 * n : 4]] == cases.EDGE_COUNTS == [int(c) for c in counts[2 : 4 * n : 4]]
    assert not with_2049 or counts[-1] == 2049
    _assert_oracle(orc, engine, batch, range(batch.n_docs))


def test_scan_across_tile_edges(orc, engine):
    batch, docs = cases.tile_edges()
    _summarize(engine, batch)
    _assert_arrays(engine, batch)
    _assert_oracle(orc, engine, batch, range(batch.n_docs))
    sizes = lambda d: [b.count('{"type"') for b in engine.map_summary_doc(d)[1]]  # noqa: E731
    assert sizes(docs["b64_65"])[:2] == [32, 33] and sizes(docs["b63_64"])[:2] == [31, 33]


def test_summarize_leaves_the_replay_state_untouched(orc, engine):
    b = MapStreamBuilder()
    for d in range(6):
        b.begin_doc()
        for i in range(40 + 30 * d):
            b.add_message(d, i + 1, {"type": "set", "key": str(97 * i % 211) if i % 2 else f"k{i}",
                                     "value": {"type": "Plain", "value": "v" * (i % 9)}})
        b.local_submit(d, {"type": "set", "key": "local", "value": {"type": "Plain", "value": d}})
        b.local_submit(d, {"type": "delete", "key": "k0"})
    batch = b.finish()
    engine.map_load_sparse(batch)
    engine.map_run_sparse_tiered()
    c0, e0 = engine.map_fetch_sparse()
    engine.map_summarize(batch.keys, batch.values)
    c1, e1 = engine.map_fetch_sparse()
    assert np.array_equal(c0, c1) and np.array_equal(e0, e1)
    assert np.array_equal(e1, orc.map_replay_sparse(batch)[1])
    pc, ps, pe = engine.map_pending(batch)
    oc, os_, oe = orc.map_pending(batch)
    assert np.array_equal(pc, oc) and np.array_equal(ps, os_) and np.array_equal(pe, oe)
    _assert_oracle(orc, engine, batch, range(batch.n_docs))  # (the blobs outlive the pending run)


def test_ids_outside_the_tables_fail_their_document_alone(orc, engine):
    b = MapStreamBuilder()
    for d in range(3):
        b.begin_doc()
        b.add_message(d, 0, {"type": "set", "key": "1", "value": {"type": "Plain", "value": "one"}})
    b.add_message(1, 0, {"type": "set", "key": "zz-last", "value": {"type": "Plain", "value": "last value"}})
    batch = b.finish()
    for keys, values in ((batch.keys[:-1], batch.values), (batch.keys, batch.values[:-1])):
        _summarize(engine, batch, keys, values)
        with pytest.raises(native.EngineError) as ei:
            engine.map_summary_doc(1)
        assert ei.value.code == FMT_E_USAGE
        _assert_oracle(orc, engine, batch, (0, 2))
        _assert_arrays(engine, batch, keys, values)


def test_calls_out_of_order(engine):
    batch, _ = cases.directed()
    engine.map_load_sparse(batch)
    with pytest.raises(native.EngineError) as ei:  # before a sparse run
        engine.map_summarize(batch.keys, batch.values)
    assert ei.value.code == FMT_E_USAGE
    with pytest.raises(native.EngineError) as ei:  # a load drops the last summary
        engine.map_summary_doc(0)
    assert ei.value.code == FMT_E_USAGE


def test_after_a_plain_run_that_refused_a_document(orc, engine):
    b = MapStreamBuilder()
    for n in (3, 2049, 10):  # 2049 distinct keys: past the LDS tier
        d = b.begin_doc()
        for i in range(n):
            b.add_message(d, 0, {"type": "set", "key": str(i), "value": {"type": "Plain", "value": i % 5}})
    batch = b.finish()
    with pytest.raises(native.EngineError) as ei:
        _summarize(engine, batch, tiered=False)
    assert ei.value.code == FMT_E_CAPACITY and "tiered" in str(ei.value)
    t = _summarize(engine, batch, tiered=True)
    assert t["host_ordered_docs"] == 1
    _assert_oracle(orc, engine, batch, range(3))


def test_benchmarked_shape(orc, engine):
    batch = workloads.map_stream(2000, 1000, key_pool=1 << 20, seed=5)
    values = [workloads.map_value_json(i) for i in range(50 + 1000 + 1)]
    t = _summarize(engine, batch, values=values)
    assert t["host_ordered_docs"] == 0
    counts = _assert_arrays(engine, batch, values=values)
    assert counts.max() > 1
    bad = []
    for d in range(0, 2000, 10):  # (one small batch per sampled document: its own keys only)
        small = cases.compact(batch, [d])
        small.values = values
        if engine.map_summary_doc(d) != orc.map_summary(small, 0):
            bad.append(d)
    assert not bad, bad[:5]

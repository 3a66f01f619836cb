"""Bulk SnapshotV1 summaries on the GPU (include/fmt_v1.h: summaryV1Kernel's segmentation, text and
first removers, the remove-order join and the JSON on the host): each test is a load, a run,
mt_summarize_v1 and a per-document comparison with summary.v1_summary over the ORACLE's replay and
the oracle's stamps (v1_bulk.reference), never over the engine's own bulk output."""
import json

import pytest

import v1_bulk
from fluidframework_amd import native, summary, workloads
from fluidframework_amd.streams import MergeTreeStreamBuilder, flag_remove_order
from test_snapshot_v1 import NAMES, _collab_batch, _v1_blobs, obliterate_v1_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _bulk(engine, batch, chunk=summary.V1_CHUNK_SIZE, run=True):
    if run:
        engine.mt_load(batch)
        engine.mt_run()
    t = engine.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch), chunk=chunk)
    assert t["bytes"] > 0 and t["threads"] >= 1
    return [engine.mt_summary_v1(d) for d in range(batch.n_docs)]


def _fixture_docs(b, names):
    from golden_data import snapshot_trees

    want = []
    for name in names:
        head, bodies = _v1_blobs(snapshot_trees("v1")[name])
        b.begin_doc_from_summary(head, bodies)
        want.append((head, bodies))
    return want


def test_v1_fixtures_as_one_batch(engine):
    b = MergeTreeStreamBuilder()
    want = _fixture_docs(b, NAMES)
    assert any(bodies for _, bodies in want)
    assert _bulk(engine, b.finish()) == want


@pytest.mark.parametrize("make", [_collab_batch, obliterate_v1_batch], ids=["collab", "obliterate"])
def test_merge_info_equals_the_oracle(orc, engine, make):
    batch = make()
    state = v1_bulk.oracle_state(orc, batch)
    assert v1_bulk.set_remover_pairs(state) > 0
    if make is obliterate_v1_batch:
        assert v1_bulk.stamp_counts(state)[2] > 0  # moved stamps
    want = v1_bulk.reference(batch, state)
    got = _bulk(engine, batch)
    for d in range(batch.n_docs):
        assert got[d] == want[d], d


def test_conflict_farm_at_two_chunk_sizes(orc, engine):
    batch = v1_bulk.farm_batch()
    state = v1_bulk.oracle_state(orc, batch)
    assert v1_bulk.stamp_counts(state)[1] > 0  # more than one stamp somewhere
    assert max(int(h["n_leaves"]) for h, *_ in state) > 256  # past the compact tier
    want = v1_bulk.reference(batch, state, chunk=v1_bulk.FARM_CHUNK)
    assert all(len(bodies) >= 1 for _, bodies in want)
    got = _bulk(engine, batch, chunk=v1_bulk.FARM_CHUNK)
    for d in range(batch.n_docs):
        assert got[d] == want[d], d
    want = v1_bulk.reference(batch, state)
    got = _bulk(engine, batch, run=False)  # (the blobs of the call before are replaced)
    for d in range(batch.n_docs):
        assert got[d] == want[d], d


def test_huge_document_equals_the_per_document_host_path(engine):
    """The size test_gpu_huge.test_huge_remove_order_on_gpu uses (the engine's state there == the oracle's)."""
    batch = workloads.as_legacy_load(workloads.t3_stream(40000, 20000, n_clients=63, max_lag=2000, max_range=60, seed=43))
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers()
    assert int(hdrs[0]["n_leaves"]) > 2048  # (past the large tier)
    lv, ch, pr = engine.mt_doc(0, hdrs[0])
    rm = summary.removers_from_engine(lv, int(hdrs[0]["n_leaves"]), engine.mt_remove_order(0, hdrs[0]), batch.ops)
    assert any(len(s) > 1 for s in rm.values())
    names = v1_bulk.names(batch, 0)
    want = summary.v1_summary(hdrs[0], lv, ch, pr, batch.keys, batch.values, names, rm)
    assert len(want[1]) >= 1
    assert _bulk(engine, batch, run=False) == [want]


def test_adjust_numbers_in_solo_segments(orc, engine):
    from feature_pairs import ADJUSTED_KEYS, adjust_rm_batch

    batch, _ = adjust_rm_batch(narrow=True)
    numbers = []
    state = v1_bulk.oracle_state(orc, batch, numbers=numbers)
    values = [summary.values_with_numbers(batch.values, numbers[d]) for d in range(batch.n_docs)]
    want = v1_bulk.reference(batch, state, values=values)
    # a computed number in a solo segment's props, as values_with_numbers renders it
    seen = 0
    for d, (head, bodies) in enumerate(want):
        computed = {summary.js_number(float(x)) for x in numbers[d]}
        for blob in [head] + bodies:
            for s in json.loads(blob)["segments"]:
                if isinstance(s, dict) and "json" in s and isinstance(s["json"], dict):
                    props = s["json"].get("props", {})
                    seen += any(k in ADJUSTED_KEYS and json.dumps(v) in computed for k, v in props.items())
    assert seen > 0
    got = _bulk(engine, batch)
    for d in range(batch.n_docs):
        assert got[d] == want[d], d


LOADED_STAMP_HEAD = json.dumps({  # test_snapshot_v1.test_v1_merge_info_segments_load_with_their_stamps
    "version": "1", "segmentCount": 3, "length": 4, "startIndex": 0,
    "segments": [{"json": "a", "seq": 3, "client": "B"},
                 {"json": "bc", "removedSeq": 4, "removedClient": "C"},
                 {"json": "d", "seq": 2, "client": "C", "removedSeq": 5, "removedClient": "B", "removedClientIds": ["B", "D"],
                  "movedSeq": 4, "movedSeqs": [4, 6], "movedClientIds": ["D", "B"]}],
    "headerMetadata": {"minSequenceNumber": 1, "sequenceNumber": 6, "orderedChunkMetadata": [{"id": "header"}],
                       "totalLength": 4, "totalSegmentCount": 3}})


def test_refused_documents_leave_their_neighbours_alone(engine):
    """A failed replay keeps its status; a loaded stamp above minSeq ("Not supported") is
    FMT_E_UNSUPPORTED; the documents beside them get their blobs."""
    b = MergeTreeStreamBuilder()
    want = _fixture_docs(b, ["headerAndBody"])
    d = b.begin_doc("", observer="A")
    d.add_message({"clientId": "B", "sequenceNumber": 1, "referenceSequenceNumber": 0, "minimumSequenceNumber": 0,
                   "type": "op", "contents": {"pos1": 5, "seg": "x", "type": 0}})  # insert past the end
    b.begin_doc_from_summary(LOADED_STAMP_HEAD, [])
    want += _fixture_docs(b, ["withMarkers"])
    batch = b.finish()
    engine.mt_load(batch)
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    assert [int(s) for s in hdrs["status"]] == [0, native.FMT_E_DATA, 0, 0]
    engine.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
    assert [engine.mt_summary_v1(0), engine.mt_summary_v1(3)] == want
    for doc, code in ((1, native.FMT_E_DATA), (2, native.FMT_E_UNSUPPORTED)):
        with pytest.raises(native.EngineError) as e:
            engine.mt_summary_v1(doc)
        assert e.value.code == code, doc


def test_local_batch_and_call_order_are_refused():
    from local_farm import fixture_local_batch

    e = native.Engine(0)
    try:
        batch = fixture_local_batch(max_fixtures=1)[0]
        with pytest.raises(native.EngineError) as err:  # before any load
            e.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
        assert err.value.code == native.FMT_E_USAGE
        e.mt_load(batch)
        with pytest.raises(native.EngineError) as err:  # loaded, not run
            e.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
        assert err.value.code == native.FMT_E_USAGE
        e.mt_run()
        with pytest.raises(native.EngineError) as err:
            e.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
        assert err.value.code == native.FMT_E_UNSUPPORTED
    finally:
        e.close()

"""Engine reuse: stations (a small batch plus everything public to fetch after running it) and the
tour over them, shared by test_engine_reuse_stations.py (no GPU) and test_gpu_engine_reuse.py.

A context keeps its ~120 device and host buffers from batch to batch and only grows them; about twenty
flags and the plan of the last load decide which of them a run and a fetch look at. The question the
tour asks: does batch B give the same bytes on an engine that has just served batch A as on a fresh
one, for every ordered pair (A, B) of stations? The batches come from the generators the other suites
already use; nothing here makes ops of its own.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import feature_pairs as fp
from mt_compare import compare_doc

MAX_DOCS = 48
MAX_OPS_PER_DOC = 600  # "a few hundred"; stations built from pinned fixtures name their larger shape


@dataclass
class Station:
    name: str
    family: str            # "mt" or "map"
    build: object          # () -> batch
    mode: str = ""         # map: "dense", "sparse", "tiered"
    pending: bool = False  # map: the pending view on top of the sparse run
    summarize: bool = False  # map: fmt_map_summarize on top of the (tiered) run
    cap_catchup: int = 0
    facts: dict = field(default_factory=dict)  # what native.mt_plan must show (test_engine_reuse_stations)
    larger: str = ""       # why the station is past MAX_OPS_PER_DOC, when it is
    value_base: bool = False  # merge-tree: document-local value ids (doc_value_base)

    @functools.cached_property
    def batch(self):
        b = self.build()
        return b[0] if isinstance(b, tuple) else b


# --------------------------------------------------------------------------------- merge-tree batches
def _conflict(n_docs, seed, ops_per_doc=300):
    from fluidframework_amd import workloads

    return workloads.with_insert_props(workloads.conflict_farm(n_docs, n_clients=8, ops_per_doc=ops_per_doc, seed=seed))


def _stepdown():
    import descend_cascade

    return descend_cascade.grow_then_shrink_batch()


def _adjust():
    from test_annotate_adjust import adjust_fixture_batch

    return adjust_fixture_batch(narrow=True)


def _catchup():
    from test_catchup import fixture_batch

    return fixture_batch()


def _rm_order():
    import v1_bulk

    return v1_bulk.farm_batch()


def _local():
    import local_farm

    return local_farm.local_farm_batch(range(4), steps=150)


def _relpos():
    import marker_docs

    return marker_docs.marker_batch(6, 200, seed=3)


def _snapshot():
    import summary_edges

    return summary_edges.batch("props")


def _snapshot_info():
    import summary_edges

    return summary_edges.batch("first_remover")


def _obliterate():
    """Every third 2.3.0 obliterate fixture as documents (golden_data.prefix_batch), every 40th of them (16); the odd
    ones re-encoded as sided obliterates with about half of the endpoints exclusive
    (test_obliterate_sided.as_sided), the even ones left non-sided."""
    import v1_bulk
    from golden_data import prefix_batch
    from test_obliterate_sided import OB_FIXTURES, as_sided

    batch, _ = prefix_batch(OB_FIXTURES[::3])
    batch = v1_bulk.concat_docs(batch, range(0, batch.n_docs, 40))
    sided = as_sided(batch.ops, np.random.default_rng(5))
    offs = np.asarray(batch.doc_op_offsets).astype(np.int64)
    for d in range(1, batch.n_docs, 2):
        batch.ops[offs[d]: offs[d + 1]] = sided[offs[d]: offs[d + 1]]
    return batch


def _adjust_doc_local():
    """marker_docs documents with adjusts through the builder's localizing path, forced on a small batch
    by unreferenced values (as test_doc_local_values does): doc_value_base, adjusts, relative positions."""
    import marker_docs
    from fluidframework_amd.streams import MergeTreeStreamBuilder

    b = MergeTreeStreamBuilder()
    for d in range(12):
        init, msgs = marker_docs.doc_messages(d, 250, 7, True)
        doc = b.begin_doc(init)
        for m in msgs:
            doc.add_message(m)
    b.values.items += [f'"pad{i}"' for i in range(40000)]
    return b.finish()


def _large_growth():
    import growth

    return growth.growth_batch([("", 3000, 1), ("", 4000, 2), ("", 3000, 3)])


def _writers40():
    from fluidframework_amd import workloads

    return workloads.conflict_farm(4, n_clients=40, ops_per_doc=600, seed=4)


def _huge(seed, first):
    """A summary-loaded document of 2,100 segments (past the large tier's 2,048 leaves) and 300 ops among
    300-op conflict-farm documents: first of 7, or seventh of 13."""
    from fluidframework_amd import workloads
    from huge_edges import concat_batches

    farm = workloads.conflict_farm(6, n_clients=8, ops_per_doc=300, seed=seed)
    t3 = workloads.t3_stream(2100, 300, n_clients=8, max_lag=100, seed=seed + 1)
    return concat_batches([t3, farm] if first else [farm, t3, farm])


def _summary_header(n_segs):
    import json
    import random

    rnd = random.Random(n_segs)
    texts = [rnd.choice("abcdefgh") for _ in range(n_segs)]
    return json.dumps({
        "chunkStartSegmentIndex": 0, "chunkSegmentCount": n_segs, "chunkLengthChars": n_segs, "totalLengthChars": n_segs,
        "totalSegmentCount": n_segs, "chunkSequenceNumber": 0, "segmentTexts": texts,
        "headerMetadata": {"orderedChunkMetadata": [{"id": "header"}], "sequenceNumber": 0, "totalLength": n_segs,
                           "totalSegmentCount": n_segs}})


def _refused(seed, first):
    """Two local farms (local_farm.LocalFarm, 100 steps) and one summary-loaded document of 2,100 segments,
    first or last: local records keep it out of the huge tier, so the plan refuses it alone."""
    import local_farm
    from fluidframework_amd.streams import MergeTreeStreamBuilder

    b = MergeTreeStreamBuilder()
    if first:
        b.begin_doc_from_summary(_summary_header(2100), observer="observer")
    for sd in (seed, seed + 1):
        local_farm.LocalFarm(sd, builder=b).run(100)
    if not first:
        b.begin_doc_from_summary(_summary_header(2100), observer="observer")
    return b.finish()


def _v1_reload():
    import test_snapshot_v1

    r = test_snapshot_v1.v1_reload_batches()
    return r[0] if isinstance(r, (list, tuple)) else r


PLAIN = dict(obliterates=False, local=False, any_adjust=False, catchup=False, rm_order=False, snapshot=False,
             snapshot_info=False, relpos=False, huge=False, refused=False)


def _facts(**kw):
    return dict(PLAIN, **kw)


FIXTURE = "the pinned 0.40 conflict-farm fixtures: 6 documents of 2,040 ops"

MT_STATIONS = [
    Station("plain", "mt", lambda: _conflict(48, 5, 1000), facts=_facts(),
            larger="1,000 ops a document take some of them past the compact tier's 256 leaves"),
    Station("stepdown", "mt", _stepdown, facts=_facts(),
            larger="grow_then_shrink_batch: 992 ops take one document up to the small tier and back down"),
    Station("obliterate_adjust", "mt", lambda: fp.adjust_ob_batch(False), facts=_facts(obliterates=True, any_adjust=True)),
    Station("adjust", "mt", _adjust, facts=_facts(any_adjust=True), larger=FIXTURE),
    Station("catchup", "mt", _catchup, cap_catchup=fp.CAP_CU, facts=_facts(catchup=True), larger=FIXTURE),
    Station("catchup_rm_order", "mt", lambda: fp.catchup_pair_batches(only="rm")["rm"], cap_catchup=fp.CAP_CU,
            facts=_facts(catchup=True, rm_order=True), larger=FIXTURE),
    Station("rm_order", "mt", _rm_order, facts=_facts(rm_order=True),
            larger="v1_bulk.farm_batch: 1,000 ops a document reach the compact -> small cascade with remove order"),
    Station("local", "mt", _local, facts=_facts(local=True)),
    Station("relpos", "mt", _relpos, facts=_facts(relpos=True)),
    Station("snapshot", "mt", _snapshot, facts=_facts(snapshot=True, rm_order=True)),
    Station("snapshot_info", "mt", _snapshot_info, facts=_facts(snapshot=True, snapshot_info=True, rm_order=True),
            larger="summary_edges first_remover: one document of 4,097 ops past the large tier's writers"),
    Station("obliterate", "mt", _obliterate, facts=_facts(obliterates=True),
            larger="the pinned 2.3.0 obliterate fixtures: up to 2,040 ops a document"),
    Station("adjust_doc_local", "mt", _adjust_doc_local, facts=_facts(any_adjust=True, relpos=True), value_base=True),
    Station("large_growth", "mt", _large_growth, facts=_facts(),
            larger="growth.growth_batch: 3,000-4,000 ops a document to end past 512 segments"),
    Station("writers40", "mt", _writers40, facts=_facts()),
    Station("huge_first", "mt", lambda: _huge(3, True), facts=_facts(snapshot=True, huge=True)),
    Station("huge_mid", "mt", lambda: _huge(5, False), facts=_facts(snapshot=True, huge=True)),
    Station("refused_first", "mt", lambda: _refused(11, True), facts=_facts(local=True, snapshot=True, refused=True)),
    Station("refused_last", "mt", lambda: _refused(21, False), facts=_facts(local=True, snapshot=True, refused=True)),
    Station("v1_reload", "mt", _v1_reload, facts=_facts(snapshot=True, snapshot_info=True),
            larger="test_snapshot_v1.v1_reload_batches: reloaded 0.40 fixtures, about 2,000 ops a document"),
    Station("plain3", "mt", lambda: _conflict(3, 9), facts=_facts()),
]


# --------------------------------------------------------------------------------------- map batches
def _map_dense(key_bound):
    """map_edges.dense's first MAX_DOCS documents (of 57), key ids and key_bound as they are."""
    from dataclasses import replace

    import map_edges as me

    batch, _ = me.dense(key_bound)
    offs = np.asarray(batch.doc_op_offsets)[: MAX_DOCS + 1]
    return replace(batch, ops=batch.ops[: int(offs[-1])].copy(), doc_op_offsets=offs.copy())


def _map_farm(n_docs, seed):
    from test_map_pending import pending_farm

    return pending_farm(n_docs, 80, seed=seed)


def _map_limits(which):
    import map_edges as me

    return me.SPARSE_GROUPS[which]()


def _map_summary_edges():
    """map_summary_cases.edges: three of its four documents at every live count (42 of 56)."""
    import map_summary_cases as cases

    return cases.compact(cases.edges(False), [4 * i + j for i in range(len(cases.EDGE_COUNTS)) for j in range(3)])


MAP_STATIONS = [
    Station("map_dense_lds", "map", lambda: _map_dense(65), mode="dense"),
    Station("map_dense_hbm", "map", lambda: _map_dense(2561), mode="dense"),
    Station("map_sparse", "map", lambda: _map_limits("limits_ok"), mode="sparse"),
    Station("map_tiered_keys", "map", lambda: _map_limits("limits_keys"), mode="tiered"),
    Station("map_tiered_ops", "map", lambda: _map_limits("limits_ops"), mode="tiered"),
    Station("map_tiered_none", "map", lambda: _map_farm(12, 4), mode="tiered", pending=True),
    Station("map_pending", "map", lambda: _map_farm(48, 2), mode="sparse", pending=True),
    Station("map_summary", "map", _map_summary_edges, mode="tiered", summarize=True),
    Station("map_sparse3", "map", lambda: _map_farm(3, 7), mode="sparse", pending=True),
]

STATIONS = MT_STATIONS + MAP_STATIONS
BY_NAME = {s.name: s for s in STATIONS}


def plan_facts(batch):
    """The facts of native.mt_plan (fmt_mt_load's host half) and of the batch that the station table names."""
    from fluidframework_amd import native

    p = native.mt_plan(batch)
    assert p.status == 0, p.message
    return dict(obliterates=p.obliterates, local=p.local, any_adjust=p.any_adjust, catchup=p.catchup_ops > 0,
                rm_order=p.rm_order_ops > 0, snapshot=batch.snapshots is not None,
                snapshot_info=getattr(batch, "snapshot_info", None) is not None,
                relpos=getattr(batch, "relpos", None) is not None and len(batch.relpos) > 0,
                huge=len(p.huge_docs) > 0, refused=len(p.refused) > 0)


def refused_headers(batch):
    """What fmt_mt_fetch_headers returns between the load and the first run (fmt.h "Call order"): the
    plan's refusal headers, every other header zero."""
    from fluidframework_amd import native

    out = np.zeros(batch.n_docs, dtype=native.DOC_RESULT_DTYPE)
    for doc, status, fail_seq, cur_seq, min_seq in native.mt_plan(batch).refused.tolist():
        out[doc]["status"], out[doc]["fail_seq"], out[doc]["cur_seq"], out[doc]["min_seq"] = status, fail_seq, cur_seq, min_seq
    return out


def bad_mt_batches():
    """Two batches fmt_mt_load must refuse on the host: the adjust station with two document offsets
    swapped, and with a value id at FMT_MT_VALUE_COMPUTED or above, which an annotate-adjust batch may
    not hold."""
    from dataclasses import replace

    b = BY_NAME["adjust"].batch
    offs = np.asarray(b.doc_op_offsets).copy()
    offs[1], offs[2] = offs[2], offs[1]
    kv = np.asarray(b.props_kv).copy()
    i = int(np.flatnonzero((kv & 0xFFFF) != 0xFFFF)[0])
    kv[i] = (kv[i] & 0xFFFF0000) | 0x9000
    return {"offsets": replace(b, doc_op_offsets=offs), "value_id": replace(b, props_kv=kv)}


# ---------------------------------------------------------------------------------------------- tour
def euler_tour(n):
    """A closed walk over stations 0..n-1 in which every ordered pair of distinct stations occurs exactly
    once as consecutive steps: an Euler circuit of the complete digraph (every vertex has in-degree =
    out-degree = n - 1, and it is strongly connected), by Hierholzer's algorithm with each vertex's
    unused edges taken in ascending order of their head. n * (n - 1) + 1 entries, first == last."""
    nxt = [[v for v in range(n - 1, -1, -1) if v != u] for u in range(n)]  # popped from the end: ascending
    stack, walk = [0], []
    while stack:
        u = stack[-1]
        if nxt[u]:
            stack.append(nxt[u].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk


def tour_segments(n, n_segments):
    """The tour's steps cut into n_segments runs of consecutive steps. Each is a list of station
    indices whose first entry is the station BEFORE the segment's first step (replayed so that no pair
    is lost at a cut); consecutive entries are the segment's pairs."""
    walk = euler_tour(n)
    edges = len(walk) - 1
    per = -(-edges // n_segments)
    return [walk[k: min(k + per, edges) + 1] for k in range(0, edges, per)]


# -------------------------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def mt_oracle(orc, name):
    s = BY_NAME[name]
    return fp.Oracle(orc, s.batch, fp.LARGE_CAPS, cap_catchup=s.cap_catchup, index=s.facts["huge"])


@functools.lru_cache(maxsize=None)
def map_oracle(orc, name):
    """What the oracle says a map station fetches: dense slots, or (counts, entries), the pending view
    and the summaries."""
    s, b = BY_NAME[name], BY_NAME[name].batch
    out = {}
    if s.mode == "dense":
        out["dense"] = orc.map_replay(b, threads=8)[0]
    else:
        counts, entries, _ = orc.map_replay_sparse(b, threads=8)
        out["sparse"] = (counts, entries)
    if s.pending:
        out["pending"] = orc.map_pending(b)
    if s.summarize:
        out["summary"] = [orc.map_summary(b, d) for d in range(b.n_docs)]
    return out


# ------------------------------------------------------------------------------------------- fetches
STAT_FIELDS = ("ops", "docs", "launches", "bytes_read", "bytes_written")  # (the others hold a time)


def _stats(engine):
    st = engine.stats()
    return tuple(int(getattr(st, f)) for f in STAT_FIELDS)


def run_station(engine, s, twice=False):
    """Load and run station s (twice: the run issued twice before anything is fetched)."""
    b = s.batch
    if s.family == "mt":
        engine.mt_load(b)
        engine.mt_run()
        if twice:
            engine.mt_run()
        return
    if s.mode == "dense":
        engine.map_load(b)
        run = engine.map_run
    else:
        engine.map_load_sparse(b)
        run = engine.map_run_sparse_tiered if s.mode == "tiered" else engine.map_run_sparse
    run()
    if twice:
        run()


def fetch_station(engine, s):
    """Everything public that applies to the loaded and run station s, as a flat dict name -> bytes /
    str / tuple, comparable with ==. The numpy arrays are kept beside it under "_arrays" for the oracle
    comparisons."""
    return _fetch_mt(engine, s) if s.family == "mt" else _fetch_map(engine, s)


def _or_code(f, d):
    """f(d), or ("error", code) for a document that has no summary (its replay status)."""
    from fluidframework_amd import native

    try:
        return f(d)
    except native.EngineError as e:
        return ("error", e.code)


def _fetch_mt(engine, s):
    import v1_bulk

    b, f = s.batch, s.facts
    got, arr = {}, {}
    got["stats_run"] = _stats(engine)
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    got["stats_headers"] = _stats(engine)
    # every field takes part: fmt.h documents no field of fmt_mt_doc_result as depending on scheduling
    got["headers"] = hdrs.tobytes()
    arr["headers"] = hdrs
    got["digests"] = engine.mt_digests().tobytes()
    offs, ranges = engine.mt_catchup_all()
    got["catchup_all"] = (offs.tobytes(), ranges.tobytes())
    arr["catchup_all"] = (offs, ranges)
    keys, values = getattr(b, "keys", None) or [], getattr(b, "values", None) or []
    engine.mt_summarize_legacy(keys, values)
    v1 = not f["local"]
    if v1:
        engine.mt_summarize_v1(keys, values, v1_bulk.all_names(b))
    docs = []
    for d in range(b.n_docs):
        h = hdrs[d]
        lv, ch, pr = engine.mt_doc(d, h)
        docs.append((h, lv, ch, pr))
        got[f"doc{d}"] = (lv.tobytes(), ch.tobytes(), pr.tobytes())
        got[f"rm{d}"] = engine.mt_remove_order(d, h).tobytes()
        got[f"cu{d}"] = engine.mt_catchup(d, h).tobytes()
        got[f"nums{d}"] = engine.mt_numbers(d).tobytes()
        ro, rt = engine.mt_regen(d)
        got[f"regen{d}"] = (ro.tobytes(), rt.tobytes())
        got[f"legacy_props{d}"] = engine.mt_legacy_props(d, h).tobytes()
        got[f"hi{d}"] = engine.mt_rm_clients_hi(d, h).tobytes()
        got[f"hi2{d}"] = engine.mt_rm_clients_hi2(d, h).tobytes()
        got[f"legacy{d}"] = _or_code(engine.mt_summary, d)
        if v1:
            got[f"v1_{d}"] = _or_code(engine.mt_summary_v1, d)
    arr["docs"] = docs
    got["_arrays"] = arr
    return got


def _fetch_map(engine, s):
    b = s.batch
    got, arr = {}, {}
    got["stats_run"] = _stats(engine)
    if s.mode == "dense":
        slots = engine.map_fetch()
        got["dense"] = slots.tobytes()
        arr["dense"] = slots
        got["stats_fetch"] = _stats(engine)
        got["_arrays"] = arr
        return got
    counts, entries = engine.map_fetch_sparse()
    got["sparse"] = (counts.tobytes(), entries.tobytes())
    arr["sparse"] = (counts, entries)
    got["stats_fetch"] = _stats(engine)
    if s.summarize:
        engine.map_summarize(b.keys, b.values)
        got["summary"] = [engine.map_summary_doc(d) for d in range(b.n_docs)]
        o, t, nb = engine.map_summary_arrays(len(entries))
        got["summary_arrays"] = (o.tobytes(), t.tobytes(), nb.tobytes())
        got["stats_summary"] = _stats(engine)
    if s.pending:
        pc, ps, pe = engine.map_pending(b)
        got["pending"] = (pc.tobytes(), ps.tobytes(), pe.tobytes())
        arr["pending"] = (pc, ps, pe)
        got["stats_pending"] = _stats(engine)
    got["_arrays"] = arr
    return got


def same(a, b):
    """The names under which two fetches of a station differ (bit-equal: [])."""
    assert a.keys() == b.keys()
    return [k for k in a if k != "_arrays" and a[k] != b[k]]


# --------------------------------------------------------------------------- comparisons with the oracle
def check_mt_arrays(orc, s, got):
    """The fetched state against the oracle, directly: every header and leaf field, text and prop sets
    (mt_compare.compare_doc), the computed numbers and the catch-up ranges."""
    o = mt_oracle(orc, s.name)
    arr = got["_arrays"]
    offs, ranges = arr["catchup_all"]
    refused = refused_headers(s.batch)
    for d, doc in enumerate(arr["docs"]):
        if refused[d]["status"] != 0:  # (the oracle has no such limit: the header is the plan's refusal, nothing else)
            assert doc[0].tobytes() == refused[d].tobytes(), (s.name, d, doc[0])
            assert got[f"legacy{d}"] == ("error", int(refused[d]["status"])), (s.name, d)
            continue
        exp = o.doc(d)
        assert int(doc[0]["status"]) == int(exp[0]["status"]) == 0, (s.name, d, int(doc[0]["status"]))
        diffs = compare_doc(exp, doc)
        assert not diffs, f"{s.name} doc {d}: {diffs[:5]}"
        if o.numbers is not None:
            assert got[f"nums{d}"] == np.asarray(o.numbers[d], dtype=np.float64).tobytes(), (s.name, d)
        if s.cap_catchup:
            n = int(exp[0]["n_catchup"])
            mine = ranges[int(offs[d]): int(offs[d + 1])]
            assert int(doc[0]["n_catchup"]) == n == len(mine) and np.array_equal(mine, o.cu[d][:n]), (s.name, d)


def check_mt_full(orc, engine, s, got):
    """The fresh reference: feature_pairs.check_doc over every document with everything the station
    records (numbers, getAtSeq prop sets and the bulk legacy summary for annotate-adjust; stamp lists
    and the SnapshotV1 summary for remove order; catch-up ranges), then check_mt_arrays."""
    o = mt_oracle(orc, s.name)
    b, f = s.batch, s.facts
    hdrs = got["_arrays"]["headers"]
    refused = refused_headers(b)
    for d, doc in enumerate(got["_arrays"]["docs"]):
        h = hdrs[d]
        # (document-local ids: check_doc's summaries read batch-global values; check_mt_arrays below holds the state)
        if refused[d]["status"] != 0 or s.value_base:
            continue
        adjust = f["any_adjust"]
        fp.check_doc(o, d, doc, nums=engine.mt_numbers(d) if adjust else None,
                     legacy=engine.mt_legacy_props(d, h) if adjust else None,
                     engine_summary=got[f"legacy{d}"] if adjust else None,
                     rm=engine.mt_remove_order(d, h) if f["rm_order"] and b.clients else None,
                     cu=engine.mt_catchup(d, h) if s.cap_catchup else None)
    check_mt_arrays(orc, s, got)


def check_map(orc, s, got):
    """A map station's fetches against the oracle: slots, counts and entries, the pending view, the
    summary blobs, all equal (integer state and bytes; no tolerance)."""
    want, arr = map_oracle(orc, s.name), got["_arrays"]
    if s.mode == "dense":
        assert np.array_equal(arr["dense"], want["dense"]), s.name
        return
    (gc, ge), (wc, we) = arr["sparse"], want["sparse"]
    assert np.array_equal(gc, wc) and np.array_equal(ge, we), s.name
    if s.pending:
        for g, w in zip(arr["pending"], want["pending"]):
            assert np.array_equal(g, w), s.name
    if s.summarize:
        bad = [d for d, (g, w) in enumerate(zip(got["summary"], want["summary"])) if g != w]
        assert not bad, (s.name, bad[:5])


def check_station(orc, s, got):
    check_mt_arrays(orc, s, got) if s.family == "mt" else check_map(orc, s, got)

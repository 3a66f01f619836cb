"""GPU: fmt_mt_fetch_prop_runs_all and fmt_mt_fetch_props_all (include/fmt_runs.h, csrc/runs.hip) against
the definition restated over the oracle's replay of the same batch (runs_cases.expected_runs).

start, len, first_leaf and flags are compared bit for bit with the oracle's runs. `props` names a record of
the engine's own table, whose ids the oracle does not share (it numbers only the sets that survive), so a
run's set is compared with the oracle's by its entries, and the whole 16-byte records are compared bit for
bit with expected_runs over the engine's own per-document fetch, which fixes the id as the lowest one."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import runs_cases
import text_cases
from fluidframework_amd import native, workloads
from runs_cases import NO_CLASS, expected_runs

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = dict(cap_leaves=4096, cap_chars=1 << 17, cap_props=1024)
STRUCT = ["start", "len", "first_leaf", "flags"]


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _run(engine, batch):
    engine.mt_load(batch)
    engine.mt_run()
    return engine.mt_headers(raise_on_failed_docs=False)


def _entries(table, pid):
    return frozenset() if pid == NO_CLASS else frozenset(native.propset_entries(table, pid))


def _check(orc, engine, batch, hdrs):
    """Both calls against the oracle and the per-document fetch; returns (offsets, runs, oracle results)."""
    offs, runs = engine.mt_prop_runs()
    poffs, props = engine.mt_props_all()
    assert offs.dtype == np.uint64 and runs.dtype == native.PROP_RUN_DTYPE and props.dtype == native.PROPSET_DTYPE
    assert len(offs) == len(poffs) == batch.n_docs + 1 and int(offs[-1]) == len(runs) and int(poffs[-1]) == len(props)
    rc, oh, ol, oc, op, _ = orc.mt_replay_batch(batch, threads=16, **CAPS)
    for d in range(batch.n_docs):
        got = runs[int(offs[d]) : int(offs[d + 1])]
        table = props[int(poffs[d]) : int(poffs[d + 1])]
        if int(hdrs[d]["status"]) != 0:
            assert len(got) == 0 and len(table) == 0, d
            continue
        assert int(oh[d]["status"]) == 0 and int(oh[d]["n_leaves"]) == int(hdrs[d]["n_leaves"]), d
        want = expected_runs(oh[d], ol[d], op[d])
        assert len(got) == len(want), d
        for f in STRUCT:
            assert np.array_equal(got[f], want[f]), (d, f)
        assert [_entries(table, int(p)) for p in got["props"]] == [_entries(op[d], int(p)) for p in want["props"]], d
        assert int(got["len"].sum()) == int(hdrs[d]["visible_len"]), d
        leaves, chars, own = engine.mt_doc(d, hdrs[d])
        assert table.tobytes() == own.tobytes(), d
        assert got.tobytes() == expected_runs(hdrs[d], leaves, own).tobytes(), d
    return offs, runs, (oh, ol, op)


def test_farm(orc, engine):
    batch = runs_cases.farm_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    offs, runs, (oh, ol, op) = _check(orc, engine, batch, hdrs)
    multi, several = runs_cases.vacuity(offs, runs, oh, ol)
    assert multi >= 1 and several >= 1  # runs of two or more leaves, documents of two or more runs


def test_chunk_edges(orc, engine):
    batch, docs = runs_cases.edge_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    assert [int(n) for n in hdrs["n_leaves"]] == [n for _, n, _, _, _, _ in docs]
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    assert np.diff(offs).tolist() == [n_runs for _, _, _, _, _, n_runs in docs]
    by = {name: d for d, (name, *_) in enumerate(docs)}
    of = lambda name: runs[int(offs[by[name]]) : int(offs[by[name] + 1])]  # noqa: E731
    poffs, props = engine.mt_props_all()
    for n in (63, 64, 65, 129):
        assert of(f"one_class_{n}")[["start", "len", "first_leaf"]].tolist() == [(0, n, 0)]
        assert of(f"alternating_{n}")["first_leaf"].tolist() == list(range(n))
    assert of("change_63_64")[STRUCT].tolist() == [(0, 64, 0, 0), (64, 65, 64, 0)]
    assert of("change_64_65")[STRUCT].tolist() == [(0, 65, 0, 0), (65, 64, 65, 0)]
    assert of("removed_between")[STRUCT].tolist() == [(0, 64, 0, 0)]
    assert of("removed_lane_63")[STRUCT].tolist() == [(0, 128, 0, 0)]
    assert of("removed_lane_0")[STRUCT].tolist() == [(0, 127, 1, 0)]
    assert of("removed_63_then_change")[STRUCT].tolist() == [(0, 63, 0, 0), (63, 65, 64, 0)]
    assert of("removed_64_then_same")[STRUCT].tolist() == [(0, 128, 0, 0)]
    assert of("markers_ends_and_64")[STRUCT].tolist() == [(0, 1, 0, 1), (1, 63, 1, 0), (64, 1, 64, 1), (65, 63, 65, 0), (128, 1, 128, 1)]
    assert of("markers_adjacent")["flags"].tolist() == [0, 1, 1, 0]
    assert of("marker_removed_between")[STRUCT].tolist() == [(0, 2, 0, 0)]
    # {"a":1,"b":2} next to {"b":2,"a":1}: two records of one class, the run names the lower
    d = by["ab_ba"]
    table = props[int(poffs[d]) : int(poffs[d + 1])]
    leaves, _, _ = engine.mt_doc(d, hdrs[d])
    ids = sorted(int(p) for p in leaves["props"])
    assert ids[0] != ids[1] and native.propset_entries(table, ids[0]) != native.propset_entries(table, ids[1])
    assert of("ab_ba")[["len", "props"]].tolist() == [(2, ids[0])]
    # a leaf whose only key was annotated to null next to a leaf without props
    assert of("null_annotated")[["len", "props"]].tolist() == [(2, NO_CLASS)]


def test_tile_edges(orc, engine):
    T = native.text_tile_leaves()
    batch, docs = runs_cases.tile_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    from mt_compare import emu_caps

    assert [int(n) for n in hdrs["n_leaves"]] == [T + 40] * 3
    assert emu_caps(False)[0] < T + 40 <= emu_caps(True)[0]  # past the small tier's leaves, within the large tier's
    assert not len(native.mt_plan(batch).huge_docs)
    assert [int(x) for x in np.diff(native.text_plan(hdrs).doc_first)] == [2, 2, 2]
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    first = {}
    for d, (name, specs, removed) in enumerate(docs):
        leaves, _, table = engine.mt_doc(d, hdrs[d])
        assert (leaves["len"] == 1).all()
        for k in removed:
            assert int(leaves[k]["rm_seq"]) != text_cases.NOT_REMOVED
        assert int((leaves["rm_seq"] != text_cases.NOT_REMOVED).sum()) == len(removed)
        first[name] = {int(r["first_leaf"]): r for r in runs[int(offs[d]) : int(offs[d + 1])]}
        if name != "markers":
            span = {int(leaves[k]["props"]) for k in range(T - 3, T + 4)}
            assert len(span) == 1 and int(leaves[T - 4]["props"]) not in span and int(leaves[T + 4]["props"]) not in span
        else:
            assert all(int(leaves[k]["pad"]) & text_cases.LEAF_MARKER for k in (T - 1, T))
    assert int(first["span"][T - 3]["len"]) == 7 and not [k for k in first["span"] if T - 3 < k <= T + 3]
    assert int(first["span_removed"][T - 3]["len"]) == 6 and not [k for k in first["span_removed"] if T - 3 < k <= T + 3]
    assert [int(first["markers"][k]["flags"]) for k in (T - 2, T - 1, T, T + 1)] == [0, 1, 1, 0]


def test_tiers(orc, engine):
    from test_gpu_text import tier_batch

    T = native.text_tile_leaves()
    batch, huge = tier_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    assert [int(x) for x in native.mt_plan(batch).huge_docs] == [huge]
    plan = native.text_plan(hdrs)
    assert int(plan.doc_first[huge + 1] - plan.doc_first[huge]) >= 3
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    # alternating classes and leaf T - 1 removed: leaves T - 2 and T are one run across the tile edge
    mine = runs[int(offs[huge]) : int(offs[huge + 1])]
    assert mine[mine["len"] > 1][STRUCT].tolist() == [(T - 2, 2, T - 2, 0)]
    # a huge document whose middle tile lies wholly inside one run
    batch, huge = runs_cases.huge_middle_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all() and [int(x) for x in native.mt_plan(batch).huge_docs] == [huge]
    leaves, _, _ = engine.mt_doc(huge, hdrs[huge])
    assert len(leaves) == 2 * T + 53 and (leaves["len"] == 1).all()  # still one leaf per segment
    assert len({int(p) for p in leaves[T - 5 : 2 * T + 6]["props"]}) == 1
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    mine = runs[int(offs[huge]) : int(offs[huge + 1])]
    long = mine[mine["len"] > 1]
    assert long[STRUCT].tolist() == [(T - 5, T + 11, T - 5, 0)]
    assert len(mine) == (T - 5) + 1 + (2 * T + 52 - (2 * T + 6)) + 1


def test_obliterate_fixtures(orc, engine):
    from golden_data import prefix_batch, replay_fixtures

    fx = [(name, b, ge[-1:], ini, res[-1:]) for name, b, ge, ini, res in
          list(replay_fixtures("replay_obliterate_2.3.0.npz"))[:8]]
    batch, _ = prefix_batch(fx)
    assert batch.n_docs == 8
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    _check(orc, engine, batch, hdrs)


def test_local_views_with_pending_ops(orc, engine):
    batch = runs_cases.pending_local_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    last = engine.mt_formatted(batch.keys, batch.values)[-1]
    assert "".join(t for t, _, _ in last) == ">01PENDING234ote56789"
    assert [t for t, p, _ in last if p == {"bold": True}] == ["1PE"]  # the pending annotate: two leaves, one run


def test_failed_documents_have_empty_spans(orc, engine):
    from test_gpu_text import failing_batch

    batch, bad, refused = failing_batch()
    hdrs = _run(engine, batch)
    status = [int(x) for x in hdrs["status"]]
    assert status[bad] == native.FMT_E_DATA and status[refused] != 0
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    poffs, _ = engine.mt_props_all()
    for d in (bad, refused):
        assert offs[d] == offs[d + 1] and poffs[d] == poffs[d + 1]
    assert int(offs[1]) >= 1 and int(offs[-1]) > int(offs[-2])
    assert engine.mt_formatted(batch.keys, batch.values)[bad] is None


def _raw(engine, fn, offs, out, cap):
    return getattr(engine.L, fn)(engine.h, None if offs is None else native._ptr(offs), None if out is None else native._ptr(out), cap)


@pytest.mark.parametrize("fn,dtype", [("fmt_mt_fetch_prop_runs_all", native.PROP_RUN_DTYPE),
                                      ("fmt_mt_fetch_props_all", native.PROPSET_DTYPE)])
def test_contract(orc, engine, fn, dtype):
    batch = runs_cases.farm_batch()
    engine.mt_load(batch)
    offs = np.zeros(batch.n_docs + 1, dtype=np.uint64)
    assert _raw(engine, fn, offs, None, 0) == native.FMT_E_USAGE  # before the run
    assert b"before fmt_mt_run" in engine.L.fmt_last_error(engine.h)
    engine.mt_run()
    assert _raw(engine, fn, offs, None, 0) == native.FMT_OK  # the sizing call
    sized = offs.copy()
    total = int(offs[-1])
    assert total > 0 and (np.diff(offs.astype(np.int64)) >= 0).all()
    sentinel = np.frombuffer(b"\xAB" * (total * dtype.itemsize), dtype=dtype).copy()
    out = sentinel.copy()
    offs[:] = 0
    assert _raw(engine, fn, offs, out, total - 1) == native.FMT_E_USAGE  # one record short
    assert out.tobytes() == sentinel.tobytes() and np.array_equal(offs, sized)
    assert _raw(engine, fn, None, out, total) == native.FMT_E_USAGE  # offsets are required
    assert _raw(engine, fn, offs, out, total) == native.FMT_OK and np.array_equal(offs, sized)
    again = sentinel.copy()
    assert _raw(engine, fn, offs, again, total) == native.FMT_OK
    assert out.tobytes() == again.tobytes() and out.tobytes() != sentinel.tobytes()  # two calls, equal bytes
    bulk = engine.mt_prop_runs() if dtype == native.PROP_RUN_DTYPE else engine.mt_props_all()
    assert np.array_equal(bulk[0], sized) and bulk[1].tobytes() == out.tobytes()


def test_runs_texts_and_summaries_do_not_disturb_each_other(orc, engine):
    import v1_bulk

    batch = v1_bulk.farm_batch()
    hdrs = _run(engine, batch)
    n = batch.n_docs
    offs, runs, _ = _check(orc, engine, batch, hdrs)
    texts = engine.mt_texts(0)
    engine.mt_summarize_legacy(batch.keys, batch.values)
    blobs = [engine.mt_summary(d) for d in range(n)]
    o2, r2 = engine.mt_prop_runs()
    assert np.array_equal(o2, offs) and r2.tobytes() == runs.tobytes()
    assert [engine.mt_summary(d) for d in range(n)] == blobs
    # a text read and a summary between the sizing call and the fill
    o3 = np.zeros(n + 1, dtype=np.uint64)
    assert _raw(engine, "fmt_mt_fetch_prop_runs_all", o3, None, 0) == native.FMT_OK
    t2 = engine.mt_texts(0x20)
    engine.mt_summarize_legacy(batch.keys, batch.values)
    out = np.zeros(len(runs), dtype=native.PROP_RUN_DTYPE)
    assert _raw(engine, "fmt_mt_fetch_prop_runs_all", o3, out, len(out)) == native.FMT_OK
    assert np.array_equal(o3, offs) and out.tobytes() == runs.tobytes()
    again = engine.mt_texts(0)
    assert np.array_equal(again[0], texts[0]) and np.array_equal(again[1], texts[1]) and len(t2[1]) >= len(texts[1])
    assert [engine.mt_summary(d) for d in range(n)] == blobs


def test_engine_reuse_gives_the_second_batch(orc, engine):
    T = native.text_tile_leaves()
    big, _ = runs_cases.huge_middle_batch(T)
    _run(engine, big)
    first = engine.mt_prop_runs()
    small = workloads.conflict_farm(5, n_clients=4, ops_per_doc=150, seed=31)
    hdrs = _run(engine, small)
    offs, runs, _ = _check(orc, engine, small, hdrs)
    assert len(runs) != len(first[1])
    fresh = native.Engine(0)
    try:
        _run(fresh, small)
        other = fresh.mt_prop_runs()
    finally:
        fresh.close()
    assert np.array_equal(offs, other[0]) and runs.tobytes() == other[1].tobytes()


# ---- hosts
def _formatted_per_document(engine, batch, hdrs, placeholder):
    """mt_formatted restated a document at a time from mt_doc: walk the visible leaves, join text while the
    resolved property dicts are equal."""
    out = []
    for d in range(batch.n_docs):
        if int(hdrs[d]["status"]) != 0:
            out.append(None)
            continue
        leaves, chars, table = engine.mt_doc(d, hdrs[d])
        doc = []
        for L in leaves:
            if int(L["rm_seq"]) != text_cases.NOT_REMOVED:
                continue
            marker = bool(int(L["pad"]) & text_cases.LEAF_MARKER)
            pid = int(L["props"])
            props = None
            if pid != NO_CLASS and int(table[pid]["n"]):
                props = {batch.keys[e >> 16]: json.loads(batch.values[e & 0xFFFF]) for e in native.propset_entries(table, pid)}
            o = int(L["char_off"])
            text = (chr(placeholder) if placeholder else "") if marker else \
                chars[o : o + int(L["len"])].tobytes().decode("utf-16-le", "surrogatepass")
            if doc and not marker and not doc[-1][2] and doc[-1][1] == props:
                doc[-1][0] += text
            else:
                doc.append([text, props, marker])
        out.append([tuple(x) for x in doc])
    return out


def test_formatted_equals_a_per_document_restatement(orc, engine):
    for batch in (runs_cases.farm_batch(), runs_cases.edge_batch()[0]):
        hdrs = _run(engine, batch)
        for ph in (0, 0x20):
            assert engine.mt_formatted(batch.keys, batch.values, ph) == _formatted_per_document(engine, batch, hdrs, ph)
    got = engine.mt_formatted(batch.keys, batch.values)
    by = {name: d for d, (name, *_) in enumerate(runs_cases.edge_documents())}
    assert got[by["ab_ba"]] == [("xx", {"a": 1, "b": 2}, False)] and got[by["null_annotated"]] == [("xx", None, False)]
    assert [(t, m) for t, _, m in got[by["markers_adjacent"]]] == [("x", False), ("", True), ("", True), ("x", False)]


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_js_formatted_equals_python_on_the_farm(orc, engine, tmp_path):
    from test_napi_text import _write

    farm = runs_cases.farm_batch()
    _write(tmp_path, farm, [], 0)
    env = dict(os.environ, FMT_NAPI_BACKTRACE=os.environ.get("FMT_NAPI_BACKTRACE", "1"))
    r = subprocess.run([NODE, os.path.join(REPO, "tests", "js", "runs_driver.js"), str(tmp_path)], capture_output=True,
                       text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    _run(engine, farm)
    for key, ph in (("plain", 0), ("spaced", 0x20)):
        want = [[[t, p, m] for t, p, m in doc] for doc in engine.mt_formatted(farm.keys, farm.values, ph)]
        assert got[key] == want, key
    assert got["refusedWhileBusy"] is True
    assert sum(len(doc) for doc in got["plain"]) == int(engine.mt_prop_runs()[0][-1]) > farm.n_docs

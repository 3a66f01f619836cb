"""GPU: fmt_mt_fetch_text_all (include/fmt_text.h, csrc/text.hip) against the definition restated over
the oracle's replay of the same batch (text_cases.expected_units) and against visible_text of the
per-document fetch, bit for bit on uint16 units and uint64 offsets."""
import numpy as np
import pytest

import text_cases
from fluidframework_amd import native, workloads
from fluidframework_amd.streams import MergeTreeStreamBuilder
from mt_compare import visible_text
from text_cases import expected_units, msg, units_of

pytestmark = pytest.mark.gpu
SPACE = 0x20
CAPS = dict(cap_leaves=4096, cap_chars=1 << 17, cap_props=1024)


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _run(engine, batch):
    engine.mt_load(batch)
    engine.mt_run()
    return engine.mt_headers(raise_on_failed_docs=False)


def _expected(orc, batch, hdrs, placeholder):
    """Offsets and units from the oracle's state; a document the engine did not finish has no units."""
    rc, oh, ol, oc, op, _ = orc.mt_replay_batch(batch, threads=16, **CAPS)
    parts = []
    for d in range(batch.n_docs):
        ok = int(hdrs[d]["status"]) == 0
        if ok:
            assert int(oh[d]["status"]) == 0 and int(oh[d]["n_leaves"]) == int(hdrs[d]["n_leaves"]), d
        parts.append(expected_units(oh[d], ol[d], oc[d], placeholder) if ok else np.zeros(0, "<u2"))
    offs = np.zeros(batch.n_docs + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return offs, np.concatenate(parts) if parts else np.zeros(0, "<u2")


def _check(orc, engine, batch, hdrs, placeholders=(0, SPACE), per_doc=True):
    for ph in placeholders:
        offs, units = engine.mt_texts(ph)
        want_offs, want = _expected(orc, batch, hdrs, ph)
        assert offs.dtype == np.uint64 and units.dtype == np.dtype("<u2")
        assert np.array_equal(offs, want_offs), ph
        assert np.array_equal(units, want), ph
        if ph:
            ok = hdrs["status"] == 0
            assert np.array_equal(np.diff(offs)[ok], hdrs["visible_len"][ok].astype(np.uint64))
    if per_doc:
        strings = engine.mt_text_strings(0)
        for d in range(batch.n_docs):
            if int(hdrs[d]["status"]) == 0:
                leaves, chars, _ = engine.mt_doc(d, hdrs[d])
                assert strings[d] == visible_text(hdrs[d], leaves, chars), d
            else:
                assert strings[d] == ""


def farm_batch():
    return workloads.conflict_farm(64, n_clients=8, ops_per_doc=200, seed=23)


def test_farm(orc, engine):
    batch = farm_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    _check(orc, engine, batch, hdrs)


def test_chunk_and_copy_edges(orc, engine):
    batch, docs = text_cases.edge_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    assert [int(n) for n in hdrs["n_leaves"]] == [n for _, n, _ in docs]
    _check(orc, engine, batch, hdrs)
    by = {name: d for d, (name, _, _) in enumerate(docs)}
    s, sp = engine.mt_text_strings(0), engine.mt_text_strings(SPACE)
    assert s[by["empty"]] == "" and s[by["all_removed"]] == "" and s[by["one"]] == "x"
    assert [len(s[by[k]]) for k in ("63", "64", "65")] == [63, 64, 65]
    alpha = "".join(chr(ord("a") + k % 26) for k in range(64))
    assert s[by["removed_ends"]] == alpha[1:63]
    assert s[by["long_leaf"]] == "a" + "".join(chr(0x100 + i) for i in range(300)) + "z"
    assert s[by["markers"]] == "onetwo" and sp[by["markers"]] == " onetwo "
    odd = "a\ud800b\udfffc\uffffde\u0000f\u0000"
    assert np.array_equal(units_of(s[by["odd_units"]]), units_of(odd))


GROWTH = ((5, 7), (60, 4), (120, 5), (400, 2), (20, 3), (120, 8))  # (ops, seed) of tier_batch's growth documents
HUGE_AT = 4                                                           # the huge document's index: after four of them


def tier_batch(T):
    """Growth documents that finish in the micro, compact, small and large tiers (test_tile_edges_and_tiers
    checks which), and in their middle one summary-loaded document of 2T + 52 one-unit segments (the
    huge tier), whose leaf T - 1 is removed and whose leaf T stays: the tile edge."""
    import growth

    n = 2 * T + 52
    b = MergeTreeStreamBuilder()

    def grow(n_ops, seed):
        d = b.begin_doc("", observer="observer")
        for m in growth.growth_messages(n_ops=n_ops, seed=seed, initial=""):
            d.add_message(m)

    for n_ops, seed in GROWTH[:HUGE_AT]:
        grow(n_ops, seed)
    texts = [{"text": chr(0x4E00 + i), "props": {"k": i % 2}} for i in range(n)]
    h = b.begin_doc_from_summary(text_cases.summary_header(texts), observer="observer")
    h.add_message(msg("B", 1, {"type": 1, "pos1": T - 1, "pos2": T}))
    for n_ops, seed in GROWTH[HUGE_AT:]:
        grow(n_ops, seed)
    return b.finish(), HUGE_AT


def growth_tiers():
    """The tier each growth document of tier_batch finishes in and its header there: the engine's own
    source compiled for the CPU, launched tier by tier as the runtime does (micro_cascade.Cascade,
    DESIGN.md section 6). Each document replays alone, so the batch around it does not matter."""
    import growth
    import micro_cascade as mc

    c = mc.Cascade(growth.growth_batch([("", n_ops, seed) for n_ops, seed in GROWTH]))
    for tier in (mc.MICRO, mc.COMPACT, mc.SMALL, mc.LARGE):
        c.run(tier)
    return [int(t) for t in c.done_in], c.hdr, mc


def test_tile_edges_and_tiers(orc, engine):
    T = native.text_tile_leaves()
    batch, huge = tier_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    # the tiers: the cascade puts the growth documents in micro, compact, small, large, micro, small, and
    # what the GPU returned for them is that tier's result; the plan routes the loaded document to the huge tier
    tiers, emu, mc = growth_tiers()
    assert tiers == [mc.MICRO, mc.COMPACT, mc.SMALL, mc.LARGE, mc.MICRO, mc.SMALL]
    others = [d for d in range(batch.n_docs) if d != huge]
    for k, d in enumerate(others):
        for f in ("status", "n_leaves", "n_chars", "n_props", "visible_len", "cur_seq"):
            assert int(hdrs[d][f]) == int(emu[k][f]), (d, f)
        leaf_cap, char_cap = mc.caps(tiers[k])
        assert int(hdrs[d]["n_leaves"]) <= leaf_cap and int(hdrs[d]["n_chars"]) <= char_cap
        if tiers[k] > mc.MICRO:  # it did not fit the tier below at its end either
            below = mc.caps(tiers[k] - 1)
            assert int(hdrs[d]["n_leaves"]) > below[0] or int(hdrs[d]["n_chars"]) > below[1]
    assert [int(x) for x in native.mt_plan(batch).huge_docs] == [huge]
    assert int(hdrs[huge]["n_leaves"]) >= 2 * T + 5 and (hdrs["n_leaves"] > T).sum() == 1
    plan = native.text_plan(hdrs)
    assert int(plan.doc_first[huge + 1] - plan.doc_first[huge]) >= 3
    leaves, cc, _ = engine.mt_doc(huge, hdrs[huge])
    assert int(leaves[T - 1]["rm_seq"]) != text_cases.NOT_REMOVED and int(leaves[T]["rm_seq"]) == text_cases.NOT_REMOVED
    _check(orc, engine, batch, hdrs)
    s = engine.mt_text_strings(0)[huge]
    n = 2 * T + 52
    assert s == "".join(chr(0x4E00 + i) for i in range(n) if i != T - 1)


def test_obliterate_farm(orc, engine):
    from golden_data import prefix_batch, replay_fixtures

    fx = [(name, b, ge[-1:], ini, res[-1:]) for name, b, ge, ini, res in
          list(replay_fixtures("replay_obliterate_2.3.0.npz"))[:8]]
    batch, texts = prefix_batch(fx)
    assert batch.n_docs == 8
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    _check(orc, engine, batch, hdrs)
    assert engine.mt_text_strings(0) == list(texts)


def test_local_views_with_pending_ops(orc, engine):
    batch = text_cases.pending_local_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    _check(orc, engine, batch, hdrs)
    assert engine.mt_text_strings(0)[-1] == ">01PENDING234ote56789"
    assert engine.mt_text_strings(0) == [text_cases.oracle_doc(orc, batch, d).text() for d in range(batch.n_docs)]


def failing_batch():
    """good, FMT_E_DATA (an insert past the end), good, a local farm, a document the plan refuses (2,100
    loaded segments in a batch with local records: no tier holds it), good."""
    import local_farm

    b = MergeTreeStreamBuilder()

    def good(text):
        d = b.begin_doc(text, observer="observer")
        d.add_message(msg("B", 1, {"type": 0, "pos1": 1, "seg": "+"}))

    good("first")
    d = b.begin_doc("ab", observer="observer")
    d.add_message(msg("B", 1, {"type": 0, "pos1": 5, "seg": "x"}))
    good("second")
    local_farm.LocalFarm(7, builder=b).run(60)
    n_farm = len(b.docs) - 3
    b.begin_doc_from_summary(text_cases.summary_header(["s"] * 2100), observer="observer")
    good("last")
    return b.finish(), 1, 3 + n_farm


def test_failed_documents_have_empty_spans(orc, engine):
    batch, bad, refused = failing_batch()
    hdrs = _run(engine, batch)
    status = [int(x) for x in hdrs["status"]]
    assert status[bad] == native.FMT_E_DATA and status[refused] != 0
    assert [s for d, s in enumerate(status) if d not in (bad, refused)] == [0] * (batch.n_docs - 2)
    _check(orc, engine, batch, hdrs)
    s = engine.mt_text_strings(0)
    assert (s[0], s[bad], s[2], s[refused], s[-1]) == ("f+irst", "", "s+econd", "", "l+ast")


def _raw(engine, placeholder, offs, out, cap):
    return engine.L.fmt_mt_fetch_text_all(engine.h, placeholder, native._ptr(offs), None if out is None else native._ptr(out), cap)


def test_contract(orc, engine):
    batch = farm_batch()
    engine.mt_load(batch)
    offs = np.zeros(batch.n_docs + 1, dtype=np.uint64)
    assert _raw(engine, 0, offs, None, 0) == native.FMT_E_USAGE  # before the run
    assert b"before fmt_mt_run" in engine.L.fmt_last_error(engine.h)
    engine.mt_run()
    hdrs = engine.mt_headers()
    want_offs, want = _expected(orc, batch, hdrs, 0)
    assert _raw(engine, 0, offs, None, 0) == native.FMT_OK and np.array_equal(offs, want_offs)  # offsets only
    total = int(offs[-1])
    out = np.full(total, 0xABCD, dtype="<u2")
    offs[:] = 0
    assert _raw(engine, 0, offs, out, total - 1) == native.FMT_E_USAGE  # one unit short
    assert (out == 0xABCD).all() and np.array_equal(offs, want_offs)
    assert _raw(engine, 0, None, out, total) == native.FMT_E_USAGE  # offsets are required
    assert _raw(engine, 0, offs, out, total) == native.FMT_OK and np.array_equal(out, want)


def test_placeholders_do_not_leak_into_each_other(orc, engine):
    from marker_docs import marker_batch

    batch = marker_batch(6, 200, seed=9)
    hdrs = _run(engine, batch)
    want = {ph: _expected(orc, batch, hdrs, ph) for ph in (0, SPACE, 0xFFFC)}
    assert len(want[SPACE][1]) > len(want[0][1])
    for ph in (0, SPACE, 0, 0xFFFC, SPACE, 0):
        offs, units = engine.mt_texts(ph)
        assert np.array_equal(offs, want[ph][0]) and np.array_equal(units, want[ph][1]), ph
    # the sizing call of one placeholder, then the fill of another
    offs = np.zeros(batch.n_docs + 1, dtype=np.uint64)
    assert _raw(engine, SPACE, offs, None, 0) == native.FMT_OK
    out = np.zeros(int(want[0][0][-1]), dtype="<u2")
    assert _raw(engine, 0, offs, out, len(out)) == native.FMT_OK
    assert np.array_equal(offs, want[0][0]) and np.array_equal(out, want[0][1])


def test_summaries_and_texts_do_not_disturb_each_other(orc, engine):
    import v1_bulk

    batch = v1_bulk.farm_batch()
    hdrs = _run(engine, batch)
    n = batch.n_docs
    engine.mt_summarize_legacy(batch.keys, batch.values)
    before = [engine.mt_summary(d) for d in range(n)]
    offs, units = engine.mt_texts(0)
    want_offs, want = _expected(orc, batch, hdrs, 0)
    assert np.array_equal(offs, want_offs) and np.array_equal(units, want)
    assert [engine.mt_summary(d) for d in range(n)] == before  # the blobs made before the text call
    engine.mt_summarize_legacy(batch.keys, batch.values)
    assert [engine.mt_summary(d) for d in range(n)] == before
    # a V1 summary between the sizing call and the fill, and after
    o2 = np.zeros(n + 1, dtype=np.uint64)
    assert _raw(engine, 0, o2, None, 0) == native.FMT_OK
    engine.mt_summarize_v1(batch.keys, batch.values, v1_bulk.all_names(batch))
    v1 = [engine.mt_summary_v1(d) for d in range(n)]
    out = np.zeros(len(want), dtype="<u2")
    assert _raw(engine, 0, o2, out, len(out)) == native.FMT_OK
    assert np.array_equal(o2, want_offs) and np.array_equal(out, want)
    assert [engine.mt_summary_v1(d) for d in range(n)] == v1
    offs, units = engine.mt_texts(0)
    assert np.array_equal(offs, want_offs) and np.array_equal(units, want)


def test_engine_reuse_gives_the_second_batch(orc, engine):
    T = native.text_tile_leaves()
    big, _ = tier_batch(T)
    _run(engine, big)
    engine.mt_texts(SPACE)
    small = workloads.conflict_farm(5, n_clients=4, ops_per_doc=150, seed=31)
    hdrs = _run(engine, small)
    got = engine.mt_texts(SPACE)
    want_offs, want = _expected(orc, small, hdrs, SPACE)
    assert np.array_equal(got[0], want_offs) and np.array_equal(got[1], want)
    fresh = native.Engine(0)
    try:
        _run(fresh, small)
        other = fresh.mt_texts(SPACE)
    finally:
        fresh.close()
    assert np.array_equal(got[0], other[0]) and np.array_equal(got[1], other[1])

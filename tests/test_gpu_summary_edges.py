"""The summary-edge corpus (tests/summary_edges.py) on the GPU: summaryRunsKernel, summaryV1Kernel and
the host formatters against both references, every family as it is, escalated to the large tier and
escalated to the huge tier. Per family and tier: one load, one run, then one mt_summarize_legacy and
one mt_summarize_v1 per chunk size (1, each document's own total - 1 and total, 10000). Expected
bytes come from oracle.mt_replay_summary, summary.legacy_summary over the fetched state and
v1_bulk.reference over the oracle's state; the census promises are checked on the fetched state,
which is what the kernels read."""
from collections import Counter

import pytest

import summary_edges as se
from fluidframework_amd import native, summary

pytestmark = pytest.mark.gpu

SMALL_TIER_CHARS = 2048  # the small tier's text (test_gpu_parity.test_mt_large_documents_escalate_to_large_tier)


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _is_huge(engine, d):
    try:
        engine.huge_profile(d)
    except native.EngineError as err:
        assert err.code == native.FMT_E_USAGE
        return False
    return True


@pytest.mark.parametrize("tier", se.TIERS)
@pytest.mark.parametrize("family", list(se.FAMILIES))
def test_family_equals_both_references(orc, engine, family, tier):
    bt, names = se.batch(family, tier)
    adjust = bt.adjusts is not None
    engine.mt_load(bt)
    engine.mt_run()
    hdrs = engine.mt_headers()
    assert (hdrs["status"] == 0).all()
    state, seen = [], Counter()
    for d in range(bt.n_docs):
        h = hdrs[d]
        if tier == "large":
            assert SMALL_TIER_CHARS < int(h["n_chars"]) <= native.capacity()[1] and not _is_huge(engine, d), names[d]
        if tier == "huge":
            assert int(h["n_chars"]) > native.capacity()[1] and _is_huge(engine, d), names[d]
        lv, ch, pr = engine.mt_doc(d, h)
        view = engine.mt_legacy_props(d, h) if adjust else None
        vals = summary.values_with_numbers(bt.values, engine.mt_numbers(d)) if adjust else bt.values
        state.append((h, lv, ch, pr, view, vals))
        cen, runs = se.census(h, lv, ch, pr, int(h["min_seq"]), view)
        seen += cen
        assert runs == [summary._utf16_len(t) for t, _, _ in summary.legacy_segments(h, lv, ch, pr, int(h["min_seq"]), view)], names[d]
    assert [k for k in se.promises(family, tier) if not seen[k]] == []
    if family == "first_remover":
        facts = {name: se.remover_census(bt, d, state) for d, name in enumerate(names)}
        assert [facts[f"{n}_records"]["n_records"] for n in (64, 65, 4097)] == [64, 65, 4097]
        assert all(facts[f"{n}_records"][k] == 1 for n in (64, 65, 4097) for k in ("first", "middle", "last"))
        assert facts["remover_second_in_group"]["not_first_of_seq"] >= 1 and facts["loaded_then_removed"]["loadseg_prefix"] == 3

    want = se.legacy_reference(family, tier)
    for chunk in sorted({c for _, c in want}):
        engine.mt_summarize_legacy(bt.keys, bt.values, chunk=chunk)
        for d in [d for d, c in want if c == chunk]:
            h, lv, ch, pr, view, vals = state[d]
            got = engine.mt_summary(d)
            assert got == want[d, chunk], (names[d], chunk)
            assert got == summary.legacy_summary(h, lv, ch, pr, bt.keys, vals, chunk, view), (names[d], chunk)

    want = se.v1_reference(family, tier)
    clients = [bt.clients[d] for d in range(bt.n_docs)]
    for chunk in sorted({c for _, c in want}):
        engine.mt_summarize_v1(bt.keys, bt.values, clients, chunk=chunk)
        for d in [d for d, c in want if c == chunk]:
            assert engine.mt_summary_v1(d) == want[d, chunk], (names[d], chunk)


def test_a_failed_neighbour_keeps_its_status(orc, engine):
    bt = se.neighbours_batch()
    engine.mt_load(bt)
    engine.mt_run()
    hdrs = engine.mt_headers(raise_on_failed_docs=False)
    assert [int(s) for s in hdrs["status"]] == [0, native.FMT_E_DATA, 0]
    engine.mt_summarize_legacy(bt.keys, bt.values)
    engine.mt_summarize_v1(bt.keys, bt.values, [bt.clients[d] for d in range(bt.n_docs)])
    for fetch in (engine.mt_summary, engine.mt_summary_v1):
        with pytest.raises(native.EngineError) as err:
            fetch(1)
        assert err.value.code == native.FMT_E_DATA
    rc, oh, ol, oc, op, _ = orc.mt_replay_batch(bt, cap_leaves=se.CAP_LEAVES, cap_chars=1 << 14, cap_props=se.CAP_PROPS)
    for d in (0, 2):
        assert engine.mt_summary(d) == orc.mt_replay_summary(bt, d, bt.keys, bt.values), d
        h = hdrs[d]
        lv, ch, pr = engine.mt_doc(d, h)
        assert engine.mt_summary(d) == summary.legacy_summary(h, lv, ch, pr, bt.keys, bt.values), d
        assert engine.mt_summary_v1(d) == summary.v1_summary(oh[d], ol[d], oc[d], op[d], bt.keys, bt.values, bt.clients[d],
                                                             orc.mt_removers(bt, d)), d

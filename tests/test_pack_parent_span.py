"""packParent scours the children of one parent block in one pass (csrc/mt_engine.h scourSpan): one find,
one char offset, one text move and one compaction of the leaf registers for the whole span, with the
decisions of the per-block scour and nothing appended across a block boundary. The directed documents of
pack_span_docs.py through every instantiation under host emulation, and the same documents and a T1-shaped
batch on the device; every compared field, the state digest and the visible text against the oracle's.

The largest span a packParent can see is 45 leaves, not 7 x 7: it starts from a block that is left with
fewer than four (`full_span_7x7`). The adjust documents carry managers on leaves that the span appends and
drops, the sided obliterates live references on leaves that it appends (pack_span_docs.add_doc2).
"""
import numpy as np
import pytest

import pack_span_docs as pd
from descend_cascade import DescendCascade
from digest import state_digest
from micro_cascade import COMPACT, LARGE, MICRO, OK, SMALL
from mt_compare import compare_doc, emu_replay, emu_replay_local, visible_text

TIERS = {"micro": MICRO, "compact": COMPACT, "small": SMALL, "large": LARGE}
CAPS = dict(cap_leaves=2048, cap_chars=1 << 14, cap_props=1024)


def _ref(orc, bt, threads=8):
    ref = orc.mt_replay_batch(bt, threads=threads, **CAPS)[:5]
    assert ref[0] == 0 and (ref[1]["status"] == OK).all()
    return ref


@pytest.fixture(scope="module")
def plain(orc):
    bt, names = pd.plain_batch()
    return bt, names, _ref(orc, bt)


@pytest.fixture(scope="module")
def wide(orc):
    bt, names = pd.wide_batch()
    return bt, names, _ref(orc, bt)


def _same(ref, d, got):
    rc, oh, ol, oc, op = ref
    exp = (oh[d], ol[d], oc[d], op[d])
    assert not compare_doc(exp, got), d
    assert state_digest(*got) == state_digest(*exp), d
    assert visible_text(*got[:3]) == visible_text(*exp[:3]), d


def test_documents_are_what_they_are_meant_to_be(plain, wide):
    """The oracle's final leaf count, block count and depth: a document that no longer reaches packParent,
    or in which a pair merges that must not (or does not that must), fails here."""
    for (bt, names, (rc, oh, ol, oc, op)), cases in ((plain, pd.plain_cases()), (wide, pd.wide_cases())):
        for d, name in enumerate(names):
            specs, gone, n_blocks, depth = cases[name]
            assert int(oh[d]["n_leaves"]) == len(specs) - gone, name
            assert (int(oh[d]["n_blocks"]), int(oh[d]["depth"])) == (n_blocks, depth), name
    bt, names, (rc, oh, ol, oc, op) = plain
    d = names.index("pair_across_blocks")  # "ab" | "cd" ended on two sides of a boundary, twice
    assert list(ol[d]["len"][7:9]) == [2, 2] and ol[d]["block"][7] != ol[d]["block"][8]
    d = names.index("pair_inside_child")
    assert 4 in ol[d]["len"][: int(oh[d]["n_leaves"])]
    d = names.index("straddle_63_64")  # (two drops in front of them: leaves 63 | 64 became leaf 61)
    assert ol[d]["len"][61] == 4 and visible_text(oh[d], ol[d], oc[d]).count("pqrs") == 1


@pytest.mark.parametrize("tier", list(TIERS))
def test_plain_instantiations_match_oracle(plain, tier):
    bt, names, ref = plain
    cas = DescendCascade(bt)
    st = cas.launch(TIERS[tier], None)
    assert (st == OK).all(), st
    for d in range(bt.n_docs):
        _same(ref, d, cas.doc(d))


@pytest.mark.parametrize("tier", ["compact", "small", "large"])
def test_span_across_leaves_127_128(wide, tier):
    bt, names, ref = wide
    cas = DescendCascade(bt)
    st = cas.launch(TIERS[tier], None)
    assert (st == OK).all(), st
    for d in range(bt.n_docs):
        _same(ref, d, cas.doc(d))


# leaves of four units in the oracle's result: the pairs that merged, per document
VARIANTS = {
    "obliterate": (pd.obliterate_batch, [2, 2]),
    # a manager on the appended leaf of a pair and on a dropped leaf, in two children each; then no managers
    "adjust": (pd.adjust_batch, [2, 2]),
    # a live reference on the appended leaf of the first pair (moved onto its head), on the head of the second
    # pair, and one whose range swallows the second pair's head
    "sided_obliterate": (pd.sided_obliterate_batch, [2, 2, 1]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("large", [False, True])
def test_obliterate_and_adjust_variants_match_oracle(orc, variant, large):
    build, fours = VARIANTS[variant]
    bt = build()
    ref = _ref(orc, bt, threads=4)
    assert [list(ref[2][d]["len"][: int(ref[1][d]["n_leaves"])]).count(4) for d in range(bt.n_docs)] == fours
    if variant == "adjust":  # the adjusted dead leaves are gone like the plain ones: both documents end alike
        assert int(ref[1][0]["n_leaves"]) == int(ref[1][1]["n_leaves"]) == 18
    hdr, lv, ch, pr = emu_replay(bt, large=large)[:4]
    for d in range(bt.n_docs):
        _same(ref, d, (hdr[d], lv[d], ch[d], pr[d]))


@pytest.mark.parametrize("mode", ["small_first", "large_only", "compact_first"])
def test_held_leaf_in_a_middle_child(orc, mode):
    bt = pd.local_batch()
    ref = _ref(orc, bt, threads=4)
    assert [int(x) for x in ref[1]["n_leaves"]] == [14, 12, 13]  # held: nothing merges; not held: three become one
    hdr, lv, ch, pr = emu_replay_local(bt, large_only=mode == "large_only", compact_first=mode == "compact_first")
    for d in range(bt.n_docs):
        _same(ref, d, (hdr[d], lv[d], ch[d], pr[d]))


@pytest.mark.gpu
def test_device_cascade_matches_oracle(orc, plain, wide):
    """256 T1-shaped documents of 600 ops through the whole cascade, then the directed documents."""
    from fluidframework_amd import native, workloads

    eng = native.Engine(0)
    try:
        t1 = workloads.conflict_farm(256, n_clients=8, ops_per_doc=600, seed=11)
        t1_ref = orc.mt_replay_batch(t1, threads=16, cap_leaves=8192, cap_chars=1 << 17, cap_props=1024)[:5]
        assert t1_ref[0] == 0
        for bt, ref in ((t1, t1_ref), (plain[0], plain[2]), (wide[0], wide[2])):
            eng.mt_load(bt)
            eng.mt_run()
            hdrs = eng.mt_headers(raise_on_failed_docs=False)
            assert (hdrs["status"] == OK).all(), np.unique(hdrs["status"])
            for d in range(bt.n_docs):
                lv, ch, pr = eng.mt_doc(d, hdrs[d])
                _same(ref, d, (hdrs[d], lv, ch, pr))
    finally:
        eng.close()

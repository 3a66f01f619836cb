"""The stations and the tour of tests/engine_reuse.py, without a GPU: every station's batch replays on
the oracle, its plan (native.mt_plan, fmt_mt_load's host half) shows exactly the facts its row names,
every fact is present in at least two stations and absent from at least two, the stations stay small,
and the tour holds every ordered pair of stations."""
from collections import Counter

import numpy as np
import pytest

import engine_reuse as er

MT = [s.name for s in er.MT_STATIONS]
MAPS = [s.name for s in er.MAP_STATIONS]


@pytest.mark.parametrize("name", MT)
def test_merge_tree_station_replays_and_plans_as_its_row_says(orc, name):
    s = er.BY_NAME[name]
    o = er.mt_oracle(orc, name)
    assert (o.h["status"] == 0).all()
    assert int(o.h["n_leaves"].sum()) > 0
    assert er.plan_facts(s.batch) == s.facts
    if s.cap_catchup:
        assert int(o.h["n_catchup"].sum()) > 0


def test_stepdown_station_moves_down_a_tier(orc):
    """The row "one step-down": in the host emulation of the cascade (descend_cascade.DescendCascade) the
    document goes up past the compact tier's 256 leaves and steps down again at least once."""
    import descend_cascade

    c = descend_cascade.DescendCascade(er.BY_NAME["stepdown"].batch)
    c.rounds(descend_cascade.ROUNDS)
    assert int(c.downs.sum()) >= 1


@pytest.mark.parametrize("name", MAPS)
def test_map_station_replays(orc, name):
    s, b = er.BY_NAME[name], er.BY_NAME[name].batch
    want = er.map_oracle(orc, name)
    if s.mode == "dense":
        assert (b.key_bound <= 2560) == (name == "map_dense_lds")
        assert int((want["dense"]["value"] != 0xFFFFFFFF).sum()) > 0
        return
    counts = want["sparse"][0]
    assert int(counts.sum()) > 0
    offs = np.asarray(b.doc_op_offsets).astype(np.int64)
    distinct = []  # keys after the document's last clear
    for d in range(b.n_docs):
        ops = b.ops[offs[d]: offs[d + 1]]
        clears = np.flatnonzero(ops["kind_value"] >> 30 == 2)
        distinct.append(len(np.unique(ops["key"][clears[-1] + 1 if len(clears) else 0:])))
    over = max(distinct) > 2048 or int(np.diff(offs).max()) > 16384  # past the LDS tier (fmt.h FMT_MAP_SPARSE_MAX_*)
    assert over == (name in ("map_tiered_keys", "map_tiered_ops")), name
    if s.pending:
        assert len(b.local_ops) > 0 and int(want["pending"][0].sum()) > 0
    if s.summarize:
        live = set(int(c) for c in counts)
        assert {63, 64, 65, 2047, 2048} <= live  # each side of the 64- and 2,048-entry steps


def test_every_fact_is_in_two_stations_and_out_of_two():
    for fact in er.PLAIN:
        have = [s.name for s in er.MT_STATIONS if s.facts[fact]]
        lack = [s.name for s in er.MT_STATIONS if not s.facts[fact]]
        assert len(have) >= 2 and len(lack) >= 2, (fact, have, lack)


def test_plain_station_climbs_the_cascade_with_checkpoints(orc):
    """The row "micro -> compact -> small with checkpoints": no remove order, adjust, obliterate or local
    records (so fmt_mt_load takes the checkpoint slab and the step-down lists), documents that end past
    the compact tier's 256 leaves (they climbed micro -> compact -> small) beside ones that stay below."""
    s = er.BY_NAME["plain"]
    f = er.plan_facts(s.batch)
    assert not (f["rm_order"] or f["any_adjust"] or f["obliterates"] or f["local"])
    n = er.mt_oracle(orc, "plain").h["n_leaves"]
    assert int((n > 256).sum()) >= 2 and int((n <= 256).sum()) >= 2 and int(n.max()) <= 512, sorted(n)


def test_obliterate_station_holds_sided_and_non_sided_ops():
    ops = er.BY_NAME["obliterate"].batch.ops
    assert int((ops["type"] == 4).sum()) > 50 and int((ops["type"] == 5).sum()) > 50
    assert int(((ops["type"] == 5) & (ops["flags"] & 16 != 0)).sum()) > 0  # exclusive ends among the sided ones


def test_escalation_and_value_base_stations(orc):
    """Large-tier escalation: documents past the small tier's 512 leaves, and one batch past 31 writers;
    huge at load: 2,049+ segments; the document-local station carries doc_value_base."""
    assert int((er.mt_oracle(orc, "large_growth").h["n_leaves"] > 512).sum()) >= 2
    assert int(er.BY_NAME["writers40"].batch.ops["client"].max()) > 31
    for name in ("huge_first", "huge_mid"):
        b = er.BY_NAME[name].batch
        assert int((b.snapshots["n_header"] + b.snapshots["n_body"]).max()) >= 2049
    assert er.BY_NAME["adjust_doc_local"].batch.value_base is not None
    assert all(s.batch.value_base is None for s in er.MT_STATIONS if not s.value_base)
    r = er.refused_headers(er.BY_NAME["refused_first"].batch)
    assert int(r[0]["status"]) == -5 and not r[1:].tobytes().strip(b"\0")


def test_stations_stay_small():
    for s in er.STATIONS:
        b = s.batch
        assert b.n_docs <= er.MAX_DOCS, s.name
        per_doc = int(np.diff(np.asarray(b.doc_op_offsets).astype(np.int64)).max())
        if s.family == "mt":
            assert per_doc <= er.MAX_OPS_PER_DOC or s.larger, (s.name, per_doc)
    assert er.BY_NAME["plain"].batch.n_docs == er.BY_NAME["map_pending"].batch.n_docs == 48
    assert er.BY_NAME["plain3"].batch.n_docs == er.BY_NAME["map_sparse3"].batch.n_docs == 3


@pytest.mark.parametrize("n", [2, 3, 7, len(er.STATIONS)])
def test_tour_holds_every_ordered_pair(n):
    walk = er.euler_tour(n)
    assert walk[0] == walk[-1] and len(walk) == n * (n - 1) + 1
    pairs = Counter(zip(walk, walk[1:]))
    assert len(pairs) == n * (n - 1) and set(pairs.values()) == {1}
    assert all(a != b and 0 <= a < n and 0 <= b < n for a, b in pairs)


def test_segments_lose_no_pair_at_a_cut():
    n = len(er.STATIONS)
    segs = er.tour_segments(n, n)
    pairs = Counter(p for seg in segs for p in zip(seg, seg[1:]))
    assert len(pairs) == n * (n - 1) and set(pairs.values()) == {1}
    assert all(a[-1] == b[0] for a, b in zip(segs, segs[1:]))


def test_the_plan_refuses_the_bad_batches_of_the_failed_load_test():
    """Descending doc_op_offsets went through fmt_mt_load unchecked before this test existed (only the
    first and last entry were looked at); the device takes offsets[d + 1] - offsets[d] as a count."""
    from fluidframework_amd import native

    bad = er.bad_mt_batches()
    p = native.mt_plan(bad["offsets"])
    assert p.status == native.FMT_E_USAGE and "ascending" in p.message
    p = native.mt_plan(bad["value_id"])
    assert p.status == native.FMT_E_DATA, p.message

"""GPU: fmt_mt_query_positions (include/fmt_pos.h, csrc/pos.hip) against the definition restated over the
oracle's replay of the same batch (pos_cases.expected_hits).

Every field but `props` is compared bit for bit with the oracle's hits. `props` names a record of the
engine's own table, whose ids the oracle does not share, so a hit's set is compared with the oracle's by its
entries, and the whole 32-byte records are compared bit for bit with expected_hits over the engine's own
per-document fetch."""
import base64
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import pos_cases
import text_cases
from fluidframework_amd import native, workloads
from fluidframework_amd.native import (FMT_E_DATA, FMT_E_UNSUPPORTED, FMT_E_USAGE, POS_F_END, POS_F_HIDDEN_LOCALLY, POS_F_MARKER,
                                       POS_HIT_DTYPE, VIEW_LOCAL)
from fluidframework_amd.streams import MergeTreeStreamBuilder
from pos_cases import expected_hits, pack, view_length
from text_cases import msg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = dict(cap_leaves=4096, cap_chars=1 << 17, cap_props=1024)
PLAIN = [f for f in POS_HIT_DTYPE.names if f != "props"]
SPARE = 63  # a short client id no batch below writes with (each test asserts it)


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _run(engine, batch):
    engine.mt_load(batch)
    engine.mt_run()
    return engine.mt_headers(raise_on_failed_docs=False)


def _oracle(orc, batch):
    rc, oh, ol, oc, op, _ = orc.mt_replay_batch(batch, threads=16, **CAPS)
    return oh, ol, oc, op


def _entries(table, pid):
    return frozenset() if pid == 0xFFFF else frozenset(native.propset_entries(table, pid))


def _check(engine, batch, hdrs, state, q, offs):
    """mt_positions against the oracle's state and the per-document fetch; returns the hits."""
    oh, ol, oc, op = state
    got = engine.mt_positions(q, offs)
    assert got.dtype == POS_HIT_DTYPE and len(got) == len(q)
    obl = native.mt_plan(batch).obliterates
    poffs, props = engine.mt_props_all()
    for d in range(batch.n_docs):
        a, b = int(offs[d]), int(offs[d + 1])
        if a == b:
            continue
        mine, qs = got[a:b], q[a:b]
        if int(hdrs[d]["status"]) != 0:
            want = np.zeros(b - a, dtype=POS_HIT_DTYPE)
            want["status"] = int(hdrs[d]["status"])
            assert mine.tobytes() == want.tobytes(), d
            continue
        assert int(oh[d]["status"]) == 0 and int(oh[d]["n_leaves"]) == int(hdrs[d]["n_leaves"]), d
        assert (int(oh[d]["min_seq"]), int(oh[d]["cur_seq"])) == (int(hdrs[d]["min_seq"]), int(hdrs[d]["cur_seq"])), d
        want = expected_hits(oh[d], ol[d], oc[d], qs, obl)
        for f in PLAIN:
            assert np.array_equal(mine[f], want[f]), (d, f)
        table = props[int(poffs[d]) : int(poffs[d + 1])]
        leaf = (want["status"] == 0) & ((want["flags"] & POS_F_END) == 0)  # the hits that name a leaf, so a prop set
        assert np.array_equal(mine["props"][~leaf], want["props"][~leaf]), d
        assert [_entries(table, int(p)) for p in mine["props"][leaf]] == [_entries(op[d], int(p)) for p in want["props"][leaf]], d
        leaves, chars, _ = engine.mt_doc(d, hdrs[d])
        assert mine.tobytes() == expected_hits(hdrs[d], leaves, chars, qs, obl).tobytes(), d
        bad = mine[mine["status"] != 0]
        assert not any(int(bad[f].max(initial=0)) for f in PLAIN if f != "status") and not int(bad["props"].max(initial=0)), d
    return got


def _writers(batch, d):
    a, b = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
    ids, counts = np.unique(batch.ops["client"][a:b], return_counts=True)
    return [int(x) for x in ids[np.argsort(-counts, kind="stable")]]


def _ends_and_random(length, rnd, n_random=8):
    return [p for p in (0, 1, length - 1, length, length + 1) if p >= 0] + [rnd.randrange(length + 1) for _ in range(n_random)]


def _every(length):
    return list(range(length + 2))


def _queries(state, views_of, positions_of):
    """views_of(d, header) -> [(ref_seq, client)]; positions_of(d, length in that view) -> [pos]."""
    oh, ol, _, _ = state
    per_doc = []
    for d in range(len(oh)):
        qs = []
        for ref, client in views_of(d, oh[d]):
            length = view_length(oh[d], ol[d], ref, client) if int(oh[d]["status"]) == 0 else 3
            qs += [(p, ref, client) for p in positions_of(d, length)]
        per_doc.append(qs)
    return pack(per_doc)


def _four_views(batch):
    """The local view, cur_seq with a non-writer, a mid-window r with a writer, the same r with a non-writer."""
    def views(d, h):
        w = _writers(batch, d)
        assert SPARE not in w
        mid = (int(h["min_seq"]) + int(h["cur_seq"])) // 2
        return [(VIEW_LOCAL, 0), (int(h["cur_seq"]), SPARE), (mid, w[0] if w else 1), (mid, SPARE)]
    return views


def test_farm(orc, engine):
    batch = workloads.conflict_farm(200, n_clients=8, ops_per_doc=200, seed=29)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    state = _oracle(orc, batch)
    rnd = random.Random(5)
    q, offs = _queries(state, _four_views(batch), lambda d, n: _ends_and_random(n, rnd))
    got = _check(engine, batch, hdrs, state, q, offs)
    ok = got[got["status"] == 0]
    assert len(ok) > 40 * batch.n_docs and (got["status"] == FMT_E_DATA).sum() >= 4 * batch.n_docs - 8
    assert (ok["flags"] & POS_F_HIDDEN_LOCALLY).any() and (ok["flags"] & POS_F_END).sum() >= 4 * batch.n_docs
    # the writer's mid-window view differs from the non-writer's somewhere: its own later inserts and removes
    per = 4 * 13
    differ = 0
    for d in range(batch.n_docs):
        mine = q[int(offs[d]) : int(offs[d + 1])]
        lens = [int(mine[k * (len(mine) // 4) + 3]["pos"]) for k in range(4)] if len(mine) == per else None
        differ += lens is not None and lens[2] != lens[3]
    assert differ > batch.n_docs // 4


def test_chunk_edges(orc, engine):
    batch, docs = text_cases.edge_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    assert [int(n) for n in hdrs["n_leaves"]] == [n for _, n, _ in docs]
    state = _oracle(orc, batch)

    def views(d, h):
        return [(VIEW_LOCAL, 0), (int(h["cur_seq"]), SPARE), (int(h["cur_seq"]) // 2, 1), (int(h["cur_seq"]) // 2, SPARE)]

    q, offs = _queries(state, views, lambda d, n: _every(n))
    got = _check(engine, batch, hdrs, state, q, offs)
    by = {name: d for d, (name, _, _) in enumerate(docs)}

    def local(name):
        d = by[name]
        mine, qs = got[int(offs[d]) : int(offs[d + 1])], q[int(offs[d]) : int(offs[d + 1])]
        return mine[qs["ref_seq"] == VIEW_LOCAL]

    assert local("empty")[["status", "flags", "leaf"]].tolist() == [(0, POS_F_END, 0), (FMT_E_DATA, 0, 0)]
    assert local("all_removed")[["status", "flags", "leaf"]].tolist() == [(0, POS_F_END, 3), (FMT_E_DATA, 0, 0)]
    for n in (63, 64, 65):
        assert local(str(n))["leaf"].tolist() == list(range(n)) + [n, 0]
    assert local("removed_ends")["leaf"].tolist() == list(range(1, 63)) + [64, 0]
    long = local("long_leaf")
    assert long["leaf"].tolist() == [0] + [1] * 300 + [2, 3, 0] and long["offset"][1:301].tolist() == list(range(300))
    assert long["unit"][1:301].tolist() == [0x100 + i for i in range(300)]
    marks = local("markers")
    assert marks["flags"].tolist() == [POS_F_MARKER, 0, 0, 0, 0, 0, 0, POS_F_MARKER, POS_F_END, 0]
    assert marks["leaf_len"].tolist() == [1, 3, 3, 3, 3, 3, 3, 1, 0, 0]
    odd = local("odd_units")
    assert odd["unit"][:-2].tolist() == text_cases.units_of("a\ud800b\udfffc￿de\u0000f\u0000").tolist()


def test_tile_edges(orc, engine):
    import runs_cases

    T = native.text_tile_leaves()
    batch, docs = runs_cases.tile_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all() and [int(n) for n in hdrs["n_leaves"]] == [T + 40] * 3
    assert [int(x) for x in np.diff(native.text_plan(hdrs).doc_first)] == [2, 2, 2]
    state = _oracle(orc, batch)

    def views(d, h):  # leaves 0..T+39 were inserted at seq 1..T+40: seq T puts the view's end at the tile edge
        return [(VIEW_LOCAL, 0), (int(h["cur_seq"]), SPARE), (T, SPARE), (T + 1, 2), (T + 20, 1)]  # (1: A; 2: B, who removes)

    q, offs = _queries(state, views, lambda d, n: sorted({p for p in list(range(T - 2, T + 3)) + [0, n - 1, n, n + 1] if p >= 0}))
    got = _check(engine, batch, hdrs, state, q, offs)
    for d, (name, specs, removed) in enumerate(docs):
        mine, qs = got[int(offs[d]) : int(offs[d + 1])], q[int(offs[d]) : int(offs[d + 1])]
        loc = mine[qs["ref_seq"] == VIEW_LOCAL]
        at = {int(p): h for p, h in zip(qs[qs["ref_seq"] == VIEW_LOCAL]["pos"], loc)}
        if name == "span":
            assert [int(at[p]["leaf"]) for p in range(T - 2, T + 3)] == list(range(T - 2, T + 3))
        elif name == "span_removed":  # leaf T - 1 is removed: position T - 1 is leaf T, the second tile's first
            assert [int(at[p]["leaf"]) for p in range(T - 2, T + 3)] == [T - 2, T, T + 1, T + 2, T + 3]
            before = mine[(qs["ref_seq"] == T + 20) & (qs["pos"] == T - 1)][0]  # before the remove: the leaf is there
            assert int(before["leaf"]) == T - 1 and int(before["flags"]) == POS_F_HIDDEN_LOCALLY and int(before["local_pos"]) == T - 1
        else:
            assert [int(at[p]["flags"]) for p in range(T - 2, T + 3)] == [0, POS_F_MARKER, POS_F_MARKER, 0, 0]
        edge = mine[(qs["ref_seq"] == T) & (qs["pos"] == T)][0]
        assert int(edge["flags"]) == POS_F_END and int(edge["leaf_start"]) == T  # a view that ends with the first tile


def test_tiers(orc, engine):
    from test_gpu_text import tier_batch

    T = native.text_tile_leaves()
    batch, huge = tier_batch(T)
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    assert [int(x) for x in native.mt_plan(batch).huge_docs] == [huge]
    plan = native.text_plan(hdrs)
    assert int(plan.doc_first[huge + 1] - plan.doc_first[huge]) >= 3
    state = _oracle(orc, batch)
    rnd = random.Random(9)
    n = 2 * T + 52

    def views(d, h):
        if d == huge:  # loaded at seq 0, leaf T - 1 removed at seq 1 by client B
            return [(VIEW_LOCAL, 0), (1, SPARE), (0, SPARE), (0, _writers(batch, d)[0])]
        return _four_views(batch)(d, h)

    def positions(d, length):
        if d != huge:
            return _ends_and_random(length, rnd)
        # the first, middle and last tile, both tile edges, the position just after the removed leaf, the ends
        return sorted({0, 1, T // 2, T - 3, T - 2, T - 1, T, T + 1, T + T // 2, 2 * T - 2, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 30,
                       length - 1, length, length + 1})

    q, offs = _queries(state, views, positions)
    got = _check(engine, batch, hdrs, state, q, offs)
    mine, qs = got[int(offs[huge]) : int(offs[huge + 1])], q[int(offs[huge]) : int(offs[huge + 1])]
    loc = {int(p): h for p, h in zip(qs[qs["ref_seq"] == VIEW_LOCAL]["pos"], mine[qs["ref_seq"] == VIEW_LOCAL])}
    assert [int(loc[p]["leaf"]) for p in (T - 2, T - 1, T)] == [T - 2, T, T + 1]  # leaf T - 1 is removed
    assert int(loc[T - 1]["unit"]) == 0x4E00 + T and int(loc[2 * T + 30]["leaf"]) == 2 * T + 31
    assert int(loc[n - 1]["flags"]) == POS_F_END and int(loc[n]["status"]) == FMT_E_DATA
    old = {int(p): h for p, h in zip(qs[(qs["ref_seq"] == 0) & (qs["client"] == SPARE)]["pos"],
                                     mine[(qs["ref_seq"] == 0) & (qs["client"] == SPARE)])}
    assert int(old[T - 1]["leaf"]) == T - 1 and int(old[T - 1]["flags"]) == POS_F_HIDDEN_LOCALLY and int(old[T - 1]["local_pos"]) == T - 1
    assert int(old[T]["leaf"]) == T and int(old[T]["local_pos"]) == T - 1 and int(old[n]["flags"]) == POS_F_END
    assert int(old[n]["local_pos"]) == n - 1


def rules_batch():
    """One document, three writers. "0123456789"; 1: A inserts "aaa" at 2; 2: B inserts "bbb" at 0, concurrently;
    3: B removes "aa2"; 4: C removes "a23", concurrently with 3 ("a2": two removers); 5: A inserts "zz" at 1."""
    b = MergeTreeStreamBuilder()
    d = b.begin_doc(initial_text="0123456789", observer="observer")
    d.add_message(msg("A", 1, {"type": 0, "pos1": 2, "seg": "aaa"}, ref=0))
    d.add_message(msg("B", 2, {"type": 0, "pos1": 0, "seg": "bbb"}, ref=0))
    d.add_message(msg("B", 3, {"type": 1, "pos1": 6, "pos2": 9}, ref=2))
    d.add_message(msg("C", 4, {"type": 1, "pos1": 7, "pos2": 10}, ref=2))
    d.add_message(msg("A", 5, {"type": 0, "pos1": 1, "seg": "zz"}, ref=4))
    batch = b.finish()
    ids = {name: k for k, name in enumerate(batch.clients[0])}
    return batch, ids["A"], ids["B"], ids["C"]


def test_remote_view_rules(orc, engine):
    batch, A, B, C = rules_batch()
    assert SPARE not in (A, B, C)
    hdrs = _run(engine, batch)
    assert int(hdrs[0]["status"]) == 0 and (int(hdrs[0]["min_seq"]), int(hdrs[0]["cur_seq"])) == (0, 5)
    state = _oracle(orc, batch)
    want = {(VIEW_LOCAL, 0): "bzzbb01a456789",
            (0, A): "zz01aaa23456789",    # A's inserts are above ref_seq 0: A sees them (its later "zz" too),
            (0, B): "bbb013456789",       # B does not; it sees its own insert and its own remove (of "2");
            (0, SPARE): "0123456789",     # nobody else sees either
            (2, A): "bzzbb01aaa23456789", # both removes are above ref_seq 2: A still sees the text,
            (2, B): "bbb01a3456789",      # B's own remove hides "aa2" for B only,
            (2, C): "bbb01aa456789",      # C's hides "a23" for C only
            (3, A): "bzzbb01a3456789",    # at 3 B's remove holds for everybody, C's "3" not yet
            (3, C): "bbb01a456789",
            (4, SPARE): "bbb01a456789",
            (4, A): "bzzbb01a456789",     # A's insert at 5: A's alone at ref_seq 4
            (5, SPARE): "bzzbb01a456789"}
    order = list(want)
    q, offs = _queries(state, lambda d, h: order, lambda d, n: _every(n))
    got = _check(engine, batch, hdrs, state, q, offs)
    leaves, chars, _ = engine.mt_doc(0, hdrs[0])
    both = (1 << B) | (1 << C)
    assert [int(L["rm_seq"]) for L in leaves if int(L["rm_clients"]) == both] == [3, 3]  # "a" and "2": removed by two clients
    local_units = pos_cases.view_units(leaves, VIEW_LOCAL, 0)[0]
    at = 0
    hidden = 0
    for view in order:
        n = len(want[view])
        mine = got[at : at + n + 2]
        at += n + 2
        assert text_cases.units_of(want[view]).tolist() == mine["unit"][:n].tolist(), view
        assert (mine["status"][: n + 1] == 0).all() and int(mine[n]["flags"]) == POS_F_END and int(mine[n + 1]["status"]) == FMT_E_DATA
        assert int(mine[n]["local_pos"]) == len(want[(VIEW_LOCAL, 0)]) and int(mine[n]["leaf_start"]) == n
        for h in mine[:n]:
            before = int(local_units[: int(h["leaf"])].sum())
            if int(leaves[int(h["leaf"])]["rm_seq"]) != text_cases.NOT_REMOVED:  # hidden locally: the flag, and no offset added
                assert int(h["flags"]) & POS_F_HIDDEN_LOCALLY and int(h["local_pos"]) == before, view
                hidden += 1
            else:
                assert not int(h["flags"]) & POS_F_HIDDEN_LOCALLY and int(h["local_pos"]) == before + int(h["offset"]), view
                assert chr(int(h["unit"])) == want[(VIEW_LOCAL, 0)][int(h["local_pos"])], view
    assert at == len(got) and hidden >= 10


def test_pending_local_ops(orc, engine):
    batch = text_cases.pending_local_batch()
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    state = _oracle(orc, batch)
    last = batch.n_docs - 1
    me, other = batch.clients[last].index("A"), batch.clients[last].index("B")
    rnd = random.Random(3)

    def views(d, h):
        cur = int(h["cur_seq"])
        if d == last:
            return [(VIEW_LOCAL, 0), (cur, other), (cur, me)]
        return [(VIEW_LOCAL, 0), (cur, SPARE), (cur, 0), ((int(h["min_seq"]) + cur) // 2, 1)]

    q, offs = _queries(state, views, lambda d, n: _every(n) if d == last else _ends_and_random(n, rnd))
    got = _check(engine, batch, hdrs, state, q, offs)
    mine = got[int(offs[last]) : int(offs[last + 1])]
    local, remote = ">01PENDING234ote56789", ">01234remote56789"

    def text(a, n):
        return mine["unit"][a : a + n].tobytes().decode("utf-16-le")

    assert text(0, len(local)) == local                                      # the pending insert, not the pending-removed text
    assert text(len(local) + 2, len(remote)) == remote                        # B at cur_seq: the opposite
    assert text(len(local) + len(remote) + 4, len(local)) == local            # the observer's own id: the local view
    own = mine[len(local) + len(remote) + 4 :][: len(local) + 2]
    assert own.tobytes() == mine[: len(local) + 2].tobytes()
    rem = mine[len(local) + 2 :][: len(remote)]
    assert [int(h["local_pos"]) for h in rem[6:9]] == [13, 13, 13] and (rem["flags"][6:9] == POS_F_HIDDEN_LOCALLY).all()  # "rem"
    assert not rem["flags"][:6].any() and not rem["flags"][9:].any()


def test_refusals(orc, engine):
    batch = workloads.conflict_farm(6, n_clients=4, ops_per_doc=150, seed=31)
    hdrs = _run(engine, batch)
    state = _oracle(orc, batch)
    lo, hi = int(hdrs[2]["min_seq"]), int(hdrs[2]["cur_seq"])
    assert 0 < lo < hi
    per_doc = [[] for _ in range(batch.n_docs)]
    per_doc[2] = [(0, hi, 64), (0, hi, -1), (0, lo - 1, 1), (0, hi + 1, 1), (0, lo, 1), (0, hi, 1), (0, lo - 1, 64), (0, VIEW_LOCAL, 64)]
    per_doc[4] = [(0, VIEW_LOCAL, 0)]
    q, offs = pack(per_doc)
    got = _check(engine, batch, hdrs, state, q, offs)
    assert got["status"].tolist() == [FMT_E_UNSUPPORTED, FMT_E_UNSUPPORTED, FMT_E_USAGE, FMT_E_USAGE, 0, 0, FMT_E_UNSUPPORTED, 0, 0]


def test_obliterate_fixtures_refuse_remote_views(orc, engine):
    from golden_data import prefix_batch, replay_fixtures

    fx = [(name, b, ge[-1:], ini, res[-1:]) for name, b, ge, ini, res in
          list(replay_fixtures("replay_obliterate_2.3.0.npz"))[:4]]
    batch, texts = prefix_batch(fx)
    assert batch.n_docs == 4 and native.mt_plan(batch).obliterates
    hdrs = _run(engine, batch)
    assert (hdrs["status"] == 0).all()
    state = _oracle(orc, batch)
    q, offs = _queries(state, lambda d, h: [(VIEW_LOCAL, 0), (int(h["cur_seq"]), SPARE), (int(h["cur_seq"]), 1)],
                       lambda d, n: _every(n))
    got = _check(engine, batch, hdrs, state, q, offs)
    remote = q["ref_seq"] != VIEW_LOCAL
    assert (got["status"][remote] == FMT_E_UNSUPPORTED).all() and remote.sum() > 8
    for d in range(4):
        mine = got[int(offs[d]) : int(offs[d + 1])]
        n = len(texts[d])
        assert mine["unit"][:n].tolist() == text_cases.units_of(texts[d]).tolist() and int(mine[n]["flags"]) == POS_F_END


def test_failed_documents_answer_with_their_status(orc, engine):
    from test_gpu_text import failing_batch

    batch, bad, refused = failing_batch()
    hdrs = _run(engine, batch)
    status = [int(x) for x in hdrs["status"]]
    assert status[bad] == FMT_E_DATA and status[refused] != 0
    state = _oracle(orc, batch)
    q, offs = _queries(state, lambda d, h: [(VIEW_LOCAL, 0), (int(h["cur_seq"]), SPARE)], lambda d, n: [0, 1, n, n + 1])
    got = _check(engine, batch, hdrs, state, q, offs)
    for d in (bad, refused):
        assert (got[int(offs[d]) : int(offs[d + 1])]["status"] == status[d]).all() and int(offs[d + 1] - offs[d]) == 8
    for d, text in ((0, "f+irst"), (2, "s+econd"), (batch.n_docs - 1, "l+ast")):
        mine = got[int(offs[d]) : int(offs[d + 1])]
        assert mine["status"].tolist() == [0, 0, 0, FMT_E_DATA] * 2 and [chr(int(u)) for u in mine["unit"][:2]] == list(text[:2])


def _raw(engine, offs, q, n, out):
    return engine.L.fmt_mt_query_positions(engine.h, None if offs is None else native._ptr(offs), None if q is None else native._ptr(q),
                                           n, None if out is None else native._ptr(out))


def _farm64():
    return workloads.conflict_farm(64, n_clients=8, ops_per_doc=200, seed=23)


def _farm_queries(batch, state, seed=7):
    rnd = random.Random(seed)
    return _queries(state, _four_views(batch), lambda d, n: _ends_and_random(n, rnd))


def test_contract(orc, engine):
    batch = _farm64()
    state = _oracle(orc, batch)
    q, offs = _farm_queries(batch, state)
    engine.mt_load(batch)
    out = np.zeros(len(q), dtype=POS_HIT_DTYPE)
    assert _raw(engine, offs, q, len(q), out) == FMT_E_USAGE  # before the run
    assert b"before fmt_mt_run" in engine.L.fmt_last_error(engine.h)
    with pytest.raises(native.EngineError):
        engine.mt_positions(q, offs)
    engine.mt_run()
    hdrs = engine.mt_headers()
    sentinel = np.frombuffer(b"\xAB" * (len(q) * 32), dtype=POS_HIT_DTYPE).copy()
    for bad in (offs[::-1].copy(), offs + np.uint64(1), np.concatenate([offs[:-1], [offs[-1] + np.uint64(1)]]).astype(np.uint64),
                np.concatenate([offs[:3], [offs[2] - np.uint64(1)], offs[4:]]).astype(np.uint64)):
        out = sentinel.copy()
        assert _raw(engine, bad, q, len(q), out) == FMT_E_USAGE
        assert out.tobytes() == sentinel.tobytes()  # nothing written
    assert _raw(engine, None, q, len(q), out) == FMT_E_USAGE and _raw(engine, offs, None, len(q), out) == FMT_E_USAGE
    with pytest.raises(native.EngineError):
        engine.mt_positions(q, offs[:-1])
    # zero queries: accepted, nothing written
    out = sentinel.copy()
    assert _raw(engine, np.zeros(batch.n_docs + 1, dtype=np.uint64), None, 0, None) == native.FMT_OK
    assert len(engine.mt_positions(q[:0], np.zeros(batch.n_docs + 1, dtype=np.uint64))) == 0
    # two calls, equal bytes
    first = _check(engine, batch, hdrs, state, q, offs)
    again = sentinel.copy()
    assert _raw(engine, offs, q, len(q), again) == native.FMT_OK
    assert again.tobytes() == first.tobytes() != sentinel.tobytes()


def test_queries_texts_runs_and_summaries_do_not_disturb_each_other(orc, engine):
    import v1_bulk

    batch = v1_bulk.farm_batch()
    hdrs = _run(engine, batch)
    n = batch.n_docs
    state = _oracle(orc, batch)
    q, offs = _farm_queries(batch, state)
    hits = _check(engine, batch, hdrs, state, q, offs)
    texts, runs = engine.mt_texts(0), engine.mt_prop_runs()
    engine.mt_summarize_legacy(batch.keys, batch.values)
    blobs = [engine.mt_summary(d) for d in range(n)]
    digests = engine.mt_digests()
    assert engine.mt_positions(q, offs).tobytes() == hits.tobytes()
    assert [engine.mt_summary(d) for d in range(n)] == blobs
    # queries between the sizing call and the fill of the text and the runs reads
    to = np.zeros(n + 1, dtype=np.uint64)
    assert engine.L.fmt_mt_fetch_text_all(engine.h, 0, native._ptr(to), None, 0) == native.FMT_OK
    ro = np.zeros(n + 1, dtype=np.uint64)
    assert engine.L.fmt_mt_fetch_prop_runs_all(engine.h, native._ptr(ro), None, 0) == native.FMT_OK
    assert engine.mt_positions(q, offs).tobytes() == hits.tobytes()
    units = np.zeros(len(texts[1]), dtype="<u2")
    assert engine.L.fmt_mt_fetch_text_all(engine.h, 0, native._ptr(to), native._ptr(units), len(units)) == native.FMT_OK
    out = np.zeros(len(runs[1]), dtype=native.PROP_RUN_DTYPE)
    assert engine.L.fmt_mt_fetch_prop_runs_all(engine.h, native._ptr(ro), native._ptr(out), len(out)) == native.FMT_OK
    assert np.array_equal(to, texts[0]) and np.array_equal(units, texts[1])
    assert np.array_equal(ro, runs[0]) and out.tobytes() == runs[1].tobytes()
    engine.mt_summarize_legacy(batch.keys, batch.values)
    assert [engine.mt_summary(d) for d in range(n)] == blobs and np.array_equal(engine.mt_digests(), digests)
    assert engine.mt_positions(q, offs).tobytes() == hits.tobytes()
    # and a run after the queries gives the same state
    engine.mt_run()
    assert np.array_equal(engine.mt_digests(), digests) and engine.mt_positions(q, offs).tobytes() == hits.tobytes()


def test_engine_reuse_gives_the_second_batch(orc, engine):
    from test_gpu_text import tier_batch

    big, huge = tier_batch(native.text_tile_leaves())
    _run(engine, big)
    qb, ob = pack([[(0, VIEW_LOCAL, 0), (5, VIEW_LOCAL, 0)] for _ in range(big.n_docs)])
    first = engine.mt_positions(qb, ob)
    small = workloads.conflict_farm(5, n_clients=4, ops_per_doc=150, seed=31)
    hdrs = _run(engine, small)
    state = _oracle(orc, small)
    q, offs = _farm_queries(small, state, seed=11)
    got = _check(engine, small, hdrs, state, q, offs)
    assert len(got) != len(first)
    fresh = native.Engine(0)
    try:
        _run(fresh, small)
        other = fresh.mt_positions(q, offs)
    finally:
        fresh.close()
    assert got.tobytes() == other.tobytes()


# ---- hosts
def test_positions_local_gives_the_same_answers(orc, engine):
    batch = _farm64()
    hdrs = _run(engine, batch)
    rnd = random.Random(13)
    per_doc = [[(p, VIEW_LOCAL, 0) for p in _ends_and_random(int(hdrs[d]["visible_len"]), rnd)] for d in range(batch.n_docs)]
    q, offs = pack(per_doc)
    want = engine.mt_positions(q, offs)
    docs = np.repeat(np.arange(batch.n_docs), np.diff(offs).astype(np.int64))
    shuffle = np.array(rnd.sample(range(len(q)), len(q)))
    got = engine.mt_positions_local(docs[shuffle], q["pos"][shuffle])
    assert got.tobytes() == want[shuffle].tobytes() and (got["status"] == 0).sum() > 10 * batch.n_docs
    assert len(engine.mt_positions_local([], [])) == 0
    with pytest.raises(native.EngineError):
        engine.mt_positions_local([batch.n_docs], [0])


NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_js_positions_equal_python_on_the_farm(orc, engine, tmp_path):
    from test_napi_text import _write

    farm = _farm64()
    state = _oracle(orc, farm)
    q, offs = _farm_queries(farm, state)
    _write(tmp_path, farm, [], 0)
    (tmp_path / "queries.bin").write_bytes(q.tobytes())
    (tmp_path / "qoffs.bin").write_bytes(offs.tobytes())
    env = dict(os.environ, FMT_NAPI_BACKTRACE=os.environ.get("FMT_NAPI_BACKTRACE", "1"))
    r = subprocess.run([NODE, os.path.join(REPO, "tests", "js", "pos_driver.js"), str(tmp_path)], capture_output=True,
                       text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    _run(engine, farm)
    want = engine.mt_positions(q, offs)
    assert base64.b64decode(got["hits"]) == want.tobytes() and (want["status"] == 0).sum() > 40 * farm.n_docs
    assert got["objectsMatch"] is True and got["refusedWhileBusy"] is True and got["enumerable"] is False

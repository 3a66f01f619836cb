"""SharedMap edge streams on the CPU: the oracle equals a Python dict, and the builders keep their promises.

tests/map_edges.py builds the streams `workloads.map_stream` cannot (long clear-free tails, full hash
tables, colliding keys, gapped seqs) and replays them through a Python dict. Here, without a GPU:
the C++ oracle (the checker of every other map test) equals that dict replay on all of them, and each
builder's documents really have the tail lengths, distinct keys, live keys and home slots it states,
so the GPU tests of test_gpu_map_edges.py keep reaching the code they are written for.
"""
import numpy as np
import pytest

import map_edges as me
from fluidframework_amd.streams import MAP_CLEAR, MAP_KIND_SHIFT


def _measure(ops):
    """A document's facts, measured without numpy tricks (map_edges._facts promises the same)."""
    kinds = [kv >> MAP_KIND_SHIFT for kv in ops["kind_value"].tolist()]
    c = max((i + 1 for i, k in enumerate(kinds) if k == MAP_CLEAR), default=0)
    return {"n": len(kinds), "tail": len(kinds) - c, "distinct": len(set(ops["key"][c:].tolist())),
            "live": len(me.dict_replay(ops))}


@pytest.mark.parametrize("name", list(me.SPARSE_GROUPS))
def test_sparse_oracle_equals_dict_replay(orc, name):
    batch, facts = me.SPARSE_GROUPS[name]()
    counts, entries, _ = orc.map_replay_sparse(batch, threads=4)
    refused = [d for d, f in enumerate(facts) if f.get("refused")]
    counts, entries = me.drop_docs(counts, entries, refused)  # (the oracle has no limits)
    wc, we = me.sparse_reference(name)
    assert np.array_equal(counts, wc)
    assert np.array_equal(entries, we)
    assert int(wc.sum()) == sum(f["live"] for d, f in enumerate(facts) if d not in refused) > 0


@pytest.mark.parametrize("key_bound", me.DENSE_KEY_BOUNDS)
def test_dense_oracle_equals_dict_replay(orc, key_bound):
    batch, facts = me.dense(key_bound)
    exp, _ = orc.map_replay(batch, threads=4)
    want = me.dense_reference(key_bound)
    assert np.array_equal(exp, want)
    assert int((want["value"] != 0xFFFFFFFF).sum()) == sum(f["live"] for f in facts) > 0
    assert [f["n"] for f in facts[-len(me.RAGGED):]] == me.RAGGED


@pytest.mark.parametrize("name", list(me.SPARSE_GROUPS) + [f"dense{k}" for k in me.DENSE_KEY_BOUNDS])
def test_builders_promise_what_they_build(name):
    batch, facts = me.dense(int(name[5:])) if name.startswith("dense") else me.SPARSE_GROUPS[name]()
    assert len(facts) == batch.n_docs
    for d, f in enumerate(facts):
        got = _measure(me.doc_ops(batch, d))
        assert got == {k: f[k] for k in got}, d
    for d in range(batch.n_docs):
        o = me.doc_ops(batch, d)
        assert (o["doc"] == d).all() and (o["key"] < batch.key_bound).all()
        s = o["seq"].astype(np.int64)
        assert len(s) == 0 or (s[0] >= 1 and (np.diff(s) > 0).all()), d


def test_tails_cover_every_table_size_switch():
    """a: tails exactly 0, 1, 32|33, 64|65, ... 512|513, 1024 (table sizes 64 .. 2048 and both sides of
    each switch), whole and behind a clear at ordinal 64, 65 and 1000; every tail op has its own key."""
    batch, facts = me.tails()
    assert [f["tail"] for f in facts] == me.TAILS * len(me.TAIL_PREFIXES)
    assert me.TAILS == [0, 1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024]
    assert [f["n"] - f["tail"] for f in facts] == [p for p in (0, 64, 65, 1000) for _ in me.TAILS]
    for d, f in enumerate(facts):
        assert f["distinct"] == f["tail"], d
        o = me.doc_ops(batch, d)
        c = f["n"] - f["tail"]
        assert c == 0 or o["kind_value"][c - 1] >> MAP_KIND_SHIFT == MAP_CLEAR
        assert not set(o["key"][:c].tolist()) & set(o["key"][c:].tolist())
    assert sum(f["live"] for f in facts) > 0.7 * sum(f["tail"] for f in facts)


def test_clear_positions():
    """b: a clear as the last op leaves nothing, whatever the length; the other documents as listed."""
    batch, facts = me.clears()
    assert facts[0] == {"n": 1, "tail": 0, "distinct": 0, "live": 0}
    assert (facts[1]["n"], facts[1]["tail"], facts[1]["live"]) == (51, 50, 50)
    assert [(f["n"], f["tail"], f["live"]) for f in facts[2:8]] == [(n, 0, 0) for n in (1, 64, 65, 1024, 1025, 4096)]
    assert [(f["n"], f["tail"]) for f in facts[8:11]] == [(162, 70), (1100, 76), (1100, 75)]
    assert (facts[11]["n"], facts[11]["live"]) == (100, 0)
    assert [(f["n"], f["live"]) for f in facts[12:]] == [(3, 2), (4, 1)]


def test_histories_are_long_and_clear_free():
    """c: no clear, the stated distinct keys, at least a quarter of them live; with four ops per key or
    more a key's ops fall into several 64-op chunks."""
    batch, facts = me.histories()
    assert [(f["n"], f["distinct"]) for f in facts[: me.N_HISTORIES]] == me.HISTORIES
    assert me.HISTORIES[-1] == (16384, 2048) and {n for n, _ in me.HISTORIES} == {1024, 1025, 4096, 16384}
    for d, f in enumerate(facts):
        assert f["tail"] == f["n"], d
        if d < me.N_HISTORIES:
            assert 4 * f["live"] >= f["distinct"], d
            if f["n"] >= 4 * f["distinct"]:
                o = me.doc_ops(batch, d)
                pairs = np.unique(np.stack([o["key"].astype(np.int64), np.arange(f["n"]) // 64]), axis=1)
                assert pairs.shape[1] >= 3 * f["distinct"], d  # three chunks per key on average
    assert (facts[me.N_HISTORIES]["n"], facts[me.N_HISTORIES]["live"]) == (1100, 1100)  # every op a birth
    # one key over a whole chunk: 64 sets (value of the last lane, birth of the first), or set / delete by turns
    for d, chunk, live in [(-6, 1, True), (-5, 1, False), (-4, 1, True), (-3, 16, True), (-2, 16, False), (-1, 16, True)]:
        o = me.doc_ops(batch, batch.n_docs + d)[chunk * 64 : chunk * 64 + 64]
        key = int(o["key"][0])
        assert (o["key"] == key).all()
        entry = [e for e in me.dict_replay(me.doc_ops(batch, batch.n_docs + d)) if e[0] == key]
        assert bool(entry) == live
    o = me.doc_ops(batch, batch.n_docs - 6)
    (e,) = [e for e in me.dict_replay(o) if e[0] == int(o["key"][64])]
    assert e[1:] == (int(o["kind_value"][127]) & me.VALUE_MASK, 65)


def test_limits_sit_exactly_on_the_limits():
    """d: 2048 / 2049 distinct keys after the last clear, 16384 / 16385 ops; the full table's last key
    needs all 2048 probes (under the mirrored hash, which chooses it and computes no expected value)."""
    batch, facts = me.limits_ok()
    assert [(f["n"], f["distinct"]) for f in facts[:2]] == [(16384, 2048), (16384, 2048)]
    assert facts[1]["live"] == 48
    assert facts[2]["n"] - facts[2]["tail"] == 3001 and facts[2]["distinct"] == 100
    o = me.doc_ops(batch, 0)
    last = facts[0]["last_key"]
    first_seen = int(np.nonzero(o["key"] == last)[0][0])
    assert first_seen >= 16384 - 64 and len(set(o["key"][:first_seen].tolist())) == 2047
    (free,) = me.sp_free_slots(np.unique(o["key"][:first_seen]), 2048)
    assert int(me.sp_home(last, 2048)) == (free + 1) % 2048  # its chain: home, ..., 2047, 0, ..., free
    _, facts = me.limits_keys()
    assert [f["distinct"] for f in facts] == [100, 2049, 300] and [bool(f.get("refused")) for f in facts] == [False, True, False]
    _, facts = me.limits_ops()
    assert [f["n"] for f in facts] == [300, 16385, 2000] and [bool(f.get("refused")) for f in facts] == [False, True, False]


def test_probe_keys_share_their_home_slot():
    """e: the colliding keys really collide under the mirrored hash, and their chains wrap."""
    batch, facts = me.probes()
    assert batch.key_bound == 2**32 - 1
    for d in range(4):
        slots, home, count = facts[d]["home"]
        o = me.doc_ops(batch, d)
        keys = np.unique(o["key"][f_tail(facts[d]):])
        assert len(keys) == count == facts[d]["distinct"]
        assert (me.sp_home(keys, slots) == home).all()
        assert home + count > slots                      # the chain wraps past the last slot
        assert slots // 2 >= facts[d]["tail"] > slots // 4 or slots == 2048  # the kernel picks this table size
    assert facts[0]["n"] <= 1024 < facts[1]["n"] and facts[0]["tail"] > 512
    assert (me.doc_ops(batch, 4)["key"] % (1 << 12) == 0).all() and (me.doc_ops(batch, 5)["key"] % (1 << 20) == 0).all()
    assert (me.doc_ops(batch, 6)["key"] % (1 << 20) == 0).all() and facts[6]["n"] > 1024
    assert {0, 2**32 - 2} <= set(me.doc_ops(batch, 7)["key"].tolist())


def f_tail(f):
    return f["n"] - f["tail"]


def test_seqs_and_values():
    """f: first seq 1 and 7, gaps, last seq 0xFFFFFFFF; every special value id ends up in a live entry."""
    batch, facts = me.seqs()
    firsts = {int(me.doc_ops(batch, d)["seq"][0]) for d in range(batch.n_docs)}
    lasts = {int(me.doc_ops(batch, d)["seq"][-1]) for d in range(batch.n_docs)}
    assert {1, 7} <= firsts and 0xFFFFFFFF in lasts
    _, entries = me.sparse_reference("seqs")
    assert set(me.SPECIAL_VALUES.tolist()) <= set(entries["value"].tolist())
    assert int(entries["birth_seq"].max()) > 1 << 31


def test_pipeline_gives_every_wave_three_documents():
    """g: 8192 documents for 256 CUs x 5 workgroups x 2 waves, lengths of period 7, clear-free."""
    batch, facts = me.pipeline()
    assert batch.n_docs == 8192 >= 3 * 256 * 5 * 2
    assert [f["n"] for f in facts[:14]] == [0, 1, 65, 1024, 1025, 33, 1100] * 2
    assert all(f["tail"] == f["n"] for f in facts)
    assert sum(f["live"] for f in facts) > batch.n_docs

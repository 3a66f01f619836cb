"""GPU parity of the sparse map path's HBM tier (fmt_map_run_sparse_tiered, csrc/map_sparse_large.hip).

Documents the LDS tier refuses (more than 2048 distinct keys after the last clear, or more than 16384
ops) are replayed by the tile kernels; every count and every entry field, in order, is compared with
two references that have no limits: a Python dict replayed op by op (map_edges.dict_sparse) and the
C++ oracle (oracle.map_replay_sparse). Integer state, no tolerance. The shapes are the smallest at
which the tier can go wrong: documents just past either limit, lengths around a multiple of the
256-op tile, clears on tile boundaries, births on the first and last op of a tile, every atomic of a
document in three slots, probe chains of 70 keys (one wrapping past the table's end), gapped seqs.

Run with `pytest -m gpu`.
"""
import ctypes
import functools

import numpy as np
import pytest

import map_edges as me
from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_CAPACITY, FMT_E_DATA, FMT_OK, MAP_ENTRY_DTYPE
from fluidframework_amd.streams import (MAP_CLEAR, MAP_DELETE, MAP_EV_ACK, MAP_EV_ROLLBACK, MAP_EV_SUBMIT, MAP_KIND_SHIFT,
                                        MAP_LOCAL_OP_DTYPE, MAP_SET, MapBatch)

pytestmark = pytest.mark.gpu

T = 256                      # csrc/map_plan.h kMapLargeTile
K = 65                       # K * T - 1 = 16639 >= 16385: the shortest tile multiples past the LDS tier
OVER = me.SPARSE_MAX_OPS + 1


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _fetch_raw(engine, batch):
    """fmt_map_fetch_sparse's return code beside what it filled."""
    counts = np.full(batch.n_docs, 0xDEADBEEF, dtype=np.uint32)
    entries = np.zeros(max(len(batch.ops), 1), dtype=MAP_ENTRY_DTYPE)
    n = ctypes.c_uint64()
    rc = native.lib().fmt_map_fetch_sparse(engine.h, counts.ctypes.data_as(ctypes.c_void_p),
                                           entries.ctypes.data_as(ctypes.c_void_p), len(entries), ctypes.byref(n))
    return rc, counts, entries[: n.value]


def _assert_sparse(batch, got, want, who):
    """Counts and every entry field equal; on a difference, name the first document and rank."""
    (gc, ge), (wc, we) = got, want
    if np.array_equal(gc, wc) and np.array_equal(ge, we):
        return
    go = np.concatenate([[0], np.cumsum(gc.astype(np.int64))])
    wo = np.concatenate([[0], np.cumsum(wc.astype(np.int64))])
    for d in range(batch.n_docs):
        g, w = ge[go[d] : go[d + 1]], we[wo[d] : wo[d + 1]]
        if not np.array_equal(g, w):
            k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            pytest.fail(f"vs {who}: document {d} ({len(me.doc_ops(batch, d))} ops): {len(g)} entries, {len(w)} expected; "
                        f"first difference at rank {k}: {g[k : k + 2]} != {w[k : k + 2]}")
    pytest.fail(f"vs {who}: counts differ")


def _doc_entries(counts, entries, d):
    o = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    return entries[o[d] : o[d + 1]]


def _tiered(engine, batch, runs=1):
    engine.map_load_sparse(batch)
    for _ in range(runs):
        engine.map_run_sparse_tiered()
    rc, counts, entries = _fetch_raw(engine, batch)
    assert rc == FMT_OK, engine.L.fmt_last_error(engine.h).decode()
    return counts, entries


def _check_both(orc, engine, batch, want, runs=2):
    """The tiered run (twice by default: the tables are initialised again) against both references."""
    got = _tiered(engine, batch, runs)
    _assert_sparse(batch, got, want, "dict replay")
    oc, oe, _ = orc.map_replay_sparse(batch, threads=16)
    _assert_sparse(batch, got, (oc, oe), "oracle")
    return got


# ------------------------------------------------------------------------------------ the two limits
@pytest.mark.parametrize("name", ["limits_keys", "limits_ops"])
def test_the_two_limits(orc, engine, name):
    """2049 distinct keys in 4096 ops, and 16385 ops over 500 keys: refused by the plain run, complete
    after the tiered one; the register-path and streaming neighbours bit-equal to the plain run's; the
    plain run on the same loaded batch still refuses afterwards."""
    batch, facts = me.SPARSE_GROUPS[name]()
    want = me.dict_sparse(batch)
    engine.map_load_sparse(batch)
    engine.map_run_sparse()
    rc, pc, pe = _fetch_raw(engine, batch)
    assert rc == FMT_E_CAPACITY and pc[1] == 0
    for _ in ("first run", "second run"):
        engine.map_run_sparse_tiered()
        rc, counts, entries = _fetch_raw(engine, batch)
        assert rc == FMT_OK
        _assert_sparse(batch, (counts, entries), want, "dict replay")
        oc, oe, _ = orc.map_replay_sparse(batch, threads=16)
        _assert_sparse(batch, (counts, entries), (oc, oe), "oracle")
        assert counts[1] == facts[1]["live"] > 0
        for d in (0, 2):
            assert counts[d] == pc[d] and _doc_entries(counts, entries, d).tobytes() == _doc_entries(pc, pe, d).tobytes()
    s = engine.stats()
    assert s.launches == 8 and s.ops == len(batch.ops) and s.docs == 3
    engine.map_run_sparse()
    rc, counts, _ = _fetch_raw(engine, batch)
    assert rc == FMT_E_CAPACITY and counts[1] == 0
    assert engine.stats().launches == 1


# --------------------------------------------------------------------------------- clears and empties
@functools.lru_cache(maxsize=None)
def _clears():
    rng = np.random.default_rng(201)
    keys = me._distinct_keys(rng, 400)
    docs = [me._join(me._history(rng, 16999, keys), me._clear()),                  # 0: a clear as the very last op
            me._join(me._history(rng, 16500, keys), me._deletes(rng.permutation(keys)))]  # 1: every key ends deleted
    for at in (66 * T - 1, 66 * T, 66 * T + 1):                                     # 2-4: the clear's ordinal
        docs.append(me._join(me._history(rng, at - 1, keys), me._clear(), me._history(rng, 17500 - at, keys[:300])))
    before, after = me._distinct_keys(rng, 3000, 0, me.POOL // 2), me._distinct_keys(rng, 2049, me.POOL // 2, me.POOL)
    docs.append(me._join(me._sets(rng, before), me._clear(), me._history(rng, 14000, after)))  # 5
    batch, facts = me._batch(docs, me.POOL)
    return batch, facts, me.dict_sparse(batch)


def test_clears_and_empties(orc, engine):
    """Every document is longer than 16384 ops. A clear as the last op and a document whose keys all end
    deleted have count 0 without being refused; a clear at ordinal 66 T - 1, 66 T (the last op of a
    tile) and 66 T + 1 (the first op of the next); 3000 keys before a clear and 2049 after it, of which
    only the latter appear."""
    batch, facts, want = _clears()
    assert all(f["n"] > me.SPARSE_MAX_OPS for f in facts)
    assert [f["n"] - f["tail"] for f in facts[2:5]] == [66 * T - 1, 66 * T, 66 * T + 1]
    assert facts[5]["distinct"] == 2049 and facts[5]["n"] - facts[5]["tail"] == 3001
    counts, entries = _check_both(orc, engine, batch, want)
    assert counts[0] == 0 and counts[1] == 0 and facts[0]["live"] == facts[1]["live"] == 0
    assert all(counts[d] == facts[d]["live"] > 0 for d in range(2, 6))
    assert (_doc_entries(counts, entries, 5)["key"] >= me.POOL // 2).all()


# ----------------------------------------------------------------------------------------- tile edges
@functools.lru_cache(maxsize=None)
def _tile_edges():
    rng = np.random.default_rng(202)
    keys = me._distinct_keys(rng, 600, 0, me.POOL // 2)
    gone = me._distinct_keys(rng, 400, 0, me.POOL // 2)
    docs = [me._history(rng, K * T - 1, keys),
            me._history(rng, K * T, keys),
            me._history(rng, K * T + 1, keys),
            me._sets(rng, me._distinct_keys(rng, K * T + 1)),  # every op a birth: first and last op of every tile
            me._join(me._history(rng, K * T - 400, gone), me._deletes(gone),
                     me._sets(rng, np.array([me.POOL - 1], dtype=np.uint32)))]  # the final op bears the only live key
    batch, facts = me._batch(docs, me.POOL)
    return batch, facts, me.dict_sparse(batch)


def test_tile_edges(orc, engine):
    """K T - 1, K T and K T + 1 ops (the last tile one op short, whole, and a single op); a document
    whose every op is a birth, so births sit on the first and last op of each tile and the ranks cross
    every tile base; a document whose only live key is born by its final op, alone in the last tile."""
    batch, facts, want = _tile_edges()
    assert [f["n"] for f in facts] == [K * T - 1, K * T, K * T + 1, K * T + 1, K * T + 1] and K * T - 1 >= OVER
    assert facts[3]["live"] == K * T + 1 and facts[4]["live"] == 1
    counts, entries = _check_both(orc, engine, batch, want)
    assert counts.tolist() == [f["live"] for f in facts]
    last = me.doc_ops(batch, 4)[-1]
    assert _doc_entries(counts, entries, 4).tolist() == [(me.POOL - 1, int(last["kind_value"]) & me.VALUE_MASK, K * T + 1)]


# ----------------------------------------------------- contention, probe chains, gapped seqs (one batch)
CHAIN, CHAIN_SLOTS = 70, 65536  # 17000 ops: the smallest power of two >= 34000
CHAIN_HOMES = (1000, CHAIN_SLOTS - 20)  # the second chain wraps past the table's end


@functools.lru_cache(maxsize=None)
def _hot():
    rng = np.random.default_rng(203)
    three = me._distinct_keys(rng, 3, 1, me.POOL)
    contention = me._ops(np.arange(20000) % 2 * MAP_DELETE, three[rng.integers(0, 3, 20000)], me._values(rng, 20000))
    chains = [me.keys_with_home(rng, h, CHAIN_SLOTS, CHAIN) for h in CHAIN_HOMES]
    both = np.concatenate(chains)
    probes = me._join(me._sets(rng, chains[0]), me._sets(rng, chains[1]),
                      me._history(rng, 17000 - 2 * CHAIN, np.concatenate([both, me._distinct_keys(rng, 200, 1, me.POOL)])))
    gapped = me._gapped(rng, me._history(rng, 17000, me._distinct_keys(rng, 700)), last=0xFFFFFFFF)
    batch, facts = me._batch([contention, probes, gapped], me.PROBE_KEY_BOUND, chains={1: chains})
    return batch, facts, me.dict_sparse(batch)


def test_contention_probe_chains_and_gapped_seqs(orc, engine):
    """20000 ops over 3 keys, sets and deletes by turns, so every atomic of the document lands in three
    slots; 70 keys with one home slot in the 65536-slot table, twice, one chain wrapping past the
    table's end; seqs with random gaps up to 0xFFFFFFFF (birth_seq is the op's seq, not its ordinal)."""
    batch, facts, want = _hot()
    assert MAP_SET == 0 and facts[0]["n"] == 20000 and facts[0]["distinct"] == 3
    assert facts[1]["n"] == 17000 and 2 * 17000 <= CHAIN_SLOTS < 4 * 17000
    for keys, home in zip(facts[1]["chains"], CHAIN_HOMES):
        assert len(set(keys.tolist())) == CHAIN and (me.sp_home(keys, CHAIN_SLOTS) == home).all()
    assert CHAIN_HOMES[1] + CHAIN > CHAIN_SLOTS
    seqs = me.doc_ops(batch, 2)["seq"].astype(np.int64)
    assert seqs[-1] == 0xFFFFFFFF and (np.diff(seqs) > 1).sum() > 16000
    counts, entries = _check_both(orc, engine, batch, want)
    assert counts.tolist() == [f["live"] for f in facts] and counts[1] >= CHAIN
    assert int(_doc_entries(counts, entries, 2)["birth_seq"].max()) > 1 << 31


# --------------------------------------------------------------------------------------- batch shapes
@functools.lru_cache(maxsize=None)
def _shape(name):
    rng = np.random.default_rng(204)
    small = lambda: [me._history(rng, 300, me._distinct_keys(rng, 100)), me._history(rng, 2000, me._distinct_keys(rng, 300)),
                     me._ops([], [], [])]  # noqa: E731  (register path, streaming, empty)
    long_ = lambda: me._history(rng, OVER, me._distinct_keys(rng, 500))  # noqa: E731
    wide = lambda: me._history(rng, 4096, me._distinct_keys(rng, me.SPARSE_MAX_KEYS + 1))  # noqa: E731
    docs = {"first": [long_()] + small(), "last": small() + [wide()], "alone": [long_()],
            "adjacent": small() + [wide(), long_()] + small()}[name]
    batch, facts = me._batch(docs, me.POOL)
    return batch, facts, me.dict_sparse(batch)


@pytest.mark.parametrize("name", ["first", "last", "alone", "adjacent"])
def test_batch_shapes(orc, engine, name):
    """The overflowing document first, last, alone in its batch, and two of them side by side (one over
    each limit) between LDS-tier documents, an empty one among them."""
    batch, facts, want = _shape(name)
    counts, _ = _check_both(orc, engine, batch, want, runs=1)
    assert counts.tolist() == [f["live"] for f in facts]
    assert engine.stats().launches == 8


def test_nothing_overflows(orc, engine):
    """A batch the LDS tier completes: the tiered run's result and stats record equal the plain run's."""
    batch, facts = me.limits_ok()
    engine.map_load_sparse(batch)
    engine.map_run_sparse()
    plain = engine.map_fetch_sparse()
    ps = engine.stats()
    engine.map_run_sparse_tiered()
    got = engine.map_fetch_sparse()
    ts = engine.stats()
    _assert_sparse(batch, got, plain, "the plain run")
    _assert_sparse(batch, got, me.sparse_reference("limits_ok"), "dict replay")
    oc, oe, _ = orc.map_replay_sparse(batch, threads=16)
    _assert_sparse(batch, got, (oc, oe), "oracle")
    assert ts.launches == ps.launches == 1
    assert (ts.ops, ts.docs, ts.bytes_read, ts.bytes_written) == (ps.ops, ps.docs, ps.bytes_read, ps.bytes_written)


# ------------------------------------------------------------------------------------------- bad key
@pytest.mark.parametrize("where", ["before_clear", "after_clear"])
def test_bad_key_in_a_long_document(engine, where):
    """A key id >= key_bound in a 17000-op document (which the LDS tier never scans): FMT_E_DATA at fetch,
    whether the op comes before or after the document's last clear."""
    rng = np.random.default_rng(205)
    keys = me._distinct_keys(rng, 300)
    doc = me._join(me._history(rng, 8999, keys), me._clear(), me._history(rng, 8000, keys))
    at = 4000 if where == "before_clear" else 13000
    doc["key"][at] = me.POOL + 5
    assert (doc["kind_value"][at] >> MAP_KIND_SHIFT) in (MAP_SET, MAP_DELETE)
    batch, _ = me._batch([me._history(rng, 300, keys), doc], me.POOL)
    engine.map_load_sparse(batch)
    engine.map_run_sparse_tiered()
    rc, _, _ = _fetch_raw(engine, batch)
    assert rc == FMT_E_DATA
    with pytest.raises(native.EngineError) as ei:
        engine.map_fetch_sparse()
    assert ei.value.code == FMT_E_DATA


# ------------------------------------------------------------------------------------ pending on top
def test_pending_view_over_a_long_document(orc, engine):
    """fmt_map_pending_run after the tiered run: a 16385-op document (and a small neighbour) with a few
    dozen submit / ack / rollback events each equals the oracle's pending restatement."""
    rng = np.random.default_rng(206)
    keys = me._distinct_keys(rng, 500)
    seq_batch, _ = me._batch([me._history(rng, OVER, keys), me._history(rng, 200, keys[:40])], me.POOL)
    events, offs = [], [0]
    for d in range(2):
        unacked = []
        for _ in range(48):
            r = rng.random()
            if r < 0.6 or not unacked:
                # (clears only in the neighbour: a pending clear hides every sequenced entry)
                kind = [MAP_SET, MAP_SET, MAP_DELETE, MAP_CLEAR if d == 1 else MAP_DELETE][int(rng.integers(0, 4))]
                key = 0 if kind == MAP_CLEAR else int(rng.choice(keys[:60]) if rng.random() < 0.8 else rng.integers(0, me.POOL))
                kv = (kind << MAP_KIND_SHIFT) | (int(rng.integers(0, 1000)) if kind == MAP_SET else 0)
                unacked.append((key, kv))
                events.append((d, key, MAP_EV_SUBMIT, kv))
            elif r < 0.8:
                key, kv = unacked.pop(0)
                events.append((d, key, MAP_EV_ACK, kv))
            else:
                key, kv = unacked.pop()
                events.append((d, key, MAP_EV_ROLLBACK, kv))
        offs.append(len(events))
    batch = MapBatch(seq_batch.ops, seq_batch.doc_op_offsets, me.POOL, [], [],
                     np.array(events, dtype=np.uint32).view(MAP_LOCAL_OP_DTYPE).reshape(-1), np.array(offs, dtype=np.uint64))
    got = _tiered(engine, batch)
    _assert_sparse(batch, got, me.dict_sparse(batch), "dict replay")
    counts, status, entries = engine.map_pending(batch)
    ec, es, ee = orc.map_pending(batch)
    assert status.tolist() == es.tolist() == [0, 0]
    _assert_sparse(batch, (counts, entries), (ec, ee), "oracle pending view")
    assert counts[0] > 100 and (entries["birth_seq"] >= 0x80000000).any()


# -------------------------------------------------------------------------------------- one wider case
def test_one_wider_case(orc, engine):
    """One document of 3 x 10^5 ops over 6 x 10^4 keys (1172 tiles, a 2^20-slot table) and 64 documents
    of 20000 ops in one batch, against the oracle."""
    rng = np.random.default_rng(207)
    docs = [me._history(rng, 300_000, me._distinct_keys(rng, 60_000))]
    docs += [me._history(rng, 20000, me._distinct_keys(rng, 500 + 40 * d)) for d in range(64)]
    batch, facts = me._batch(docs, me.POOL)
    got = _tiered(engine, batch)
    oc, oe, _ = orc.map_replay_sparse(batch, threads=16)
    _assert_sparse(batch, got, (oc, oe), "oracle")
    assert got[0].tolist() == [f["live"] for f in facts] and got[0][0] > 10_000
    assert engine.stats().launches == 8

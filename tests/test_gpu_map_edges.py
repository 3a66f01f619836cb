"""GPU parity of the SharedMap kernels on the edge streams of tests/map_edges.py.

mapSparseKernel (groups a-g) and mapLwwKernel / mapLwwHbmKernel + mapLwwFinishKernel (group h)
against two references, a Python dict replayed op by op and the C++ oracle: every count and every
entry field, every dense slot, equal (integer state, no tolerance). The streams are the ones
`workloads.map_stream` cannot make: clear-free tails up to 16384 ops, hash tables at load 1, probe
chains that wrap, clears on chunk boundaries, seqs with gaps up to 0xFFFFFFFF, a batch that hands
every wave several documents of different paths. test_map_edges.py holds the builders to that.

Run with `pytest -m gpu`.
"""
import ctypes
import re

import numpy as np
import pytest

import map_edges as me
from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_CAPACITY, FMT_E_DATA, MAP_ENTRY_DTYPE, MAP_SLOT_DTYPE
from fluidframework_amd.streams import MAP_OP_DTYPE, MapBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = native.Engine(0)
    yield e
    e.close()


def _sparse(engine, batch):
    engine.map_load_sparse(batch)
    engine.map_run_sparse()
    return engine.map_fetch_sparse()


def _assert_sparse(batch, got, want, who):
    """Counts and every entry field equal; on a difference, name the first document that differs."""
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


def _oracle_sparse(orc, batch, refused=()):
    counts, entries, _ = orc.map_replay_sparse(batch, threads=16)
    return me.drop_docs(counts, entries, refused) if refused else (counts, entries)


@pytest.mark.parametrize("name", ["tails", "clears", "histories", "limits_ok", "probes", "seqs"])
def test_map_sparse_edges(orc, engine, name):
    """Groups a-f through mapSparseKernel: table sizes 64 .. 2048 on both sides of each switch, clears
    on chunk and path boundaries, clear-free histories of up to 16384 ops over up to 2048 keys (the
    table at load 1, its last key probing all 2048 slots), probe chains that wrap, gapped seqs."""
    batch, facts = me.SPARSE_GROUPS[name]()
    got = _sparse(engine, batch)
    _assert_sparse(batch, got, me.sparse_reference(name), "dict replay")
    _assert_sparse(batch, got, _oracle_sparse(orc, batch), "oracle")
    assert int(got[0].sum()) == sum(f["live"] for f in facts) > 0
    engine.map_run_sparse()  # a second run over the same tables and parked words
    _assert_sparse(batch, engine.map_fetch_sparse(), me.sparse_reference(name), "dict replay (second run)")


def _fetch_sparse_raw(engine, batch):
    """fmt_map_fetch_sparse's return code beside the counts and entries it fills before it returns an
    error (Engine.map_fetch_sparse raises on the code and hides them)."""
    counts = np.full(batch.n_docs, 0xDEADBEEF, dtype=np.uint32)
    entries = np.zeros(max(len(batch.ops), 1), dtype=MAP_ENTRY_DTYPE)
    n = ctypes.c_uint64()
    rc = native.lib().fmt_map_fetch_sparse(engine.h, counts.ctypes.data_as(ctypes.c_void_p),
                                           entries.ctypes.data_as(ctypes.c_void_p), len(entries), ctypes.byref(n))
    return rc, counts, entries[: n.value]


@pytest.mark.parametrize("name", ["limits_keys", "limits_ops"])
def test_map_sparse_refusals_leave_the_neighbours_alone(orc, engine, name):
    """2049 distinct keys, or 16385 ops, in one document: FMT_E_CAPACITY and count 0 for it, and the
    documents before and after it (a register-path and a streaming one) equal to both references."""
    batch, facts = me.SPARSE_GROUPS[name]()
    refused = [d for d, f in enumerate(facts) if f.get("refused")]
    assert refused == [1]
    engine.map_load_sparse(batch)
    engine.map_run_sparse()
    rc, counts, entries = _fetch_sparse_raw(engine, batch)
    assert rc == FMT_E_CAPACITY
    assert counts[1] == 0
    _assert_sparse(batch, (counts, entries), me.sparse_reference(name), "dict replay")
    _assert_sparse(batch, (counts, entries), _oracle_sparse(orc, batch, refused), "oracle")
    assert int(counts.sum()) == facts[0]["live"] + facts[2]["live"] > 0
    with pytest.raises(native.EngineError) as ei:
        engine.map_fetch_sparse()
    assert ei.value.code == FMT_E_CAPACITY


def test_map_sparse_pipeline_of_mixed_documents(orc, engine):
    """Group g: enough documents that every wave takes three or more, lengths 0, 1, 65, 1024, 1025, 33,
    1100 by turns, so the prefetched records and offsets cross register-path, streaming and empty
    documents in every order a period of 7 gives. Two runs, both equal to both references."""
    cus = int(re.search(r"CUs=(\d+)", engine.device_info()).group(1))
    n_docs = max(me.PIPELINE_DOCS, cus * 5 * 2 * 3)  # CUs x workgroups per CU (LDS) x waves x 3 documents
    batch, facts = me.pipeline(n_docs)
    want = me.sparse_reference("pipeline", n_docs)
    oracle = _oracle_sparse(orc, batch)
    first = _sparse(engine, batch)
    engine.map_run_sparse()
    second = engine.map_fetch_sparse()
    for got in (first, second):
        _assert_sparse(batch, got, want, "dict replay")
        _assert_sparse(batch, got, oracle, "oracle")
    assert int(first[0].sum()) == sum(f["live"] for f in facts) > n_docs


def _dense(engine, batch):
    engine.map_load(batch)
    engine.map_run()
    return engine.map_fetch()


def _assert_dense(batch, got, want, who):
    if np.array_equal(got, want):
        return
    d, k = (int(x[0]) for x in np.nonzero(got != want))
    pytest.fail(f"vs {who}: document {d} ({len(me.doc_ops(batch, d))} ops) key {k}: {got[d, k]} != {want[d, k]}")


@pytest.mark.parametrize("key_bound", me.DENSE_KEY_BOUNDS)
def test_map_lww_edges(orc, engine, key_bound):
    """Group h: the clear, long-history and gapped-seq documents and ragged lengths 0 .. 3000, key ids
    folded into 1, 63, 64, 65 and 2560 ids (mapLwwKernel) and 2561 (mapLwwHbmKernel + mapLwwFinishKernel);
    a second run checks the table fills between runs."""
    batch, facts = me.dense(key_bound)
    want = me.dense_reference(key_bound)
    exp, _ = orc.map_replay(batch, threads=16)
    got = _dense(engine, batch)
    _assert_dense(batch, got, want, "dict replay")
    _assert_dense(batch, got, exp, "oracle")
    assert int((got["value"] != 0xFFFFFFFF).sum()) == sum(f["live"] for f in facts) > 0
    engine.map_run()
    _assert_dense(batch, engine.map_fetch(), want, "dict replay (second run)")


@pytest.mark.parametrize("key_bound", [2560, 2561])
def test_map_replay_device_edges(orc, engine, key_bound):
    """The same batches through fmt_map_replay_device on torch-owned buffers, both sides of the LDS /
    HBM-table switch, twice over the same output buffer."""
    import torch

    batch, facts = me.dense(key_bound)
    want = me.dense_reference(key_bound)
    exp, _ = orc.map_replay(batch, threads=16)
    raw = torch.from_numpy(np.ascontiguousarray(batch.ops).view(np.uint8).copy()).cuda()
    offs = torch.from_numpy(np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64).view(np.int64).copy()).cuda()
    out = torch.full((batch.n_docs * key_bound * 8,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for run in ("first", "second"):
        engine.map_replay_device(raw.data_ptr(), offs.data_ptr(), batch.n_docs, key_bound, out.data_ptr())
        engine.map_check()
        got = out.cpu().numpy().view(MAP_SLOT_DTYPE).reshape(batch.n_docs, key_bound)
        _assert_dense(batch, got, want, f"dict replay ({run} run)")
        _assert_dense(batch, got, exp, f"oracle ({run} run)")
    assert int((got["value"] != 0xFFFFFFFF).sum()) == sum(f["live"] for f in facts) > 0


def test_map_seq_zero_is_refused_at_load(engine):
    """Seq 0 is the dense kernels' "nothing seen yet", so a set at seq 0 would be dropped there and kept
    by the sparse kernel: both loads refuse it with FMT_E_DATA (fmt.h fmt_map_op: seqs are >= 1), in
    the first document or a later one; the same documents from seq 1 load and replay."""
    ops = np.zeros(5, dtype=MAP_OP_DTYPE)
    ops["doc"] = [0, 0, 1, 1, 1]
    ops["key"] = [3, 4, 5, 3, 6]
    ops["seq"] = [1, 2, 1, 5, 9]
    ops["kind_value"] = [7, 8, 9, 10, 11]  # sets
    offs = np.array([0, 2, 5], dtype=np.uint64)
    for zero_at in (0, 2):
        bad = ops.copy()
        bad["seq"][zero_at] = 0
        for load in (engine.map_load, engine.map_load_sparse):
            with pytest.raises(native.EngineError) as ei:
                load(MapBatch(bad, offs, 8, [], []))
            assert ei.value.code == FMT_E_DATA
            assert "seq 0" in str(ei.value)
    good = MapBatch(ops, offs, 8, [], [])
    counts, entries = _sparse(engine, good)
    assert counts.tolist() == [2, 3]
    assert entries.tolist() == [(3, 7, 1), (4, 8, 2), (5, 9, 1), (3, 10, 5), (6, 11, 9)] == me.dict_replay(ops[:2]) + me.dict_replay(ops[2:])
    assert np.array_equal(_dense(engine, good), me.dict_dense(good))

"""Batches and references of the bulk SnapshotV1 tests (test_v1_bulk_cpu.py, test_gpu_v1_bulk.py).

The reference of every comparison is summary.v1_summary over the oracle's replay with the oracle's
remove stamps (orc.mt_removers), computed once per batch and shared."""
import functools

import numpy as np

from fluidframework_amd import summary, workloads
from fluidframework_amd.streams import flag_remove_order

FARM_CHUNK = 64
SYNTHETIC_NAMES = [f"c{k}" for k in range(254)]  # generated farms carry no client names


def names(batch, d):
    return batch.clients[d] if batch.clients else SYNTHETIC_NAMES


def all_names(batch):
    return [names(batch, d) for d in range(batch.n_docs)]


@functools.lru_cache(maxsize=None)
def farm_batch():
    """48 conflict-farm documents with props on inserts, remove order flagged: up to 377 leaves (the
    compact -> small cascade), 3,439 leaves removed above minSeq, 2,439 of them with more than one
    stamp, 67-372 V1 segments per document."""
    batch = workloads.with_insert_props(workloads.conflict_farm(48, n_clients=8, ops_per_doc=1000, seed=31))
    flag_remove_order(batch.ops, batch.doc_op_offsets)
    return batch


def oracle_state(orc, batch, cap_leaves=4096, cap_chars=1 << 16, cap_props=1024, numbers=None):
    """[(header, leaves, chars, props, removers)] per document of the oracle's replay (every status 0)."""
    rc, h, l, c, p, _ = orc.mt_replay_batch(batch, threads=8, cap_leaves=cap_leaves, cap_chars=cap_chars,
                                            cap_props=cap_props, numbers=numbers)
    assert rc == 0 and (h["status"] == 0).all()
    return [(h[d], l[d], c[d], p[d], orc.mt_removers(batch, d)) for d in range(batch.n_docs)]


def reference(batch, state, chunk=summary.V1_CHUNK_SIZE, values=None):
    """[(header blob, [bodies])] per document: summary.v1_summary over the oracle's state and stamps."""
    return [summary.v1_summary(h, l, c, p, batch.keys, values[d] if values else batch.values, names(batch, d), rm,
                               chunk_size=chunk)
            for d, (h, l, c, p, rm) in enumerate(state)]


def stamp_counts(state):
    """(leaves removed above minSeq, those with more than one stamp, those with a sliceRemove stamp)."""
    removed = multi = moved = 0
    for h, l, _, _, rm in state:
        ms = int(h["min_seq"])
        for i in range(int(h["n_leaves"])):
            r = int(l[i]["rm_seq"])
            if r != summary.NOT_REMOVED and r > ms:
                removed += 1
                multi += len(rm[i]) > 1
                moved += any(k == 1 for _, _, k in rm[i])
    return removed, multi, moved


def set_remover_pairs(state):
    """Leaves above minSeq with two or more setRemove stamps."""
    n = 0
    for h, l, _, _, rm in state:
        ms = int(h["min_seq"])
        for i in range(int(h["n_leaves"])):
            r = int(l[i]["rm_seq"])
            if r != summary.NOT_REMOVED and r > ms:
                n += sum(k == 0 for _, _, k in rm[i]) >= 2
    return n


def concat_docs(batch, docs):
    """The documents `docs` of `batch`, as a batch (same arena and tables)."""
    from dataclasses import replace

    offs, ops = [0], []
    for d in docs:
        a, b = int(batch.doc_op_offsets[d]), int(batch.doc_op_offsets[d + 1])
        ops.append(batch.ops[a:b])
        offs.append(offs[-1] + (b - a))
    return replace(batch, ops=np.concatenate(ops).copy(), doc_op_offsets=np.asarray(offs, dtype=np.uint64),
                   doc_init=batch.doc_init[list(docs)].copy(),
                   clients=[batch.clients[d] for d in docs] if batch.clients else [])

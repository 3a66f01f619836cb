"""SharedMap edge streams and their plain reference (used by test_map_edges.py and test_gpu_map_edges.py).

The reference is a Python dict replayed op by op (`dict_replay`): a dict keeps insertion order, keeps
the position of a key that is set again and moves a deleted and re-set key to the end, which is the JS
Map contract the kernels reproduce. Expected values come from it (and from the C++ oracle) alone: no
hash, no ordinals, no kernel constants.

The builders make the streams `workloads.map_stream` never does (one clear per 41 ops leaves a tail of
about 40 ops, whatever the document length): long clear-free tails, clears at chosen ordinals, full
hash tables, colliding keys, seqs with gaps. Each returns (MapBatch, facts): facts[d] holds what the
builder promises of document d: `n` ops, `tail` (ops after the last clear), `distinct` (keys touched
in the tail) and `live` (keys that end live). test_map_edges.py checks the promises on the CPU, so a
builder swapped for something tamer is noticed.
"""
import functools

import numpy as np

from fluidframework_amd.native import MAP_ENTRY_DTYPE, MAP_SLOT_DTYPE
from fluidframework_amd.streams import (MAP_ABSENT, MAP_CLEAR, MAP_DELETE, MAP_KIND_SHIFT, MAP_OP_DTYPE, MAP_SET,
                                        MAP_VALUE_UNDEFINED, MapBatch)

VALUE_MASK = 0x3FFFFFFF
POOL = 1 << 20
SPARSE_MAX_KEYS, SPARSE_MAX_OPS = 2048, 16384  # fmt.h FMT_MAP_SPARSE_MAX_KEYS / _MAX_OPS


# ------------------------------------------------------------------------------------ the reference
def dict_replay(ops):
    """[(key, value, birth_seq)] of one document's MAP_OP_DTYPE records, in Map order."""
    m = {}
    for key, seq, kv in zip(ops["key"].tolist(), ops["seq"].tolist(), ops["kind_value"].tolist()):
        kind = kv >> MAP_KIND_SHIFT
        if kind == MAP_SET:
            e = m.get(key)
            if e is None:
                m[key] = [kv & VALUE_MASK, seq]  # an absent key is appended, born at this set
            else:
                e[0] = kv & VALUE_MASK           # a present key keeps its place and its birth
        elif kind == MAP_DELETE:
            m.pop(key, None)
        else:
            m.clear()
    return [(k, v, b) for k, (v, b) in m.items()]


def to_dense(entries, key_bound):
    """MAP_SLOT_DTYPE rows of one document: FMT_MAP_ABSENT and birth 0 for keys that are not live."""
    rows = np.zeros(key_bound, dtype=MAP_SLOT_DTYPE)
    rows["value"] = MAP_ABSENT
    for k, v, b in entries:
        rows[k] = (v, b)
    return rows


def doc_ops(batch, d):
    return batch.ops[int(batch.doc_op_offsets[d]) : int(batch.doc_op_offsets[d + 1])]


def dict_sparse(batch, refused=()):
    """(counts, entries packed in document order) as fmt_map_fetch_sparse lays them out; the documents
    in `refused` (over a limit of the sparse path) have no entries."""
    per_doc = [[] if d in refused else dict_replay(doc_ops(batch, d)) for d in range(batch.n_docs)]
    counts = np.array([len(e) for e in per_doc], dtype=np.uint32)
    flat = [e for doc in per_doc for e in doc]
    entries = np.array(flat, dtype=np.uint32).reshape(-1, 3).view(MAP_ENTRY_DTYPE).reshape(-1)
    return counts, entries


def dict_dense(batch):
    return np.stack([to_dense(dict_replay(doc_ops(batch, d)), batch.key_bound) for d in range(batch.n_docs)])


def drop_docs(counts, entries, docs):
    """(counts, entries) of a packed sparse result without the entries of `docs` (counts set to 0)."""
    c = counts.astype(np.int64)
    keep = np.repeat(~np.isin(np.arange(len(c)), list(docs)), c)
    out = counts.copy()
    out[list(docs)] = 0
    return out, entries[keep]


# ---------------------------------------------------------------------------------- building blocks
SPECIAL_VALUES = np.array([0, 49, 50, MAP_VALUE_UNDEFINED], dtype=np.uint32)


def _values(rng, n, special=0.25):
    v = rng.integers(0, MAP_VALUE_UNDEFINED, n, dtype=np.uint32)
    return np.where(rng.random(n) < special, SPECIAL_VALUES[rng.integers(0, 4, n)], v).astype(np.uint32)


def _ops(kinds, keys, values):
    """Records with seq = 1-based ordinal (the doc field is filled by _batch)."""
    kinds = np.asarray(kinds, dtype=np.uint32)
    o = np.zeros(len(kinds), dtype=MAP_OP_DTYPE)
    o["key"] = np.where(kinds == MAP_CLEAR, 0, np.asarray(keys, dtype=np.uint32))
    o["seq"] = np.arange(1, len(kinds) + 1, dtype=np.uint32)
    o["kind_value"] = (kinds << np.uint32(MAP_KIND_SHIFT)) | np.where(kinds == MAP_SET, values, 0).astype(np.uint32)
    return o


def _sets(rng, keys):
    return _ops(np.full(len(keys), MAP_SET), keys, _values(rng, len(keys)))


def _deletes(keys):
    return _ops(np.full(len(keys), MAP_DELETE), keys, np.zeros(len(keys), dtype=np.uint32))


def _clear():
    return _ops([MAP_CLEAR], [0], [0])


def _join(*parts):
    o = np.concatenate(parts)
    o["seq"] = np.arange(1, len(o) + 1, dtype=np.uint32)
    return o


def _distinct_keys(rng, k, lo=0, hi=POOL):
    got = np.zeros(0, dtype=np.int64)
    while len(got) < k:
        got = np.unique(np.concatenate([got, rng.integers(lo, hi, 2 * k + 16)]))
    return rng.permutation(got)[:k].astype(np.uint32)


def _history(rng, n, keys, p_set=0.6, p_clear=0.0):
    """n random sets / deletes (p_set / 1 - p_set) over `keys`, every key touched when n >= len(keys)."""
    k = len(keys)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, max(n - k, 0))])[:n]
    rng.shuffle(idx)
    r = rng.random(n)
    kinds = np.where(r < p_clear, MAP_CLEAR, np.where(rng.random(n) < p_set, MAP_SET, MAP_DELETE))
    return _ops(kinds, np.asarray(keys)[idx], _values(rng, n))


def _facts(ops):
    """What the builders promise of a document (test_map_edges.py measures the same another way)."""
    kinds = ops["kind_value"] >> np.uint32(MAP_KIND_SHIFT)
    clears = np.nonzero(kinds == MAP_CLEAR)[0]
    c = int(clears[-1]) + 1 if len(clears) else 0
    uniq, last = np.unique(ops["key"][c:][::-1], return_index=True)  # a key is live iff its last op is a set
    live = int((kinds[c:][::-1][last] == MAP_SET).sum())
    return {"n": len(ops), "tail": len(ops) - c, "distinct": len(uniq), "live": live}


def _batch(docs, key_bound, **extra):
    lens = [len(d) for d in docs]
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    ops = np.concatenate(docs) if docs else np.zeros(0, dtype=MAP_OP_DTYPE)
    ops["doc"] = np.repeat(np.arange(len(docs), dtype=np.uint32), lens)
    facts = [dict(_facts(d)) for d in docs]
    for name, per_doc in extra.items():
        for d, v in per_doc.items():
            facts[d][name] = v
    ops.setflags(write=False)  # shared between tests: nobody edits it
    return MapBatch(ops, offs, key_bound, [], []), facts


# ------------------------------------------------------------------------ the hash, to choose inputs
def sp_home(keys, slots):
    """Home slot of a key in a `slots`-slot table: a mirror of spHash in csrc/map_sparse.hip
    (key * 0x9e3779b1 >> (32 - log2 slots)). It only CHOOSES inputs (keys that collide, a key whose
    probe chain is the whole table); no expected value is computed with it."""
    shift = 32 - (int(slots).bit_length() - 1)
    return ((np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


def sp_free_slots(keys, slots):
    """The slots linear probing leaves free after `keys` (which slots are taken does not depend on the order)."""
    taken = set()
    for h in sp_home(keys, slots).tolist():
        while h in taken:
            h = (h + 1) % slots
        taken.add(h)
    return sorted(set(range(slots)) - taken)


def keys_with_home(rng, home, slots, count, hi=1 << 32):
    cand = np.arange(1, min(hi, slots * count * 4), dtype=np.uint64)
    cand = cand[sp_home(cand, slots) == home]
    return rng.permutation(cand)[:count].astype(np.uint32)


# ------------------------------------------------------------------------------------------- groups
TAILS = [0, 1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024]
TAIL_PREFIXES = [0, 64, 65, 1000]  # ordinal of the clear that ends the prefix (0: no prefix)


@functools.lru_cache(maxsize=None)
def tails():
    """a. Tail lengths at every table-size switch, as whole documents and behind a prefix that ends in
    a clear at ordinal 64 (last lane of chunk 0), 65 (first lane of chunk 1) and 1000. Every op of the
    tail has its own key (4 sets to 1 delete), none of them a key of the prefix."""
    rng = np.random.default_rng(101)
    docs = []
    for p in TAIL_PREFIXES:
        for m in TAILS:
            keys = _distinct_keys(rng, m, POOL // 2, POOL)
            tail = _ops(np.where(rng.random(m) < 0.8, MAP_SET, MAP_DELETE), keys, _values(rng, m))
            if p == 0:
                docs.append(tail)
            else:
                docs.append(_join(_history(rng, p - 1, _distinct_keys(rng, 40, 0, POOL // 2)), _clear(), tail))
    return _batch(docs, POOL)


CLEAR_LAST = [1, 64, 65, 1024, 1025, 4096]


def _clear_docs(rng):
    pool = _distinct_keys(rng, 300)
    docs = [_clear(),                                              # clear as the only op
            _join(_clear(), _sets(rng, pool[:50]))]                # clear first
    docs += [_join(_history(rng, n - 1, pool[: max(1, n // 3)]), _clear()) for n in CLEAR_LAST]  # clear last
    docs.append(_join(_history(rng, 90, pool[:30]), _clear(), _clear(), _history(rng, 70, pool[:40])))
    for at in (1024, 1025):                                        # the register / streaming boundary
        docs.append(_join(_history(rng, at - 1, pool), _clear(), _history(rng, 1100 - at, pool[100:160])))
    docs.append(_deletes(pool[rng.integers(0, 30, 100)]))          # deletes only
    a, b, c = (pool[i : i + 1] for i in range(3))
    docs.append(_join(_sets(rng, a), _deletes(b), _sets(rng, c)))  # a delete of a key never set
    docs.append(_join(_sets(rng, a), _sets(rng, b), _sets(rng, a), _deletes(a)))  # a's last op is a delete
    return docs


@functools.lru_cache(maxsize=None)
def clears():
    """b. Clear positions: only op, first, last (n = 1 .. 4096), two in a row, at ordinal 1024 / 1025 of
    1100; deletes only, a delete of a key never set, a key whose last op is a delete."""
    return _batch(_clear_docs(np.random.default_rng(102)), POOL)


HISTORIES = [(1024, 700), (1024, 1024), (1025, 700), (1025, 1024), (4096, 700), (4096, 1500), (4096, 2048),
             (16384, 700), (16384, 1500), (16384, 2048)]


def _one_key_chunk(rng, n, chunk, key, others, alternate, first_kind=MAP_SET):
    """n ops over `others`, but chunk `chunk`'s 64 lanes all hit `key` (which no other op touches):
    64 sets, or set / delete by turns starting with first_kind."""
    o = _history(rng, n, others)
    if alternate:
        kinds = (np.arange(64) + (0 if first_kind == MAP_SET else 1)) % 2  # 0 = set, 1 = delete
    else:
        kinds = np.zeros(64, dtype=np.int64)
    o[chunk * 64 : chunk * 64 + 64] = _ops(kinds, np.full(64, key), _values(rng, 64))
    return _join(o)


def _history_docs(rng):
    docs = [_history(rng, n, _distinct_keys(rng, k)) for n, k in HISTORIES]
    # every op a birth: the entry of rank r is written over the parked words of ordinal r itself
    docs.append(_sets(rng, _distinct_keys(rng, 1100)))
    docs.append(_join(_sets(rng, _distinct_keys(rng, 200, POOL // 2, POOL)),
                      _history(rng, 1300, _distinct_keys(rng, 500, 0, POOL // 2))))
    others = _distinct_keys(rng, 120, 0, POOL // 2)
    for n, chunk in ((192, 1), (1088, 16)):  # register and streaming path
        docs.append(_one_key_chunk(rng, n, chunk, POOL - 5, others, alternate=False))
        docs.append(_one_key_chunk(rng, n, chunk, POOL - 6, others, alternate=True))                      # ends deleted
        docs.append(_one_key_chunk(rng, n, chunk, POOL - 7, others, alternate=True, first_kind=MAP_DELETE))  # ends set
    return docs


N_HISTORIES = len(HISTORIES)


@functools.lru_cache(maxsize=None)
def histories():
    """c. Long histories without a clear: set / delete 60 / 40 over 700 .. 2048 keys in 1024 .. 16384 ops;
    documents whose every op creates an entry; a chunk whose 64 lanes all set one key, or set and delete
    it by turns."""
    return _batch(_history_docs(np.random.default_rng(103)), POOL)


def _full_table_doc(rng):
    """16384 ops over 2048 distinct keys. The last key to appear (alone, in the last chunk) has its home
    one past the only slot the other 2047 leave free, so its probe chain is the whole table: all 2048
    probes are needed."""
    others = _distinct_keys(rng, SPARSE_MAX_KEYS - 1)
    (free,) = sp_free_slots(others, SPARSE_MAX_KEYS)
    cand = np.setdiff1d(np.arange(POOL, dtype=np.uint32), others)
    last = cand[sp_home(cand, SPARSE_MAX_KEYS) == (free + 1) % SPARSE_MAX_KEYS][:1]
    tail = _history(rng, 63, others[:40])
    return _join(_history(rng, SPARSE_MAX_OPS - 64, others), tail[:30], _sets(rng, last), tail[30:]), int(last[0])


def _neighbours(rng):
    return [_history(rng, 300, _distinct_keys(rng, 100)), _history(rng, 2000, _distinct_keys(rng, 300))]


@functools.lru_cache(maxsize=None)
def limits_ok():
    """d. At the limits of the streaming path, all succeeding: 2048 keys at load 1 in 16384 ops; 2048 keys
    of which 2000 end deleted; 3000 keys before a clear and 100 after it."""
    rng = np.random.default_rng(104)
    full, last_key = _full_table_doc(rng)
    keys = _distinct_keys(rng, SPARSE_MAX_KEYS)
    end = np.concatenate([_deletes(keys[:2000]), _sets(rng, keys[2000:])])
    mostly_deleted = _join(_history(rng, SPARSE_MAX_OPS - SPARSE_MAX_KEYS, keys), rng.permutation(end))
    after_clear = _join(_sets(rng, _distinct_keys(rng, 3000)), _clear(), _history(rng, 150, _distinct_keys(rng, 100)))
    return _batch([full, mostly_deleted, after_clear], POOL, last_key={0: last_key})


@functools.lru_cache(maxsize=None)
def limits_keys():
    """d. 2049 distinct keys (document 1): FMT_E_CAPACITY and count 0; its neighbours are unaffected."""
    rng = np.random.default_rng(105)
    a, b = _neighbours(rng)
    return _batch([a, _history(rng, 4096, _distinct_keys(rng, SPARSE_MAX_KEYS + 1)), b], POOL, refused={1: True})


@functools.lru_cache(maxsize=None)
def limits_ops():
    """d. 16385 ops (document 1): FMT_E_CAPACITY and count 0; its neighbours are unaffected."""
    rng = np.random.default_rng(106)
    a, b = _neighbours(rng)
    return _batch([a, _history(rng, SPARSE_MAX_OPS + 1, _distinct_keys(rng, 500)), b], POOL, refused={1: True})


PROBE_KEY_BOUND = 0xFFFFFFFF
PROBE_HOME_2048, PROBE_HOME_128 = 1900, 120  # 600 keys from slot 1900 and 40 from slot 120 wrap round


@functools.lru_cache(maxsize=None)
def probes():
    """e. Probe chains: 600 keys with one home slot in the 2048-slot table (register and streaming
    path) and 40 with one home in the 128-slot table (tail 40), both chains wrapping past the last
    slot; keys that are multiples of 2^12 and 2^20; key 0 and key_bound - 1 = 2^32 - 2."""
    rng = np.random.default_rng(107)
    big = keys_with_home(rng, PROBE_HOME_2048, 2048, 600)
    small = keys_with_home(rng, PROBE_HOME_128, 128, 40)
    docs = [_join(_sets(rng, big), _history(rng, 300, big)),
            _join(_sets(rng, big), _history(rng, 900, big)),
            _sets(rng, small),
            _join(_history(rng, 100, big[:50]), _clear(), _sets(rng, small)),
            _history(rng, 900, _distinct_keys(rng, 300, 1, 1 << 20) << np.uint32(12)),
            _history(rng, 900, _distinct_keys(rng, 300, 1, 1 << 12) << np.uint32(20)),
            _history(rng, 1500, _distinct_keys(rng, 400, 1, 1 << 12) << np.uint32(20)),
            _history(rng, 200, np.array([0, PROBE_KEY_BOUND - 1, 1, PROBE_KEY_BOUND - 2], dtype=np.uint32))]
    return _batch(docs, PROBE_KEY_BOUND, home={0: (2048, PROBE_HOME_2048, 600), 1: (2048, PROBE_HOME_2048, 600),
                                               2: (128, PROBE_HOME_128, 40), 3: (128, PROBE_HOME_128, 40)})


def _gapped(rng, ops, first=None, last=None):
    """`ops` with random gaps between seqs (strictly increasing), the first or the last seq as given."""
    n = len(ops)
    seqs = np.unique(rng.integers(2, 0xFFFFFFFF, 2 * n + 16, dtype=np.uint64))
    seqs = np.sort(rng.permutation(seqs)[:n])
    if first is not None:
        seqs[0] = first
    if last is not None:
        seqs[-1] = last
    out = ops.copy()
    out["seq"] = seqs.astype(np.uint32)
    return out


def _seq_docs(rng):
    docs = []
    for n in (1, 64, 700, 1500):
        h = _history(rng, n, _distinct_keys(rng, n // 3 + 1), p_clear=0.003)
        from_seven = h.copy()
        from_seven["seq"] += 6
        docs += [h, from_seven, _gapped(rng, h, first=1), _gapped(rng, h, last=0xFFFFFFFF)]
    keys = _distinct_keys(rng, 8)
    docs.append(_gapped(rng, _ops(np.zeros(200), keys[rng.integers(0, 8, 200)], _values(rng, 200, special=1.0)),
                        last=0xFFFFFFFF))
    return docs


@functools.lru_cache(maxsize=None)
def seqs():
    """f. Seqs and values: first seq 1 and 7, random gaps, last seq 0xFFFFFFFF; value ids 0, 49, 50 and
    FMT_MAP_VALUE_UNDEFINED. (Seq 0 is refused at load: test_gpu_map_edges.py.)"""
    return _batch(_seq_docs(np.random.default_rng(108)), POOL)


PIPELINE_LENGTHS = [0, 1, 65, 1024, 1025, 33, 1100]
PIPELINE_DOCS = 8192  # 256 CUs x 5 workgroups x 2 waves take 3 documents each at 7680


def pipeline(n_docs=None):
    return _pipeline(n_docs or PIPELINE_DOCS)


@functools.lru_cache(maxsize=None)
def _pipeline(n_docs):
    """g. The software pipeline with mixed documents: lengths cycle with period 7 through empty, one-op,
    register-path and streaming documents, clear-free, about n / 4 keys per document out of 2^20."""
    rng = np.random.default_rng(109)
    lens = np.array(PIPELINE_LENGTHS, dtype=np.int64)[np.arange(n_docs) % len(PIPELINE_LENGTHS)]
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    total = int(offs[-1])
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), lens)
    per = np.repeat(lens // 4 + 1, lens)
    ops = _ops(np.where(rng.random(total) < 0.6, MAP_SET, MAP_DELETE),
               (rng.integers(0, 1 << 30, total) % per * 4099 + doc * 7919) % POOL, _values(rng, total))
    ops["seq"] = np.arange(total) - np.repeat(offs[:-1], lens) + 1
    return _batch([ops[offs[d] : offs[d + 1]] for d in range(n_docs)], POOL)


DENSE_KEY_BOUNDS = [1, 63, 64, 65, 2560, 2561]  # 2560: the largest LDS table; 2561: the HBM-table kernels
RAGGED = [0, 1, 63, 64, 65, 1024, 1025, 3000]


@functools.lru_cache(maxsize=None)
def dense(key_bound):
    """h. The histories of b, c and f and ragged documents (a clear per 300 ops), key ids folded into
    key_bound."""
    rng = np.random.default_rng(110)
    docs = _clear_docs(rng) + _history_docs(rng) + _seq_docs(rng)
    docs += [_history(rng, n, _distinct_keys(rng, min(n, 3000) + 1), p_clear=1 / 300) for n in RAGGED]
    for d in docs:
        d["key"] %= np.uint32(key_bound)
    return _batch(docs, key_bound)


SPARSE_GROUPS = {"tails": tails, "clears": clears, "histories": histories, "limits_ok": limits_ok,
                 "limits_keys": limits_keys, "limits_ops": limits_ops, "probes": probes, "seqs": seqs,
                 "pipeline": pipeline}


def sparse_reference(name, n_docs=None):
    """dict_replay over a sparse group, computed once; refused documents have no entries."""
    return _sparse_reference(name, (n_docs or PIPELINE_DOCS) if name == "pipeline" else None)


@functools.lru_cache(maxsize=None)
def _sparse_reference(name, n_docs):
    batch, facts = SPARSE_GROUPS[name]() if n_docs is None else SPARSE_GROUPS[name](n_docs)
    counts, entries = dict_sparse(batch, refused={d for d, f in enumerate(facts) if f.get("refused")})
    counts.setflags(write=False)
    entries.setflags(write=False)
    return counts, entries


@functools.lru_cache(maxsize=None)
def dense_reference(key_bound):
    out = dict_dense(dense(key_bound)[0])
    out.setflags(write=False)
    return out

"""Bulk SnapshotV1 summaries without a GPU: the C ABI of include/fmt_v1.h is exported, and the bulk
path's host formatter (runtime.cpp v1Blobs through fmt_internal_v1_format: JSON, merge info, the
do-while chunking of SnapshotV1.emit, snapshotV1.ts:126-168) is byte-identical to summary.v1_summary
when it is fed the segment records the kernel writes (summary.v1_segment_records of the oracle's
state: the first remove stamp in the record, the later ones as remove-order entries)."""
import ctypes
import os
import re
import subprocess

import pytest

import v1_bulk
from fluidframework_amd import native, summary
from test_snapshot_v1 import NAMES, _collab_batch, _load_v1, obliterate_v1_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libfmt():
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "fluidframework_amd", "csrc")], check=True)
    return ctypes.CDLL(native.LIB_PATH)


def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    return sorted(set(re.findall(r"^(?:int|void|const char\*)\s+(fmt_\w+)\(", text, re.M)))


def test_library_exports_every_symbol_fmt_v1_declares(libfmt):
    fns = _declared("fmt_v1.h")
    assert len(fns) == 3
    assert not [f for f in fns if not hasattr(libfmt, f)]
    assert sorted(native.EXPORTED_SYMBOLS_V1) == fns
    assert not set(fns) & set(native.EXPORTED_SYMBOLS) and not set(fns) & set(_declared("fmt.h"))
    assert hasattr(libfmt, "fmt_internal_v1_format")


def _formatted(batch, state, chunk):
    out = []
    for d, (h, l, c, p, rm) in enumerate(state):
        segs, text, later = summary.v1_segment_records(h, l, c, p, rm)
        out.append(native.v1_format(segs, text, p[: int(h["n_props"])], later, batch.keys, batch.values,
                                    v1_bulk.names(batch, d), int(h["min_seq"]), int(h["cur_seq"]), chunk))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_formatter_writes_the_v1_fixtures(orc, libfmt, name):
    batch, head, bodies = _load_v1(name)
    state = v1_bulk.oracle_state(orc, batch, cap_leaves=1 << 16, cap_chars=1 << 20)
    assert v1_bulk.reference(batch, state) == [(head, bodies)]
    assert _formatted(batch, state, summary.V1_CHUNK_SIZE) == [(head, bodies)]


@pytest.mark.parametrize("make", [_collab_batch, obliterate_v1_batch], ids=["collab", "obliterate"])
def test_formatter_writes_merge_info(orc, libfmt, make):
    batch = make()
    state = v1_bulk.oracle_state(orc, batch)
    removed, multi, moved = v1_bulk.stamp_counts(state)
    assert removed > 0 and multi > 0 and (make is _collab_batch or moved > 0)
    assert _formatted(batch, state, summary.V1_CHUNK_SIZE) == v1_bulk.reference(batch, state)


def test_formatter_chunks_the_conflict_farm(orc, libfmt):
    batch = v1_bulk.farm_batch()
    state = v1_bulk.oracle_state(orc, batch)
    want = v1_bulk.reference(batch, state, chunk=v1_bulk.FARM_CHUNK)
    assert v1_bulk.stamp_counts(state)[:2] == (3439, 2439)
    assert all(1 <= len(bodies) <= 11 for _, bodies in want)
    assert _formatted(batch, state, v1_bulk.FARM_CHUNK) == want


def test_segment_records_refuse_an_unknown_remover(orc):
    batch = _collab_batch()
    h, l, c, p, rm = v1_bulk.oracle_state(orc, batch)[0]
    leaf = next(i for i in range(int(h["n_leaves"])) if summary.NOT_REMOVED != int(l[i]["rm_seq"]) > int(h["min_seq"]))
    with pytest.raises(ValueError):
        summary.v1_segment_records(h, l, c, p, {k: v for k, v in rm.items() if k != leaf})


def test_formatter_refuses_a_client_without_a_name(orc, libfmt):
    batch = _collab_batch()
    h, l, c, p, rm = v1_bulk.oracle_state(orc, batch)[0]
    segs, text, later = summary.v1_segment_records(h, l, c, p, rm)
    assert (segs["flags"] & native.V1_SOLO).any()
    with pytest.raises(native.EngineError) as e:
        native.v1_format(segs, text, p[: int(h["n_props"])], later, batch.keys, batch.values, [], int(h["min_seq"]),
                         int(h["cur_seq"]))
    assert e.value.code == native.FMT_E_USAGE

"""The host half of the bulk SharedMap summaries (csrc/map_sum_plan.h through
native.map_summary_format, no device): key ranks and value units, the JS object order, the blob split
and the formatter over the sparse path's entries (oracle.map_replay_sparse). Every summary must equal
oracle.map_summary(batch, doc) byte for byte, which tests/test_oracle_golden.py pins to map.spec.ts.
The same documents run on the device in tests/test_gpu_map_summary.py.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import map_summary_cases as cases
from fluidframework_amd import native
from fluidframework_amd.native import FMT_E_USAGE, MAP_SUMMARY_CONTENT
from fluidframework_amd.streams import MapStreamBuilder, is_array_index_key, js_key_order

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def directed(orc):
    batch, docs = cases.directed()
    counts, entries, _ = orc.map_replay_sparse(batch)
    got = native.map_summary_format(counts, entries, batch.keys, batch.values, threads=3)
    want = [orc.map_summary(batch, d) for d in range(batch.n_docs)]
    return batch, docs, got, want


def _members(blob):
    return list(json.loads(blob).keys())  # (json keeps the text's member order)


def _content(header):
    return list(json.loads(header)["content"].keys())


def test_every_directed_document_equals_the_oracle(directed):
    batch, docs, got, want = directed
    for name, d in docs.items():
        if isinstance(d, int):
            assert got[d] == want[d], name


def test_key_classification_and_order(directed):
    batch, docs, got, want = directed
    born = docs["keys_born"]
    assert all(is_array_index_key(k) for k in cases.INDEX_KEYS)
    assert not any(is_array_index_key(k) for k in cases.PLAIN_KEYS + [cases.ESCAPED_KEY])
    assert set(cases.INDEX_KEYS + cases.PLAIN_KEYS + [cases.ESCAPED_KEY]) <= set(born)
    header, blobs = got[docs["keys"]]
    assert blobs == []
    order = _content(header)
    assert order == js_key_order(born) and order != born
    assert order[:4] == ["0", "7", "10", "4294967294"]


def test_undefined_values_have_no_value_member(directed):
    batch, docs, got, want = directed
    header, blobs = got[docs["undefined"]]
    assert header == '{"blobs":[],"content":{"1":{"type":"Plain"},"3":{"type":"Plain","value":"three"},' \
                     '"b":{"type":"Plain"},"a":{"type":"Plain","value":null}}}'


def test_separate_blob_threshold_counts_utf16_units(directed):
    batch, docs, got, want = directed
    header, blobs = got[docs["units_8191_8192"]]
    assert [_members(x) for x in blobs] == [["k8192"]]
    assert _content(header) == ["2", "k8191"]
    header, blobs = got[docs["non_bmp"]]  # 8192 units in 16382 bytes; 8191 units in 16379
    assert [_members(x) for x in blobs] == [["pairs8192"]]
    assert len(blobs[0].encode("utf-8")) > 16384
    assert _content(header) == ["5", "pairs8191"]
    header, blobs = got[docs["lone_surrogate"]]
    assert blobs == [] and '"a\\ud800b"' in header and '"\\udfff"' in header


def test_flush_threshold_is_exclusive(directed):
    batch, docs, got, want = directed
    assert got[docs["exactly_16384"]][1] == []
    header, blobs = got[docs["just_16385"]]
    assert [_members(x) for x in blobs] == [["a"]]
    assert _content(header) == ["b"]


def test_overflowing_entry_contribution_is_dropped(directed):
    batch, docs, got, want = directed
    header, blobs = got[docs["dropped"]]
    assert [_members(x) for x in blobs] == [["4", "e1"], ["e2", "e3", "e4"]]
    assert _content(header) == ["e0"]


def test_separate_and_flushed_blobs_interleave(directed):
    batch, docs, got, want = directed
    header, blobs = got[docs["interleaved"]]
    assert [_members(x) for x in blobs] == [["S1"], ["a", "b"], ["S2"], ["c", "d", "e"]]
    assert json.loads(header)["blobs"] == ["blob0", "blob1", "blob2", "blob3"]
    assert _content(header) == ["f"]
    header, blobs = got[docs["many_flushes"]]
    assert len(blobs) >= 3 and [len(_members(x)) for x in blobs][:2] == [2, 3]


def test_empty_documents(directed):
    batch, docs, got, want = directed
    assert got[docs["empty"]] == ('{"blobs":[],"content":{}}', [])
    assert got[docs["emptied"]] == ('{"blobs":[],"content":{}}', [])


def test_arrays_of_the_host_hook(directed, orc):
    batch, docs, got, want = directed
    counts, entries, _ = orc.map_replay_sparse(batch)
    ordered, tags, n_blobs, status = native.map_summary_order(counts, entries, batch.keys, batch.values)
    assert (status == 0).all()
    at = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    d = docs["interleaved"]
    names = [batch.keys[int(k)] for k in ordered["key"][at[d] : at[d + 1]]]
    assert names == ["a", "S1", "b", "c", "S2", "d", "e", "f"]
    assert list(tags[at[d] : at[d + 1]]) == [1, 0, 1, 3, 2, 3, 3, MAP_SUMMARY_CONTENT] and n_blobs[d] == 4
    assert [n_blobs[d] for d in range(batch.n_docs)] == [len(w[1]) for w in want]
    # the same multiset of entries per document
    for d in range(batch.n_docs):
        assert sorted(map(tuple, ordered[at[d] : at[d + 1]])) == sorted(map(tuple, entries[at[d] : at[d + 1]]))


@pytest.mark.parametrize("which", ["key", "value"])
def test_an_id_outside_the_tables_fails_its_document_alone(orc, which):
    b = MapStreamBuilder()
    for d in range(3):
        b.begin_doc()
        b.add_message(d, 0, {"type": "set", "key": "1", "value": {"type": "Plain", "value": "one"}})
    # the last key and the last value of the dictionaries, in document 1 only
    b.add_message(1, 0, {"type": "set", "key": "zz-last", "value": {"type": "Plain", "value": "last value"}})
    batch = b.finish()
    counts, entries, _ = orc.map_replay_sparse(batch)
    keys = batch.keys[:-1] if which == "key" else batch.keys
    values = batch.values[:-1] if which == "value" else batch.values
    got = native.map_summary_format(counts, entries, keys, values)
    assert isinstance(got[1], native.EngineError) and got[1].code == FMT_E_USAGE
    assert got[0] == orc.map_summary(batch, 0) and got[2] == orc.map_summary(batch, 2)
    assert native.map_summary_order(counts, entries, keys, values)[3].tolist() == [0, FMT_E_USAGE, 0]
    full = native.map_summary_format(counts, entries, batch.keys, batch.values)
    assert full[1] == orc.map_summary(batch, 1)


def test_randomised_documents(orc):
    batch = cases.randomised()
    counts, entries, _ = orc.map_replay_sparse(batch)
    want = [orc.map_summary(batch, d) for d in range(batch.n_docs)]
    blobs = [len(w[1]) for w in want]
    assert 0 in blobs and 1 in blobs and max(blobs) >= 2, "the random family must cover 0, 1 and >= 2 blobs"
    assert sum(1 for n in blobs if n) > batch.n_docs // 2
    assert counts.min() == 0 and counts.max() > 64
    for threads in (1, 5):
        got = native.map_summary_format(counts, entries, batch.keys, batch.values, threads=threads)
        bad = [d for d in range(batch.n_docs) if got[d] != want[d]]
        assert not bad, bad[:5]


def test_tile_edge_documents_are_what_they_claim(orc):
    """The documents the GPU tests use for flush boundaries on tile edges, checked here on the host."""
    batch, docs = cases.tile_edges()
    counts, entries, _ = orc.map_replay_sparse(batch)
    got = native.map_summary_format(counts, entries, batch.keys, batch.values, threads=2)
    for name, d in docs.items():
        assert got[d] == orc.map_summary(batch, d), name
    sizes = lambda name: [len(_members(x)) for x in got[docs[name]][1]]  # noqa: E731
    assert sizes("b64_65")[:2] == [32, 33]  # entries 0..31, 32..64: the second boundary is 64 -> 65
    assert sizes("b63_64")[:2] == [31, 33]  # entries 0..30, 31..63: 63 -> 64
    assert set(sizes("two_per_tile")[1:]) == {31} and len(sizes("two_per_tile")) >= 20


def test_header_declares_what_the_library_exports():
    import ctypes
    import re

    text = open(os.path.join(REPO, "include", "fmt_map_summary.h")).read()
    fns = sorted(set(re.findall(r"^(?:int|void|const char\*)\s+(fmt_\w+)\(", text, re.M)))
    assert fns == sorted(native.EXPORTED_SYMBOLS_MAP_SUMMARY) and len(fns) == 3
    assert not set(fns) & set(native.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, f) for f in fns + ["fmt_internal_map_summary_format", "fmt_internal_map_summary_arrays"])


def test_host_half_under_sanitizers(tmp_path):
    """tests/san/map_sum_plan_san.cpp: a stand-alone program over map_sum_plan.h (directed documents,
    randomised ones against a straight restatement of the rule), built with ASan and UBSan."""
    exe = tmp_path / "map_sum_plan_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    "-o", str(exe), os.path.join(REPO, "tests", "san", "map_sum_plan_san.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout

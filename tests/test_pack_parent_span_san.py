"""tests/san/pack_span_san.cpp: the directed plain documents of pack_span_docs.py replayed through the
emulated engine in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
(-fno-sanitize-recover: the first report aborts). It runs as an ordinary child process on the CPU; nothing
of it is loaded into Python. The shifts of scourSpan's 64-bit masks and the two-row source indices of
deleteSpanLeaves are what it is there for: the documents put the span at leaf 0, across leaves 63 | 64 and
127 | 128, and fill it to its 45 leaves.
"""
import os
import subprocess

import numpy as np
import pytest

import pack_span_docs as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_MARKER = 0xFFFFFFFF


def _dump(path, batch, expect, first_tier):
    parts = [np.ascontiguousarray(batch.ops).view(np.uint8).reshape(-1),
             np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64),
             np.ascontiguousarray(batch.text, dtype="<u2"),
             np.ascontiguousarray(batch.doc_init, dtype=np.uint32).reshape(-1),
             np.ascontiguousarray(batch.props_off, dtype=np.uint32),
             np.ascontiguousarray(batch.props_kv, dtype=np.uint32),
             np.asarray(expect, dtype=np.uint32)]
    head = np.array([parts[0].nbytes, len(parts[1]), len(parts[2]), len(parts[3]), len(parts[4]), len(parts[5]),
                     int(getattr(batch, "marker_id_key", NO_MARKER)), first_tier], dtype=np.uint64)
    with open(path, "wb") as f:
        for a in [head] + parts:
            raw = a.tobytes()
            f.write(raw + b"\0" * (-len(raw) % 8))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pack_span_san") / "pack_span_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(REPO, "tests", "san", "pack_span_san.cpp")], check=True)
    return exe


@pytest.mark.parametrize("which", ["plain", "wide"])
def test_directed_documents_under_sanitizers(program, tmp_path, which):
    (bt, names), cases, first = ((pd.plain_batch(), pd.plain_cases(), 0) if which == "plain" else
                                 (pd.wide_batch(), pd.wide_cases(), 1))  # (the wide documents are past the micro tier)
    expect = [len(cases[n][0]) - cases[n][1] for n in names]
    dump = tmp_path / f"{which}.bin"
    _dump(dump, bt, expect, first)
    r = subprocess.run([str(program), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{bt.n_docs} documents, tiers {first}..3: ok" in r.stdout

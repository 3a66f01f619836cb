"""GPU, through the N-API addon (tests/js/text_driver.js): MergeTreeReplay.texts() (fetchTextAll) equals
Engine.mt_text_strings() on the conflict farm of test_gpu_text.py, handed to the addon as the packed
batch, and on a second batch the JS stream builder packs from messages: a marker document and a
document of 200 writers. getText(doc) agrees for every document. fetchRmClientsHi2 of the 200-writer
document, whose leaves hold remove stamps of short ids 130, 141, 195 and 200, equals
Engine.mt_rm_clients_hi2 and the oracle's remove stamps."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from fluidframework_amd import native
from fluidframework_amd.streams import MergeTreeStreamBuilder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "tests", "js", "text_driver.js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]
N_WRITERS = 200


def many_writer_messages():
    """200 writers insert one unit each at the front (short ids 1..200 in order; minSeq stays 0, so no id
    is recycled and no leaf merges), then six of them remove concurrently (refSeq 200): short id 70 one
    leaf; 130 and 195 the same leaf; 200 one leaf; 141 two leaves; 6 one leaf."""
    def m(client, seq, ref, contents):
        return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": 0,
                "type": "op", "contents": contents}

    msgs = [m(f"c{i}", i + 1, i, {"type": 0, "pos1": 0, "seg": chr(0x61 + i % 26)}) for i in range(N_WRITERS)]
    removes = [(70, 10, 11), (130, 20, 21), (195, 20, 21), (200, 30, 31), (141, 40, 42), (6, 50, 51)]
    for k, (short, a, b) in enumerate(removes):
        msgs.append(m(f"c{short - 1}", N_WRITERS + 1 + k, N_WRITERS, {"type": 1, "pos1": a, "pos2": b}))
    return msgs


def built_docs():
    from marker_docs import doc_messages

    init, msgs = doc_messages(0, 200, seed=4)
    return [{"initial": init, "msgs": msgs}, {"initial": "", "msgs": many_writer_messages()}], 1


def build(docs):
    b = MergeTreeStreamBuilder()
    for d in docs:
        doc = b.begin_doc(d["initial"], observer="A")
        for m in d["msgs"]:
            doc.add_message(m)
    return b.finish()


def _write(tmp_path, farm, docs, hi_doc):
    for name, arr in (("ops.bin", farm.ops), ("offs.bin", np.asarray(farm.doc_op_offsets, dtype=np.uint64)),
                      ("text.bin", np.asarray(farm.text, dtype="<u2")), ("doc_init.bin", np.asarray(farm.doc_init, dtype=np.uint32)),
                      ("props_off.bin", np.asarray(farm.props_off, dtype=np.uint32)),
                      ("props_kv.bin", np.asarray(farm.props_kv, dtype=np.uint32))):
        (tmp_path / name).write_bytes(np.ascontiguousarray(arr).tobytes())
    (tmp_path / "meta.json").write_text(json.dumps({"keys": farm.keys, "values": farm.values, "nDocs": farm.n_docs,
                                                    "docs": docs, "hiDoc": hi_doc}))


def test_js_texts_and_high_remove_clients(orc, tmp_path):
    from mt_compare import oracle_rm_clients_hi, oracle_rm_clients_hi2
    from test_gpu_text import farm_batch

    farm = farm_batch()
    docs, hi_doc = built_docs()
    _write(tmp_path, farm, docs, hi_doc)
    env = dict(os.environ, FMT_NAPI_BACKTRACE=os.environ.get("FMT_NAPI_BACKTRACE", "1"))
    r = subprocess.run([NODE, DRIVER, str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    built = build(docs)
    eng = native.Engine(0)
    try:
        want = {}
        for name, batch in (("packed", farm), ("built", built)):
            eng.mt_load(batch)
            eng.mt_run()
            want[name] = (eng.mt_text_strings(0), eng.mt_text_strings(0x20))
        hdr = eng.mt_headers()[hi_doc]
        hi, hi2 = eng.mt_rm_clients_hi(hi_doc, hdr), eng.mt_rm_clients_hi2(hi_doc, hdr)
    finally:
        eng.close()
    for name in ("packed", "built"):
        assert got[name]["texts"] == want[name][0] and got[name]["each"] == want[name][0], name
        assert got[name]["spaced"] == want[name][1], name
    assert len(want["packed"][0]) == 64 and want["built"][1][0] != want["built"][0][0]  # (the marker document)
    # the 200-writer document: ids 128..191 in word 0 and 192..253 in word 1 of each leaf's pair
    n = int(hdr["n_leaves"])
    assert got["nLeaves"] == n == N_WRITERS
    js_hi = np.array([int(x) for x in got["hi"]], dtype=np.uint64)
    js_hi2 = np.array([int(x) for x in got["hi2"]], dtype=np.uint64).reshape(n, 2)
    assert np.array_equal(js_hi2, hi2) and np.array_equal(js_hi2, oracle_rm_clients_hi2(built, hi_doc, n))
    assert np.array_equal(js_hi, hi) and np.array_equal(js_hi, oracle_rm_clients_hi(built, hi_doc, n))
    bit = lambda c, base: np.uint64(1) << np.uint64(c - base)  # noqa: E731
    both = np.nonzero((js_hi2[:, 0] != 0) & (js_hi2[:, 1] != 0))[0]
    assert len(both) == 1 and js_hi2[both[0]].tolist() == [int(bit(130, 128)), int(bit(195, 192))]
    assert sorted(js_hi2[:, 0][js_hi2[:, 0] != 0].tolist()) == sorted([int(bit(130, 128))] + [int(bit(141, 128))] * 2)
    assert js_hi2[:, 1][js_hi2[:, 1] != 0].tolist().count(int(bit(200, 192))) == 1
    assert (js_hi != 0).sum() == 1 and int(js_hi[js_hi != 0][0]) == int(bit(70, 64))
    assert not np.array_equal(js_hi2[:, 0], js_hi) and not np.array_equal(js_hi2[:, 1], js_hi2[:, 0])

"""The N-API addon over the sparse map path's HBM tier: replayMapSparse(batch, {tiered: true}).

From Node, map_edges.limits_keys() (2049 distinct keys in one document) replays with the same counts
and entries as the Python host's Engine.map_run_sparse_tiered; the default call still rejects with
FMT_E_CAPACITY. Skipped like tests/test_napi.py when Node is absent.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_edges as me

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "fluidframework_amd")
ADDON = os.path.join(PKG, "fmt_napi.node")

NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")


@pytest.fixture(scope="module")
def addon():
    if not os.path.exists(ADDON):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "napi")], check=True)
    return ADDON


@pytest.mark.gpu
def test_js_tiered_sparse_map_on_gpu(addon, tmp_path):
    from fluidframework_amd import native

    batch, facts = me.limits_keys()
    np.ascontiguousarray(batch.ops).tofile(tmp_path / "ops.bin")
    np.ascontiguousarray(batch.doc_op_offsets, dtype=np.uint64).tofile(tmp_path / "offs.bin")
    js = f"""const fmt=require({json.dumps(os.path.join(PKG, 'js', 'fmt.js'))});const fs=require('fs');
const rd=(n)=>{{const b=fs.readFileSync({json.dumps(str(tmp_path))}+'/'+n);return b.buffer.slice(b.byteOffset,b.byteOffset+b.byteLength);}};
(async()=>{{
const batch={{ops:new Uint8Array(rd('ops.bin')),docOpOffsets:new BigUint64Array(rd('offs.bin')),keyBound:{batch.key_bound},keys:[],values:[]}};
const e=new fmt.Engine(0);let plain='resolved';
try{{await e.replayMapSparse(batch);}}catch(x){{plain=x.code;}}
const r=await e.replayMapSparse(batch,{{tiered:true}});
const out={{plain,counts:Array.from(r.counts),entries:[0,1,2].map((d)=>r.rawEntries(d))}};
try{{await e.replayMapSparse(batch,{{}});out.again='resolved';}}catch(x){{out.again=x.code;}}
e.close();process.stdout.write(JSON.stringify(out));}})().catch((e)=>{{console.error(e);process.exit(1);}});"""
    script = tmp_path / "tiered.js"
    script.write_text(js)
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["plain"] == "FMT_E_CAPACITY" and out["again"] == "FMT_E_CAPACITY"
    eng = native.Engine(0)
    try:
        eng.map_load_sparse(batch)
        eng.map_run_sparse_tiered()
        counts, entries = eng.map_fetch_sparse()
    finally:
        eng.close()
    assert out["counts"] == counts.tolist() == [f["live"] for f in facts] and counts[1] > 0
    o = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    for d in range(3):
        assert out["entries"][d] == [list(x) for x in entries[o[d] : o[d + 1]].tolist()], f"document {d}"

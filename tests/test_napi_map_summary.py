"""Bulk SharedMap summaries through the N-API addon and the JavaScript driver (GPU): one small batch goes
through replayMapSparse(batch, {tiered: true}) and SparseMapReplay.summarizeAll(); every document's
{header, blobs} (summaryOf) equals what the Python engine returns for the same messages and what
js/summary.js's mapSummary builds from the same entries (SparseMapReplay.summarize)."""
import json
import os
import shutil
import subprocess

import pytest

import map_summary_cases as cases
from fluidframework_amd import native
from fluidframework_amd.streams import MapStreamBuilder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed")]


def _messages():
    """Per document its set / delete messages: index and plain keys, values that flush and that stand alone."""
    docs = []
    for d in range(12):
        msgs = []
        for i in range(5 + 9 * d):
            key = str((37 * i + d) % 101) if i % 2 else f"k{i}"
            units = [8, 700, 3000, 8191, 8192][(i + d) % 5]
            value = {"type": "Plain"} if i % 11 == 10 else {"type": "Plain", "value": cases.sval(units, "abc"[i % 3])}
            msgs.append({"type": "set", "key": key, "value": value})
            if i % 13 == 12:
                msgs.append({"type": "delete", "key": f"k{i - 4}"})
        docs.append(msgs)
    docs.append([])
    return docs


def test_js_summaries_equal_the_python_engine_and_the_js_host(tmp_path):
    docs = _messages()
    b = MapStreamBuilder()
    for msgs in docs:
        d = b.begin_doc()
        for m in msgs:
            b.add_message(d, 0, m)
    batch = b.finish()
    eng = native.Engine(0)
    try:
        eng.map_load_sparse(batch)
        eng.map_run_sparse_tiered()
        eng.map_summarize(batch.keys, batch.values)
        want = [eng.map_summary_doc(d) for d in range(batch.n_docs)]
    finally:
        eng.close()
    assert max(len(bl) for _, bl in want) >= 2
    (tmp_path / "docs.json").write_text(json.dumps(docs))
    js = f"""const fmt=require({json.dumps(os.path.join(REPO, 'fluidframework_amd', 'js', 'fmt.js'))});
const docs=JSON.parse(require('fs').readFileSync({json.dumps(str(tmp_path / 'docs.json'))}));
(async()=>{{
const mb=new fmt.MapStreamBuilder();
for(const msgs of docs){{const d=mb.beginDoc();let s=0;for(const m of msgs) mb.addMessage(d,++s,m);}}
const e=new fmt.Engine(0);const r=await e.replayMapSparse(mb.finish(),{{tiered:true}});
const t=await r.summarizeAll({{threads:4}});const out={{t,docs:[],host:[]}};
for(let d=0;d<docs.length;d++){{const a=r.summaryOf(d),h=r.summarize(d);out.docs.push([a.header,a.blobs]);
 out.host.push(a.header===h.header&&JSON.stringify(a.blobs)===JSON.stringify(h.blobs));}}
e.close();process.stdout.write(JSON.stringify(out));}})().catch((e)=>{{console.error(e);process.exit(1);}});"""
    script = tmp_path / "map_summary.js"
    script.write_text(js)
    r = subprocess.run([NODE, str(script)], capture_output=True, text=True, timeout=120, cwd=REPO,
                       env=dict(os.environ, FMT_NAPI_BACKTRACE="1"))
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert [(h, bl) for h, bl in out["docs"]] == [(h, bl) for h, bl in want]
    assert all(out["host"])
    assert out["t"]["hostOrderedDocs"] == 0 and out["t"]["threads"] == 4 and out["t"]["bytes"] > 0

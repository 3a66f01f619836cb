"use strict";
// Drives MergeTreeReplay.texts() (fluidframework_amd/js/fmt.js, the addon's fetchTextAll) and the addon's
// fetchRmClientsHi2 on the GPU.
//
//   node text_driver.js <dir>   <dir>/meta.json: {keys, values, nDocs, docs, hiDoc} and the packed batch
//                               of nDocs documents as ops.bin, offs.bin, text.bin, doc_init.bin,
//                               props_off.bin, props_kv.bin (the layouts fixture_driver.js pack writes);
//                               docs: [{initial, msgs}], packed here by the JS stream builder into a
//                               second batch, whose document hiDoc has writers with short ids >= 128.
// Prints one JSON line: {packed: {texts, spaced, each}, built: {texts, spaced, each}, hi, hi2, nLeaves}:
// texts(), texts(" ") and getText(doc) of every document of either batch, and the words of
// fetchRmClientsHi / fetchRmClientsHi2 of document hiDoc of the second (decimal strings).
const fs = require("fs");
const path = require("path");
const fmt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js", "fmt.js"));
const addon = require(path.join(__dirname, "..", "..", "fluidframework_amd", "fmt_napi.node"));

function view(dir, name, Type) {
	const b = fs.readFileSync(path.join(dir, name));
	const ab = b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength);
	return new Type(ab);
}

function read(r, n) {
	const each = [];
	for (let d = 0; d < n; d++) each.push(r.getText(d));
	return { texts: r.texts(), spaced: r.texts(" "), each };
}

async function main() {
	const dir = process.argv[2];
	const meta = JSON.parse(fs.readFileSync(path.join(dir, "meta.json"), "utf8"));
	const packed = {
		ops: view(dir, "ops.bin", Uint8Array), docOpOffsets: view(dir, "offs.bin", Uint8Array),
		text: view(dir, "text.bin", Uint16Array), docInit: view(dir, "doc_init.bin", Uint32Array),
		propsOff: view(dir, "props_off.bin", Uint32Array), propsKv: view(dir, "props_kv.bin", Uint32Array),
		keys: meta.keys, values: meta.values, nDocs: meta.nDocs,
	};
	const b = new fmt.MergeTreeStreamBuilder();
	for (const d of meta.docs) {
		const doc = b.beginDoc(d.initial, "A");
		for (const m of d.msgs) doc.addMessage(m);
	}
	const built = b.finish();
	const eng = new fmt.Engine(0);
	try {
		const out = {};
		out.packed = read(await eng.replayMergeTree(packed), meta.nDocs);
		const r = await eng.replayMergeTree(built);
		out.built = read(r, meta.docs.length);
		out.nLeaves = r.header(meta.hiDoc).nLeaves;
		out.hi = Array.from(addon.fetchRmClientsHi(eng.ctx, meta.hiDoc, out.nLeaves), (x) => x.toString());
		out.hi2 = Array.from(addon.fetchRmClientsHi2(eng.ctx, meta.hiDoc, out.nLeaves), (x) => x.toString());
		console.log(JSON.stringify(out));
	} finally {
		eng.close();
	}
}

main().catch((e) => { console.error(e); process.exit(1); });

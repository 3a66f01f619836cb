"use strict";
// Drives MergeTreeReplay.formatted() (fluidframework_amd/js/fmt.js, the addon's fetchPropRunsAll) on the GPU.
//
//   node runs_driver.js <dir>   <dir>/meta.json: {keys, values, nDocs} and the packed batch of nDocs
//                               documents as ops.bin, offs.bin, text.bin, doc_init.bin, props_off.bin,
//                               props_kv.bin (the layouts fixture_driver.js pack writes).
// Prints one JSON line: {plain, spaced, refusedWhileBusy}: formatted() and formatted(" ") of the batch, and
// whether fetchPropRunsAll threw while a replay was running on the context.
const fs = require("fs");
const path = require("path");
const fmt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js", "fmt.js"));
const addon = require(path.join(__dirname, "..", "..", "fluidframework_amd", "fmt_napi.node"));

function view(dir, name, Type) {
	const b = fs.readFileSync(path.join(dir, name));
	const ab = b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength);
	return new Type(ab);
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
	const eng = new fmt.Engine(0);
	try {
		const running = eng.replayMergeTree(packed);
		let refusedWhileBusy = false;
		try {
			addon.fetchPropRunsAll(eng.ctx, meta.nDocs);
		} catch (e) {
			refusedWhileBusy = true;
		}
		const r = await running;
		console.log(JSON.stringify({ plain: r.formatted(), spaced: r.formatted(" "), refusedWhileBusy }));
	} finally {
		eng.close();
	}
}

main().catch((e) => { console.error(e); process.exit(1); });

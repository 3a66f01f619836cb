"use strict";
// Drives MergeTreeReplay.textRanges() and the addon's fetchTextRanges (fluidframework_amd/js/fmt.js) on the GPU.
//
//   node range_driver.js <dir>   <dir>/meta.json: {keys, values, nDocs} and the packed batch of nDocs documents
//                                as ops.bin, offs.bin, text.bin, doc_init.bin, props_off.bin, props_kv.bin (the
//                                layouts fixture_driver.js pack writes), and the queries: ranges.bin (16-byte
//                                fmt_mt_range_query records packed per document) and qoffs.bin (nDocs + 1 uint64).
// Prints one JSON line: {plain, placeholder, stringsMatch, refusedWhileBusy, enumerable}: the addon's hits and
// units in base64 without a placeholder and with U+FFFC; whether textRanges() over the same queries, last
// first, gives each range's text and span in the queries' order (null for a failed one); whether
// fetchTextRanges threw while a replay was running on the context; whether the addon lists fetchTextRanges.
const fs = require("fs");
const path = require("path");
const fmt = require(path.join(__dirname, "..", "..", "fluidframework_amd", "js", "fmt.js"));
const addon = require(path.join(__dirname, "..", "..", "fluidframework_amd", "fmt_napi.node"));

function view(dir, name, Type) {
	const b = fs.readFileSync(path.join(dir, name));
	const ab = b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength);
	return new Type(ab);
}

function b64(r) {
	return { hits: Buffer.from(r.hits).toString("base64"),
		units: Buffer.from(r.units.buffer, r.units.byteOffset, r.units.byteLength).toString("base64") };
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
	const queries = view(dir, "ranges.bin", Uint8Array).buffer, qoffs = view(dir, "qoffs.bin", Uint8Array).buffer;
	const eng = new fmt.Engine(0);
	try {
		const running = eng.replayMergeTree(packed);
		let refusedWhileBusy = false;
		try {
			addon.fetchTextRanges(eng.ctx, meta.nDocs, 0, qoffs, queries);
		} catch (e) {
			refusedWhileBusy = true;
		}
		const r = await running;
		const plain = addon.fetchTextRanges(eng.ctx, meta.nDocs, 0, qoffs, queries);
		const placeholder = addon.fetchTextRanges(eng.ctx, meta.nDocs, 0xfffc, qoffs, queries);
		// the same queries as objects, last first, through textRanges()
		const qv = new DataView(queries), ov = new DataView(qoffs), hv = new DataView(plain.hits);
		const list = [];
		for (let d = 0; d < meta.nDocs; d++) {
			for (let k = ov.getUint32(8 * d, true); k < ov.getUint32(8 * d + 8, true); k++) {
				const end = qv.getUint32(16 * k + 4, true), refSeq = qv.getInt32(16 * k + 8, true);
				list.push({ doc: d, start: qv.getUint32(16 * k, true), end: end === fmt.constants.RANGE_TO_END ? undefined : end,
					refSeq: refSeq === fmt.constants.POS_VIEW_LOCAL ? undefined : refSeq, client: qv.getInt32(16 * k + 12, true), k });
			}
		}
		list.reverse();
		const objs = r.textRanges(list);
		let stringsMatch = objs.length === list.length;
		objs.forEach((h, i) => {
			const o = 24 * list[i].k, status = hv.getInt32(o + 16, true);
			const at = Number(hv.getBigUint64(o, true)), units = hv.getUint32(o + 8, true);
			const want = status === 0 ? Array.from(plain.units.subarray(at, at + units), (u) => String.fromCharCode(u)).join("") : null;
			stringsMatch = stringsMatch && h.status === status && h.span === hv.getUint32(o + 12, true) && h.text === want;
		});
		console.log(JSON.stringify({ plain: b64(plain), placeholder: b64(placeholder), stringsMatch, refusedWhileBusy,
			enumerable: Object.keys(addon).includes("fetchTextRanges") }));
	} finally {
		eng.close();
	}
}

main().catch((e) => { console.error(e); process.exit(1); });

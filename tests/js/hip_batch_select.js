// GPU test helper: JSMpeg.HIPBatch.select -- a few frames of one stream through decode(), decodeAsync() and enqueue(), and
// through a HIPBatchRouter; prints the md5 of the selected pictures' planes (Y | Cr | Cb), the picture table's `decoded` flags and
// what forEachFrame hands out, for the Python side to hold against the golden fixture.
//   node hip_batch_select.js <stream.m1v> <width> <height> <pictures> <frames, comma separated>
'use strict';
const fs = require('fs');
const crypto = require('crypto');
const { HIPBatch, HIPBatchRouter } = require('../../jsmpeg_amd/js/batch-hip.js').install();

const [file, w, h, pictures, list] = process.argv.slice(2);
const es = new Uint8Array(fs.readFileSync(file));
const frames = list.split(',').map((x) => parseInt(x, 10));
const md5 = (planes) => { const m = crypto.createHash('md5'); m.update(planes.y); m.update(planes.cr); m.update(planes.cb); return m.digest('hex'); };

(async () => {
  const out = { ok: true, modes: {} };
  const b = new HIPBatch({ width: parseInt(w, 10), height: parseInt(h, 10), maxStreams: 2, maxPictures: 2 * parseInt(pictures, 10) + 8, maxBytes: 2 * es.length + 65536, device: 0 });
  b.upload([es, es]);
  out.whole = b.decode();
  const requests = frames.map((f, k) => [k % 2, f]).concat([[1, 100000]]);
  let malformed = 'accepted';
  try { b.select([[0]]); } catch (e) { malformed = e instanceof TypeError ? 'TypeError' : String(e); }
  out.malformed = malformed;
  let outOfRange = 'accepted';
  try { b.select([[2, 0]]); } catch (e) { outOfRange = /stream 2 of 2/.test(e.message) ? 'refused' : e.message; }
  out.outOfRange = outOfRange;
  b.select(requests);
  for (const mode of ['decode', 'decodeAsync', 'enqueue']) {
    const n = mode === 'decode' ? b.decode() : await b[mode]();
    const sel = b.selected();
    const decoded = [];
    for (let p = 0; p < n; p++) if (b.pictureInfo(p).decoded) decoded.push(p);
    const handed = [];
    b.forEachFrame((f) => handed.push({ stream: f.stream, index: f.index, picture: f.picture, md5: md5(f) }));
    out.modes[mode] = { pictures: n, selected: sel, md5: sel.map((p) => (p === null ? null : md5(b.readPlanes(p)))), decoded, info: b.selectInfo(), handed };
  }
  let inFlight = 'none';
  const p = b.enqueue();
  try { b.select(null); } catch (e) { inFlight = /in flight/.test(e.message) ? 'refused' : e.message; }
  await p;
  out.inFlight = inFlight;
  b.select(null);
  out.cleared = { pictures: b.decode(), selected: b.selected() };
  let d = 0;
  for (let q = 0; q < out.cleared.pictures; q++) d += b.pictureInfo(q).decoded;
  out.cleared.decoded = d;
  b.destroy();
  // the router passes the requests through to the batch of the stream's size
  const router = new HIPBatchRouter({ maxPicturesPerStream: parseInt(pictures, 10) + 8, maxBytesPerStream: es.length + 65536, device: 0 });
  const got = [];
  router.select([[1, frames[0]], { stream: 0, frame: frames[frames.length - 1] }]);
  out.routerFrames = router.decode([es, es], { onFrame: (f) => got.push({ stream: f.stream, index: f.index, md5: md5(f) }) });
  out.router = { handed: got, selected: router.selected(), info: router.selectInfo() };
  router.destroy();
  process.stdout.write(JSON.stringify(out) + '\n');
})().catch((e) => { process.stdout.write(JSON.stringify({ ok: false, error: String(e && e.stack || e) }) + '\n'); process.exitCode = 1; });

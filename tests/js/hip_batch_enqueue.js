// GPU test helper: two JSMpeg.HIPBatch objects, a chain of enqueue() promises each, from ONE event loop -- while a long
// crypto.pbkdf2 holds the only thread of libuv's pool (run with UV_THREADPOOL_SIZE=1): the decodes must all be through before
// it, which shows that they took no pool thread.  Every picture of every pass against the oracle's hashes.
//   node hip_batch_enqueue.js <hashes.json> <w> <h> <dir A> <nA> <dir B> <nB> <passes>
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const { HIPBatch } = require('../../jsmpeg_amd/js/batch-hip.js').install();

const [hashFile, w, h, dirA, nA, dirB, nB, passes] = process.argv.slice(2);
const want = JSON.parse(fs.readFileSync(hashFile, 'utf8'));
const load = (dir, n) => Array.from({ length: parseInt(n, 10) }, (_, i) => new Uint8Array(fs.readFileSync(path.join(dir, 's' + i + '.m1v'))));
const order = [];
let pbkdf2Done = false;
crypto.pbkdf2('secret', 'salt', 3000000, 64, 'sha512', () => { pbkdf2Done = true; order.push('pbkdf2'); });

function make(streams) {
  const total = streams.reduce((a, b) => a + b.length, 0);
  const b = new HIPBatch({ width: parseInt(w, 10), height: parseInt(h, 10), maxStreams: streams.length, maxPictures: 4096, maxBytes: total + 65536, device: 0 });
  b.upload(streams);
  return b;
}
function gate(name, b, key) {
  const got = b.frameHashes(), exp = [];
  for (const s of want[key]) exp.push(...s);
  if (got.length !== exp.length || got.some((x, i) => x !== exp[i])) throw new Error(name + ': a picture differs from the oracle');
}
async function chain(name, b, key, k) {
  const rc = [];
  for (let i = 0; i < k; i++) {
    const n = await b.enqueue();
    rc.push(n);
    gate(name, b, key);
  }
  order.push(name);
  return rc;
}
(async () => {
  const a = make(load(dirA, nA)), b = make(load(dirB, nB));
  const k = parseInt(passes, 10);
  const t0 = Date.now();
  const [ra, rb] = await Promise.all([chain('A', a, 'A', k), chain('B', b, 'B', k)]);
  const ms = Date.now() - t0;
  let second = 'none';
  const p = a.enqueue();
  try { a.upload([new Uint8Array(16)]); } catch (e) { second = /in flight/.test(e.message) ? 'refused' : e.message; }
  await p;
  a.destroy(); b.destroy();
  process.stdout.write(JSON.stringify({ ok: true, picturesA: ra, picturesB: rb, ms, pbkdf2_before: pbkdf2Done, order, second }) + '\n');
})().catch((e) => { process.stdout.write(JSON.stringify({ ok: false, error: String(e && e.stack || e) }) + '\n'); process.exitCode = 1; });

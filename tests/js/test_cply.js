// Node side of the compressed .ply: the addon's cplyInfo / loadCply / exportCply and the component shim's loader and exportCply({of,
// shDegree, morton}), on a file tests/test_cply_node.py wrote, against what the ctypes binding returned for the same cloud.
//   node test_cply.js cpu inria.ply compressed.ply          -- the sniff only (no GPU)
//   node test_cply.js gpu scene.ply pose.json expect.json
// expect.json: {splats, shDegree, hide: [ids], all, visible, plain: hex of the whole file each}
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }
function throwsRange(fn) { try { fn(); } catch (e) { return e instanceof RangeError; } return false; }
const bytesOf = (p) => { const b = fs.readFileSync(p); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length); };
const hex = (ab) => Buffer.from(ab).toString('hex');

const [mode, a, b, c] = process.argv.slice(2);
for (const f of ['cplyInfo', 'loadCply', 'exportCply']) ok(typeof native[f] === 'function', 'addon exports ' + f);
ok(typeof GaussianSplatting.prototype.exportCply === 'function', 'the shim has exportCply');
ok(throwsRange(() => GaussianSplatting.prototype.exportCply.call({ handle: null }, { of: 'some' })), 'exportCply: an unknown filter name is refused');
if (mode === 'cpu') {
  ok(native.cplyInfo(bytesOf(a)) === null, 'an INRIA .ply is not a compressed file');
  const info = native.cplyInfo(bytesOf(b));
  ok(info && info.splats === 300 && info.chunks === 2 && info.shDegree === 1 && info.chunkFloats === 18, 'cplyInfo: ' + JSON.stringify(info));
  ok(native.cplyInfo(new ArrayBuffer(0)) === null, 'no bytes: no header');
  console.log('cply cpu checks ok');
  process.exit(0);
}
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(b, 'utf8'));
const expect = JSON.parse(fs.readFileSync(c, 'utf8'));
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };

(async () => {
  const comp = new GaussianSplatting({ src: a, shDegree: expect.shDegree }).init(null);
  const count = await comp.loadData(camera, entity, null, a);        // a .ply whose header cplyInfo accepts: loadCply
  ok(count === expect.splats && native.count(comp.handle) === count, 'loaded ' + count + ' of ' + expect.splats);
  ok(hex(comp.exportCply()) === expect.all, 'exportCply(): the host writer\'s bytes');
  ok(hex(comp.exportCply({ morton: false, shDegree: 0 })) === expect.plain, 'exportCply({morton: false, shDegree: 0})');
  comp.hideSplats(expect.hide);
  ok(hex(comp.exportCply({ of: 'visible', shDegree: 1 })) === expect.visible, 'exportCply({of: visible})');
  ok(hex(native.exportCply(comp.handle, 1, 0, 1, true)) === expect.visible, 'the addon with (1, 0)');
  let threw = false;
  try { comp.exportCply({ shDegree: 4 }); } catch (e) { threw = true; }
  ok(threw, 'a degree outside 0 .. 3 is refused');
  comp.remove();
  console.log('cply gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

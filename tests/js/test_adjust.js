// Node side of the in-place changes: the addon's adjustColour / replaceSplat / replaceSh and the component shim's adjustColour({of, matrix,
// offset, alphaScale, alphaOffset}) / replaceSplat / replaceSh, on a scene tests/test_adjust_node.py wrote, against what the ctypes binding
// returned for the same steps.
//   node test_adjust.js cpu                                 -- exports only (no GPU)
//   node test_adjust.js gpu scene.splat pose.json expect.json
// expect.json: {select: [ids], matrix, offset, alphaScale, alphaOffset, hit, first, other: hex rows, shFirst, sh: [floats], sh2: [floats],
// steps: {adjusted, replaced, shReplaced: sha256 of what export returns after each step}}.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }
function throwsRange(fn) { try { fn(); } catch (e) { return e instanceof RangeError; } return false; }
function throws(fn) { try { fn(); } catch (e) { return true; } return false; }
const sha = (buf) => crypto.createHash('sha256').update(Buffer.from(buf)).digest('hex');

const [mode, scenePath, posePath, expectPath] = process.argv.slice(2);
for (const f of ['adjustColour', 'replaceSplat', 'replaceSh']) {
  ok(typeof native[f] === 'function', 'addon exports ' + f);
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
}
ok(throwsRange(() => GaussianSplatting.prototype.adjustColour.call({ handle: null }, { of: 'some' })), 'adjustColour: an unknown filter name is refused');
if (mode === 'cpu') { console.log('adjust cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const want = JSON.parse(fs.readFileSync(expectPath, 'utf8'));
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const count = await comp.loadData(camera, entity, null, scenePath);
  ok(count > 0 && native.count(comp.handle) === count, 'loaded ' + count);
  ok(native.pushSh(comp.handle, Float32Array.from(want.sh), 1) === want.sh.length / 12, 'SH rows pushed');
  native.setStateIds(comp.handle, Uint32Array.from(want.select), 2, 0);      // selected
  // the identity through the shim's defaults changes nothing
  const before = sha(comp.exportSplat());
  ok(comp.adjustColour() === count && sha(comp.exportSplat()) === before, 'the default adjustment is the identity');
  const hit = comp.adjustColour({ of: 'selected', matrix: want.matrix, offset: want.offset, alphaScale: want.alphaScale, alphaOffset: want.alphaOffset });
  ok(hit === want.hit, 'adjusted ' + hit + ' splats, expected ' + want.hit);
  ok(sha(comp.exportSplat()) === want.steps.adjusted.rows && sha(comp.exportPly({ shDegree: 1 })) === want.steps.adjusted.ply, 'rows and SH rows after adjustColour');
  const other = Buffer.from(want.other, 'hex');
  ok(comp.replaceSplat(want.first, new Uint8Array(other)) === other.length / 32, 'replaceSplat returns the rows written');
  ok(sha(comp.exportSplat()) === want.steps.replaced.rows, 'rows after replaceSplat');
  ok(native.count(comp.handle) === count, 'the count stays');
  ok(comp.replaceSh(want.shFirst, Float32Array.from(want.sh2), 1) === want.sh2.length / 12, 'replaceSh returns the rows written');
  ok(sha(comp.exportPly({ shDegree: 1 })) === want.steps.shReplaced.ply, 'SH rows after replaceSh');
  // the addon's own argument checks and the library's refusals
  ok(throws(() => native.replaceSplat(comp.handle, count, new Uint8Array(32))), 'a range beyond the count is refused');
  ok(throws(() => native.replaceSplat(comp.handle, 0, new Uint8Array(33))), 'rows that are no multiple of 32 bytes are refused');
  ok(throws(() => native.replaceSh(comp.handle, 0, new Float32Array(12), 2)), 'another degree than the store is refused');
  ok(throws(() => native.adjustColour(comp.handle, [1, 0, 0, 0, NaN, 0, 0, 0, 1], [0, 0, 0], 1, 0, 0, 0)), 'a NaN parameter is refused');
  ok(sha(comp.exportPly({ shDegree: 1 })) === want.steps.shReplaced.ply, 'refused calls change nothing');
  comp.remove();
  console.log('adjust gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

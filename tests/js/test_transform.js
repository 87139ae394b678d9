// Node side of gs_transform: the addon's transform and the component shim's transform({of, rotation, scale, translation}), on a scene
// tests/test_transform_node.py wrote, against what the ctypes binding returned for the same steps.
//   node test_transform.js cpu                                 -- exports only (no GPU)
//   node test_transform.js gpu scene.splat pose.json expect.json
// expect.json: {select: [ids], rotation, scale, translation, hit, sh: [floats], steps: {moved, shifted: sha256 of what export returns after each step}}.
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
ok(typeof native.transform === 'function', 'addon exports transform');
ok(typeof GaussianSplatting.prototype.transform === 'function', 'the shim has transform');
ok(throwsRange(() => GaussianSplatting.prototype.transform.call({ handle: null }, { of: 'some' })), 'transform: an unknown filter name is refused');
if (mode === 'cpu') { console.log('transform cpu checks ok'); process.exit(0); }
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
  ok(comp.transform() === count && sha(comp.exportSplat()) === before, 'the default transform is the identity');
  const hit = comp.transform({ of: 'selected', rotation: want.rotation, scale: want.scale, translation: want.translation });
  ok(hit === want.hit, 'moved ' + hit + ' splats, expected ' + want.hit);
  ok(sha(comp.exportSplat()) === want.steps.moved.rows && sha(comp.exportPly({ shDegree: 1 })) === want.steps.moved.ply, 'rows and SH rows after transform');
  ok(native.transform(comp.handle, [1, 0, 0, 0], 1, want.translation, 0, 0) === count, 'the addon call returns the splats moved');
  ok(sha(comp.exportSplat()) === want.steps.shifted.rows, 'rows after the translation of all');
  ok(native.count(comp.handle) === count, 'the count stays');
  // the addon's own argument checks and the library's refusals
  ok(throws(() => native.transform(comp.handle, [1, 0, 0], 1, [0, 0, 0], 0, 0)), 'a quaternion of three numbers is refused');
  ok(throws(() => native.transform(comp.handle, [0, 0, 0, 0], 1, [0, 0, 0], 0, 0)), 'a quaternion of norm 0 is refused');
  ok(throws(() => native.transform(comp.handle, [1, 0, 0, 0], 0, [0, 0, 0], 0, 0)), 'a scale of 0 is refused');
  ok(throws(() => native.transform(comp.handle, [1, 0, 0, 0], 1, [0, NaN, 0], 0, 0)), 'a NaN parameter is refused');
  ok(sha(comp.exportSplat()) === want.steps.shifted.rows, 'refused calls change nothing');
  comp.remove();
  console.log('transform gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

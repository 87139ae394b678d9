// Node side of the export: the addon's exportSplat / exportPly and the component shim's exportSplat({of}) / exportPly({of, shDegree}), on a
// scene tests/test_export_node.py wrote, against what the ctypes binding returned for the same cloud.
//   node test_export.js cpu                                 -- exports only (no GPU)
//   node test_export.js gpu scene.splat pose.json expect.json
// expect.json: {hide: [ids], all: {...}, visible: {...}} with, per filter, {rows, first, last: hex of a 32-byte row, plyBytes, plyFirst,
// plyLast: hex of a 68-byte vertex}.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }
function throwsRange(fn) { try { fn(); } catch (e) { return e instanceof RangeError; } return false; }
const hex = (buf, at, n) => Buffer.from(buf, at, n).toString('hex');

const [mode, scenePath, posePath, expectPath] = process.argv.slice(2);
for (const f of ['exportSplat', 'exportPly']) {
  ok(typeof native[f] === 'function', 'addon exports ' + f);
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
  ok(throwsRange(() => GaussianSplatting.prototype[f].call({ handle: null }, { of: 'some' })), f + ': an unknown filter name is refused');
}
if (mode === 'cpu') { console.log('export cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const expect = JSON.parse(fs.readFileSync(expectPath, 'utf8'));
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };

function check(name, rows, ply, want) {
  ok(rows instanceof ArrayBuffer && rows.byteLength === 32 * want.rows, name + ': ' + rows.byteLength + ' bytes of rows, expected ' + 32 * want.rows);
  ok(hex(rows, 0, 32) === want.first && hex(rows, rows.byteLength - 32, 32) === want.last, name + ': first and last row');
  ok(ply instanceof ArrayBuffer && ply.byteLength === want.plyBytes, name + ': ' + ply.byteLength + ' bytes of .ply, expected ' + want.plyBytes);
  const head = Buffer.from(ply, 0, 64).toString('latin1');
  ok(head.startsWith('ply\nformat binary_little_endian 1.0\nelement vertex ' + want.rows + '\n'), name + ': the header names ' + want.rows + ' vertices');
  const at = ply.byteLength - 68 * want.rows;
  ok(hex(ply, at, 68) === want.plyFirst && hex(ply, ply.byteLength - 68, 68) === want.plyLast, name + ': first and last vertex');
}

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const count = await comp.loadData(camera, entity, null, scenePath);
  ok(count > 0 && native.count(comp.handle) === count, 'loaded ' + count);
  check('all', comp.exportSplat(), comp.exportPly({ shDegree: 0 }), expect.all);
  ok(expect.all.rows === count, 'every splat is exported');
  comp.hideSplats(expect.hide);
  // the shim's 'visible' is the filter (HIDDEN, 0)
  check('visible', comp.exportSplat({ of: 'visible' }), comp.exportPly({ of: 'visible' }), expect.visible);
  check('(1, 0)', native.exportSplat(comp.handle, 1, 0), native.exportPly(comp.handle, 1, 0, 3), expect.visible);
  ok(expect.visible.rows === count - expect.hide.length, 'the hidden splats are left out');
  ok(comp.exportSplat({ of: 'selected' }).byteLength === 0, 'nothing is selected');
  check('all again', comp.exportSplat({ of: 'all' }), comp.exportPly({ of: 'all' }), expect.all);
  let threw = false;
  try { comp.exportPly({ shDegree: 4 }); } catch (e) { threw = true; }
  ok(threw, 'a degree outside 0 .. 3 is refused');
  comp.remove();
  console.log('export gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

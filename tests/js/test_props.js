// Node side of the per-splat properties: the addon's propRange / histogram / selectRange and the component shim's histogram / selectRange,
// on a scene tests/test_props_node.py wrote.
//   node test_props.js cpu                                  -- exports only (no GPU)
//   node test_props.js gpu scene.splat pose.json
// pose.json: {width, height, proj[16], camera[16], object[16]} -- three.js world matrices, column-major.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }
function throwsRange(fn) { try { fn(); } catch (e) { return e instanceof RangeError; } return false; }
const sum = (a) => a.reduce((s, v) => s + v, 0);

const [mode, scenePath, posePath] = process.argv.slice(2);
for (const f of ['propRange', 'histogram', 'selectRange'])
  ok(typeof native[f] === 'function', 'addon exports ' + f);
for (const f of ['histogram', 'selectRange'])
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
ok(throwsRange(() => GaussianSplatting.prototype.histogram.call({ handle: null }, 'radius')), 'an unknown property name is refused');
ok(throwsRange(() => GaussianSplatting.prototype.histogram.call({ handle: null }, 'alpha', { of: 'some' })), 'an unknown filter name is refused');
ok(throwsRange(() => GaussianSplatting.prototype.selectRange.call({ handle: null }, 'Alpha', 0, 1)), 'property names are lower case');
if (mode === 'cpu') { console.log('props cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height, vp = { width: W, height: H };
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };
const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
function draw(comp) { comp.tick(); return Uint8Array.from(comp.render(camera, vp)); }

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const count = await comp.loadData(camera, entity, null, scenePath);
  ok(count > 0 && native.count(comp.handle) === count, 'loaded ' + count);
  const rowsBytes = fs.readFileSync(scenePath);
  const alpha = new Array(256).fill(0);
  for (let i = 0; i < count; i++) alpha[rowsBytes[32 * i + 27]]++;

  // the alpha histogram over the bytes' own range: one bin per byte value, and it sums to count
  const f0 = draw(comp);
  const h = comp.histogram('alpha', { bins: 256, lo: 0, hi: 256 });
  ok(h.counts instanceof Uint32Array && h.counts.length === 256 && sum(h.counts) === count, 'histogram(alpha) sums to count');
  ok(same(Array.from(h.counts), alpha) && h.passing === count && h.below === 0 && h.above === 0 && h.nan === 0, 'one bin per alpha byte');
  ok(same(draw(comp), f0) && f0.some((v) => v !== 0), 'a histogram changes no frame');

  // bounds left out: propRange first
  const auto = comp.histogram('alpha', { bins: 256 });
  const r = native.propRange(comp.handle, 6, 0, 0);
  ok(r.count === count && auto.lo === r.min && auto.hi === r.max && r.min >= 0 && r.max <= 255 && r.min < r.max, 'propRange(alpha): ' + r.min + ' .. ' + r.max);
  ok(sum(auto.counts) === count && auto.below === 0 && auto.above === 0, 'histogram(alpha, {bins: 256}) sums to count');
  const x = comp.histogram('x', { bins: 64 });
  ok(sum(x.counts) === count && x.lo < x.hi && x.counts[0] >= 1 && x.counts[63] >= 1, 'histogram(x) spans its own range');
  const s = comp.histogram('size2', { bins: 100, lo: 0 });
  ok(sum(s.counts) === count && s.lo === 0 && s.hi > 0, 'size2 is positive');

  // selectRange: select, then hide, then delete -- count falls by the first 17 bins
  const low = sum(h.counts.subarray(0, 17));
  ok(low > 0 && low < count, low + ' splats have alpha <= 16');
  ok(comp.selectRange('alpha', 0, 16) === low, 'selectRange selects ' + low);
  ok(comp.histogram('alpha', { bins: 256, lo: 0, hi: 256, of: 'selected' }).passing === low, "of: 'selected'");
  ok(comp.selectRange('alpha', 0, 16, { invert: true }) === count - low, 'invert reaches the others');
  ok(comp.histogram('alpha', { of: 'selected', lo: 0, hi: 256 }).passing === count, 'everything is selected now');
  ok(comp.selectRange('alpha', 0, 16, { hide: true }) === low, 'hide ' + low);
  const vis = comp.histogram('alpha', { bins: 256, lo: 0, hi: 256, of: 'visible' });
  ok(vis.passing === count - low && sum(vis.counts.subarray(0, 17)) === 0 && same(Array.from(vis.counts.subarray(17)), alpha.slice(17)), "of: 'visible'");
  ok(comp.histogram('alpha', { of: 'selected', lo: 0, hi: 256 }).passing === count - low, 'the visible selection');
  draw(comp);
  ok(comp.stats().nHidden === low, 'stats().nHidden');
  const old = comp.deleteHidden();
  ok(old.length === count - low && native.count(comp.handle) === count - low && comp.loadedVertexCount === count - low, 'deleteHidden lowers count by ' + low);
  const after = comp.histogram('alpha', { bins: 256, lo: 0, hi: 256 });
  ok(same(Array.from(after.counts), Array.from(vis.counts)) && after.passing === count - low, 'the histogram after the deletion');

  ok(throwsRange(() => comp.histogram('alpha', { bins: 0 })) && throwsRange(() => comp.histogram('alpha', { bins: 4097 })), 'bins outside 1 .. 4096 are refused');
  let threw = false;
  try { comp.selectRange('x', NaN, 1); } catch (e) { threw = true; }
  ok(threw, 'a NaN bound is refused');
  comp.remove();
  console.log('props gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

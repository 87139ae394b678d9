// Node side of the per-splat contribution: the addon's renderContrib / contribClear / contribInfo and the component shim's
// accumulateSeen / clearSeen / 'seen', on a scene tests/test_contrib_node.py wrote; the answers go to stdout as JSON for the
// Python side to compare with capi.
//   node test_contrib.js cpu                                  -- exports only (no GPU)
//   node test_contrib.js gpu scene.splat pose.json
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
for (const f of ['renderContrib', 'contribClear', 'contribInfo'])
  ok(typeof native[f] === 'function', 'addon exports ' + f);
for (const f of ['accumulateSeen', 'clearSeen'])
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
ok(throwsRange(() => GaussianSplatting.prototype.histogram.call({ handle: null }, 'Seen')), 'property names are lower case');
let threw = false;
try { GaussianSplatting.prototype.accumulateSeen.call({ handle: null }); } catch (e) { threw = true; }
ok(threw, 'accumulateSeen needs a frame first');
if (mode === 'cpu') { console.log('contrib cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height, vp = { width: W, height: H };
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };
const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const count = await comp.loadData(camera, entity, null, scenePath);
  ok(count > 0, 'loaded ' + count);
  let i0 = native.contribInfo(comp.handle);
  ok(i0.rows === 0 && i0.frames === 0, 'no store before the first contribution frame');
  const empty = comp.histogram('seen', { bins: 4, lo: 0, hi: 1 });
  ok(empty.passing === count && empty.counts[0] === count, 'an empty store: every value is 0');
  comp.tick();
  const plain = Uint8Array.from(comp.render(camera, vp));
  const info = comp.accumulateSeen();
  ok(info.rows === count && info.frames === 1, 'accumulateSeen: ' + JSON.stringify(info));
  // the addon's own call: the frame's colour is gs_render's; a second frame doubles the store
  const p = comp._renderParams(camera, vp, undefined);
  const img = native.renderContrib(comp.handle, p, true);
  ok(img instanceof Uint8Array && same(Array.from(img), Array.from(plain)) && plain.some((v) => v !== 0), "renderContrib's colour is render's");
  ok(native.renderContrib(comp.handle, p, false) === null, 'no image asked for');
  ok(native.contribInfo(comp.handle).frames === 3, 'three frames');
  comp.clearSeen();
  i0 = native.contribInfo(comp.handle);
  ok(i0.rows === 0 && i0.frames === 0, 'clearSeen');
  comp.accumulateSeen();
  const r = native.propRange(comp.handle, 16, 0, 0);
  const h = comp.histogram('seen', { bins: 64 });
  ok(h.lo === r.min && h.hi === r.max && sum(h.counts) === count && r.count === count && r.min === 0 && r.max > 0, "histogram('seen') spans propRange");
  const unseen = comp.selectRange('seen', 0, 0, { hide: true });
  ok(unseen > 0 && unseen < count, unseen + ' splats add nothing to this view');
  const old = comp.deleteHidden();
  ok(old.length === count - unseen && native.contribInfo(comp.handle).rows === count - unseen, 'deleteHidden carries the store along');
  const after = comp.histogram('seen', { bins: 64, lo: h.lo, hi: h.hi });
  comp.tick();
  ok(same(Array.from(Uint8Array.from(comp.render(camera, vp))), Array.from(plain)), 'the view is what it was');
  console.log('RESULT ' + JSON.stringify({ count, min: r.min, max: r.max, counts: Array.from(h.counts), unseen, after: Array.from(after.counts) }));
  comp.remove();
  console.log('contrib gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

// Node side of the editing calls: the addon's setState / setStateIds / selectBox / selectSphere / selectRect / compact and the component
// shim's hideSplats / showAll / selectBox / selectRect / deleteHidden, on a scene tests/test_edit_node.py wrote.
//   node test_edit.js cpu                                  -- exports only (no GPU)
//   node test_edit.js gpu scene.splat pose.json
// pose.json: {width, height, proj[16], camera[16], object[16], box[16]} -- three.js world matrices, column-major.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }

const [mode, scenePath, posePath] = process.argv.slice(2);
for (const f of ['setState', 'setStateIds', 'selectBox', 'selectSphere', 'selectRect', 'compact'])
  ok(typeof native[f] === 'function', 'addon exports ' + f);
for (const f of ['hideSplats', 'showAll', 'selectBox', 'selectRect', 'deleteHidden'])
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
if (mode === 'cpu') { console.log('edit cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height, vp = { width: W, height: H };
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };
const boxEntity = { matrixWorld: { elements: pose.box } };
const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);

async function component() {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const n = await comp.loadData(camera, entity, null, scenePath);
  ok(n > 0, 'loaded ' + n);
  return comp;
}
function draw(comp) { comp.tick(); return Uint8Array.from(comp.render(camera, vp)); }

(async () => {
  const comp = await component();
  const n0 = native.count(comp.handle);
  const f0 = draw(comp);
  ok(f0.some((v) => v !== 0), 'the frame is not empty');

  // hide by pick(x, y): the picked pixel changes, and showAll brings the frame back (leaving the selected bit alone)
  let hit = null, px = 0, py = 0;
  for (py = H >> 1; py < H && !hit; py += 7) for (px = W >> 1; px < W && !hit; px += 7) hit = comp.pick(px, py);
  ok(hit && hit.index >= 0 && hit.index < n0, 'pick found a splat');
  px -= 7; py -= 7;
  ok(comp.pick(px, py).index === hit.index, 'the pixel that was picked');
  const o = 4 * (py * W + px);
  native.setStateIds(comp.handle, new Uint32Array([hit.index]), 2);      // (clearBits undefined: 0)
  ok(same(draw(comp), f0), 'the selected bit changes no pixel');
  ok(comp.hideSplats([hit.index]) === 1, 'hideSplats takes a plain array');
  const f1 = draw(comp);
  ok(!same(f1.subarray(o, o + 4), f0.subarray(o, o + 4)), 'the picked pixel changes once its surface splat is hidden');
  ok(comp.stats().nHidden === 1, 'stats().nHidden');
  const again = comp.pick(px, py);
  ok(!again || again.index !== hit.index, 'a hidden splat is never picked');
  ok(comp.showAll() === n0, 'showAll reaches every splat');
  ok(same(draw(comp), f0) && comp.stats().nHidden === 0, 'showAll brings the frame back');

  // selectBox {invert, hide} == the same box as cutoutEntity
  const outside = comp.selectBox(boxEntity, { invert: true, hide: true });
  ok(outside > 0 && outside < n0, 'the box cuts: ' + outside + ' of ' + n0 + ' outside');
  const fa = draw(comp);
  const cut = await component();
  cut.cutout = boxEntity;
  const fb = draw(cut);
  ok(!same(fa, f0), 'hiding what lies outside the box changes the picture');
  ok(same(fa, fb), 'selectBox {invert, hide} draws the frame of the same box as cutoutEntity');
  ok(comp.selectBox(boxEntity) === n0 - outside, 'selectBox without options selects what lies inside');
  cut.remove();

  // selectRect: among what is drawn; its arguments are checked
  // (every editing call drops the order, as a push does: a tick before each)
  const rect = (...r) => { draw(comp); return comp.selectRect(...r); };
  const all = rect(0, 0, W, H), quarter = rect(0, 0, W >> 1, H >> 1), huge = rect(-1e12, -1e12, 1e12, 1e12);
  ok(all > 0 && quarter > 0 && quarter < all && huge === all, 'selectRect: ' + quarter + ' of ' + all + ' in the top-left quarter');
  let threw = false;
  try { comp.selectRect(0, NaN, W, H); } catch (e) { threw = e instanceof RangeError; }
  ok(threw, 'a NaN in the rectangle is refused');

  // deleteHidden lowers count; the frame stays
  const old = comp.deleteHidden();
  ok(old instanceof Uint32Array && old.length === n0 - outside && native.count(comp.handle) === n0 - outside && comp.loadedVertexCount === n0 - outside,
    'deleteHidden lowers count to ' + (n0 - outside));
  ok(old.every((v, i) => i === 0 || v > old[i - 1]), 'the index map is increasing');
  ok(same(draw(comp), fa), 'the frame after deleteHidden is the frame before it');
  ok(comp.deleteHidden().length === n0 - outside, 'nothing hidden: nothing happens');
  comp.remove();
  console.log('edit gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

// Node side of the highlighted selection and of mask / lasso selection: the addon's selectMask / maskPolygon / highlightInfo and the
// component shim's highlightSelected / selectMask / selectLasso, on a scene tests/test_highlight_node.py wrote; the frames go to files
// that it compares with the ctypes path, the counts to one JSON line.
//   node test_highlight.js cpu                                  -- exports and maskPolygon only (no GPU)
//   node test_highlight.js gpu scene.splat out_prefix pose.json
// pose.json: {width, height, proj[16], camera[16], object[16], lasso[[x, y], ...], color[3], weight}
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }

const [mode, scenePath, outPrefix, posePath] = process.argv.slice(2);
for (const f of ['selectMask', 'maskPolygon', 'highlightInfo'])
  ok(typeof native[f] === 'function', 'addon exports ' + f);
for (const f of ['highlightSelected', 'selectMask', 'selectLasso', 'highlightInfo'])
  ok(typeof GaussianSplatting.prototype[f] === 'function', 'the shim has ' + f);
// maskPolygon needs no context: a square over pixel centres 2..5, even-odd
const sq = native.maskPolygon([2, 2, 6, 2, 6, 6, 2, 6], 8, 8);
ok(sq instanceof Uint8Array && sq.length === 64, 'maskPolygon returns width x height bytes');
ok(sq.every((v, i) => v === ((i % 8 >= 2 && i % 8 < 6 && (i >> 3) >= 2 && (i >> 3) < 6) ? 1 : 0)), 'maskPolygon fills the square');
ok(native.maskPolygon([1, 1, 5, 5], 8, 8).every((v) => v === 0), 'fewer than three points: an empty mask');
let threw = false;
try { native.maskPolygon([1, 1, 5], 8, 8); } catch (e) { threw = e instanceof RangeError; }
ok(threw, 'an odd number of coordinates is refused');
if (mode === 'cpu') { console.log('highlight cpu checks ok'); process.exit(0); }
ok(mode === 'gpu', 'unknown mode ' + mode);

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height, vp = { width: W, height: H };
const camera = { matrixWorld: { elements: pose.camera }, projectionMatrix: { elements: pose.proj } };
const entity = { matrixWorld: { elements: pose.object } };
const dump = (tag, a) => fs.writeFileSync(outPrefix + '.' + tag, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
const option = (pose.color[0] | pose.color[1] << 8 | pose.color[2] << 16) + pose.weight * 16777216;

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  ok(await comp.loadData(camera, entity, null, scenePath) > 0, 'loaded');
  const draw = () => { comp.tick(); return Uint8Array.from(comp.render(camera, vp)); };
  const plain = draw();
  dump('plain.rgba', plain);
  ok(comp.highlightInfo().lastFrame === 0 && comp.highlightInfo().value === 0, 'off by default');

  // the option without a selection changes nothing; the lasso selects; the next frame shows it
  comp.highlightSelected(pose.color, pose.weight);
  ok(comp.highlightInfo().value === option, 'highlightSelected sets option 23 to ' + option);
  ok(same(draw(), plain) && comp.highlightInfo().lastFrame === 0, 'no store: the plain frame from the plain kernels');
  const hit = comp.selectLasso(pose.lasso);
  const lit = draw();
  dump('lit.rgba', lit);
  ok(comp.highlightInfo().lastFrame === 1, 'the highlighting kernels ran');
  ok(!same(lit, plain), 'the selection shows');
  comp.highlightSelected();
  ok(comp.highlightInfo().value === 0, 'no arguments: off');
  ok(same(draw(), plain), 'switched off: the plain frame again');
  comp.highlightSelected(pose.color, 0);
  ok(comp.highlightInfo().value < 16777216, 'weight 0: off');

  // the same lasso as a flat array and as a mask; visibleOnly takes fewer
  draw();
  const flat = comp.selectLasso([].concat(...pose.lasso));
  draw();
  const byMask = comp.selectMask(native.maskPolygon([].concat(...pose.lasso), W, H));
  draw();
  const visible = comp.selectLasso(pose.lasso, { visibleOnly: true });
  draw();
  const inverted = comp.selectLasso(pose.lasso, { invert: true });
  draw();
  const all = comp.selectMask(new Uint8Array(W * H).fill(1));
  ok(flat === hit && byMask === hit, 'points as pairs, flat, or as a mask: ' + hit + ' / ' + flat + ' / ' + byMask);
  ok(visible > 0 && visible < hit, 'visibleOnly selects fewer: ' + visible + ' of ' + hit);
  // hide: the lasso's splats leave the next order
  draw();
  const hidden = comp.selectLasso(pose.lasso, { hide: true });
  draw();
  ok(hidden === hit && comp.stats().nHidden === hit, 'hide: ' + comp.stats().nHidden + ' hidden');
  threw = false;
  try { native.selectMask(comp.handle, comp._renderParams(camera, vp), new Uint8Array(W * H - 1), null, 2, 0, 0); } catch (e) { threw = e instanceof RangeError; }
  ok(threw, 'a mask smaller than the frame is refused');
  comp.remove();
  console.log(JSON.stringify({ hit, visible, inverted, all }));
  console.log('highlight gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

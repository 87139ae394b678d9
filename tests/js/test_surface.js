// Node side of the surface output: the addon's renderSurface / pick and the component shim's renderSurface / pick(x, y) on a scene
// tests/test_surface_node.py wrote; the planes and hits go to files that it compares with the ctypes path.
//   node test_surface.js cpu                                  -- exports only (no GPU)
//   node test_surface.js gpu scene.splat out_prefix pose.json
// pose.json: {width, height, proj[16], points[[x, y], ...], centre[x, y], translate[3]} -- identity camera and entity poses.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }

const [mode, scenePath, outPrefix, posePath] = process.argv.slice(2);
ok(typeof native.renderSurface === 'function' && typeof native.pick === 'function', 'addon exports renderSurface and pick');
ok(typeof GaussianSplatting.prototype.renderSurface === 'function' && typeof GaussianSplatting.prototype.pick === 'function',
  'the shim has renderSurface and pick');
if (mode === 'cpu') { console.log('surface cpu checks ok'); process.exit(0); }

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height, NONE = 0xFFFFFFFF;
const at = (t) => ({ elements: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, t[0], t[1], t[2], 1] });
const dump = (tag, a) => fs.writeFileSync(outPrefix + '.' + tag, Buffer.from(a.buffer, a.byteOffset, a.byteLength));

async function component(t) {
  const camera = { matrixWorld: at(t), projectionMatrix: { elements: pose.proj } };
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const n = await comp.loadData(camera, { matrixWorld: at(t) }, null, scenePath);
  ok(n > 0, 'loaded ' + n);
  comp.tick();
  return { comp, camera };
}

(async () => {
  const { comp, camera } = await component([0, 0, 0]);
  const vp = { width: W, height: H };
  const s = comp.renderSurface(camera, vp);
  ok(s.rgba.length === W * H * 4 && s.id.length === W * H && s.depth.length === W * H && s.alpha.length === W * H, 'plane sizes');
  ok(s.id instanceof Uint32Array && s.depth instanceof Float32Array && s.alpha instanceof Float32Array, 'plane types');
  ok(comp.stats().surface === 1, 'stats().surface is 1 after renderSurface');
  dump('rgba', s.rgba); dump('id', s.id); dump('depth', s.depth); dump('alpha', s.alpha);
  // the addon's pick against the planes
  const flat = new Int32Array(pose.points.length * 2);
  pose.points.forEach((p, i) => { flat[2 * i] = p[0]; flat[2 * i + 1] = p[1]; });
  const hits = native.pick(comp.handle, comp._renderParams(camera, vp), flat);
  ok(hits.length === pose.points.length, 'one hit per point');
  let none = 0, some = 0;
  hits.forEach((h, i) => {
    const [x, y] = pose.points[i], o = y * W + x, tag = 'point (' + x + ', ' + y + '): ';
    if (s.id[o] === NONE) { none++; ok(h.index === -1 && h.position === null, tag + 'index -1 and position null for "none"'); }
    else { some++; ok(h.index === s.id[o] && h.position && h.position.length === 3, tag + 'index equals the id plane'); }
    ok(h.depth === s.depth[o] && h.alpha === s.alpha[o], tag + 'depth and alpha equal the planes');
    // the shim's pick(x, y): the same hit, null for none
    const sh = comp.pick(x, y);
    if (s.id[o] === NONE) ok(sh === null, tag + 'shim pick is null');
    else ok(sh.index === h.index && sh.depth === h.depth && sh.alpha === h.alpha && sh.position[2] === h.position[2], tag + 'shim pick equals the addon');
  });
  ok(none > 0 && some > 0, 'the points hold hits and a "none"');
  let threw = false;
  try { native.pick(comp.handle, comp._renderParams(camera, vp), new Int32Array([W, 0])); } catch (e) { threw = /outside/.test(String(e.message)); }
  ok(threw, 'a point outside the frame throws');
  comp.render(camera, vp);
  ok(comp.stats().surface === 0, 'stats().surface is 0 after a plain render');
  const base = comp.pick(pose.centre[0], pose.centre[1]);
  ok(base !== null, 'the centre pixel has a surface');
  comp.remove();

  // a translated entity (and camera: the same picture): the hit's world position moves with it, and projects to the picked pixel
  const t = pose.translate;
  const moved = await component(t);
  moved.comp.render(moved.camera, vp);
  const hit = moved.comp.pick(pose.centre[0], pose.centre[1]);
  moved.comp.remove();
  ok(hit !== null && hit.index === base.index, 'the translated entity hits the same splat');
  for (let k = 0; k < 3; k++) {
    ok(hit.position[k] === base.position[k], 'object-space position unchanged');
    ok(Math.abs(hit.worldPosition[k] - (base.worldPosition[k] + t[k])) < 1e-4, 'world position = untranslated + translation');
  }
  const v = [hit.worldPosition[0] - t[0], hit.worldPosition[1] - t[1], hit.worldPosition[2] - t[2], 1], P = pose.proj, c = [0, 0, 0, 0];
  for (let r = 0; r < 4; r++) for (let k = 0; k < 4; k++) c[r] += P[4 * k + r] * v[k];      // three.js clip = projectionMatrix * view
  const sx = (c[0] / c[3] * 0.5 + 0.5) * W, sy = (1 - (c[1] / c[3] * 0.5 + 0.5)) * H;
  ok(c[3] > 0 && Math.abs(sx - pose.splat_centre[0]) < 0.01 && Math.abs(sy - pose.splat_centre[1]) < 0.01,
    'the world position projects to the splat\'s centre through the camera (' + sx + ', ' + sy + ')');
  fs.writeFileSync(outPrefix + '.hits.json', JSON.stringify({ hits, base, moved: hit }));
  console.log('surface gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

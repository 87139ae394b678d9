// Node side of the parallel-projection cameras: the constant RENDER_PARALLEL of the addon and of the component shim, and frames drawn
// through the shim with { flags: RENDER_PARALLEL } on a scene tests/test_parallel_node.py wrote; the frames go to files that it compares
// with the ctypes path.
//   node test_parallel.js cpu                                  -- constants only (no GPU)
//   node test_parallel.js gpu scene.splat out_prefix pose.json
// pose.json: {width, height, proj[16] (an orthographic projectionMatrix), persp[16], obj[16]} -- identity camera pose.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, native, RENDER_PARALLEL } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }

const [mode, scenePath, outPrefix, posePath] = process.argv.slice(2);
ok(RENDER_PARALLEL === 32, 'the shim exports RENDER_PARALLEL = 32');
ok(native.RENDER_PARALLEL === 32, 'the addon exports RENDER_PARALLEL = 32');
if (mode === 'cpu') { console.log('parallel cpu checks ok'); process.exit(0); }

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height;
const eye = { elements: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] };
const camera = { matrixWorld: eye, projectionMatrix: { elements: pose.proj } };
const vp = { width: W, height: H };
const dump = (tag, a) => fs.writeFileSync(outPrefix + '.' + tag, Buffer.from(a.buffer, a.byteOffset, a.byteLength));

(async () => {
  const comp = new GaussianSplatting({ src: scenePath }).init(null);
  const n = await comp.loadData(camera, { matrixWorld: { elements: pose.obj } }, null, scenePath);
  ok(n > 0, 'loaded ' + n);
  comp.tick();
  dump('parallel.rgba', comp.render(camera, vp, { flags: RENDER_PARALLEL }));
  dump('plain.rgba', comp.render(camera, vp));
  dump('parallel_again.rgba', comp.render(camera, vp, { flags: RENDER_PARALLEL }));
  // a perspective matrix with the flag is refused
  let threw = false;
  try { comp.render({ matrixWorld: eye, projectionMatrix: { elements: pose.persp } }, vp, { flags: RENDER_PARALLEL }); } catch (e) { threw = true; }
  ok(threw, 'a perspective projectionMatrix with RENDER_PARALLEL throws');
  comp.remove();
  console.log('parallel gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

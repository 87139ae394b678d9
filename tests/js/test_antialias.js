// Node side of the anti-aliased splats: the component shim's `antialias` property (schema, init, update on a live component) and the
// addon's stats field, on a scene tests/test_antialias_node.py wrote; the frames go to files that it compares with the ctypes path.
//   node test_antialias.js cpu                                  -- schema and shim only (no GPU)
//   node test_antialias.js gpu scene.splat out_prefix pose.json
// pose.json: {width, height, proj[16]} -- identity camera and entity poses.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, schema, native } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

function ok(cond, what) { if (!cond) { console.error('FAIL: ' + what); process.exit(1); } }

const [mode, scenePath, outPrefix, posePath] = process.argv.slice(2);
ok(schema.antialias && schema.antialias.type === 'boolean' && schema.antialias.default === false, 'schema.antialias: boolean, default false');
ok(typeof GaussianSplatting.prototype.update === 'function', 'the shim has update()');
if (mode === 'cpu') { console.log('antialias cpu checks ok'); process.exit(0); }

const pose = JSON.parse(fs.readFileSync(posePath, 'utf8'));
const W = pose.width, H = pose.height;
const eye = { elements: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] };
const camera = { matrixWorld: eye, projectionMatrix: { elements: pose.proj } };
const vp = { width: W, height: H };
const dump = (tag, a) => fs.writeFileSync(outPrefix + '.' + tag, Buffer.from(a.buffer, a.byteOffset, a.byteLength));

async function component(data) {
  const comp = new GaussianSplatting(Object.assign({ src: scenePath }, data)).init(null);
  const n = await comp.loadData(camera, { matrixWorld: eye }, null, scenePath);
  ok(n > 0, 'loaded ' + n);
  comp.tick();
  return comp;
}

(async () => {
  // set at init
  const a = await component({ antialias: true });
  const calls = [];
  const setOption = native.setOption;
  dump('init_on.rgba', a.render(camera, vp));
  ok(a.stats().antialias === 1, 'stats().antialias is 1 with antialias: true');
  a.remove();

  // toggled on a live component: the next frame changes, and only option 20 is set, once per change
  const b = await component({});
  dump('live_off.rgba', b.render(camera, vp));
  ok(b.stats().antialias === 0, 'stats().antialias is 0 by default');
  native.setOption = (h, opt, v) => { calls.push([opt, v]); return setOption(h, opt, v); };
  b.update({ antialias: true });
  b.update({ antialias: true });
  dump('live_on.rgba', b.render(camera, vp));
  ok(b.stats().antialias === 1, 'stats().antialias follows the property');
  b.update({ antialias: false });
  dump('live_off_again.rgba', b.render(camera, vp));
  ok(b.stats().antialias === 0, 'stats().antialias is 0 again');
  b.update({});
  native.setOption = setOption;
  ok(JSON.stringify(calls) === JSON.stringify([[20, 1], [20, 0]]), 'update sets option 20 and nothing else, once per change: ' + JSON.stringify(calls));
  b.remove();
  console.log('antialias gpu checks ok');
})().catch((e) => { console.error(e); process.exit(1); });

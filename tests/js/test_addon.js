// node test_addon.js cpu <goldenDir>
// node test_addon.js gpu <goldenDir> <scene.splat> <out.rgba> <width> <height> <yawDeg>
// Exercises the N-API addon + component shim.  Exit code 0 = all checks passed.
'use strict';
const fs = require('fs');
const path = require('path');
const PKG_JS = path.join(__dirname, '..', '..', 'aframe-gaussian-splatting_amd', 'js');
const { GaussianSplatting, schema, native, register } = require(path.join(PKG_JS, 'gaussian_splatting.js'));

const [mode, goldenDir] = process.argv.slice(2);
const manifest = JSON.parse(fs.readFileSync(path.join(goldenDir, 'manifest.json'), 'utf8'));
const TA = { f4: Float32Array, f8: Float64Array, u4: Uint32Array, i4: Int32Array, u1: Uint8Array, i2: Int16Array, u2: Uint16Array };
function loadCase(name) {
  const d = manifest[name]; const out = { meta: d.meta };
  if (Object.keys(d.arrays).length) {
    const raw = fs.readFileSync(path.join(goldenDir, name + '.bin'));
    for (const k of Object.keys(d.arrays)) {
      const a = d.arrays[k]; const T = TA[a.dtype];
      const ab = raw.buffer.slice(raw.byteOffset + a.offset, raw.byteOffset + a.offset + a.count * T.BYTES_PER_ELEMENT);
      out[k] = new T(ab);
    }
  }
  return out;
}
function same(a, b) {
  if (a.length !== b.length) return false;
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i] && !(a[i] !== a[i] && b[i] !== b[i])) return false;
  return true;
}
let checks = 0;
function ok(cond, what) { checks++; if (!cond) { console.error('FAIL:', what); process.exit(1); } }

// ---- surface
ok(schema.src.default === 'train.splat' && schema.pixelRatio.default === 1 && schema.xrPixelRatio.default === 0.5 &&
   schema.cutoutEntity.type === 'selector', 'schema defaults (index.js:2-7)');
for (const m of ['init', 'loadData', 'pushDataBuffer', 'tick', 'getProjectionMatrix', 'getModelViewMatrix', 'createWorker', 'processPlyBuffer'])
  ok(typeof GaussianSplatting.prototype[m] === 'function', 'method ' + m);
ok(same(native.scaledSize(2064, 2208, 0.5), [1032, 1104]) && same(native.scaledSize(800, 600, 0), [800, 600]), 'scaledSize');

// ---- host helpers vs golden vectors captured from the reference
for (const name of Object.keys(manifest).filter((k) => manifest[k].kind === 'camera')) {
  const c = loadCase(name);
  ok(same(native.modelViewMatrix(c.cam_world, c.obj_world), c.gs_mv), name + ' gsModelViewMatrix');
  ok(same(native.projectionMatrix(c.proj), c.gs_proj), name + ' gsProjectionMatrix');
  const t = native.tickUniforms(c.cam_world, c.obj_world, c.cutout_world);
  ok(same(t.view, c.view), name + ' view');
  if (c.cutout) ok(same(t.cutout, c.cutout), name + ' cutout');
}
for (const name of Object.keys(manifest).filter((k) => manifest[k].kind === 'ply')) {
  const c = loadCase(name);
  const rows = new Uint8Array(native.plyToSplat(c.ply.buffer.slice(c.ply.byteOffset, c.ply.byteOffset + c.ply.byteLength)));
  ok(same(rows, c.rows), name + ' processPlyBuffer');
}
try { native.plyToSplat(Buffer.from('ply\nnope')); ok(false, 'bad header must throw'); } catch (e) {
  ok(e.message === manifest.ply_errors.meta.no_end_header, 'PLY header message: ' + e.message);
}

if (mode === 'cpu') {
  let threw = false;
  try { native.create(0); } catch (e) { threw = true; ok(/no CPU fallback|HIP/.test(e.message), 'create error text: ' + e.message); }
  if (!fs.existsSync('/dev/kfd')) ok(threw, 'create() must fail without a GPU (no CPU fallback)');
  console.log('addon cpu checks ok:', checks);
  process.exit(0);
}

// ---- GPU: worker protocol against the reference worker's golden outputs
const [scenePath, outPath, W, H, yaw] = process.argv.slice(4);
const comp = new GaussianSplatting({ src: scenePath, pixelRatio: 1 }).init(null);
for (const name of Object.keys(manifest).filter((k) => manifest[k].kind === 'ply')) {   // processPlyBuffer on the GPU
  const c = loadCase(name);
  const rows = new Uint8Array(comp.processPlyBuffer(c.ply.buffer.slice(c.ply.byteOffset, c.ply.byteOffset + c.ply.byteLength)));
  ok(same(rows, c.rows), name + ' processPlyBuffer (GPU)');
}
try { comp.processPlyBuffer(Buffer.from('ply\nnope')); ok(false, 'bad header must throw'); } catch (e) {
  ok(e.message === manifest.ply_errors.meta.no_end_header, 'PLY header message (GPU path): ' + e.message);
}
for (const name of Object.keys(manifest).filter((k) => manifest[k].kind === 'sort')) {
  const c = loadCase(name);
  let reply = null;
  const self = { postMessage: (m) => { reply = m; } };
  comp.createWorker(self);
  self.onmessage({ data: { method: 'clear' } });
  let o = 0;
  for (const n of c.meta.pushes) {
    const m = new Float32Array(n * 16);
    for (let i = 0; i < n; i++) for (let k = 0; k < 4; k++) m[i * 16 + 12 + k] = c.rows4[(o + i) * 4 + k];
    self.onmessage({ data: { method: 'push', matrices: m.buffer } });
    o += n;
  }
  self.onmessage({ data: { method: 'sort', view: c.view.buffer.slice(c.view.byteOffset, c.view.byteOffset + 16), cutout: c.cutout } });
  ok(same(reply.sortedIndexes, c.sorted), name + ' worker protocol');
}
{
  let reply = null;
  const self = { postMessage: (m) => { reply = m; } };
  comp.createWorker(self);
  self.onmessage({ data: { method: 'clear' } });
  self.onmessage({ data: { method: 'sort', view: new Float32Array([0, 0, 1, -6]).buffer } });
  ok(reply.sortedIndexes.length === 1 && reply.sortedIndexes[0] === 0, 'sort before push -> [0]');
}

// ---- GPU: loadData (progressive chunks) -> tick -> render, written out for the Python side to compare
const { composeYaw: compose, perspective } = require('./mini_three.js');
const camera = { matrixWorld: compose([0, 1.6, 0], 0), projectionMatrix: perspective(80, W / H, 0.005, 10000) };
const object = { matrixWorld: compose([0, 1.5, -2], Number(yaw)) };
comp.loadData(camera, object, null, scenePath, 100003).then((n) => {
  ok(n === Math.floor(fs.statSync(scenePath).size / 32), 'loadedVertexCount ' + n);
  comp.tick();
  ok(comp.instanceCount === comp.sortedIndexes.length && comp.instanceCount > 0, 'instanceCount');
  const img = comp.render(camera, { width: Number(W), height: Number(H) });
  ok(img.length === W * H * 4, 'framebuffer size');
  fs.writeFileSync(outPath, Buffer.from(img.buffer, img.byteOffset, img.byteLength));
  fs.writeFileSync(outPath + '.idx', Buffer.from(comp.sortedIndexes.buffer, comp.sortedIndexes.byteOffset, comp.sortedIndexes.byteLength));
  const strip = comp.render(camera, { width: Number(W), height: Number(H), x0: 16, x1: 48 });
  ok(strip.length === 32 * H * 4, 'strip size');
  ok(comp.render(camera, { width: Number(W), height: Number(H) }) === img, 'the frame buffer is reused (page-locked, no per-call allocation)');
  {
    // GS_OPT_SEG_COUNT (21) and the two statistics at the end of gs_stats: segCount, nRuns.  (GS_OPT_ROW_WALK 18 off meanwhile: a walked
    // frame builds no lists and counts no segments.)
    const first = Uint8Array.from(img), s0 = comp.stats();
    ok((s0.segCount === 0 || s0.segCount === 1) && s0.nRuns > 0 && s0.nRuns <= s0.nPairs, 'stats(): segCount ' + s0.segCount + ', nRuns ' + s0.nRuns);
    native.setOption(comp.handle, 18, 0); native.setOption(comp.handle, 21, 2);
    ok(same(comp.render(camera, { width: Number(W), height: Number(H) }), first) && comp.stats().segCount === 1, 'setOption(21, 2): same frame, segCount 1');
    native.setOption(comp.handle, 21, 0);
    ok(same(comp.render(camera, { width: Number(W), height: Number(H) }), first) && comp.stats().segCount === 0, 'setOption(21, 0): same frame, segCount 0');
    let refused = false;
    try { native.setOption(comp.handle, 21, 3); } catch (e) { refused = e.code === 'GS-1'; }
    ok(refused, 'setOption(21, 3) is GS_E_BADARG');
    native.setOption(comp.handle, 21, 1); native.setOption(comp.handle, 18, 1);
  }
  // ---- the reference's rhythm: fire-and-forget sort, single flight (index.js:201-207, 438-455): tick posts the sort, the frames drawn
  // until its reply arrives use the last COMPLETED order, the reply installs the new one.  Pose A = the order held now; pose B = the
  // entity turned by 70 degrees.
  const keep = Uint32Array.from(comp.sortedIndexes), keepImg = Uint8Array.from(img);
  const vp = { width: Number(W), height: Number(H) };
  const objectA = object, objectB = { matrixWorld: compose([0, 1.5, -2], Number(yaw) + 70) };
  comp.object = objectB;
  const staleWant = Uint8Array.from(comp.render(camera, vp));                  // pose B drawn with A's order: what the reference shows meanwhile
  comp.tick();                                                                  // (synchronously: B's order ...)
  const keepB = Uint32Array.from(comp.sortedIndexes), freshWant = Uint8Array.from(comp.render(camera, vp));   // ... and B's frame
  ok(!same(keepB, keep) && !same(freshWant, staleWant), 'the two poses have different orders and the stale order shows');
  comp.object = objectA; comp.tick(); comp.object = objectB;                   // back to: A's order installed, pose B to come
  const pending = comp.tickAsync();
  ok(pending && typeof pending.then === 'function' && comp.sortReady === false, 'tickAsync posts the sort and returns');
  ok(comp.tickAsync() === null, 'a second tick while the sort is in flight does nothing (sortReady)');
  let stale = null, threw = null;
  try { stale = Uint8Array.from(comp.render(camera, vp)); } catch (e) { threw = e.code || String(e); }
  ok(threw === null, 'render() while the sort is in flight does not throw (' + threw + ')');
  ok(stale && same(stale, staleWant), 'render() while the sort is in flight draws with the last completed order (index.js:201-207)');
  ok(same(comp.sortedIndexes, keep), 'sortedIndexes is still the completed order');
  return pending.then((idx) => {
    ok(comp.sortReady === true && comp.instanceCount === idx.length && same(idx, keepB), 'asynchronous order == synchronous order of the new pose');
    ok(same(comp.render(camera, vp), freshWant), 'after the reply: render() draws the new order');
    comp.object = objectA;
    const p2 = comp.tickAsync();
    ok(same(comp.tickFinish(), keep) && comp.sortReady === true, 'tickFinish() collects the posted sort at once');
    return p2;
  }).then(() => {
    ok(same(comp.render(camera, vp), keepImg), 'pose A again, through the posted sort');
    // the draw off the JS thread (napi_async_work) still owns the context while it runs: a context is single-caller
    const pr = comp.renderAsync(camera, vp);
    let busy = false;
    try { comp.render(camera, vp); } catch (e) { busy = e.code === 'GS_BUSY'; }
    ok(busy, 'the context refuses other calls while renderAsync owns it');
    return pr;
  }).then((img2) => {
    ok(same(img2, keepImg), 'asynchronous frame == synchronous frame');
    // JS-visible rate: tick + render into the reused page-locked frame, synchronously, one frame at a time
    const frames = 200;
    const t0 = process.hrtime.bigint();
    for (let i = 0; i < frames; i++) { comp.tick(); comp.render(camera, { width: Number(W), height: Number(H) }); }
    const sec = Number(process.hrtime.bigint() - t0) / 1e9;
    console.log('js-visible frames/s (tick + render into host memory, ' + W + 'x' + H + ', ' + n + ' splats): ' + (frames / sec).toFixed(1));
    // throughput mode: frames queued on the pipeline lanes, pixels copied into page-locked frames behind their kernels
    const q = [];
    for (let i = 0; i < 7; i++) q.push(comp.frameQueued(camera, { width: Number(W), height: Number(H) }));
    comp.sync();
    ok(new Set(q).size === 7 && q.every((f) => same(f, keepImg)), 'queued frames == synchronous frame, one buffer per frame in flight');
    for (let pass = 0; pass < 2; pass++) {           // (the first pass lets the library settle its buffers: a retry is legal there)
      const t1 = process.hrtime.bigint();
      for (let i = 0; i < frames; i++) { comp.frameQueued(camera, { width: Number(W), height: Number(H) }); if (i % 7 === 6) { try { comp.sync(); } catch (e) { if (e.code !== 'GS-9') throw e; } } }
      try { comp.sync(); } catch (e) { if (e.code !== 'GS-9') throw e; }
      const sec2 = Number(process.hrtime.bigint() - t1) / 1e9;
      if (pass) console.log('js-visible frames/s, queued (7 between syncs, ' + W + 'x' + H + '): ' + (frames / sec2).toFixed(1));
    }
    // several GPUs, from JavaScript: the partition, and a frame through the gathered path on a communicator of one rank
    const parts = native.partition([1032, 1032], 2);
    ok(parts.length === 2 && parts[0].view === 0 && parts[0].owner === 0 && parts[1].view === 1 && parts[1].owner === 1 &&
       parts[1].x0 === 0 && parts[1].x1 === 1032, 'XR partition: eye k -> rank k');
    ok(native.partition([1920], 8).every((q, i) => q.x0 === 240 * i && q.x1 === 240 * (i + 1) && q.owner === i), 'eight 240-pixel strips');
    native.commInit(comp.handle, native.commUniqueId(comp.handle), 0, 1);
    const p = comp._renderParams(camera, { width: Number(W), height: Number(H) });
    const u = comp._tickUniforms();
    native.sortGathered(comp.handle, u.view, u.cutout, p);
    native.renderGathered(comp.handle, p, 0, 0);
    const gathered = native.readGathered(comp.handle, 0, native.allocFrame(Number(W), Number(H)));
    ok(same(gathered, keepImg), 'gathered frame (world 1) == render()');
    // ONE node process, several GPUs (here: two and three "devices" on the one GPU): createMulti owns the contexts, replicates the
    // pushes, splits the frame in column strips; host-direct frames land in ONE page-locked buffer, device frames on the first GPU
    const sceneBytes = fs.readFileSync(scenePath);
    for (const devs of [[0, 0], [0, 0, 0]]) {
      const mh = native.createMulti(devs);
      ok(native.multiPushSplat(mh, sceneBytes.buffer.slice(sceneBytes.byteOffset, sceneBytes.byteOffset + sceneBytes.byteLength)) === n, 'multiPushSplat count');
      native.multiSort(mh, u.view, u.cutout, p);
      const mf = native.multiRender(mh, p, native.allocFrame(Number(W), Number(H)), 0);
      ok(same(mf, keepImg), 'one process, ' + devs.length + ' devices: host-direct frame == render()');
      const ring = [0, 1, 2, 3].map(() => native.allocFrame(Number(W), Number(H)));
      for (let attempt = 0; attempt < 4; attempt++) {
        for (const f of ring) { native.multiSort(mh, u.view, u.cutout, p); native.multiRender(mh, p, f, 8 /* GS_RENDER_ASYNC */); }
        try { native.multiSync(mh); break; } catch (e) { if (e.code !== 'GS-9' || attempt === 3) throw e; }
      }
      ok(ring.every((f) => same(f, keepImg)), 'queued host-direct frames == render()');
      native.multiSort(mh, u.view, u.cutout, p);
      native.multiRenderDevice(mh, p, 0);
      ok(same(native.multiRead(mh, 0, native.allocFrame(Number(W), Number(H))), keepImg), 'device frame gathered on the first device == render()');
      native.multiDestroy(mh);
      let dead = false;
      try { native.multiSync(mh); } catch (e) { dead = e.code === 'GS_DESTROYED'; }
      ok(dead, 'multiDestroy');
    }
    // ---- the REGISTERED component, driven the way A-Frame drives the reference's (index.js:8-23): registerComponent, init on an
    // entity of a scene that has not loaded yet, the scene's 'loaded' event, then ticks; the host's frame sink gets the pixels
    {
      let def = null;
      register({ registerComponent: (name, d) => { ok(name === 'gaussian_splatting', 'registered name'); def = d; } });
      ok(def && def.schema === schema && ['init', 'tick', 'remove'].every((m) => typeof def[m] === 'function'), 'component definition');
      const calls = [], listeners = {};
      const renderer = { setPixelRatio: (r) => calls.push(['pr', r]), xr: { setFramebufferScaleFactor: (r) => calls.push(['xr', r]) },
        getDrawingBufferSize: (v) => v.set(Number(W), Number(H)) };
      const sceneEl = { renderer, hasLoaded: false, camera: { el: { components: { camera: { camera } } } },
        addEventListener: (ev, fn) => { listeners[ev] = fn; } };
      const inst = Object.create(def);
      inst.data = { src: scenePath, cutoutEntity: null, pixelRatio: 1, xrPixelRatio: 0.5 };
      inst.el = { sceneEl, object3D: object };
      inst.init();
      ok(calls.length === 2 && calls[0][0] === 'pr' && calls[0][1] === 1 && calls[1][0] === 'xr' && calls[1][1] === 0.5, 'init applies pixelRatio / xrPixelRatio (index.js:10-15)');
      ok(typeof listeners.loaded === 'function' && inst.ready === null, 'init waits for the scene (index.js:17)');
      inst.tick();                                                   // before the load: nothing to do, nothing thrown
      const sunk = [];
      inst.frameSink = (rgba, vp) => sunk.push([Uint8Array.from(rgba), vp]);
      return listeners.loaded().then((count) => {
        ok(count === n && inst.impl.camera === camera && inst.impl.object === object && inst.impl.renderer === renderer, 'loaded -> loadData(camera, object3D, renderer, src) (index.js:18)');
        inst.tick();
        ok(inst.impl.instanceCount === keep.length && same(inst.impl.sortedIndexes, keep), 'registered tick sorts (index.js:438)');
        ok(sunk.length === 1 && sunk[0][1].width === Number(W) && same(sunk[0][0], keepImg), 'the frame sink receives the frame render() returns');
        inst.remove();
        ok(inst.impl === null, 'remove');
      });
    }
  }).then(() => {
    comp.remove();
    let gone = false;
    try { comp.tick(); } catch (e) { gone = e.code === 'GS_DESTROYED'; }
    ok(gone, 'remove() destroys the context');
    console.log('addon gpu checks ok:', checks);
  });
}).catch((e) => { console.error('FAIL:', e); process.exit(1); });

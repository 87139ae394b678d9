// gaussian_splatting.js -- host side of the drop-in, in the reference's own language.
//
// A headless mirror of the A-Frame `gaussian_splatting` component surface (reference index.js:1-23 schema/init,
// 222 loadData, 328 pushDataBuffer, 438 tick, 456/467 camera matrices, 488 createWorker, 600 processPlyBuffer):
// same property names and defaults, same method names, same worker message protocol -- but the Worker sort and
// the WebGL draw are replaced by the MI355X HIP path behind the N-API addon (gs_splat_napi.node -> libgs_splat_hip.so),
// and `render()` returns the RGBA framebuffer that three.js would have drawn.
//
// camera / object arguments are duck-typed like three.js objects: {matrixWorld: {elements[16]},
// projectionMatrix: {elements[16]}} (column-major).  There is no JS fallback for the hot path.
'use strict';
const fs = require('fs');
const native = require('./gs_splat_napi.node');

const schema = {                                   // index.js:2-7
  src: { type: 'string', default: 'train.splat' },
  cutoutEntity: { type: 'selector' },
  pixelRatio: { type: 'number', default: 1 },
  xrPixelRatio: { type: 'number', default: 0.5 },
  // beyond the reference: the highest spherical-harmonics band of a .ply to keep and evaluate per frame (view-dependent colour,
  // GS_OPT_SH_DEGREE); 0 = the reference's baked f_dc colour.  `.splat` files carry no coefficients and ignore it.
  shDegree: { type: 'number', default: 0 },
  // beyond the reference: compensate every splat's opacity for the 0.3 px^2 dilation of its projected covariance (index.js:139-141;
  // GS_OPT_ANTIALIAS) -- for scenes trained with an anti-aliased rasteriser, and for low pixelRatio / xrPixelRatio.  May be
  // changed on a live component: the next frame takes it.
  antialias: { type: 'boolean', default: false },
};
const OPT_SH_DEGREE = 19;
const OPT_ANTIALIAS = 20;
const OPT_HIGHLIGHT = 23;
// beyond the reference: GS_RENDER_PARALLEL, for params.flags -- pass { flags: RENDER_PARALLEL } as the `options` of render / frame / renderSurface /
// pick / selectRect / selectMask when `camera` is a THREE.OrthographicCamera (its projectionMatrix has the bottom row 0, 0, 0, 1): the splats are
// then projected by that camera's constant Jacobian instead of the reference's perspective focal / z (index.js:127-131)
const RENDER_PARALLEL = 32;
const ROW_LENGTH = 3 * 4 + 3 * 4 + 4 + 4;          // index.js:227

const PROP_NAMES = ['x', 'y', 'z', 'red', 'green', 'blue', 'alpha', 'size2'];   // GS_PROP_*
const PROP_FILTERS = { all: [0, 0], visible: [1, 0], selected: [3, 2] };        // (stateMask, stateValue); 1 = hidden, 2 = selected

function elementsOf(m) { return m && m.elements ? m.elements : m; }
const PROP_SEEN = 16;                              // GS_PROP_SEEN: 'seen', the contribution store in pixels (accumulateSeen)
function propId(name) {
  if (name === 'seen') return PROP_SEEN;
  const p = PROP_NAMES.indexOf(name);
  if (p < 0) throw new RangeError('unknown property ' + name + ' (one of ' + PROP_NAMES.join(' ') + ' seen)');
  return p;
}

class GaussianSplatting {
  constructor(data, options) {
    this.data = Object.assign({ src: schema.src.default, cutoutEntity: null, pixelRatio: schema.pixelRatio.default,
      xrPixelRatio: schema.xrPixelRatio.default, shDegree: schema.shDegree.default, antialias: schema.antialias.default }, data || {});
    this.device = (options && options.device) || 0;
    this.handle = native.create(this.device);       // replaces `new Worker(...)` + GL resource creation
    this.shDegree = Math.max(0, Math.min(3, Math.floor(Number(this.data.shDegree) || 0)));
    if (this.shDegree > 0) native.setOption(this.handle, OPT_SH_DEGREE, this.shDegree);
    this.antialias = false;
    this.update(this.data);
    this.loadedVertexCount = 0;
    this.rowLength = ROW_LENGTH;
    this.sortReady = true;
    this.instanceCount = 0;
    this.sortedIndexes = null;
    this.cutout = null;
  }

  // init (index.js:8-23): resolution properties are only applied when > 0; the cutout entity is resolved to its object3D.
  init(sceneEl) {
    const r = sceneEl && sceneEl.renderer;
    if (r && this.data.pixelRatio > 0 && r.setPixelRatio) r.setPixelRatio(this.data.pixelRatio);
    if (r && this.data.xrPixelRatio > 0 && r.xr && r.xr.setFramebufferScaleFactor) r.xr.setFramebufferScaleFactor(this.data.xrPixelRatio);
    if (this.data.cutoutEntity) this.cutout = this.data.cutoutEntity.object3D || this.data.cutoutEntity;
    return this;
  }

  // update (the component life cycle's): the properties that may change on a live component.  `antialias` reaches the library only
  // when it changes, and only as GS_OPT_ANTIALIAS; the next frame drawn takes it.
  update(data) {
    if (data && data.antialias !== undefined) {
      const on = data.antialias === true || data.antialias === 'true' || data.antialias === 1;
      this.data.antialias = on;
      if (on !== this.antialias) { native.setOption(this.handle, OPT_ANTIALIAS, on ? 1 : 0); this.antialias = on; }
    }
    return this;
  }

  // drawing-buffer size the reference would get from renderer.setPixelRatio / xr.setFramebufferScaleFactor
  framebufferSize(cssWidth, cssHeight, xr) {
    const [w, h] = native.scaledSize(cssWidth, cssHeight, xr ? this.data.xrPixelRatio : this.data.pixelRatio);
    return { width: w, height: h };
  }

  // loadData (index.js:222-327).  No network on the target: `src` is a path or file:// URL.  `.splat` files are
  // ingested progressively chunk by chunk exactly like the streaming branch (index.js:279-298); `.ply` is read whole,
  // converted by processPlyBuffer, then pushed (index.js:305-325).
  async loadData(camera, object, renderer, src, chunkBytes) {
    this.camera = camera; this.object = object; this.renderer = renderer;
    this.loadedVertexCount = 0;
    native.clear(this.handle);                       // worker.postMessage({method: "clear"})
    const file = String(src || this.data.src).replace(/^file:\/\//, '');
    const isPly = file.endsWith('.ply');
    const total = fs.statSync(file).size;
    const fd = fs.openSync(file, 'r');
    try {
      if (isPly) {
        const all = Buffer.alloc(total); fs.readSync(fd, all, 0, total, 0);
        const input = all.buffer.slice(all.byteOffset, all.byteOffset + total);
        if (native.cplyInfo(input)) {                // a chunked compressed .ply: decoded on the GPU, file order, SH rows under the option
          this.loadedVertexCount = native.loadCply(this.handle, input);
          this.sortReady = true;
          return this.loadedVertexCount;
        }
        const rows = this.processPlyBuffer(input);
        this.pushDataBuffer(rows, Math.floor(rows.byteLength / this.rowLength));
        if (this.shDegree > 0) {                     // the coefficients processPlyBuffer drops, in its row order
          const sh = native.plySh(this.handle, input, this.shDegree);
          if (sh.degree > 0) native.pushSh(this.handle, sh.rows, sh.degree);
        }
      } else {
        const step = chunkBytes || (1 << 22);
        let pending = Buffer.alloc(0), pos = 0;
        while (pos < total) {
          const buf = Buffer.alloc(Math.min(step, total - pos));
          fs.readSync(fd, buf, 0, buf.length, pos); pos += buf.length;
          pending = pending.length ? Buffer.concat([pending, buf]) : buf;
          if (pending.length > this.rowLength) {     // bytesRemains > rowLength (index.js:280)
            const vertexCount = Math.floor(pending.length / this.rowLength), used = vertexCount * this.rowLength;
            const ab = pending.buffer.slice(pending.byteOffset, pending.byteOffset + used);
            this.pushDataBuffer(ab, vertexCount);
            pending = pending.slice(used);
          }
        }
        if (pending.length >= this.rowLength) {
          const n = Math.floor(pending.length / this.rowLength);
          this.pushDataBuffer(pending.buffer.slice(pending.byteOffset, pending.byteOffset + n * this.rowLength), n);
        }
      }
    } finally { fs.closeSync(fd); }
    this.sortReady = true;
    return this.loadedVertexCount;
  }

  // pushDataBuffer (index.js:328-437): pack + upload + worker push, all on the GPU side now.
  pushDataBuffer(buffer, vertexCount) {
    if (vertexCount <= 0) return;
    native.pushSplat(this.handle, buffer, vertexCount);
    this.loadedVertexCount += vertexCount;
  }

  // tick (index.js:438-455) + the worker reply handler (index.js:201-207), single flight.  The reference always sorts
  // from this.camera (in XR: the head camera, one order for both eyes); passing an eye camera sorts for that eye alone
  // (SURVEY.md 8f-3): comp.tick(eye); comp.render(eye, viewport).
  tick(camera) {
    if (!this.sortReady) return;
    this.sortReady = false;
    try {
      const u = this._tickUniforms(camera);
      const indexes = native.sort(this.handle, u.view, u.cutout);
      this.sortedIndexes = indexes;
      this.instanceCount = indexes.length;
    } finally { this.sortReady = true; }
  }

  // The reference's rhythm: tick posts the sort and returns; the reply handler installs the new order and re-arms sortReady
  // (index.js:201-207, 438-455) -- and every frame drawn meanwhile uses the last COMPLETED order.  Returns the promise of the order,
  // or null while a sort is in flight.  render() / frame-less draws stay callable in between (they draw the old order); the new
  // order is installed when the promise resolves.  No second thread: gs_sort_begin enqueues the sort on a pipeline lane of its own,
  // the promise polls it (gs_sort_poll) from the event loop.
  tickAsync(camera) {
    if (!this.sortReady) return null;
    this.sortReady = false;
    const u = this._tickUniforms(camera);
    try { native.sortBegin(this.handle, u.view, u.cutout); } catch (e) { this.sortReady = true; throw e; }
    return new Promise((resolve, reject) => {
      const poll = () => {
        if (this.sortReady) { resolve(this.sortedIndexes); return; }            // (collected meanwhile by tickFinish)
        let indexes;
        try { indexes = native.sortPoll(this.handle, false, true); } catch (e) { this.sortReady = true; reject(e); return; }
        if (indexes === null) { setImmediate(poll); return; }
        this.sortedIndexes = indexes; this.instanceCount = indexes.length; this.sortReady = true;
        resolve(indexes);
      };
      setImmediate(poll);
    });
  }

  // the same reply collected at once (blocks until the posted sort has run): what a caller without an event loop turn to spare does
  tickFinish() {
    if (this.sortReady) return this.sortedIndexes;
    const indexes = native.sortPoll(this.handle, true, true);
    this.sortedIndexes = indexes; this.instanceCount = indexes.length; this.sortReady = true;
    return indexes;
  }

  _tickUniforms(camera) {
    return native.tickUniforms(elementsOf((camera || this.camera).matrixWorld), elementsOf(this.object.matrixWorld),
      this.cutout ? elementsOf(this.cutout.matrixWorld) : undefined);
  }

  getProjectionMatrix(camera) {                      // index.js:456-466
    if (!camera) camera = this.camera;
    return { elements: native.projectionMatrix(elementsOf(camera.projectionMatrix)) };
  }

  getModelViewMatrix(camera) {                       // index.js:467-487
    if (!camera) camera = this.camera;
    return { elements: native.modelViewMatrix(elementsOf(camera.matrixWorld), elementsOf(this.object.matrixWorld)) };
  }

  // The draw: onBeforeRender uniforms (index.js:184-195) + vertex/fragment/blend (index.js:77-181) -> RGBA8 pixels.
  // viewport = {width, height[, x0, x1]} in device pixels; returns Uint8Array, row 0 = top.
  // The pixels land in page-locked memory owned by the component and reused frame after frame (one buffer per strip size):
  // the returned Uint8Array is overwritten by the next render of the same size -- copy it to keep it.
  render(camera, viewport, options) {
    const p = this._renderParams(camera, viewport, options);
    return native.renderInto(this.handle, p, this._frame(p));
  }

  // One whole frame, synchronously, for a caller that wants pixels and not the index list: this frame's sort (the order stays on
  // the GPU -- tick() hands sortedIndexes back to JavaScript like the reference's worker does, ~3 MB per tick at 1 M splats) and
  // the draw.  Returns the frame like render().
  frame(camera, viewport, options) {
    const u = this._tickUniforms(camera);
    native.sort(this.handle, u.view, u.cutout, false);
    const p = this._renderParams(camera, viewport, options);
    return native.renderInto(this.handle, p, this._frame(p));
  }

  // The same draw off the JS thread (napi_async_work): resolves to the frame.  While it is in flight the component's
  // other calls throw GS_BUSY (a context is single-caller, like the reference's single-flight worker).
  renderAsync(camera, viewport, options) {
    const p = this._renderParams(camera, viewport, options);
    return native.renderAsync(this.handle, p, this._frame(p));
  }

  // Surface output (beyond the reference, whose material has depthWrite: false, index.js:177-181): the frame and, per pixel, the
  // splat at which the transmittance falls below one half (`id`, 0xFFFFFFFF: none), its window depth (0 = near, 1 = far; 1: none)
  // and the accumulated alpha -- {rgba, id: Uint32Array, depth: Float32Array, alpha: Float32Array}, row 0 = top.  Synchronous;
  // draws from the last completed order like render().
  renderSurface(camera, viewport, options) {
    return native.renderSurface(this.handle, this._renderParams(camera, viewport, options));
  }

  // Per-splat contribution (beyond the reference): one contribution frame with the component's current camera -- the camera, viewport
  // and options of the last render / frame / renderSurface call -- adds every splat's blend weights in that view to the 'seen' store,
  // in pixels.  Draw a few views, then histogram('seen'), selectRange('seen', 0, bound, {hide: true}) and deleteHidden() remove what
  // no view shows.  -> {rows, frames}: the store's length and the views accumulated so far.  clearSeen() starts over.
  accumulateSeen() {
    const v = this._lastView;
    if (!v) throw new Error('accumulateSeen: no frame has been drawn yet');
    native.renderContrib(this.handle, this._renderParams(v.camera, v.viewport, v.options), false);
    return native.contribInfo(this.handle);
  }
  clearSeen() { native.contribClear(this.handle); }

  // What a cursor, laser-controls or raycaster hit needs: the splat under pixel (x, y) of the CURRENT frame's drawing buffer (the
  // camera, viewport and options of the last render / frame / renderSurface call; column, row, row 0 = top), or null where nothing
  // is opaque enough (the transmittance never falls below one half).  -> {index, depth, alpha, position, worldPosition}:
  // `position` is the splat's centre as its .splat row stores it; `worldPosition` is that point taken to world space by the
  // entity's matrixWorld.  The rows' space is the reference's mirrored one -- getModelViewMatrix conjugates with diag(1, -1, 1)
  // and the packed centre is (x, y, -z) (index.js:350-354, 467-487) -- so the three.js object-space point matrixWorld acts on is
  // (x, -y, -z): what a raycaster's intersection.point holds.
  pick(x, y) {
    const v = this._lastView;
    if (!v) throw new Error('pick: no frame has been drawn yet');
    const hit = native.pick(this.handle, this._renderParams(v.camera, v.viewport, v.options), new Int32Array([x, y]))[0];
    if (hit.index < 0) return null;
    const m = elementsOf(this.object.matrixWorld), px = hit.position[0], py = -hit.position[1], pz = -hit.position[2];
    hit.worldPosition = [m[0] * px + m[4] * py + m[8] * pz + m[12], m[1] * px + m[5] * py + m[9] * pz + m[13],
      m[2] * px + m[6] * py + m[10] * pz + m[14]];
    return hit;
  }

  // Editing the resident cloud (gs_splat.h: one state byte per splat; 1 = hidden, 2 = selected).  A hidden splat leaves every sort, so
  // it is gone from the next tick's order on; the draws until then use the last completed order, as in the reference (index.js:201-207).
  // ids are what pick().index and renderSurface().id hold.
  hideSplats(ids) { return native.setStateIds(this.handle, ids instanceof Uint32Array ? ids : Uint32Array.from(ids), 1, 0); }
  // (clears the hidden bit alone -- the selected bit and the caller's six stay: the all-zero affine matrix maps every position into
  // the unit box, NaN positions included, so the box rule with clear = 1 reaches every splat)
  showAll() { return native.selectBox(this.handle, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], 0, 1, 0); }
  // entityOrMatrix: an entity / object3D whose unit box is the region (what cutoutEntity takes), or the 16 numbers of the
  // object-to-unit-box matrix tick builds for it.  opts.hide: hide the splats instead of selecting them; opts.invert: those outside.
  selectBox(entityOrMatrix, opts) {
    const o = opts || {};
    let box = entityOrMatrix;
    if (box && (box.object3D || box.matrixWorld)) {
      const obj = box.object3D || box;
      box = native.tickUniforms(elementsOf(this.camera.matrixWorld), elementsOf(this.object.matrixWorld), elementsOf(obj.matrixWorld)).cutout;
    }
    return native.selectBox(this.handle, box, o.hide ? 1 : 2, 0, o.invert ? 1 : 0);
  }
  // pixels of the CURRENT frame's drawing buffer (the view of the last render / frame call), row 0 = top; among what that view draws
  selectRect(x0, y0, x1, y1, opts) {
    const v = this._lastView, o = opts || {};
    if (!v) throw new Error('selectRect: no frame has been drawn yet');
    return native.selectRect(this.handle, this._renderParams(v.camera, v.viewport, v.options), [x0, y0, x1, y1], o.hide ? 1 : 2, 0, o.invert ? 1 : 0);
  }
  // Any screen-space region, as a mask image over the CURRENT frame's drawing buffer: Uint8Array(width * height), row 0 = top, non-zero =
  // inside.  opts.hide / opts.invert as above; opts.visibleOnly: only what that view shows -- the frame's surface is drawn
  // (renderSurface) and its depth plane limits the selection to the surface splats and what lies in front of them.
  selectMask(mask, opts) {
    const v = this._lastView, o = opts || {};
    if (!v) throw new Error('selectMask: no frame has been drawn yet');
    const whole = { width: v.viewport.width, height: v.viewport.height };
    const depth = o.visibleOnly ? this.renderSurface(v.camera, whole, v.options).depth : null;
    const p = this._renderParams(v.camera, whole, v.options);
    this._lastView = v;
    return native.selectMask(this.handle, p, mask, depth, o.hide ? 1 : 2, 0, o.invert ? 1 : 0);
  }
  // A lasso: points = [x, y, x, y, ...] or [[x, y], ...] in pixels of that buffer, closed by itself, even-odd fill at pixel centres
  selectLasso(points, opts) {
    const v = this._lastView;
    if (!v) throw new Error('selectLasso: no frame has been drawn yet');
    const flat = Array.isArray(points) && Array.isArray(points[0]) ? [].concat(...points) : points;
    return this.selectMask(native.maskPolygon(flat, v.viewport.width, v.viewport.height), opts);
  }
  // Show the selection: every frame tints the selected splats towards color ([r, g, b] bytes) by weight / 255 (GS_OPT_HIGHLIGHT; only
  // the colour word of a selected splat's projected record changes).  weight 0 or no arguments: off.  Takes effect with the next draw.
  highlightSelected(color, weight) {
    const c = color || [0, 0, 0], w = color ? (weight === undefined ? 128 : weight) : 0;
    native.setOption(this.handle, OPT_HIGHLIGHT, ((c[0] & 255) | (c[1] & 255) << 8 | (c[2] & 255) << 16) + (w & 255) * 16777216);
  }
  highlightInfo() { return native.highlightInfo(this.handle); }
  // The data panel: a histogram of one per-splat property -- 'x' 'y' 'z' (the rows' space, as pick().position), 'red' 'green' 'blue' 'alpha'
  // (bytes), 'size2' (the sum of the three squared axis lengths, object units^2) or 'seen' (accumulateSeen, pixels) -- over opts.of = 'all' (default) | 'visible' |
  // 'selected' (the visible selection), in opts.bins (default 256) bins over [opts.lo, opts.hi]; a bound left out is the property's own
  // minimum / maximum among those splats (propRange first).  -> {counts: Uint32Array, lo, hi, passing, below, above, nan}; an empty or
  // one-valued range is widened so that the call always has lo < hi.  Reads only: no tick, order or frame is disturbed.
  histogram(prop, opts) {
    const o = opts || {}, p = propId(prop), f = PROP_FILTERS[o.of || 'all'];
    if (!f) throw new RangeError("histogram: of must be 'all', 'visible' or 'selected'");
    let lo = o.lo, hi = o.hi;
    if (lo === undefined || hi === undefined) {
      const r = native.propRange(this.handle, p, f[0], f[1]);
      if (lo === undefined) lo = Number.isFinite(r.min) ? r.min : 0;
      if (hi === undefined) hi = Number.isFinite(r.max) ? r.max : lo;
      if (!(lo < hi)) hi = lo + (Math.abs(lo) > 1 ? Math.abs(lo) : 1);
    }
    return Object.assign(native.histogram(this.handle, p, lo, hi, o.bins === undefined ? 256 : o.bins, f[0], f[1]), { lo, hi });
  }
  // select (opts.hide: hide) the splats whose property lies in [lo, hi] (opts.invert: the others) -> how many
  selectRange(prop, lo, hi, opts) {
    const o = opts || {};
    return native.selectRange(this.handle, propId(prop), lo, hi, o.hide ? 1 : 2, 0, o.invert ? 1 : 0);
  }
  // Save the edited cloud: the splats of opts.of = 'all' (default) | 'visible' | 'selected' (as in histogram) as an ArrayBuffer of
  // 32-byte .splat rows, or as a binary .ply with up to opts.shDegree (default 3) spherical-harmonics bands where the cloud was loaded
  // with them -- what this component and the reference's loaders read.  Scale and rotation are recovered from the packed covariance
  // (gs_splat.h: gs_export_row).  Reads only; the caller owns the bytes (a download link, fs.writeFileSync).
  exportSplat(opts) {
    const f = PROP_FILTERS[(opts || {}).of || 'all'];
    if (!f) throw new RangeError("exportSplat: of must be 'all', 'visible' or 'selected'");
    return native.exportSplat(this.handle, f[0], f[1]);
  }
  exportPly(opts) {
    const o = opts || {}, f = PROP_FILTERS[o.of || 'all'];
    if (!f) throw new RangeError("exportPly: of must be 'all', 'visible' or 'selected'");
    return native.exportPly(this.handle, f[0], f[1], o.shDegree === undefined ? 3 : o.shDegree);
  }
  // ... or as a chunked compressed .ply (16 bytes per splat + one bounds record per 256; gs_splat.h: "Compressed .ply"), encoded on the
  // GPU; opts.morton (default true): rows in Morton order, so that a chunk's bounds are tight
  exportCply(opts) {
    const o = opts || {}, f = PROP_FILTERS[o.of || 'all'];
    if (!f) throw new RangeError("exportCply: of must be 'all', 'visible' or 'selected'");
    return native.exportCply(this.handle, f[0], f[1], o.shDegree === undefined ? 3 : o.shDegree, o.morton === undefined ? true : !!o.morton);
  }
  // Change resident splats in place.  adjustColour: colour' = matrix (9 numbers, row-major; default the identity) x colour + offset (3, in
  // byte units), alpha' = alphaScale x alpha + alphaOffset, for the splats of opts.of (as in histogram), on the GPU, bytes and
  // spherical-harmonics rows alike (gs_splat.h: gs_adjust_colour) -> how many were adjusted.  The order stays good: the next render shows it.
  adjustColour(opts) {
    const o = opts || {}, f = PROP_FILTERS[o.of || 'all'];
    if (!f) throw new RangeError("adjustColour: of must be 'all', 'visible' or 'selected'");
    return native.adjustColour(this.handle, o.matrix || [1, 0, 0, 0, 1, 0, 0, 0, 1], o.offset || [0, 0, 0],
      o.alphaScale === undefined ? 1 : o.alphaScale, o.alphaOffset === undefined ? 0 : o.alphaOffset, f[0], f[1]);
  }
  // transform: move, rotate and scale the splats of opts.of on the GPU, p' = scale x R p + translation in the rows' object space (rotation:
  // quaternion [w, x, y, z], need not be normalised; scale > 0; defaults: the identity), records, sort rows and spherical-harmonics rows
  // alike (gs_splat.h: gs_transform) -> how many were moved.  Drops the order like a push: the draws show the background until the next tick.
  transform(opts) {
    const o = opts || {}, f = PROP_FILTERS[o.of || 'all'];
    if (!f) throw new RangeError("transform: of must be 'all', 'visible' or 'selected'");
    return native.transform(this.handle, o.rotation || [1, 0, 0, 0], o.scale === undefined ? 1 : o.scale, o.translation || [0, 0, 0], f[0], f[1]);
  }
  // replaceSplat / replaceSh: 32-byte .splat rows (spherical-harmonics rows of `degree`) over the resident ones from index `first` on.
  // Replaced rows drop the order like a push: the draws show the background until the next tick.
  replaceSplat(first, rows) { return native.replaceSplat(this.handle, first, rows); }
  replaceSh(first, rows, degree) { return native.replaceSh(this.handle, first, rows, degree); }
  // real deletion of the hidden splats (the GPU holds the cloud twice for the duration of the call) -> Uint32Array: the old index of
  // every splat that stays
  deleteHidden() {
    const old = native.compact(this.handle);
    this.loadedVertexCount = native.count(this.handle);
    return old;
  }

  _renderParams(camera, viewport, options) {
    this._lastView = { camera, viewport, options };
    const proj = this.getProjectionMatrix(camera).elements;
    const p = Object.assign({
      modelView: this.getModelViewMatrix(camera).elements, projection: proj,
      width: viewport.width, height: viewport.height,
      focal: (viewport.height / 2.0) * Math.abs(proj[5]),
    }, options || {});
    if (viewport.x0 !== undefined) p.x0 = viewport.x0;
    if (viewport.x1 !== undefined) p.x1 = viewport.x1;
    return p;
  }

  _frame(p, slot) {
    const w = (p.x1 !== undefined ? p.x1 : p.width) - (p.x0 || 0), key = w + 'x' + p.height + (slot ? '#' + slot : '');
    if (!this._frames) this._frames = new Map();
    if (!this._frames.has(key)) this._frames.set(key, native.allocFrame(w, p.height));
    return this._frames.get(key);
  }

  // Throughput mode -- what WebGL does behind the reference's back: the draw call returns at once and frames queue up on the
  // GPU (index.js:184-207).  frameQueued = this frame's sort (the order stays on the GPU) + draw, enqueued on one of the
  // library's pipeline lanes (two frames per launch, GS_OPT_FRAME_BATCH); the pixels follow their kernels into one of
  // `QUEUE_DEPTH` page-locked frames, which is what is
  // returned -- valid after sync().  A frame that comes back incomplete (a buffer had to grow, a skipped binning round was
  // needed after all) is drawn again by sync() itself into the same frame (GS_OPT_AUTO_RETRY); sync() throws code GS-9
  // (GS_E_RETRY) only if more than QUEUE_DEPTH frames were queued between two sync() calls (frames sharing a buffer).
  frameQueued(camera, viewport, options) {
    if (!this._paired) { native.setOption(this.handle, 10, 2); this._paired = true; }   // GS_OPT_FRAME_BATCH: consecutive queued frames share their launches
    const u = this._tickUniforms(camera);
    native.sort(this.handle, u.view, u.cutout, false);
    const p = this._renderParams(camera, viewport, options);
    p.flags = (p.flags || 0) | 8;                      // GS_RENDER_ASYNC
    this._slot = ((this._slot || 0) % GaussianSplatting.QUEUE_DEPTH) + 1;
    return native.renderInto(this.handle, p, this._frame(p, this._slot));
  }

  sync() { native.sync(this.handle); }

  // The opaque scene three.js draws before the transparent splat mesh: window-space depth (depthTest: true,
  // depthWrite: false, index.js:179-180) and colour.  Float32Array / Uint8Array of width*height(*4), row 0 = top.
  setScene(depth, rgba, width, height) { native.setScene(this.handle, depth || null, rgba || null, width || 0, height || 0); }

  // createWorker (index.js:488-599): same message protocol, GPU-backed.  `self` needs postMessage; onmessage is installed.
  createWorker(self) {
    const h = native.create(this.device);
    let havePush = false;
    self.onmessage = (e) => {
      const d = e.data;
      if (d.method === 'clear') { native.clear(h); havePush = false; }
      if (d.method === 'push') { native.pushMatrices(h, d.matrices); havePush = true; }
      if (d.method === 'sort') {
        const sortedIndexes = havePush ? native.sort(h, d.view, d.cutout) : new Uint32Array(1);   // index.js:588-590
        self.postMessage({ sortedIndexes }, [sortedIndexes.buffer]);
      }
    };
    return self;
  }

  // processPlyBuffer (index.js:600-745): header on the host, importance order + row conversion on the GPU
  processPlyBuffer(inputBuffer) { return native.plyToSplatGpu(this.handle, inputBuffer); }

  stats() { return native.stats(this.handle); }

  // the reference leaks its worker and textures; this frees the context (HBM, streams, threads) at once
  remove() { native.destroy(this.handle); this._frames = null; }
}

GaussianSplatting.QUEUE_DEPTH = 7;                // frames to queue between two sync() calls in throughput mode: the first goes out alone
                                                   // at once, then GS_OPT_PIPELINE_DEPTH's default (3) pairs

// The registered component (index.js:1-23): AFRAME.registerComponent("gaussian_splatting", ...) with the reference's life cycle.
//   init    resolution properties (index.js:10-15); when the scene has loaded (index.js:17), loadData with the scene camera's
//           three.js camera, the entity's object3D, the renderer and `src` (index.js:18), and cutoutEntity -> its object3D
//           (index.js:19-21).  `this.ready` is the promise of that load.
//   tick    the reference's tick posts the worker sort (index.js:438-455) and three.js then draws the mesh; here tick sorts
//           and, if the host installed a frame sink, draws: `component.frameSink = (rgba, viewport) => ...` receives the
//           RGBA framebuffer three.js would have drawn (page-locked, reused: copy it to keep it).  The drawing-buffer size is
//           the renderer's (getDrawingBufferSize / domElement), i.e. what pixelRatio / xrPixelRatio made of the canvas.
//   remove  frees the context.
function sceneCamera(sceneEl) {                      // this.el.sceneEl.camera.el.components.camera.camera (index.js:18)
  const c = sceneEl && sceneEl.camera;
  return c && c.el && c.el.components && c.el.components.camera ? c.el.components.camera.camera : c;
}
function drawingBuffer(renderer) {
  if (!renderer) return null;
  if (renderer.getDrawingBufferSize) { const v = renderer.getDrawingBufferSize({ x: 0, y: 0, set(x, y) { this.x = x; this.y = y; return this; } });
    const w = v.width !== undefined ? v.width : v.x, h = v.height !== undefined ? v.height : v.y; if (w > 0 && h > 0) return { width: w, height: h }; }
  const el = renderer.domElement;
  return el && el.width > 0 && el.height > 0 ? { width: el.width, height: el.height } : null;
}
function register(AFRAME) {
  AFRAME.registerComponent('gaussian_splatting', {
    schema,
    init() {
      const sceneEl = this.el && this.el.sceneEl;
      this.impl = new GaussianSplatting(Object.assign({}, this.data, { cutoutEntity: null })).init(sceneEl);
      this.ready = null;
      const start = () => {
        if (this.data.cutoutEntity) this.impl.cutout = this.data.cutoutEntity.object3D;          // index.js:19-21
        this.ready = this.impl.loadData(sceneCamera(sceneEl), this.el.object3D, sceneEl.renderer, this.data.src);   // index.js:18
        return this.ready;
      };
      if (!sceneEl) return;
      if (sceneEl.hasLoaded) start(); else sceneEl.addEventListener('loaded', start);               // index.js:17
    },
    tick() {
      const g = this.impl;
      if (!g || !g.camera || !g.loadedVertexCount) return;
      g.tick();                                                                                     // index.js:438-455
      if (this.frameSink) {
        const vp = this.viewport || drawingBuffer(g.renderer);
        if (vp) this.frameSink(g.render(g.camera, vp), vp);
      }
    },
    update() { if (this.impl) this.impl.update(this.data); },
    remove() { if (this.impl) this.impl.remove(); this.impl = null; },
  });
}

module.exports = { schema, GaussianSplatting, register, native, RENDER_PARALLEL };

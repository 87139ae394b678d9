"""GPU tier: WHERE a frame lands.  Every write-out of the library -- the blend kernels' stores into a caller's device pointer on every
blend path and in both binning rounds, the surface planes, contribution frames, the host copies with a row stride (synchronous and
queued, page-locked and pageable), gs_render_stereo, frames in flight on the lanes, the gathered assembly (k_assemble) and the
gs_multi forms -- writes into a destination INSIDE a larger allocation pre-filled with the guard word 0xA5A5A5A5, a guard of at least
one whole fb_width x fb_height x 4 frame on each side, and every case asserts
  (a) every byte outside the documented rectangle is still the guard: row padding, what follows the last row's 4 * w bytes, both guards;
  (b) the rectangle equals the same columns of the BASE frame -- the tight, synchronous, full-frame gs_render of the same context and
      options -- bit for bit where x0 is a multiple of 4, within 1 LSB otherwise (include/gs_splat.h);
  (c) that BASE frame agrees with oracle.render by test_gpu_parity.pix_check (PIXEL_TOL_LSB).
Scene, frame sizes, strips and the proof that such frames can show a misplaced write: test_writeout_cpu.py.

Device destinations come from one hipMalloc per case; host destinations from one numpy array (or one gs_host_alloc block) per case whose
last byte is the guard behind the last row's 4 * w bytes, so a copy of a whole stride for the last row shows.

Budget: about 1.8 s of wall time on one MI355X as last measured (29 tests, the slowest 0.3 s: ~4000 guarded destinations, frames of 1x1
to 64x33 pixels, one context per blend path shared across shapes)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from test_gpu_parity import PATH_OPTIONS, assert_path, force_path, pix_check
from test_multirank_gpu import Ranks
from test_writeout_cpu import (EYE_YAWS, G_BYTE, POSE_YAWS, SCENE_SIZES, SIZES, STRIP_FRAME, STRIPS, camera, cloud, params, reference,
                               scene_planes)

pytestmark = pytest.mark.gpu
capi = pkg("capi")

FLIP, ASYNC = capi.RENDER_FLIP_Y, capi.RENDER_ASYNC
PATHS = ("lists", "walk", "subtile", "split", "pairs")
PERMILLES = (1000, 300)                                   # one binning round; two (the second round's write-out runs: gs_stats.unsat_tiles)
assert all(p in PATH_OPTIONS for p in PATHS) and PATH_OPTIONS["split"][capi.OPT_BLEND_SPLIT] == 1   # (every tile with an entry is split)


# ---------------------------------------------------------------- guarded allocations

def _up(n, a=256):
    return (n + a - 1) // a * a


def layout(extents, guard, offsets=None):
    """Byte offsets of destinations of `extents` bytes inside one allocation: guard, destination, guard, destination, ..., guard.
    Every destination starts offsets[k] bytes behind a 256-byte boundary; the allocation ends `guard` bytes behind the last one.
    -> (starts, total)"""
    guard = _up(max(guard, 256))
    starts, pos = [], 0
    for k, e in enumerate(extents):
        s = _up(pos + guard) + (offsets[k] if offsets else 0)
        starts.append(s)
        pos = s + e
    return starts, pos + guard


class DevAlloc:
    """one hipMalloc of nbytes, every byte the guard's"""

    _hip = None

    def __init__(self, nbytes):
        if DevAlloc._hip is None:
            DevAlloc._hip = capi.hip_runtime()
        self.hip, self.n, self.p = DevAlloc._hip, int(nbytes), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(self.n)) == 0
        assert self.p.value % 256 == 0
        self.fill()

    def fill(self):
        assert self.hip.hipMemset(self.p, G_BYTE, C.c_size_t(self.n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def read(self):
        out = np.empty(self.n, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.n), 2) == 0
        return out

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.hip.hipFree(self.p)


class HostAlloc:
    """nbytes of host memory, every byte the guard's: a numpy array, or one gs_host_alloc block (pinned=True)"""

    def __init__(self, nbytes, pinned=False):
        self.n, self.pinned = int(nbytes), pinned
        if pinned:
            self._L = capi.load()
            self._p = self._L.gs_host_alloc(self.n)
            assert self._p
            self.buf = np.ctypeslib.as_array((C.c_uint8 * self.n).from_address(self._p))
        else:
            self.buf = np.empty(self.n, np.uint8)
        self.buf[:] = G_BYTE
        self.addr = self.buf.ctypes.data

    def fill(self):
        self.buf[:] = G_BYTE

    def read(self):
        return self.buf.copy()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.pinned:
            self.buf = None
            self._L.gs_host_free(self._p)


def check(buf, rects, wants, tag, guard, tols=None):
    """buf: the whole allocation read back (uint8).  rects: (start, rows, row_bytes, stride) per destination; wants: what each holds, or
    None for a destination that must not have been written at all.  (a) and (b) of the module's docstring."""
    keep = np.ones(buf.size, bool)
    lo, hi = buf.size, 0
    for k, ((start, rows, rb, stride), want) in enumerate(zip(rects, wants)):
        if want is None:
            continue
        idx = start + np.arange(rows)[:, None] * stride + np.arange(rb)[None, :]
        lo, hi = min(lo, int(idx.min())), max(hi, int(idx.max()) + 1)
        keep[idx] = False
        got = buf[idx]
        w = np.ascontiguousarray(want).view(np.uint8).reshape(rows, rb)
        tol = tols[k] if tols else 0
        if tol == 0:
            assert np.array_equal(got, w), (tag, k, "rectangle differs from BASE in %d bytes" % int((got != w).sum()))
        else:
            d = int(np.abs(got.astype(np.int16) - w.astype(np.int16)).max())
            assert d <= tol, (tag, k, "rectangle differs from BASE by %d LSB" % d)
    assert lo >= guard and buf.size - hi >= guard, (tag, "a guard is smaller than a frame", lo, buf.size - hi, guard)
    stray = np.flatnonzero(keep & (buf != G_BYTE))
    assert stray.size == 0, (tag, "%d bytes written outside the rectangle, first at %d (rectangles: %r)" % (stray.size, int(stray[0]), rects))


def rect(start, H, w, stride=0):
    return (start, H, 4 * w, stride or 4 * w)


def extent(H, w, stride=0):
    """bytes from a destination's first to its last written byte: (H - 1) strides and one row of 4 * w bytes"""
    return (H - 1) * (stride or 4 * w) + 4 * w


def strides_of(w):
    return (0, 4 * w, 4 * w + 4, 4 * (w + 16))


# ---------------------------------------------------------------- contexts and BASE frames

class Drawer:
    """One context on one blend path (None: the default options), the cloud pushed and sorted for yaw 0, and its BASE frames: the tight,
    synchronous, full-frame gs_render for (permille, size, scene, yaw) as the context stands, each held to the oracle once."""

    def __init__(self, path, opts=()):
        self.path, self.c, self.bases, self.yaw, self.permille, self.scene = path, capi.Context(0), {}, None, None, None
        if path is not None:
            force_path(self.c, path)
        for k, v in opts:
            self.c.set_option(k, v)
        self.c.push_splat(cloud().rows)
        self.sort(0.0)

    def sort(self, yaw, want_indices=True):
        if want_indices and yaw == self.yaw:
            return
        self.c.sort(camera(*STRIP_FRAME, yaw)["view"], want_indices=want_indices)
        self.yaw = yaw

    def use(self, permille=None, scene=None):
        """options of the frames that follow: GS_OPT_NEAR_PERMILLE and the scene (W, H) or None"""
        if permille is not None and permille != self.permille:
            self.c.set_option(capi.OPT_NEAR_PERMILLE, permille)
            self.permille = permille
        if scene != self.scene:
            if scene is None:
                self.c.set_scene(None, None)
            else:
                self.c.set_scene(*scene_planes(*scene))
            self.scene = scene

    def proof(self, tag):
        """the last frame ran this drawer's path, and -- with two binning rounds -- its second round"""
        st = assert_path(self.c, self.path, tag) if self.path is not None else self.c.stats()
        if self.permille == 300:
            assert st["unsat_tiles"] > 0, (tag, "no tile was left to the second round")
        return st

    def base(self, W, H, eye_yaw=None):
        """eye_yaw: the view's own camera while the order stays the sorted one's (the eyes of a stereo frame)"""
        yaw = self.yaw if eye_yaw is None else eye_yaw
        key = (self.permille, W, H, self.scene is not None, yaw, self.yaw)
        if key not in self.bases:
            assert self.scene in (None, (W, H))
            img = self.c.render(params(W, H, yaw=yaw))
            self.proof(key)
            pix_check("writeout_%s_%s_%dx%d_scene%d_yaw%g" % (self.path, self.permille, W, H, self.scene is not None, yaw), img,
                      reference(W, H, self.scene is not None, yaw))
            img.setflags(write=False)
            self.bases[key] = img
        return self.bases[key]

    def close(self):
        self.c.close()


@pytest.fixture(scope="module")
def drawers():
    made = {}

    def get(path):
        if path not in made:
            made[path] = Drawer(path)
        return made[path]
    yield get
    for d in made.values():
        d.close()


def oriented(img, flags):
    return img[::-1] if flags & FLIP else img


def frame_bytes(W, H):
    return 4 * W * H


# ---------------------------------------------------------------- gs_render_device into a caller's pointer

@pytest.mark.parametrize("path", PATHS)
def test_render_device_every_size_and_base_offset(drawers, path):
    d = drawers(path)
    for permille in PERMILLES:
        for W, H in SIZES:
            for scene in (None, (W, H)) if (W, H) in SCENE_SIZES else (None,):
                d.use(permille, scene)
                base = d.base(W, H)
                for off in (0, 4, 8, 12):
                    for flags in (0, FLIP):
                        tag = (path, permille, W, H, scene is not None, off, flags)
                        (start,), total = layout([extent(H, W)], frame_bytes(W, H), [off])
                        with DevAlloc(total) as a:
                            d.c.render_device(params(W, H, flags=flags), a.p.value + start)
                            d.proof(tag)
                            check(a.read(), [rect(start, H, W)], [oriented(base, flags)], tag, frame_bytes(W, H))


@pytest.mark.parametrize("path", PATHS)
def test_render_device_strips_of_a_64_wide_frame(drawers, path):
    d = drawers(path)
    W, H = STRIP_FRAME
    for permille in PERMILLES:
        for scene in (None, (W, H)):
            d.use(permille, scene)
            base = d.base(W, H)
            for k, (x0, x1) in enumerate(STRIPS):
                for flags in (0, FLIP):
                    off = (0, 4, 8, 12)[(k + (flags != 0)) % 4]
                    tag = (path, permille, scene is not None, x0, x1, off, flags)
                    (start,), total = layout([extent(H, x1 - x0)], frame_bytes(W, H), [off])
                    with DevAlloc(total) as a:
                        d.c.render_device(params(W, H, x0, x1, flags=flags), a.p.value + start)
                        d.proof(tag)
                        check(a.read(), [rect(start, H, x1 - x0)], [oriented(base, flags)[:, x0:x1]], tag, frame_bytes(W, H),
                              tols=[0 if x0 % 4 == 0 else 1])


# ---------------------------------------------------------------- device forms of the surface and contribution calls

SURFACE_VIEWS = tuple((W, H, 0, W) for W, H in ((5, 17), (16, 16), (20, 16), (33, 17), (64, 33), (4, 1), (1, 1))) + \
                tuple(STRIP_FRAME + s for s in ((0, 17), (4, 8), (16, 33), (20, 64), (16, 17)))
PLANE_OFFSETS = ((0, 0, 0, 0), (4, 4, 4, 4), (0, 4, 0, 4), (4, 0, 4, 0))       # colour, id, depth, alpha


def test_surface_device_colour_and_planes(drawers):
    d = drawers("lists")
    for permille in PERMILLES:
        for W, H, x0, x1 in SURFACE_VIEWS:
            for scene in (None, (W, H)) if (W, H) in ((64, 33), (20, 16)) else (None,):
                d.use(permille, scene)
                base = d.base(W, H)
                planes = d.c.render_surface(params(W, H), rgba=False)[1:]            # the full frame's planes, tight, through the host form
                d.proof("surface planes")
                assert d.c.stats()["surface"] == 1
                sw, fb = x1 - x0, frame_bytes(W, H)
                for n, offs in enumerate(PLANE_OFFSETS):
                    for flags in (0, FLIP):
                        # one of the four destinations is NULL in turn (none in the first round): it must stay untouched
                        skip = (n + (flags != 0)) % 5 - 1
                        tag = (permille, W, H, x0, x1, scene is not None, offs, flags, skip)
                        starts, total = layout([extent(H, sw)] * 4, fb, offs)
                        wants = [oriented(base, flags)[:, x0:x1]] + [oriented(p, flags)[:, x0:x1] for p in planes]
                        wants = [None if k == skip else w for k, w in enumerate(wants)]
                        with DevAlloc(total) as a:
                            ptrs = [None if k == skip else a.p.value + s for k, s in enumerate(starts)]
                            d.c.render_surface_device(params(W, H, x0, x1, flags=flags), *ptrs)
                            d.proof(tag)
                            check(a.read(), [rect(s, H, sw) for s in starts], wants, tag, fb)


def test_contrib_device_colour(drawers):
    d = drawers("lists")
    try:
        for permille in PERMILLES:
            for W, H, x0, x1 in SURFACE_VIEWS:
                d.use(permille, None)
                base = d.base(W, H)
                for off in (0, 4, 8, 12):
                    flags = FLIP if off in (4, 12) else 0
                    tag = (permille, W, H, x0, x1, off, flags)
                    (start,), total = layout([extent(H, x1 - x0)], frame_bytes(W, H), [off])
                    with DevAlloc(total) as a:
                        d.c.render_contrib_device(params(W, H, x0, x1, flags=flags), a.p.value + start)
                        d.proof(tag)
                        check(a.read(), [rect(start, H, x1 - x0)], [oriented(base, flags)[:, x0:x1]], tag, frame_bytes(W, H))
        assert d.c.contrib_info()[1] > 0
    finally:
        d.c.contrib_clear()


# ---------------------------------------------------------------- the host path: row strides, queued frames, stereo, host planes

def _render_host(c, p, addr, stride):
    c._ck(c._L.gs_render(c._h, C.byref(p), C.c_void_p(addr), stride))


def _sync(c):
    """gs_sync; a frame the library could not draw again by itself is the caller's to repeat: False"""
    try:
        c.sync()
        return True
    except capi.GsError as e:
        assert e.code == capi.E_RETRY
        return False


@pytest.mark.parametrize("path", ("lists", "walk"))
@pytest.mark.parametrize("mode", ("sync", "async_pinned", "async_pageable"))
def test_host_frames_with_a_row_stride(path, mode):
    d = Drawer(path)
    try:
        for permille in PERMILLES:
            d.use(permille, None)
            for n, (W, H) in enumerate(SIZES):
                base = d.base(W, H)
                for k, stride in enumerate(strides_of(W)):
                    flags = FLIP if (n + k) % 2 else 0
                    tag = (path, mode, permille, W, H, stride, flags)
                    (start,), total = layout([extent(H, W, stride)], frame_bytes(W, H))
                    with HostAlloc(total, pinned=(mode == "async_pinned")) as a:
                        assert a.n == start + (H - 1) * (stride or 4 * W) + 4 * W + _up(frame_bytes(W, H))
                        for attempt in range(4):
                            a.fill()
                            if mode == "sync":
                                _render_host(d.c, params(W, H, flags=flags), a.addr + start, stride)
                                break
                            d.sort(0.0, want_indices=False)
                            _render_host(d.c, params(W, H, flags=flags | ASYNC), a.addr + start, stride)
                            if _sync(d.c):
                                break
                            assert attempt < 3
                        d.proof(tag)
                        check(a.read(), [rect(start, H, W, stride)], [oriented(base, flags)], tag, frame_bytes(W, H))
    finally:
        d.close()


def test_stereo_eyes_are_neighbours_in_one_allocation():
    d = Drawer("lists")
    try:
        for W, H in ((33, 17), (64, 33), (17, 15)):
            bases = [d.base(W, H, eye_yaw=y) for y in EYE_YAWS]                 # both eyes from the head camera's order (yaw 0)
            assert not np.array_equal(bases[0], bases[1])
            for stride in strides_of(W):
                for flags in (0, FLIP):
                    tag = (W, H, stride, flags)
                    starts, total = layout([extent(H, W, stride)] * 2, frame_bytes(W, H))
                    with HostAlloc(total) as a:
                        eyes = (capi.RenderParams * 2)(*[params(W, H, flags=flags, yaw=y) for y in EYE_YAWS])
                        outs = (C.c_void_p * 2)(*[a.addr + s for s in starts])
                        d.c._ck(d.c._L.gs_render_stereo(d.c._h, eyes, outs, stride))
                        check(a.read(), [rect(s, H, W, stride) for s in starts], [oriented(b, flags) for b in bases], tag, frame_bytes(W, H))
    finally:
        d.close()


def test_surface_host_planes_and_null_planes(drawers):
    d = drawers("lists")
    for permille in PERMILLES:
        d.use(permille, None)
        for W, H, x0, x1 in ((33, 17, 0, 33), (20, 16, 0, 20), (5, 17, 0, 5), (64, 33, 20, 63)):
            base = d.base(W, H)
            planes = d.c.render_surface(params(W, H), rgba=False)[1:]
            sw, fb = x1 - x0, frame_bytes(W, H)
            for skip in (-1, 0, 1, 2, 3):
                for flags in (0, FLIP):
                    stride = strides_of(sw)[(skip + 1 + (flags != 0)) % 4]
                    tag = (permille, W, H, x0, x1, skip, flags, stride)
                    starts, total = layout([extent(H, sw, stride)] + [extent(H, sw)] * 3, fb)
                    wants = [oriented(base, flags)[:, x0:x1]] + [oriented(p, flags)[:, x0:x1] for p in planes]
                    wants = [None if k == skip else w for k, w in enumerate(wants)]
                    with HostAlloc(total) as a:
                        ptrs = [None if k == skip else a.addr + s for k, s in enumerate(starts)]
                        s = capi.Surface(*ptrs[1:])
                        p = params(W, H, x0, x1, flags=flags)
                        d.c._ck(d.c._L.gs_render_surface(d.c._h, C.byref(p), C.c_void_p(ptrs[0]) if ptrs[0] else None, stride, C.byref(s)))
                        d.proof(tag)
                        check(a.read(), [rect(starts[0], H, sw, stride)] + [rect(t, H, sw) for t in starts[1:]], wants, tag, fb)


# ---------------------------------------------------------------- several frames in flight

@pytest.mark.parametrize("path", PATHS)
def test_six_queued_frames_into_neighbouring_device_buffers(path):
    """GS_OPT_PIPELINE_DEPTH 3, GS_OPT_FRAME_BATCH 2: six poses queued before one gs_sync, each into its own buffer of one allocation.
    Placement and pixels only: whether two frames shared their launches is the enqueue threads' timing (test_blend_paths_gpu.py)."""
    d = Drawer(path, opts=((capi.OPT_PIPELINE_DEPTH, 3),))
    try:
        for permille in PERMILLES:
            d.use(permille, None)
            for W, H in ((33, 17), (64, 33), (20, 16), (17, 15)):
                d.c.set_option(capi.OPT_FRAME_BATCH, 1)
                bases = []
                for y in POSE_YAWS:
                    d.sort(y)
                    bases.append(d.base(W, H))
                d.c.set_option(capi.OPT_FRAME_BATCH, 2)
                for flags in (0, FLIP):
                    tag = (path, permille, W, H, flags)
                    starts, total = layout([extent(H, W)] * 6, frame_bytes(W, H), (0, 4, 8, 12, 0, 4))
                    with DevAlloc(total) as a:
                        for attempt in range(4):
                            a.fill()
                            for y, s in zip(POSE_YAWS, starts):
                                d.sort(y, want_indices=False)
                                d.c.render_device(params(W, H, flags=flags | ASYNC, yaw=y), a.p.value + s)
                            if _sync(d.c):
                                break
                            assert attempt < 3
                        d.yaw = None
                        if d.path is not None:
                            assert_path(d.c, d.path, tag)
                        check(a.read(), [rect(s, H, W) for s in starts], [oriented(b, flags) for b in bases], tag, frame_bytes(W, H))
    finally:
        d.close()


# ---------------------------------------------------------------- gathered and multi-device frames (one GPU, repeated ordinals)

MULTI_SIZES = ((17, 15), (33, 17), (64, 33))                # widths 17, 33, 64: a ragged last strip; two tile columns for three ranks


@pytest.fixture(scope="module")
def plain():
    """a context with the default options, as the ranks and gs_multi's contexts have them: the BASE of the gathered frames"""
    d = Drawer(None)
    yield d
    d.close()


def _xr_bases(plain, W, H):
    plain.sort(0.0)
    return [plain.base(W, H, eye_yaw=y) for y in EYE_YAWS]


@pytest.mark.parametrize("world", (2, 3))
def test_gathered_frames_assembled_into_device_frames(plain, world):
    R = Ranks(world, cloud().rows)
    try:
        for W, H in MULTI_SIZES:
            plain.sort(0.0)
            base, fb = plain.base(W, H), frame_bytes(W, H)
            view = camera(W, H)["view"]
            for root in (0, world - 1):
                for flags in (0, FLIP):
                    tag = (world, W, H, root, flags)
                    (start,), total = layout([extent(H, W)], fb)
                    with DevAlloc(total) as a:
                        def body(rank, c, R):
                            c.sort_gathered(view, None, params(W, H))
                            c.render_gathered(params(W, H, flags=flags), root=root, device_frames=[a.p.value + start] if rank == root else None,
                                              flags=flags)
                            R.barrier.wait()
                        R.run(body)
                        check(a.read(), [rect(start, H, W)], [oriented(base, flags)], tag, fb)
            if world == 2:                                                  # the XR pair: eye k on rank k, one sort from the head camera
                bases = _xr_bases(plain, W, H)
                for flags in (0, FLIP):
                    tag = (world, W, H, "xr", flags)
                    starts, total = layout([extent(H, W)] * 2, fb)
                    with DevAlloc(total) as a:
                        def body(rank, c, R):
                            eyes = [params(W, H, flags=flags, yaw=y) for y in EYE_YAWS]
                            c.sort_gathered(view, None, eyes)
                            c.render_gathered(eyes, root=0, device_frames=[a.p.value + s for s in starts] if rank == 0 else None, flags=flags)
                            R.barrier.wait()
                        R.run(body)
                        check(a.read(), [rect(s, H, W) for s in starts], [oriented(b, flags) for b in bases], tag, fb)
    finally:
        R.close()


@pytest.mark.parametrize("world", (2, 3))
def test_multi_host_direct_device_frames_and_reads(plain, world):
    L = capi.load()
    with capi.Multi([0] * world) as m:
        m.push_splat(cloud().rows)
        for W, H in MULTI_SIZES:
            plain.sort(0.0)
            base, fb = plain.base(W, H), frame_bytes(W, H)
            view = camera(W, H)["view"]
            views = {0: [params(W, H)], FLIP: [params(W, H, flags=FLIP)]}
            wants = {0: [base], FLIP: [base[::-1]]}
            if world == 2:
                bases = _xr_bases(plain, W, H)
                for f in (0, FLIP):
                    views[("xr", f)] = [params(W, H, flags=f, yaw=y) for y in EYE_YAWS]
                    wants[("xr", f)] = [oriented(b, f) for b in bases]
            for key, vs in views.items():
                flags = key[1] if isinstance(key, tuple) else key
                arr = (capi.RenderParams * len(vs))(*vs)
                for k, stride in enumerate(strides_of(W)):
                    tag = (world, W, H, key, stride)
                    # host-direct: every device copies its strip into its columns of the caller's frame(s); queued and page-locked in turn
                    queued = k % 2 == 1
                    starts, total = layout([extent(H, W, stride)] * len(vs), fb)
                    with HostAlloc(total, pinned=queued) as a:
                        for attempt in range(4):
                            a.fill()
                            m.sort(view, None, vs)
                            ptrs = (C.c_void_p * len(vs))(*[a.addr + s for s in starts])
                            m._ck(L.gs_multi_render(m._h, arr, len(vs), ptrs, stride, flags | (ASYNC if queued else 0)))
                            try:
                                m.sync()
                                break
                            except capi.GsError as e:
                                assert e.code == capi.E_RETRY and attempt < 3
                        check(a.read(), [rect(s, H, W, stride) for s in starts], wants[key], tag + ("host-direct",), fb)
                    # gathered on devices[0] into the library's own frames, read back with a stride
                    m.sort(view, None, vs)
                    m.render_device(vs, flags=flags)
                    with HostAlloc(total) as a:
                        for v, s in enumerate(starts):
                            m._ck(L.gs_multi_read(m._h, v, C.c_void_p(a.addr + s), stride))
                        check(a.read(), [rect(s, H, W, stride) for s in starts], wants[key], tag + ("read",), fb)
                # gathered on devices[0] into the caller's device frames
                starts, total = layout([extent(H, W)] * len(vs), fb)
                with DevAlloc(total) as a:
                    m.sort(view, None, vs)
                    m.render_device(vs, device_frames=[a.p.value + s for s in starts], flags=flags)
                    m.sync()
                    check(a.read(), [rect(s, H, W) for s in starts], wants[key], (world, W, H, key, "device frames"), fb)
